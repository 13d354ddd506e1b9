#!/usr/bin/env python
"""Offline EAGLE3 draft training on MI355X with the specforge_amd path, end to end:

    pre-captured hidden-state files (the reference's format, scripts/prepare_hidden_states.py:446-480)
      -> HiddenStateIngest (normalise, right-pad, DistributedSampler-identical shards, pinned double buffer)
      -> Eagle3TrainStrategy.forward_loss (teacher soft targets, 7-step TTT unroll, CE / LK loss, metrics)
      -> TrainerCore.train_step (accumulation, DP all-reduce on boundaries, clip + AdamW)
      -> checkpoint in the reference's draft state-dict layout (export --to sglang compatible)

One process per GPU:
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_offline_eagle3.py \\
        --draft-config configs/llama3-8B-eagle3.json --features /data/hidden_states --target-head lm_head.pt \\
        --vocab-mapping vocab_mapping.pt --embedding embed_tokens.pt --batch-size 8 --max-len 2048 --epochs 1

`--topk 1,2,4,8` also reports, at every log point, the share of scored rows whose target token is among the draft's k best logits per TTT
step and the optimistic tree bound built from those rates (specforge_amd.eagle3.TopKAccumulator), over the steps since the last report.
`--chain` reports beside it the share of chains still accepted at each depth, from the joint hits of every row over the TTT steps, and
their sum, the teacher-forced accepted length (specforge_amd.eagle3.ChainAccumulator): for top-1, and for every k of `--topk`.
`--conf-bins 10 --conf-thresholds 0.3,0.5,0.7` reports how well the draft's own top-1 probability tracks its hits (expected calibration
error per TTT depth) and, per threshold, the accepted and drafted tokens of a chain that stops drafting once its confidence falls under
it (specforge_amd.eagle3.ConfidenceAccumulator).

`--synthetic N` writes N random samples of the right shapes instead of reading --features (smoke runs, no data needed).
"""
import argparse
import glob
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import torch
import torch.distributed as dist

from specforge_amd.eagle3 import ChainAccumulator, ConfidenceAccumulator, Eagle3TrainStrategy, OnlineEagle3Model, TargetHead, TopKAccumulator
from specforge_amd.ingest import HiddenStateIngest
from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3
from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend, TrainerCore


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draft-config", required=True, help="HF-style draft config json (reference configs/*.json)")
    ap.add_argument("--features", help="directory of *.ckpt hidden-state samples")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--target-head", help="torch file with the target lm_head weight [Vt, Ht]")
    ap.add_argument("--vocab-mapping", help="torch file with t2d (bool [Vt]) and d2t (int64 [Vd])")
    ap.add_argument("--embedding", help="torch file with the target embedding table [Vt, H]")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--max-len", type=int, default=2048)
    ap.add_argument("--ttt-length", type=int, default=7)
    ap.add_argument("--accumulation-steps", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--max-grad-norm", type=float, default=0.5)
    ap.add_argument("--lk-loss-type", choices=["alpha", "lambda"], default=None)
    ap.add_argument("--topk", default="", help="comma-separated k (at most 8, ascending), e.g. 1,2,4,8: report top-k hit rates per TTT step")
    ap.add_argument("--chain", action="store_true", help="report the accepted length of the draft chains from the joint hits (top-1 and every --topk k)")
    ap.add_argument("--conf-bins", type=int, default=0, help="reliability bins (at most 32) of the draft's top-1 probability per TTT step")
    ap.add_argument("--conf-thresholds", default="", help="comma-separated confidence thresholds in [0, 1] (at most 8, ascending), e.g. 0.3,0.5,0.7")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--output", default="eagle3_draft.pt")
    args = ap.parse_args()
    topk = tuple(int(k) for k in args.topk.split(",") if k.strip())
    conf_tau = tuple(float(t) for t in args.conf_thresholds.split(",") if t.strip())

    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    cfg = DraftConfig.from_hf(json.load(open(args.draft_config)))
    torch.manual_seed(args.seed)
    model = LlamaForCausalLMEagle3(cfg, device=dev)
    if args.vocab_mapping:
        vm = torch.load(args.vocab_mapping)
        model.load_vocab_mapping_tensors(vm["t2d"], vm["d2t"])
    else:  # synthetic mapping of the fixture kind (tests/test_runtime/_fixtures.py)
        ids = torch.randperm(cfg.vocab_size, generator=torch.Generator().manual_seed(0))[:cfg.draft_vocab_size].sort().values
        t2d = torch.zeros(cfg.vocab_size, dtype=torch.bool)
        t2d[ids] = True
        model.load_vocab_mapping_tensors(t2d, ids - torch.arange(cfg.draft_vocab_size))
    if args.embedding:
        model.embed_tokens.weight.data.copy_(torch.load(args.embedding).to(torch.bfloat16))
    head_w = torch.load(args.target_head) if args.target_head else torch.randn(cfg.vocab_size, cfg.target_hidden_size) * 0.02
    head = TargetHead(head_w.to(torch.bfloat16).to(dev))

    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        g = torch.Generator().manual_seed(args.seed)
        for i in range(args.synthetic):
            L = args.max_len
            torch.save({"input_ids": torch.randint(0, cfg.vocab_size, (L,), generator=g), "loss_mask": torch.ones(L, dtype=torch.long),
                        "hidden_state": torch.randn(1, L, cfg.target_hidden_size, generator=g).to(torch.bfloat16),
                        "aux_hidden_state": torch.randn(1, L, 3 * cfg.target_hidden_size, generator=g).to(torch.bfloat16)},
                       os.path.join(tmp.name, f"{i:06d}.ckpt"))
        files = sorted(glob.glob(os.path.join(tmp.name, "*.ckpt")))
    else:
        files = sorted(glob.glob(os.path.join(args.features, "**", "*.ckpt"), recursive=True))
    if not files:
        raise SystemExit("no feature files")

    ingest = HiddenStateIngest(files, batch_size=args.batch_size, max_len=args.max_len, target_hidden_size=cfg.target_hidden_size,
                               device=dev, dp_rank=rank, dp_size=world, seed=args.seed)
    steps_total = max(1, ingest.batches_per_epoch() * args.epochs // args.accumulation_steps)
    eagle = OnlineEagle3Model(model, length=args.ttt_length, lk_loss_type=args.lk_loss_type, topk=topk, chain=args.chain,
                              conf_bins=args.conf_bins, conf_thresholds=conf_tau).train()
    strategy = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=args.lr, max_grad_norm=args.max_grad_norm,
                                                                             total_steps=steps_total))
    backend.prepare_model(eagle)
    core = TrainerCore(strategy, backend, accumulation_steps=args.accumulation_steps)

    t0, tokens = time.perf_counter(), 0
    hits = TopKAccumulator(topk) if topk else None
    chain_ks = tuple(sorted({1, *topk}))
    chains = ChainAccumulator(chain_ks) if args.chain else None
    confs = ConfidenceAccumulator(args.conf_bins, conf_tau) if args.conf_bins or conf_tau else None
    for epoch in range(args.epochs):
        for batch in ingest.epoch(epoch):
            res = core.train_step(batch)
            tokens += batch.tensors["input_ids"].numel() * world
            if hits is not None and rank == 0:
                hits.update(res.metrics)
            if chains is not None and rank == 0:
                chains.update(res.metrics)
            if confs is not None and rank == 0:
                confs.update(res.metrics)
            if res.stepped and rank == 0 and core.global_step % 10 == 0:
                torch.cuda.synchronize()
                acc = float(torch.stack(res.metrics["acces"]).mean())
                print(f"step {core.global_step}/{steps_total} loss {float(res.loss):.4f} acc {acc:.3f} "
                      f"grad_norm {float(res.grad_norm):.3f} lr {backend.optimizer.get_learning_rate():.2e} "
                      f"{tokens / (time.perf_counter() - t0):.0f} tok/s", flush=True)
                if hits is not None:        # (this rank's batches since the last report)
                    sm = hits.summary()
                    for k in topk:
                        rates = " ".join(f"{sm[f'top{k}_acc_{i}']:.3f}" for i in range(args.ttt_length))
                        print(f"  top-{k} hit rate per step: {rates}   simulated_acc_len_top{k} {sm[f'simulated_acc_len_top{k}']:.3f}", flush=True)
                    hits = TopKAccumulator(topk)
                if chains is not None:
                    sm = chains.summary()
                    for k in chain_ks:
                        rates = " ".join(f"{sm[f'chain_top{k}_acc_{i}']:.3f}" for i in range(args.ttt_length))
                        print(f"  top-{k} chains alive per depth: {rates}   chain_acc_len_top{k} {sm[f'chain_acc_len_top{k}']:.3f}", flush=True)
                    chains = ChainAccumulator(chain_ks)
                if confs is not None:
                    sm = confs.summary()
                    if args.conf_bins:
                        print("  calibration per depth (ece / mean confidence / top-1 rate): "
                              + " ".join(f"{sm[f'conf_ece_{i}']:.3f}/{sm[f'conf_mean_{i}']:.3f}/{sm[f'conf_acc_{i}']:.3f}" for i in range(args.ttt_length)), flush=True)
                    for t in conf_tau:
                        nm = ConfidenceAccumulator.tau_name(t)
                        print(f"  gated at conf >= {nm}: accepted {sm[f'gated_acc_len_tau{nm}']:.3f} of {sm[f'gated_draft_len_tau{nm}']:.3f} drafted per chain "
                              f"({sm[f'gated_acc_per_draft_tau{nm}']:.3f})", flush=True)
                    confs = ConfidenceAccumulator(args.conf_bins, conf_tau)
    if rank == 0:
        state = backend.state_dict()
        torch.save(strategy.checkpoint_state_filter(state["model"]), args.output)   # reference draft checkpoint keys
        print("saved", args.output, "after", core.global_step, "optimizer steps")
    if tmp is not None:
        tmp.cleanup()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
