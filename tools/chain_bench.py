"""The joint chain fold (``Eagle3Engine.chain``: sf_chain_step + a row sum per TTT step) in the training step, on against off:

    python tools/chain_bench.py [--shapes 8x2048,1x2048] [--steps 10] [--out profiles/chain_accept_ab.jsonl]   (GPU box)

Per shape one draft at the benchmark's default configuration (Llama-3-8B dims, ttt 7, full loss mask), ``topk`` = (1, 2, 4, 8) in both
legs, one optimizer step = forward + backward + fused AdamW as bench.py times it (host clock around a device synchronise).  The legs
alternate in ONE process -- off, on, on, off -- after two warm-up steps each; a line per leg holds its samples (ms per step, ``--steps``
steps each at 8 x 2048, proportionally more at smaller shapes so that a sample stays above a second), their mean and the same-leg spread (max - min), and the ``on`` line the chain counts of its last step.  Switching ``chain``
rebuilds the engine's views, so each sample's first step is taken before the clock starts.  Lines are APPENDED to ``--out``.  No GPU:
the tool fails."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead, TrainBatch, loss_mask_suffix_counts  # noqa: E402
from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3  # noqa: E402
from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend  # noqa: E402

TOPK = (1, 2, 4, 8)


def step_lines(dev, config, B, S, steps):
    steps = steps * max(1, min(8, 16384 // (B * S)))
    cfg = dict(bench.CONFIGS[config][0])
    torch.manual_seed(0)
    model = LlamaForCausalLMEagle3(DraftConfig(**cfg), device=dev)
    t2d = torch.zeros(cfg["vocab_size"], dtype=torch.bool)
    ids = torch.randperm(cfg["vocab_size"], generator=torch.Generator().manual_seed(0))[:cfg["draft_vocab_size"]].sort().values
    t2d[ids] = True
    model.load_vocab_mapping_tensors(t2d, ids - torch.arange(cfg["draft_vocab_size"]))
    eagle = OnlineEagle3Model(model, length=7, topk=TOPK).train()
    head = TargetHead((torch.randn(cfg["vocab_size"], cfg["target_hidden_size"], device=dev) * 0.02).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    be = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-4, max_grad_norm=0.5, total_steps=10_000))
    be.prepare_model(eagle)
    lm = torch.ones(B, S, dtype=torch.int64)
    tb = TrainBatch(bench.make_batch(cfg, B, S, dev, 100, lm), {"target_repr": "hidden_state", "loss_mask_suffix_counts": loss_mask_suffix_counts(lm)})

    def one():
        out = strat.forward_loss(tb)
        be.backward(out.loss, is_boundary=True)
        be.step()
        return out

    def timed(chain, n):
        eagle.chain = chain
        one()                   # (the views of the other setting were dropped: rebuilt outside the clock)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = one()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, out

    for chain in (False, True):
        timed(chain, 2)
    acc, last = {False: [], True: []}, {}
    for chain in (False, True, True, False):
        ms, last[chain] = timed(chain, steps)
        acc[chain].append(ms)
    m = last[True].metrics
    counts = dict(chain_denoms=[float(x) for x in m["chain_denoms"]],
                  **{f"chain_top{k}_corrects": [float(x) for x in m[f"chain_top{k}_corrects"]] for k in TOPK})
    return [dict(leg="train_step", config=config, batch=B, seq=S, ttt=7, topk=list(TOPK), chain=chain, steps_per_sample=steps,
                 ms_per_step=[round(t, 3) for t in x], mean_ms=sum(x) / len(x), same_leg_spread_ms=max(x) - min(x),
                 **(counts if chain else {}))
            for chain, x in acc.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x2048,1x2048", help="BxS legs (default: the headline shape and batch 1)")
    ap.add_argument("--config", default="llama3-8b")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_accept_ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/chain_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        B, S = (int(v) for v in shape.split("x"))
        lines += step_lines(dev, args.config, B, S, args.steps)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
