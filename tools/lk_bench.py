"""LK objectives on the reduced teacher and compacted loss rows against the materialised dense path, inside the real optimizer step:

    python tools/lk_bench.py [--config llama3-8b] [--batch 8 --seq 2048] [--ttt 7] [--steps 4] [--out profiles/lk_reduced_teacher_ab.jsonl]   (GPU box)

Per ``lk_loss_type`` in {lambda, alpha} and loss-mask density in {1.0, 0.5} (bench.make_loss_mask: the turn-like spans bench.py draws),
two trainers of the same draft at the same weights: ``new`` (the defaults) and ``old`` (``materialise_soft_targets=True,
compact_loss_rows=False``: the only LK path before sf_ce_lk_grad_zt_rows).  Both are warmed up, then timed in the order new, old, old, new
-- alternating, and each leg measured twice so that the file carries its own spread.  ms/step is a host clock around a device
synchronise, optimizer step included.  One JSON line per leg: the samples, their mean and spread, the engine's arena bytes (a leg's
engine is its own; densities run 1.0 first, so the figure is the largest shape's).  Two more lines: the LK-gradient kernels alone at
rows x V bf16 logits (HIP events around the launch, the logits restored outside the timed region) beside the bytes counted from shapes.
No GPU: the tool fails."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from specforge_amd import ops  # noqa: E402
from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead, TrainBatch, loss_mask_suffix_counts  # noqa: E402
from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3  # noqa: E402
from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend  # noqa: E402


def trainer(cfg, dev, ttt, lk, old):
    torch.manual_seed(0)
    model = LlamaForCausalLMEagle3(DraftConfig(**cfg), device=dev)
    t2d = torch.zeros(cfg["vocab_size"], dtype=torch.bool)
    ids = torch.randperm(cfg["vocab_size"], generator=torch.Generator().manual_seed(0))[:cfg["draft_vocab_size"]].sort().values
    t2d[ids] = True
    model.load_vocab_mapping_tensors(t2d, ids - torch.arange(cfg["draft_vocab_size"]))
    eagle = OnlineEagle3Model(model, length=ttt, lk_loss_type=lk).train()
    head = TargetHead((torch.randn(cfg["vocab_size"], cfg["target_hidden_size"], device=dev) * 0.02).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-4, max_grad_norm=0.5, total_steps=10_000_000, warmup_ratio=0.0))
    backend.prepare_model(eagle)
    if old:
        eagle.engine.materialise_soft_targets, eagle.engine.compact_loss_rows = True, False
    return eagle, strat, backend


def kernel_lines(dev, rows, V, reps):
    """the two LK-gradient kernels alone: every row with a position mask, lambda; bytes from shapes"""
    g = torch.Generator(device=dev).manual_seed(1)
    S, Spad = rows, rows
    x0 = (torch.randn(rows, V, device=dev, generator=g) * 2).to(torch.bfloat16)
    zt = (torch.randn(rows, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    zf = zt.float()
    zmd = zf.max(-1).values.reshape(1, Spad).contiguous()
    e = torch.exp(zf - zmd.reshape(-1, 1))
    zinv = (1.0 / e.sum(-1)).reshape(1, Spad).contiguous()
    del zf
    tp = (e * zinv.reshape(-1, 1)).reshape(1, Spad, V).contiguous()
    del e
    pm = torch.ones(1, Spad, dtype=torch.int32, device=dev)
    pod = torch.rand(1, Spad, device=dev, generator=g)
    tsum = tp.sum(-1)
    kw = dict(S=S, Spad=Spad, off=0, pos_mask_pad=pm, pod_scale_pad=pod, tsum_pad=tsum, lk_loss_type="lambda", kl_scale=1.0, kl_decay=1.0,
              step_scale=1.0, kl_row_scale=1.0 / rows, accept_sum=torch.full((1,), 0.3 * rows, device=dev), mask_sum=torch.full((1,), float(rows), device=dev))
    x = torch.empty_like(x0)
    legs = {"sf_ce_lk_grad_zt_rows": (lambda: ops.ce_lk_grad_zt(x, zt, zmd, zinv, **kw),
                                      dict(logits_read=2 * V, zt_read=2 * V, grad_write=2 * V)),
            "sf_ce_lk_grad": (lambda: ops.ce_lk_grad(x, tp, **kw),
                              dict(logits_read=2 * V, target_read=4 * V, grad_write=2 * V, logits_reread_from_cache=3 * 2 * V,
                                   target_reread_from_cache=2 * 4 * V))}
    out = []
    for name, (fn, per_row) in legs.items():
        ms = []
        for i in range(2 + reps):
            x.copy_(x0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        once = rows * sum(v for k, v in per_row.items() if "reread" not in k)
        med = sorted(ms)[len(ms) // 2]
        out.append(dict(leg="kernel", kernel=name, rows=rows, V=V, dtype="bf16", hip_event_ms=[round(t, 4) for t in ms], median_ms=med,
                        bytes_per_row_from_shapes=per_row, bytes_once=once, bytes_issued=rows * sum(per_row.values()),
                        gb_per_s_on_bytes_once=once / med / 1e6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--seq", type=int, default=None)
    ap.add_argument("--ttt", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4, help="timed optimizer steps per sample (each leg gives two samples)")
    ap.add_argument("--kernel-rows", type=int, default=16384)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_reduced_teacher_ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lk_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    cfg, B0, S0, _ = bench.CONFIGS[args.config]
    cfg = dict(cfg)
    B, S = args.batch or B0, args.seq or S0
    cfg["max_position_embeddings"] = max(cfg["max_position_embeddings"], S + 16)
    lines = []
    for lk in ("lambda", "alpha"):
        legs = {name: trainer(cfg, dev, args.ttt, lk, old=(name == "old")) for name in ("new", "old")}
        for density in (1.0, 0.5):
            lm = bench.make_loss_mask(B, S, density, seed=7)
            tb = TrainBatch(bench.make_batch(cfg, B, S, dev, 100, lm), {"target_repr": "hidden_state", "loss_mask_suffix_counts": loss_mask_suffix_counts(lm)})

            def timed(name, n):
                eagle, strat, backend = legs[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    out = strat.forward_loss(tb)
                    backend.backward(out.loss, is_boundary=True)
                    backend.step()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / n, float(out.loss.detach())

            for name in ("new", "old"):
                timed(name, 2)
            acc, loss = {"new": [], "old": []}, {}
            for name in ("new", "old", "old", "new"):
                ms, loss[name] = timed(name, args.steps)
                acc[name].append(ms)
            for name in ("new", "old"):
                eng = legs[name][0].engine
                x = acc[name]
                lines.append(dict(leg=name, lk_loss_type=lk, loss_mask_density=density, loss_mask_mean=float(lm.float().mean()), config=args.config,
                                  batch=B, seq=S, ttt=args.ttt, steps_per_sample=args.steps, ms_per_step=[round(t, 3) for t in x],
                                  mean_ms=sum(x) / len(x), same_leg_spread_ms=max(x) - min(x), arena_bytes=eng.arena_bytes(), soft=eng._soft[0],
                                  teacher_compacted=eng._teacher_compacted, lm_compact=eng._lm_compact_K is not None, last_loss=loss[name]))
                print(json.dumps(lines[-1]), flush=True)
        del legs
        torch.cuda.empty_cache()
    for ln in kernel_lines(dev, args.kernel_rows, cfg["draft_vocab_size"], args.kernel_reps):
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
