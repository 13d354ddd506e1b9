"""The target-rank kernel (sf_topk_rank) beside the fused CE it runs in front of, and the metric's cost per eval forward:

    python tools/topk_rank_bench.py [--shapes 16384x32000,4096x32000] [--reps 20] [--eval-forward] [--out profiles/topk_rank_bench.jsonl]   (GPU box)

Kernel lines: bf16 logits [rows, V], every row with a loss mask and a target inside the draft vocabulary (no row takes the early exit),
thresholds (1, 2, 4, 8); on the same logits sf_ce_fused with write_grad = 0 against fp32 soft targets.  HIP events around each launch
after warm-up launches, the two kernels alternating; per kernel the samples, their median, the bytes the algorithm needs counted from the
shapes (rank: the logits once; CE: the logits once -- its second pass is meant to hit the caches -- and the fp32 targets once) and the
median's share of 8.0 TB/s.  ``--eval-forward``: one eval forward of the benchmark's default configuration with ``topk`` off and
(1, 2, 4, 8), alternating off, on, on, off (host clock around a device synchronise).  Lines are APPENDED to ``--out``.  No GPU: the tool fails."""
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
from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead, TrainBatch  # noqa: E402
from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3  # noqa: E402

HBM_PEAK = 8.0e12
TOPK = (1, 2, 4, 8)


def kernel_lines(dev, rows, V, reps):
    g = torch.Generator(device=dev).manual_seed(1)
    x = (torch.randn(rows, V, device=dev, generator=g) * 2).to(torch.bfloat16)
    tp = torch.softmax(torch.randn(rows, V, device=dev, generator=g) * 3, dim=-1).reshape(1, rows, V).contiguous()
    ones = torch.ones(1, rows, dtype=torch.int32, device=dev)
    tsum = tp.sum(-1)
    d2t = torch.zeros(V, dtype=torch.int64, device=dev)
    tgt = torch.randint(0, V, (1, rows), device=dev, generator=g)
    hit = torch.empty(len(TOPK), rows, device=dev)
    rank = torch.empty(rows, dtype=torch.int32, device=dev)
    outs = [torch.empty(rows, device=dev) for _ in range(3)]
    addr = dict(S=rows, Spad=rows, off=0, loss_mask_pad=ones, tgt_ids_pad=tgt)
    legs = {"sf_topk_rank": (lambda: ops.topk_rank(x, kk=TOPK, row_hit=hit, row_rank=rank, **addr), dict(logits_read=2 * V)),
            "sf_ce_fused(write_grad=0)": (lambda: ops.ce_fused(x, tp, pos_mask_pad=ones, tsum_pad=tsum, d2t=d2t, write_grad=False, row_loss=outs[0],
                                                               row_correct=outs[1], row_accept=outs[2], **addr),
                                          dict(logits_read=2 * V, target_read=4 * V))}
    ms = {k: [] for k in legs}
    for i in range(3 + reps):
        for name, (fn, _) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms[name].append(a.elapsed_time(b))
    assert torch.equal(hit[0], outs[1])          # threshold 1 == the CE's correct rows, on the timed inputs
    out = []
    for name, (_, per_row) in legs.items():
        med = sorted(ms[name])[len(ms[name]) // 2]
        nbytes = rows * sum(per_row.values())
        out.append(dict(leg="kernel", kernel=name, rows=rows, V=V, dtype="bf16", hip_event_ms=[round(t, 4) for t in ms[name]], median_ms=med,
                        bytes_per_row_from_shapes=per_row, bytes=nbytes, tb_per_s=nbytes / med / 1e9, fraction_of_8_tb_per_s=nbytes / (med * 1e-3) / HBM_PEAK,
                        mean_rank=float(rank.float().mean())))
    return out


def eval_forward_lines(dev, config, steps):
    cfg, B, S, _ = bench.CONFIGS[config]
    cfg = dict(cfg)
    torch.manual_seed(0)
    model = LlamaForCausalLMEagle3(DraftConfig(**cfg), device=dev)
    t2d = torch.zeros(cfg["vocab_size"], dtype=torch.bool)
    ids = torch.randperm(cfg["vocab_size"], generator=torch.Generator().manual_seed(0))[:cfg["draft_vocab_size"]].sort().values
    t2d[ids] = True
    model.load_vocab_mapping_tensors(t2d, ids - torch.arange(cfg["draft_vocab_size"]))
    eagle = OnlineEagle3Model(model, length=7).eval()
    head = TargetHead((torch.randn(cfg["vocab_size"], cfg["target_hidden_size"], device=dev) * 0.02).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    tb = TrainBatch(bench.make_batch(cfg, B, S, dev, 100, bench.make_loss_mask(B, S, 1.0, seed=7)), {"target_repr": "hidden_state"})

    def timed(topk, n):
        eagle.topk = topk
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(n):
                strat.forward_loss(tb)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    for topk in ((), TOPK):
        timed(topk, 2)
    acc = {(): [], TOPK: []}
    for topk in ((), TOPK, TOPK, ()):
        acc[topk].append(timed(topk, steps))
    timed(TOPK, 1)
    counts = [t.tolist() for t in eagle.last_topk]
    return [dict(leg="eval_forward", config=config, batch=B, seq=S, ttt=7, topk=list(topk), steps_per_sample=steps, ms_per_forward=[round(t, 3) for t in x],
                 mean_ms=sum(x) / len(x), **({"topk_corrects": counts} if topk else {})) for topk, x in acc.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x32000,4096x32000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eval-forward", action="store_true")
    ap.add_argument("--config", default="llama3-8b")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_rank_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/topk_rank_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        rows, V = (int(v) for v in shape.split("x"))
        lines += kernel_lines(dev, rows, V, args.reps)
        torch.cuda.empty_cache()
    if args.eval_forward:
        lines += eval_forward_lines(dev, args.config, args.steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
