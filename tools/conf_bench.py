"""The draft-confidence metrics (``Eagle3Engine.conf_bins`` / ``.conf_thresholds``: sf_row_conf in front of the fused CE, sf_conf_fold +
sf_chain_step + a row sum behind it, per TTT step): the streaming kernel alone, and the training step on against off:

    python tools/conf_bench.py [--kernel-shapes 16384x32000,4096x32000] [--reps 20] [--shapes 8x2048,1x2048] [--steps 10]
                               [--out profiles/conf_calibration_ab.jsonl]   (GPU box)

Kernel lines: bf16 logits [rows, V], every row with a loss mask and a target inside the draft vocabulary (no row takes an early exit);
sf_row_conf beside sf_topk_rank (thresholds 1, 2, 4, 8) on the same logits -- both read every row once and write a few words per row.
HIP events around each launch after warm-up launches, the two kernels alternating; per kernel the samples, their median and spread
(max - min), the bytes counted from the shapes (the logits once) and the median's share of 8.0 TB/s.

Step lines: per shape one draft at the benchmark's default configuration (Llama-3-8B dims, ttt 7, full loss mask), one optimizer step =
forward + backward + fused AdamW as bench.py times it (host clock around a device synchronise), the feature off and on (10 bins,
thresholds 0.3 / 0.5 / 0.7) alternating in ONE process -- off, on, on, off -- after two warm-up steps each; a line per leg holds its
samples (ms per step, ``--steps`` steps each at 8 x 2048, proportionally more at smaller shapes), their mean and the same-leg spread
(max - min), and the ``on`` line the counts of its last step.  Switching the option rebuilds the engine's views, so each sample's first
step is taken before the clock starts.  Lines are APPENDED to ``--out``.  No GPU: the tool fails."""
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

HBM_PEAK = 8.0e12
TOPK = (1, 2, 4, 8)
BINS, TAU = 10, (0.3, 0.5, 0.7)


def kernel_lines(dev, rows, V, reps):
    g = torch.Generator(device=dev).manual_seed(1)
    x = (torch.randn(rows, V, device=dev, generator=g) * 2).to(torch.bfloat16)
    ones = torch.ones(1, rows, dtype=torch.int32, device=dev)
    tgt = torch.randint(0, V, (1, rows), device=dev, generator=g)
    hit = torch.empty(len(TOPK), rows, device=dev)
    conf = torch.empty(rows, device=dev)
    addr = dict(S=rows, Spad=rows, off=0, loss_mask_pad=ones)
    legs = {"sf_row_conf": lambda: ops.row_conf(x, conf_tok=conf, **addr),
            "sf_topk_rank": lambda: ops.topk_rank(x, kk=TOPK, row_hit=hit, tgt_ids_pad=tgt, **addr)}
    ms = {k: [] for k in legs}
    for i in range(3 + reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms[name].append(a.elapsed_time(b))
    ref = torch.softmax(x[:256].float(), -1).max(-1).values
    assert bool(((conf[:256] - ref).abs() <= 1e-5 * ref).all())      # the timed launch computed the confidences
    out = []
    for name in legs:
        med = sorted(ms[name])[len(ms[name]) // 2]
        nbytes = rows * 2 * V
        out.append(dict(leg="kernel", kernel=name, rows=rows, V=V, dtype="bf16", hip_event_ms=[round(t, 4) for t in ms[name]], median_ms=med,
                        spread_ms=max(ms[name]) - min(ms[name]), bytes_per_row_from_shapes=dict(logits_read=2 * V), bytes=nbytes,
                        tb_per_s=nbytes / med / 1e9, fraction_of_8_tb_per_s=nbytes / (med * 1e-3) / HBM_PEAK,
                        mean_conf=float(conf.mean())))
    return out


def step_lines(dev, config, B, S, steps):
    steps = steps * max(1, min(8, 16384 // (B * S)))
    cfg = dict(bench.CONFIGS[config][0])
    torch.manual_seed(0)
    model = LlamaForCausalLMEagle3(DraftConfig(**cfg), device=dev)
    t2d = torch.zeros(cfg["vocab_size"], dtype=torch.bool)
    ids = torch.randperm(cfg["vocab_size"], generator=torch.Generator().manual_seed(0))[:cfg["draft_vocab_size"]].sort().values
    t2d[ids] = True
    model.load_vocab_mapping_tensors(t2d, ids - torch.arange(cfg["draft_vocab_size"]))
    eagle = OnlineEagle3Model(model, length=7).train()
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

    def timed(on, n):
        eagle.conf_bins, eagle.conf_thresholds = (BINS, TAU) if on else (0, ())
        one()                   # (the views of the other setting were dropped: rebuilt outside the clock)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = one()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, out

    for on in (False, True):
        timed(on, 2)
    acc, last = {False: [], True: []}, {}
    for on in (False, True, True, False):
        ms, last[on] = timed(on, steps)
        acc[on].append(ms)
    m = last[True].metrics
    counts = dict(conf_denoms=[float(x) for x in m["conf_denoms"]], conf_bin_counts=[x.tolist() for x in m["conf_bin_counts"]],
                  conf_gate_drafted=[x.tolist() for x in m["conf_gate_drafted"]], conf_gate_accepted=[x.tolist() for x in m["conf_gate_accepted"]])
    return [dict(leg="train_step", config=config, batch=B, seq=S, ttt=7, conf_bins=BINS if on else 0, conf_thresholds=list(TAU) if on else [],
                 steps_per_sample=steps, ms_per_step=[round(t, 3) for t in x], mean_ms=sum(x) / len(x), same_leg_spread_ms=max(x) - min(x),
                 **(counts if on else {}))
            for on, x in acc.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-shapes", default="16384x32000,4096x32000", help="rows x V legs of the kernel comparison ('' for none)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="8x2048,1x2048", help="BxS legs of the training step ('' for none)")
    ap.add_argument("--config", default="llama3-8b")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conf_calibration_ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/conf_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = []
    for shape in filter(None, args.kernel_shapes.split(",")):
        rows, V = (int(v) for v in shape.split("x"))
        lines += kernel_lines(dev, rows, V, args.reps)
        torch.cuda.empty_cache()
    for shape in filter(None, args.shapes.split(",")):
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
