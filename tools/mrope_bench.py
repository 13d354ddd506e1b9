"""Multimodal RoPE: per-token cos / sin rows gathered from the table (the default) against angles computed on the device from the ids
(``Eagle3Engine.mrope_analytic``), inside the real optimizer step:

    python tools/mrope_bench.py [--steps 6] [--warmup 3] [--out profiles/mrope_analytic_ab.jsonl]      (GPU box)

Draft dims of the reference's ``configs/qwen2-5-vl-7b-eagle3.json`` (H 3584, I 18944, 28 / 4 heads of 128, mrope_section [16, 24, 24]),
ttt 7, at 1 x 4096 and 8 x 2048.  Per shape the legs run table, analytic, analytic, table: each leg is a fresh process under its own
time limit (the parent never opens the GPU), so the table leg is measured twice and the file carries its own run-to-run spread.  A leg
that fails ends the run: nothing more is started after it.  The three-axis ids are an image-like span (the axes differ) inside the
table, delivered as a CPU tensor, as a loader does.

One JSON line per leg: ms per optimizer step (host clock around a device synchronise, optimizer step included), the engine's arena
bytes, and the host time inside ``_position_rope`` per step (what the host spends queueing the gathers / the one copy; not device
time).  A last line per shape compares the means: analytic - table against the table legs' spread."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QWEN25_VL_7B = dict(hidden_size=3584, intermediate_size=18944, num_attention_heads=28, num_key_value_heads=4, vocab_size=152064,
                    draft_vocab_size=32000, head_dim=128, target_hidden_size=3584, max_position_embeddings=8192, rms_norm_eps=1e-6,
                    rope_theta=1000000.0, rope_scaling={"type": "mrope", "mrope_section": [16, 24, 24]})
SHAPES = [(1, 4096), (8, 2048)]
ORDER = ("table", "analytic", "analytic", "table")


def leg(args):
    import torch

    import bench
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead, TrainBatch
    from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    if not torch.cuda.is_available():
        raise SystemExit("tools/mrope_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    cfg, B, S = QWEN25_VL_7B, args.batch, args.seq
    torch.manual_seed(0)
    model = LlamaForCausalLMEagle3(DraftConfig(**cfg), device=dev)
    t2d = torch.zeros(cfg["vocab_size"], dtype=torch.bool)
    ids = torch.randperm(cfg["vocab_size"], generator=torch.Generator().manual_seed(0))[:cfg["draft_vocab_size"]].sort().values
    t2d[ids] = True
    model.load_vocab_mapping_tensors(t2d, ids - torch.arange(cfg["draft_vocab_size"]))
    eagle = OnlineEagle3Model(model, length=args.ttt, mrope_analytic=args.leg == "analytic").train()
    head = TargetHead((torch.randn(cfg["vocab_size"], cfg["target_hidden_size"], device=dev) * 0.02).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-4, max_grad_norm=0.5, total_steps=10_000_000, warmup_ratio=0.0))
    backend.prepare_model(eagle)
    tensors = bench.make_batch(cfg, B, S, dev, 100)
    s = torch.arange(S)
    axes = torch.stack([s, s // 2 + 3, (s * 3) % 61])                               # temporal / height / width, all inside the table
    tensors["position_ids"] = torch.stack([axes + b for b in range(B)], 1).contiguous()    # [3, B, S], host memory
    tb = TrainBatch(tensors, {"target_repr": "hidden_state"})
    eng = eagle.engine
    host = {"s": 0.0, "n": 0}
    inner = eng._position_rope

    def timed_position_rope(*a, **kw):
        t0 = time.perf_counter()
        r = inner(*a, **kw)
        host["s"] += time.perf_counter() - t0
        host["n"] += 1
        return r

    eng._position_rope = timed_position_rope

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = strat.forward_loss(tb)
            backend.backward(out.loss, is_boundary=True)
            backend.step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, float(out.loss.detach())

    run(args.warmup)
    host.update(s=0.0, n=0)
    ms, loss = run(args.steps)
    print(json.dumps(dict(leg=args.leg, config="qwen2.5-vl-7b draft dims", batch=B, seq=S, ttt=args.ttt, steps=args.steps, warmup=args.warmup,
                          ms_per_step=round(ms, 3), arena_bytes=eng.arena_bytes(), position_rope_host_ms_per_step=round(1e3 * host["s"] / host["n"], 4),
                          rope_table_rows=int(eng.cos.shape[0]), last_loss=loss)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("table", "analytic"), default=None, help="(internal) run one leg in this process")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--ttt", type=int, default=7)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrope_analytic_ab.jsonl"))
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    lines = []
    for B, S in SHAPES:
        got = {"table": [], "analytic": []}
        for name in ORDER:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--batch", str(B), "--seq", str(S), "--ttt", str(args.ttt),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"leg {name} {B} x {S} ran past {args.leg_timeout} s: stopping, nothing more is started")
            if r.returncode != 0:
                raise SystemExit(f"leg {name} {B} x {S} ended with status {r.returncode}: stopping, nothing more is started")
            ln = json.loads(r.stdout.strip().splitlines()[-1])
            got[name].append(ln)
            lines.append(ln)
            print(json.dumps(ln), flush=True)
        mean = {k: sum(x["ms_per_step"] for x in v) / len(v) for k, v in got.items()}
        spread = max(x["ms_per_step"] for x in got["table"]) - min(x["ms_per_step"] for x in got["table"])
        lines.append(dict(leg="summary", batch=B, seq=S, table_mean_ms=mean["table"], analytic_mean_ms=mean["analytic"],
                          analytic_minus_table_ms=mean["analytic"] - mean["table"], table_spread_ms=spread,
                          analytic_within_table_spread=mean["analytic"] - mean["table"] <= spread,
                          arena_bytes_table=got["table"][0]["arena_bytes"], arena_bytes_analytic=got["analytic"][0]["arena_bytes"]))
        print(json.dumps(lines[-1]), flush=True)
        with open(args.out, "w") as f:           # (after every shape: a later failure keeps what was measured)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
