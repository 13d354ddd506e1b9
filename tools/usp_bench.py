"""USP (attention_backend "usp") step and layout-kernel timing: one JSON line per run.

    python tools/usp_bench.py --sp 2 --seq 32768 [--config llama3-8b] [--backend gloo|nccl] [--steps 3] [--warmup 1]

Starts ``--sp`` ranks (gloo: all on cuda:0, exchange staged through pinned host buffers -- a PLUMBING run, not a scaling number;
nccl: rank r on cuda:r), each training the Llama-3-8B draft dims on its shard of one 1 x seq sample.  Reports ms / step and
tokens / s (the whole sample per step), the exposed exchange time per step (a separate step with the engine synchronising around
every all-to-all), and on rank 0 the µs per launch of the layout kernels at this shape with the fraction of the 8 TB/s HBM peak
their bytes (one read + one write of the image) reach."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
T = 7


def _time_kernels(cfg, chunk, sp, dev):
    from specforge_amd import ops
    from specforge_amd.model import DraftConfig, rope_tables

    nh, nkv, hd = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    W = (nh + 2 * nkv) * hd
    c = DraftConfig(**dict(cfg, max_position_embeddings=chunk * sp + T))
    cos, sin = (t.to(dev) for t in rope_tables(c, torch.bfloat16))
    tok = torch.randn(chunk, W, device=dev).to(torch.bfloat16)
    sh = torch.empty(sp * chunk, W // sp, device=dev, dtype=torch.bfloat16)
    o_tok = torch.randn(chunk, nh * hd, device=dev).to(torch.bfloat16)
    o_sh = torch.empty(sp * chunk, nh * hd // sp, device=dev, dtype=torch.bfloat16)
    pos = torch.arange(chunk, device=dev)
    kw = dict(sp=sp, nh=nh, nkv=nkv, hd=hd, cos_t=cos, sin_t=sin, pos_ids=pos, pos_off=3)
    launches = {"pack_qkv": (lambda: ops.ulysses_pack_qkv(tok, sh, **kw), tok.numel()),
                "unpack_qkv_bwd": (lambda: ops.ulysses_pack_qkv(sh, tok, backward=True, **kw), tok.numel()),
                "pack_o": (lambda: ops.ulysses_pack_o(o_tok, o_sh, sp=sp), o_tok.numel()),
                "unpack_o": (lambda: ops.ulysses_unpack_o(o_sh, o_tok, sp=sp), o_tok.numel())}
    out = {}
    for name, (fn, n) in launches.items():
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        gbs = 2 * n * 2 / (us * 1e-6) / 1e9
        out[name] = dict(us=round(us, 2), gb_s=round(gbs, 1), frac_hbm_peak=round(gbs / HBM_PEAK_GBS, 3))
    return out


def _rank(a):
    import torch.distributed as dist

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _usp_gpu as W
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    dev = torch.device("cuda", a.rank if a.backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group(a.backend, rank=a.rank, world_size=a.sp)
    eagle, strat, backend, batch = W.setup(a.config, a.seq, dev, "usp",
                                           dict(parallel_config=ParallelConfig(world_size=a.sp, sp_size=a.sp, dp_size=1)))
    shard = usp_shard(batch, ttt_length=T, sp_rank=a.rank, sp_size=a.sp)
    for _ in range(a.warmup):
        W.step(eagle, strat, backend, shard)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        W.step(eagle, strat, backend, shard)
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    eng = eagle.engine
    eng.sp_time_exchange, eng.sp_exchange_s = True, 0.0
    W.step(eagle, strat, backend, shard)
    res = dict(ms_per_step=ms, exchange_ms_per_step=eng.sp_exchange_s * 1e3)
    if a.rank == 0:
        res["kernels"] = _time_kernels(W.dims(a.config), a.seq // a.sp, a.sp, dev)
    torch.save(res, a.out)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sp", type=int, default=2)
    ap.add_argument("--seq", type=int, default=32768)
    ap.add_argument("--config", default="llama3-8b", choices=["llama3-8b", "cfg1"])
    ap.add_argument("--backend", default="gloo", choices=["gloo", "nccl"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=1200)
    ap.add_argument("--rank", type=int, default=None)
    ap.add_argument("--port", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rank is not None:
        return _rank(a)
    if a.seq % a.sp:
        raise SystemExit("--seq must be a multiple of --sp")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    outs = [f"/tmp/usp_bench_{os.getpid()}_{r}.pt" for r in range(a.sp)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), "--port", str(port), "--sp", str(a.sp),
                               "--seq", str(a.seq), "--config", a.config, "--backend", a.backend, "--steps", str(a.steps),
                               "--warmup", str(a.warmup), "--out", outs[r]], cwd=ROOT) for r in range(a.sp)]
    try:
        rcs = [p.wait(timeout=a.timeout) for p in procs]
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        raise SystemExit("usp_bench: a rank did not finish in time")
    if any(rcs):
        raise SystemExit(f"usp_bench: rank exit codes {rcs}")
    res = [torch.load(o) for o in outs]
    for o in outs:
        os.remove(o)
    ms = max(r["ms_per_step"] for r in res)
    line = dict(metric="USP EAGLE3 draft step", config=a.config, sp=a.sp, seq=a.seq, backend=a.backend,
                devices=1 if a.backend == "gloo" else a.sp,
                kind="plumbing (ranks share one device, host-staged gloo exchange)" if a.backend == "gloo" else "rccl",
                steps=a.steps, ms_per_step=round(ms, 2), tokens_per_s=round(a.seq / ms * 1e3, 1),
                exposed_exchange_ms_per_step=round(max(r["exchange_ms_per_step"] for r in res), 2), layout_kernels=res[0]["kernels"])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
