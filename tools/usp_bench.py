"""USP (attention_backend "usp") step and layout-kernel timing: one JSON line per run.

    python tools/usp_bench.py --sp 2 --seq 32768 [--ring R] [--config llama3-8b|cfg1|hd256] [--backend gloo|nccl] [--steps 3] [--warmup 1]
                              [--loss-mask-density D]

Starts ``--sp`` ranks (gloo: all on cuda:0, exchange staged through pinned host buffers -- a PLUMBING run, not a scaling number;
nccl: rank r on cuda:r), each training the Llama-3-8B draft dims on its shard of one 1 x seq sample.  Reports ms / step and
tokens / s (the whole sample per step), the exposed exchange time per step (a separate step with the engine synchronising around
every all-to-all), and on rank 0 the µs per launch of the layout kernels at this shape with the fraction of the 8 TB/s HBM peak
their bytes (one read + one write of the image) reach.

``--ring R`` (R divides --sp): ring attention inside the SP group (ParallelConfig(sp_size=sp, sp_ring_size=R), Ulysses degree sp / R).
The line then reports per rank the ms / step, the exposed exchange time split into the Ulysses all-to-alls and the ring all-gather /
reduce-scatter, and the query-offset attention kernels at that rank's shape (its u * chunk rows at offset ring_rank * u * chunk):
µs per launch and the fraction of the 2.5 PFLOP/s MFMA peak, FLOPs from shapes as in tools/attn_bench.py (fwd 4, dQ 6, dK/dV 8 x
nh/u * hd * (q_off * Sq + Sq^2 / 2)).  ``hd256``: the head_dim-256 draft of configs/qwen3-next-80b-a3b-eagle3.json (16 / 2 heads).

``--loss-mask-density D``: the sample's loss mask is bench.py's (``make_loss_mask``: all ones at 1.0, chat-like turns below) and stays in
host memory, so every rank hands its window counts (``eagle3.loss_mask_window_counts``) to the engine -- loss-row compaction and the
gathered teacher below the 0.9 cut-off.  Without it the mask is tests/_usp_gpu.py's (density 0.5, device-resident: no host counts, the
dense rows).  Every rank reports its peak allocation (``torch.cuda.max_memory_allocated``) over the run."""
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


def _time_attention(cfg, Sq, q_off, u, dev):
    """the query-offset attention kernels at one ring rank's shape (batch 1, nh / u and nkv / u heads, 6 diagonal branches)"""
    import math

    from specforge_amd import ops

    nh, nkv, hd = cfg["num_attention_heads"] // u, cfg["num_key_value_heads"] // u, cfg["head_dim"]
    SK, nd, scale = q_off + Sq, T - 1, 1.0 / math.sqrt(hd)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g).to(torch.bfloat16)
    q, do = rnd(Sq, nh * hd), rnd(Sq, nh * hd)
    kv0 = rnd(SK, 2 * nkv * hd)
    kvd = [rnd(Sq, 2 * nkv * hd) for _ in range(nd)]
    w = nkv * hd
    o, dq = torch.empty_like(q), torch.empty_like(q)
    lse, delta = torch.empty(1, nh, Sq, device=dev), torch.zeros(1, nh, Sq, device=dev)
    dkv = torch.zeros(SK, 2 * w, device=dev)
    ws = torch.empty(max(1, ops.attn_bwd_dkv_off_workspace_floats(1, Sq, q_off, nh, nkv, hd)), device=dev)
    kvlen = torch.tensor([SK], dtype=torch.int32, device=dev)
    geo = dict(B=1, S=Sq, q_off=q_off, nh=nh, nkv=nkv, hd=hd, scale=scale)
    fwd = lambda: ops.attn_fwd_off(q, kv0[:, :w], kv0[:, w:], [t[:, :w] for t in kvd], [t[:, w:] for t in kvd], kvlen, o, lse, **geo)
    fwd()
    launches = {"attn_fwd_off": (fwd, 4), "attn_bwd_dq_off": (lambda: ops.attn_bwd_dq_off(q, do, kv0[:, :w], kv0[:, w:], kvlen, lse, delta,
                                                                                          None, dq, **geo), 6),
                "attn_bwd_dkv_off": (lambda: ops.attn_bwd_dkv_off(q, do, kv0[:, :w], kv0[:, w:], kvlen, lse, delta, dkv[:, :w], dkv[:, w:],
                                                                  workspace=ws, **geo), 8)}
    pairs = nh * hd * (q_off * Sq + Sq * Sq / 2)
    out = {}
    for name, (fn, f) in launches.items():
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        tf = f * pairs / (us * 1e-6) / 1e12
        out[name] = dict(us=round(us, 1), tflops=round(tf, 1), frac_mfma_peak=round(tf / 2500.0, 3))
    return out


def _rank(a):
    import torch.distributed as dist

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _usp_gpu as W
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    import _usp_ring_gpu as R

    W.dims = R.dims
    dev = torch.device("cuda", a.rank if a.backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group(a.backend, rank=a.rank, world_size=a.sp)
    pc = ParallelConfig(world_size=a.sp, sp_size=a.sp, sp_ring_size=a.ring, dp_size=1)
    eagle, strat, backend, batch = W.setup(a.config, a.seq, dev, "usp", dict(parallel_config=pc))
    if a.loss_mask_density is not None:
        from bench import make_loss_mask

        batch["loss_mask"] = make_loss_mask(1, a.seq, a.loss_mask_density, seed=5)     # host memory: the strategy takes the counts from it
        batch["loss_mask"][0, -1] = 0
    shard = usp_shard(batch, ttt_length=T, sp_rank=a.rank, sp_size=a.sp)
    for _ in range(a.warmup):
        W.step(eagle, strat, backend, shard)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        W.step(eagle, strat, backend, shard)
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    eng = eagle.engine
    eng.sp_time_exchange, eng.sp_exchange_s, eng.sp_ring_exchange_s = True, 0.0, 0.0
    W.step(eagle, strat, backend, shard)
    res = dict(ms_per_step=ms, exchange_ms_per_step=(eng.sp_exchange_s + eng.sp_ring_exchange_s) * 1e3,
               peak_mem_gb=torch.cuda.max_memory_allocated(dev) / 1e9, teacher_compacted=eng._teacher_compacted, soft_targets=eng._soft[0],
               lm_head_rows_compact=eng._lm_compact_K is not None)
    u = a.sp // a.ring
    if a.ring > 1:
        chunk = a.seq // a.sp
        res.update(ulysses_exchange_ms_per_step=eng.sp_exchange_s * 1e3, ring_exchange_ms_per_step=eng.sp_ring_exchange_s * 1e3,
                   ring_rank=eng.ring_rank, q_off=eng.ring_rank * u * chunk)
        for x in range(a.sp):       # one rank at a time: under gloo every rank shares the device
            if x == a.rank:
                res["attention"] = _time_attention(W.dims(a.config), u * chunk, eng.ring_rank * u * chunk, u, dev)
            dist.barrier()
    if a.rank == 0 and u > 1:
        res["kernels"] = _time_kernels(W.dims(a.config), a.seq // a.sp, u, dev)
    torch.save(res, a.out)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sp", type=int, default=2)
    ap.add_argument("--seq", type=int, default=32768)
    ap.add_argument("--ring", type=int, default=1)
    ap.add_argument("--config", default="llama3-8b", choices=["llama3-8b", "cfg1", "hd256"])
    ap.add_argument("--backend", default="gloo", choices=["gloo", "nccl"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loss-mask-density", type=float, default=None)
    ap.add_argument("--timeout", type=int, default=1200)
    ap.add_argument("--rank", type=int, default=None)
    ap.add_argument("--port", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rank is not None:
        return _rank(a)
    if a.seq % a.sp:
        raise SystemExit("--seq must be a multiple of --sp")
    if a.ring < 1 or a.sp % a.ring:
        raise SystemExit("--ring must divide --sp")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    outs = [f"/tmp/usp_bench_{os.getpid()}_{r}.pt" for r in range(a.sp)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), "--port", str(port), "--sp", str(a.sp),
                               "--seq", str(a.seq), "--ring", str(a.ring), "--config", a.config, "--backend", a.backend, "--steps", str(a.steps),
                               "--warmup", str(a.warmup), "--out", outs[r]]
                              + ([] if a.loss_mask_density is None else ["--loss-mask-density", str(a.loss_mask_density)]), cwd=ROOT)
             for r in range(a.sp)]
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
                exposed_exchange_ms_per_step=round(max(r["exchange_ms_per_step"] for r in res), 2),
                layout_kernels=res[0].get("kernels"), loss_mask_density=a.loss_mask_density,
                per_rank=[dict(rank=x, ms_per_step=round(r["ms_per_step"], 2), peak_mem_gb=round(r["peak_mem_gb"], 3),
                               teacher_compacted=r["teacher_compacted"], soft_targets=r["soft_targets"],
                               lm_head_rows_compact=r["lm_head_rows_compact"]) for x, r in enumerate(res)])
    if a.ring > 1:
        line.update(ulysses=a.sp // a.ring, ring=a.ring, ranks=[
            dict(rank=x, ring_rank=r["ring_rank"], q_off=r["q_off"], ms_per_step=round(r["ms_per_step"], 2),
                 ulysses_exchange_ms_per_step=round(r["ulysses_exchange_ms_per_step"], 2),
                 ring_exchange_ms_per_step=round(r["ring_exchange_ms_per_step"], 2), attention=r["attention"]) for x, r in enumerate(res)])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
