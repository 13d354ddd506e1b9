"""GPU half of tests/test_usp_reduced_teacher_gpu.py.  Run as a script it is one rank of a u x r SP world (gloo: every rank on cuda:0,
host-staged exchange) that trains one step of tests/_usp_gpu.py's model and sample with the loss mask kept in HOST memory (so the
strategy hands the engine its window counts) three times, each from a fresh model: ``compact`` (the default: reduced teacher over
the gathered positions, lm_head / CE on the rows with a loss), ``reduced`` (compact_loss_rows = False: the reduced teacher over all
chunk + T rows) and ``dense`` (compact_loss_rows = False, materialise_soft_targets = True: the [rows, Vt] teacher scratch and the fp32
target_p).  Per mode: the losses, accuracies, the engine's forms and the step's peak allocation above what was allocated before it."""
import argparse
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _usp_gpu as W  # noqa: E402
import _usp_ring_gpu as R  # noqa: E402

MODES = ("compact", "reduced", "dense")


def run_mode(mode, config, seq, dev, attention_backend="hip", backend_kw=None, shard=None):
    """one training step in ``mode`` -> results; ``shard(batch)`` cuts this rank's USP shard (None: the unsharded step)"""
    real, W.dims = W.dims, R.dims
    try:
        eagle, strat, backend, batch = W.setup(config, seq, dev, attention_backend, backend_kw)
    finally:
        W.dims = real
    batch["loss_mask"] = batch["loss_mask"].cpu()          # host memory: per-step row counts without a device read-back
    eng = eagle.engine
    if mode != "compact":
        eng.compact_loss_rows = False
    eng.materialise_soft_targets = mode == "dense"
    tensors = shard(batch) if shard is not None else batch
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    res = W.step(eagle, strat, backend, tensors)
    res.update(peak_delta=torch.cuda.max_memory_allocated(dev) - base, compacted=eng._teacher_compacted, soft=eng._soft[0],
               lm_compact=eng._lm_compact_K is not None)
    del eagle, strat, backend, batch, eng, tensors
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--ulysses", type=int, default=2)
    ap.add_argument("--ring", type=int, default=1)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--config", default="llama3-8b")
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as dist

    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    world = a.ulysses * a.ring
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group("gloo", rank=a.rank, world_size=world)
    out = {}
    for mode in MODES:
        pc = ParallelConfig(world_size=world, sp_size=world, sp_ring_size=a.ring, dp_size=1)
        res = run_mode(mode, a.config, a.seq, dev, "usp", dict(parallel_config=pc),
                       shard=lambda b: usp_shard(b, ttt_length=W.T, sp_rank=a.rank, sp_size=world))
        if a.rank != 0 or mode != "compact":     # (every rank holds the same reduced gradient: rank 0 writes the one compared)
            res.pop("grad")
            res.pop("params")
        out[mode] = res
    torch.save(out, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
