"""GPU half of tests/test_ingest_usp_ranged_gpu.py.  Run as a script it is one rank of a 2-rank gloo SP world on cuda:0: the same cfg-1
step (tests/_usp_gpu.py's model, head and optimizer) fed once by the ranged USP ingest and once, from a fresh model, by a full read of
the sample staged to the device and sharded there (``usp_shard``); both results go to ``--out``."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--file", required=True)
    ap.add_argument("--seq", type=int, required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as dist

    import _usp_gpu as W
    from specforge_amd.ingest import HiddenStateIngest, usp_shard
    from specforge_amd.training import ParallelConfig

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group("gloo", rank=a.rank, world_size=2)
    res = {}
    for kind in ("ranged", "full"):
        eagle, strat, backend, _ = W.setup("cfg1", a.seq, dev, "usp", dict(parallel_config=ParallelConfig(world_size=2, sp_size=2, dp_size=1)))
        if kind == "ranged":
            ing = HiddenStateIngest([a.file], batch_size=1, max_len=a.seq, device=dev, shuffle=False, sp_rank=a.rank, sp_size=2,
                                    ttt_length=W.T)
            b = next(iter(ing.epoch(0))).tensors
        else:
            ing = HiddenStateIngest([a.file], batch_size=1, max_len=a.seq, device=dev, shuffle=False)
            b = usp_shard(next(iter(ing.epoch(0))).tensors, ttt_length=W.T, sp_rank=a.rank, sp_size=2)
        b = {k: v.clone() for k, v in b.items()}
        torch.cuda.synchronize()
        res[kind] = W.step(eagle, strat, backend, b)
        del eagle, strat, backend, ing
        torch.cuda.empty_cache()
    torch.save(res, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
