"""GPU half of the ring tests (tests/test_usp_ring_gpu.py).  Run as a script it is one rank of a u x r SP world (ParallelConfig(sp_size=
u * r, sp_ring_size=r)) that exchanges over gloo (every rank on cuda:0, host-staged) or RCCL (rank x on cuda:x) and writes its results to
``--out``; the model, data and step are tests/_usp_gpu.py's."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _usp_gpu as W  # noqa: E402

# the head_dim-256 draft of the reference's configs/qwen3-next-80b-a3b-eagle3.json (16 / 2 heads; a 16000-entry draft vocabulary)
HD256 = dict(hidden_size=2048, intermediate_size=16384, num_attention_heads=16, num_key_value_heads=2, vocab_size=151936,
             draft_vocab_size=16000, head_dim=256, target_hidden_size=2048, max_position_embeddings=262144, rms_norm_eps=1e-6,
             rope_theta=10000000.0)


_BASE_DIMS = W.dims


def dims(name):
    return HD256 if name == "hd256" else _BASE_DIMS(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--ulysses", type=int, default=1)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--config", default="cfg1")
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as dist

    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    W.dims = dims
    world = a.ulysses * a.ring
    dev = torch.device("cuda", a.rank if a.backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group(a.backend, rank=a.rank, world_size=world)
    pc = ParallelConfig(world_size=world, sp_size=world, sp_ring_size=a.ring, dp_size=1)
    eagle, strat, backend, batch = W.setup(a.config, a.seq, dev, "usp", dict(parallel_config=pc))
    res = W.step(eagle, strat, backend, usp_shard(batch, ttt_length=W.T, sp_rank=a.rank, sp_size=world))
    if a.rank != 0:          # (every rank holds the same reduced gradient and weights: rank 0 writes them)
        res = dict(plosses=res["plosses"], acces=res["acces"])
    torch.save(res, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
