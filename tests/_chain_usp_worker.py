"""One step of a tiny draft with the joint chain counts on (tests/test_chain_usp.py), the same model and sample in every process
(those of tests/_topk_usp_worker.py): as a module, the step the pytest process runs unsharded; as a script, one SP rank of a two-rank
world that exchanges over gloo -- under the SIMT interpreter (``--emu LIB``, CPU tensors) or on cuda:0 (both ranks share the device,
host-staged exchanges) -- and writes its counts to ``--out``."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _topk_usp_worker as W  # noqa: E402

T, S = W.T, W.S
# the worker's draft is random and half the target ids have no draft index: only wide channels keep chains alive past depth 0
TOPK = (1, 64, 96, 128)


def setup(dev, attention_backend="hip", backend_kw=None, lk=None):
    eagle, strat, backend = W.setup(dev, attention_backend, backend_kw, lk=lk)
    eagle.topk, eagle.chain = TOPK, True
    return eagle, strat, backend


sample = W.sample


def step(eagle, strat, backend, tensors):
    from specforge_amd.eagle3 import TrainBatch

    out = strat.forward_loss(TrainBatch(dict(tensors), {"target_repr": "hidden_state"}))
    backend.backward(out.loss, is_boundary=True)
    m = out.metrics
    den, cor = eagle.last_chain
    return dict(denoms=torch.stack([t.float().cpu() for t in den]), corrects=torch.stack([t.float().cpu() for t in cor]),
                topk=torch.stack([t.float().cpu() for t in eagle.last_topk]), acc_corrects=torch.stack(m["acc_corrects"]).float().cpu(),
                acc_denoms=torch.stack(m["acc_denoms"]).float().cpu(), named_denoms=torch.stack(m["chain_denoms"]).float().cpu(),
                named={k: torch.stack(m[f"chain_top{k}_corrects"]).float().cpu() for k in TOPK})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--emu", default="")
    ap.add_argument("--lk", default="")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as dist

    from specforge_amd import _lib
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    if a.emu:
        torch.set_num_threads(1)
        os.environ["SFEMU_THREADS"] = "2"
        _lib._inject_library_for_tests(a.emu)
        dev = torch.device("cpu")
    else:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group("gloo", rank=a.rank, world_size=2)
    eagle, strat, backend = setup(dev, "usp", dict(parallel_config=ParallelConfig(world_size=2, sp_size=2, dp_size=1)), lk=a.lk or None)
    full = sample(dev)
    full.pop("attention_mask")
    res = step(eagle, strat, backend, usp_shard(full, ttt_length=T, sp_rank=a.rank, sp_size=2))
    if not a.emu:
        torch.cuda.synchronize()
    torch.save(res, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
