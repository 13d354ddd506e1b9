"""Helpers of tests/test_lk_reduced_teacher_usp.py (spawned gloo ranks import this module by name): the model, sample and step of
tests/test_usp_reduced_teacher.py with an LK objective and a half-dense turn mask."""
import os

import torch
import torch.distributed as dist

from test_usp_reduced_teacher import HT, T, VT, _cfg, _model

CHUNK = 512             # rows per rank: half of them with a loss -> >= 192 gathered teacher rows (the reduced head GEMM's floor)


def half_mask(S_):
    """a chat-like loss mask of density 0.5: 32-token prompts (no loss) between 32-token answers; every shard boundary (multiples of
    512, shifted by 16) falls inside an answer, so the overlap rows carry a loss"""
    p = torch.arange(S_)
    lm = (((p + 48) % 64) >= 32).long()[None]
    lm[0, -1] = 0
    return lm


def sample(S_, seed=11):
    g = torch.Generator().manual_seed(seed)
    return dict(input_ids=torch.randint(0, VT, (1, S_), generator=g), loss_mask=half_mask(S_),
                hidden_state=torch.randn(1, S_, 3 * HT, generator=g).to(torch.bfloat16),
                target=torch.randn(1, S_, HT, generator=g).to(torch.bfloat16))


def trainer(lk, backend_kw, attention_backend="hip"):
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    eagle = OnlineEagle3Model(_model(_cfg()), length=T, attention_backend=attention_backend, lk_loss_type=lk).train()
    head = TargetHead((0.2 * torch.randn(VT, HT, generator=torch.Generator().manual_seed(9))).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-2, total_steps=100, warmup_ratio=0.0), **backend_kw)
    backend.prepare_model(eagle)
    return eagle, strat, backend


def step(strat, backend, eagle, tensors):
    """one optimizer step -> the fields tests/test_usp.py::_compare reads, plus the path flags of the forward"""
    from specforge_amd.eagle3 import TrainBatch

    out = strat.forward_loss(TrainBatch(dict(tensors), {"target_repr": "hidden_state"}))
    eng = eagle.engine
    state = dict(soft=eng._soft[0], compacted=eng._teacher_compacted, lm_compact=eng._lm_compact_K is not None, names=eng.arena_names())
    backend.backward(out.loss, is_boundary=True)
    backend.synchronize_gradients()
    g = eng.flat.grad.float().clone()
    backend.step()
    m = out.metrics
    return dict(state, plosses=torch.stack(m["plosses"]).float(), acces=torch.stack(m["acces"]).float(),
                acceptance_rates=torch.stack(m["acceptance_rates"]).float(), acc_corrects=torch.stack(m["acc_corrects"]).float(), grad=g,
                params=eng.flat.data.clone())


def worker(rank, sp, ring, S_, port, emu_path, lk, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    os.environ["SFEMU_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=sp)
    from specforge_amd import _lib
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    _lib._inject_library_for_tests(emu_path)
    eagle, strat, backend = trainer(lk, dict(parallel_config=ParallelConfig(world_size=sp, sp_size=sp, sp_ring_size=ring, dp_size=1)),
                                    attention_backend="usp")
    res = step(strat, backend, eagle, usp_shard(sample(S_), ttt_length=T, sp_rank=rank, sp_size=sp))
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def single(emu_path, lk, S_):
    """the unsharded step in this process"""
    from specforge_amd import _lib

    _lib._inject_library_for_tests(emu_path)
    try:
        eagle, strat, backend = trainer(lk, {})
        t = sample(S_)
        t["attention_mask"] = torch.ones(1, S_, dtype=torch.long)
        return step(strat, backend, eagle, t)
    finally:
        _lib._inject_library_for_tests(None)
