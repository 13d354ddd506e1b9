"""Ring attention inside USP (``ParallelConfig(sp_size=u * r, sp_ring_size=r)``) on the HIP path, on CPU: the mesh layout of the
reference (distributed.py:133-195 + yunchang's set_seq_parallel_pg: Ulysses peers consecutive, sp_rank = ring_rank * u + ulysses_rank),
the shards against the reference's ``process_data_usp(..., ring_rank, sp_ring_size)``, and one micro-step of u x r gloo processes (the
engine code the GPU ranks run, kernels under the SIMT interpreter) against the unsharded step.  Modelled on tests/test_usp.py."""
import os
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_usp import S, T, _cfg, _compare, _free_port, _model, _normalised, _one_step, _raw, _sample, _single


# ------------------------------------------------------------------------------------------------------------------ the mesh
@pytest.mark.parametrize("world,sp,r", [(4, 4, 2), (8, 4, 2), (4, 4, 4), (8, 2, 2), (6, 6, 3)])
def test_usp_groups_layout(monkeypatch, world, sp, r):
    """every rank creates the same groups in the same order; Ulysses peers are consecutive, ring peers u apart, and the rank inside the
    SP group is ring_rank * u + ulysses_rank"""
    from specforge_amd import training

    u = sp // r
    created = {}
    for rank in range(world):
        calls = []
        fake = types.SimpleNamespace(get_world_size=lambda g=None: world, get_rank=lambda g=None, rank=rank: rank,
                                     new_group=lambda ranks, calls=calls: calls.append(tuple(ranks)) or tuple(ranks))
        monkeypatch.setattr(training, "dist", fake)
        spg, ug, rg, dpg = training.make_usp_groups(sp, r)
        created[rank] = calls
        base, sp_rank = rank - rank % sp, rank % sp
        ring_rank, uly_rank = sp_rank // u, sp_rank % u
        assert spg == tuple(range(base, base + sp))
        assert dpg == tuple(range(rank % sp, world, sp))
        assert ug == (tuple(base + ring_rank * u + j for j in range(u)) if u > 1 else None)
        assert rg == tuple(base + t * u + uly_rank for t in range(r))
        assert rg.index(rank) == ring_rank and (ug is None or ug.index(rank) == uly_rank)
    assert all(created[x] == created[0] for x in created)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="sp_ring_size"):
        training.make_usp_groups(4, 3)


@pytest.mark.parametrize("S_,u,r,ttt", [(32, 1, 2, 7), (31, 2, 2, 1), (9, 1, 4, 7), (40, 2, 2, 3)])
def test_shards_equal_reference_process_data_usp_ring(S_, u, r, ttt):
    """usp_shard(sp_rank = ring_rank * u + ulysses_rank, sp_size = u * r) is the reference's ring shard (positions included)"""
    from oracle import ref_harness

    if not ref_harness.available():
        pytest.skip("reference checkout not present")
    ref_harness.setup()
    from specforge.data.preprocessing import OfflineEagle3Dataset

    from specforge_amd.ingest import usp_shard

    sp = u * r
    raw = _raw(S_, 5 * S_ + sp)
    ref_in = dict(input_ids=raw["input_ids"][0], loss_mask=raw["loss_mask"][0], hidden_state=raw["hidden_state"],
                  aux_hidden_state=raw["aux_hidden_state"])
    for sp_rank in range(sp):
        ref = OfflineEagle3Dataset.process_data_usp(ref_in, max_len=S_, ttt_length=ttt, sp_rank=sp_rank, sp_size=sp,
                                                    ring_rank=sp_rank // u, sp_ring_size=r)
        ours = usp_shard(_normalised(raw), ttt_length=ttt, sp_rank=sp_rank, sp_size=sp)
        assert set(ref) == set(ours)
        for k in ref:
            assert torch.equal(ref[k], ours[k]), (k, sp_rank)


# ------------------------------------------------------------------------------------------------------------------ the step
def _trainer(lk, backend_kw, cfg, attention_backend="usp"):
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    eagle = OnlineEagle3Model(_model(cfg), length=T, attention_backend=attention_backend, lk_loss_type=lk).train()
    head = TargetHead(0.05 * torch.randn(cfg.vocab_size, 128, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-2, total_steps=100, warmup_ratio=0.0),
                                   **backend_kw)
    backend.prepare_model(eagle)
    return eagle, strat, backend


def _worker(rank, world, sp, r, port, emu_path, lk, nkv, out_dir, seeds):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    os.environ["SFEMU_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from specforge_amd import _lib
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    _lib._inject_library_for_tests(emu_path)
    pc = ParallelConfig(world_size=world, sp_size=sp, sp_ring_size=r, dp_size=world // sp)
    eagle, strat, backend = _trainer(lk, dict(parallel_config=pc), _cfg(nkv=nkv))
    eng = eagle.engine
    assert (eng.u, eng.ring, eng.sp) == (sp // r, r, sp) and eng.ring_rank == (rank % sp) // (sp // r)
    dp_rank, sp_rank = rank // sp, rank % sp
    res = _one_step(strat, backend, eagle, {**usp_shard(_sample(seeds[dp_rank]), ttt_length=T, sp_rank=sp_rank, sp_size=sp)})
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _single_nkv(emu_path, lk, seeds, nkv):
    """the unsharded step of a config with ``nkv`` kv heads (test_usp._single builds nkv 2)"""
    import test_usp

    real = test_usp._cfg
    test_usp._cfg = lambda nkv_=nkv, rope_scaling=None: real(nkv=nkv_, rope_scaling=rope_scaling)
    try:
        return _single(emu_path, lk, seeds)
    finally:
        test_usp._cfg = real


# Bars: about twice the difference measured on the interpreter build (recorded beside each).  The sides differ as in test_usp.py: the
# summation order of the attention (a rank's keys 0 .. own rows vs all S keys) and where the gradient sums are rounded to bf16 (per
# rank and ring block vs the whole sample); the ring adds the fp32 sum of dK0 / dV0 over the ring ranks before that rounding.
# (params: the weights whose gradient clearly exceeds the gradient difference, see test_usp._compare)
BARS = {
    "u1r2": dict(loss=2.5e-7, acc=0.0, grad=1.3e-2, params=3e-5),          # measured: loss 1.2e-7, acc 0, grad 6.5e-3, params 1.5e-5
    "u1r2-lambda": dict(loss=2.5e-7, acc=0.0, grad=8.5e-3, params=3e-5),   # measured: loss 1.2e-7, acc 0, grad 4.2e-3, params 1.5e-5
    "u2r2": dict(loss=5e-7, acc=0.0, grad=6.5e-3, params=3e-5),            # measured: loss 2.4e-7, acc 0, grad 3.2e-3, params 1.5e-5
    "u1r4": dict(loss=5e-7, acc=0.0, grad=6.5e-3, params=3e-5),            # measured: loss 2.4e-7, acc 0, grad 3.2e-3, params 1.5e-5
    "u1r4-lambda": dict(loss=2.5e-7, acc=0.0, grad=8.5e-3, params=3e-5),   # measured: loss 1.2e-7, acc 0, grad 4.2e-3, params 1.5e-5
    "u1r2-nkv1": dict(loss=2.5e-7, acc=0.0, grad=1.2e-2, params=3e-5),     # measured: loss 1.2e-7, acc 0, grad 6.0e-3, params 1.5e-5
}


@pytest.mark.parametrize("sp,r,lk,nkv,key", [
    (2, 2, None, 2, "u1r2"),
    (2, 2, "lambda", 2, "u1r2-lambda"),
    (4, 2, None, 2, "u2r2"),
    (4, 4, None, 2, "u1r4"),
    (4, 4, "lambda", 2, "u1r4-lambda"),
    (2, 2, None, 1, "u1r2-nkv1"),         # one kv head: Ulysses cannot split it, a pure ring can
], ids=lambda v: v if isinstance(v, str) else None)
def test_ring_step_matches_unsharded_step(emu_lib_path, tmp_path, sp, r, lk, nkv, key):
    seeds = [11]
    mp.spawn(_worker, args=(sp, sp, r, _free_port(), emu_lib_path, lk, nkv, str(tmp_path), seeds), nprocs=sp, join=True)
    _compare(tmp_path, sp, sp, _single_nkv(emu_lib_path, lk, seeds, nkv), seeds, BARS[key])


def test_ring_runs_are_bit_identical(emu_lib_path, tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / str(i)
        d.mkdir()
        mp.spawn(_worker, args=(2, 2, 2, _free_port(), emu_lib_path, None, 2, str(d), [11]), nprocs=2, join=True)
        runs.append([torch.load(d / f"rank{x}.pt") for x in range(2)])
    for a, b in zip(*runs):
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_ring_refusals():
    from specforge_amd.engine import Eagle3Engine
    from specforge_amd.reference_plugin import check_training_topology
    from specforge_amd.training import ParallelConfig

    with pytest.raises(ValueError, match="sp_ring_size.*sp_size"):
        ParallelConfig(sp_size=4, sp_ring_size=3)
    assert ParallelConfig(sp_size=4, sp_ring_size=2).sp_ulysses_size == 2
    assert ParallelConfig(sp_size=4).sp_ulysses_size == 4 and ParallelConfig(sp_size=4).sp_ring_size == 1

    import specforge_amd.engine as E

    class _G:          # process group stand-ins: the checks read sizes and ranks only
        def __init__(self, n):
            self.n = n

    real = (E.dist.get_world_size, E.dist.get_rank, E.dist.get_backend)
    E.dist.get_world_size, E.dist.get_rank, E.dist.get_backend = (lambda g=None: g.n), (lambda g=None: 0), (lambda g=None: "gloo")
    try:
        with pytest.raises(ValueError, match="num_key_value_heads"):       # u = 2 cannot split one kv head ...
            Eagle3Engine(_model(_cfg(nkv=1)), ttt_length=T, sp_group=_G(4), sp_ulysses_group=_G(2), sp_ring_group=_G(2))
        eng = Eagle3Engine(_model(_cfg(nkv=1)), ttt_length=T, sp_group=_G(2), sp_ring_group=_G(2))   # ... a pure ring can
        assert (eng.u, eng.ring, eng.sp) == (1, 2, 2)
        with pytest.raises(ValueError, match="sp_ring_group"):               # the subgroups must split the SP group
            Eagle3Engine(_model(_cfg()), ttt_length=T, sp_group=_G(4), sp_ulysses_group=_G(1), sp_ring_group=_G(2))
    finally:
        E.dist.get_world_size, E.dist.get_rank, E.dist.get_backend = real
    # the plugin does not wire SP: the ring refusal stays first and names the key
    t = types.SimpleNamespace(sp_ring_size=2, tp_size=1, attention_backend="usp", batch_size=1)
    with pytest.raises(ValueError, match="sp_ring_size") as ei:
        check_training_topology(t)
    assert "Python API" in str(ei.value)
