"""Ulysses sequence parallelism (attention_backend "usp") on the HIP path, on CPU: the shard layout of the reference's
``process_data_usp`` (data/preprocessing.py:446-521), the refusals, and the equivalence the USP design rests on -- with
S % sp == 0, one USP micro-step averaged over the SP ranks is the unsharded micro-step (each rank's loss is a mean over its
chunk, the chunks are equal).  Two gloo processes drive the same engine code the GPU ranks run; kernels under the SIMT
interpreter."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T = 3
S = 32


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _raw(S_, seed, Ht=16):
    g = torch.Generator().manual_seed(seed)
    return dict(input_ids=torch.randint(0, 100, (1, S_), generator=g), loss_mask=(torch.rand(1, S_, generator=g) > 0.3).long(),
                hidden_state=torch.randn(1, S_, Ht, generator=g), aux_hidden_state=torch.randn(1, S_, 3 * Ht, generator=g))


def _normalised(raw):
    lm = raw["loss_mask"].clone()
    lm[0, -1] = 0
    return dict(input_ids=raw["input_ids"], loss_mask=lm, target=raw["hidden_state"], hidden_state=raw["aux_hidden_state"])


# ------------------------------------------------------------------------------------------------------------------ sharding
@pytest.mark.parametrize("S_,sp,ttt", [(32, 2, 7), (31, 4, 1), (9, 4, 7), (5, 4, 1), (17, 2, 3)])
def test_shards_reassemble_the_sample(S_, sp, ttt):
    from specforge_amd.ingest import usp_shard

    s = _normalised(_raw(S_, S_ + sp))
    chunk = -(-S_ // sp)
    parts = [usp_shard(s, ttt_length=ttt, sp_rank=r, sp_size=sp) for r in range(sp)]
    for k in ("input_ids", "loss_mask", "target", "hidden_state"):
        whole = torch.cat([p[k][:, :chunk] for p in parts], dim=1)
        assert torch.equal(whole[:, :S_], s[k])
        assert not whole[:, S_:].any()                                  # the last shard's tail is zero padding
        for r, p in enumerate(parts):                                   # the overlap is the next shard's head
            assert p[k].shape[1] == chunk + ttt
            nxt = torch.cat([s[k], s[k].new_zeros((1, chunk * sp + ttt) + tuple(s[k].shape[2:]))], dim=1)
            assert torch.equal(p[k], nxt[:, r * chunk:r * chunk + chunk + ttt])
    assert torch.equal(torch.cat([p["position_ids"] for p in parts], dim=1), torch.arange(chunk * sp)[None])
    assert sum(int(p["attention_mask"][:, :chunk].sum()) for p in parts) == S_


@pytest.mark.parametrize("S_,sp,ttt", [(32, 2, 7), (31, 4, 1), (9, 4, 7), (5, 4, 1)])
def test_shards_equal_reference_process_data_usp(S_, sp, ttt):
    from oracle import ref_harness

    if not ref_harness.available():
        pytest.skip("reference checkout not present")
    ref_harness.setup()
    from specforge.data.preprocessing import OfflineEagle3Dataset

    from specforge_amd.ingest import usp_shard

    raw = _raw(S_, 3 * S_ + sp)
    ref_in = dict(input_ids=raw["input_ids"][0], loss_mask=raw["loss_mask"][0], hidden_state=raw["hidden_state"],
                  aux_hidden_state=raw["aux_hidden_state"])
    for r in range(sp):
        ref = OfflineEagle3Dataset.process_data_usp(ref_in, max_len=S_, ttt_length=ttt, sp_rank=r, sp_size=sp)
        ours = usp_shard(_normalised(raw), ttt_length=ttt, sp_rank=r, sp_size=sp)
        assert set(ref) == set(ours)
        for k in ref:
            assert ref[k].shape == ours[k].shape, k
            assert torch.equal(ref[k], ours[k]), (k, r)


# ------------------------------------------------------------------------------------------------------------------ the step
def _cfg(nkv=2, rope_scaling=None):
    from specforge_amd.model import DraftConfig

    return DraftConfig(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=nkv, vocab_size=256,
                       draft_vocab_size=128, head_dim=64, target_hidden_size=128, max_position_embeddings=128, rms_norm_eps=1e-5,
                       rope_scaling=rope_scaling)


def _model(cfg):
    from specforge_amd.model import LlamaForCausalLMEagle3

    m = LlamaForCausalLMEagle3(cfg)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
        t2d = torch.zeros(cfg.vocab_size, dtype=torch.bool)
        t2d[::2] = True
        m.load_vocab_mapping_tensors(t2d, torch.arange(cfg.draft_vocab_size) * 2 - torch.arange(cfg.draft_vocab_size))
    return m


def _sample(seed):
    """one normalised sample of the tiny config: [1, S] ids / mask, [1, S, 3 * 128] hidden states, [1, S, 128] target"""
    g = torch.Generator().manual_seed(seed)
    lm = (torch.rand(1, S, generator=g) > 0.25).long()
    lm[0, -1] = 0
    return dict(input_ids=torch.randint(0, 256, (1, S), generator=g), loss_mask=lm,
                hidden_state=torch.randn(1, S, 384, generator=g).to(torch.bfloat16),
                target=torch.randn(1, S, 128, generator=g).to(torch.bfloat16))


def _trainer(lk, backend_kw, attention_backend="hip"):
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    cfg = _cfg()
    eagle = OnlineEagle3Model(_model(cfg), length=T, attention_backend=attention_backend, lk_loss_type=lk).train()
    head = TargetHead(0.05 * torch.randn(cfg.vocab_size, 128, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-2, total_steps=100, warmup_ratio=0.0),
                                   **backend_kw)
    backend.prepare_model(eagle)
    return eagle, strat, backend


def _one_step(strat, backend, eagle, tensors):
    from specforge_amd.eagle3 import TrainBatch

    out = strat.forward_loss(TrainBatch(dict(tensors), {"target_repr": "hidden_state"}))
    backend.backward(out.loss, is_boundary=True)
    backend.synchronize_gradients()
    g = eagle.engine.flat.grad.float().clone()
    backend.step()
    m = out.metrics
    return dict(plosses=torch.stack(m["plosses"]).float(), acces=torch.stack(m["acces"]).float(),
                acc_corrects=torch.stack(m["acc_corrects"]).float(), grad=g, params=eagle.engine.flat.data.clone())


def _worker(rank, world, sp, port, emu_path, lk, out_dir, seeds):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    os.environ["SFEMU_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from specforge_amd import _lib
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    _lib._inject_library_for_tests(emu_path)
    eagle, strat, backend = _trainer(lk, dict(parallel_config=ParallelConfig(world_size=world, sp_size=sp, dp_size=world // sp)),
                                     attention_backend="usp")
    dp_rank, sp_rank = rank // sp, rank % sp
    res = _one_step(strat, backend, eagle, {**usp_shard(_sample(seeds[dp_rank]), ttt_length=T, sp_rank=sp_rank, sp_size=sp)})
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _single(emu_path, lk, seeds):
    """one process, no SP: the unsharded step (with draft_dp > 1: loss / n accumulated over the draft-dp groups' samples)"""
    from specforge_amd import _lib
    from specforge_amd.eagle3 import TrainBatch

    _lib._inject_library_for_tests(emu_path)
    try:
        eagle, strat, backend = _trainer(lk, {})
        pl, ac = [], []
        for i, s in enumerate(seeds):
            t = _sample(s)
            t["attention_mask"] = torch.ones(1, S, dtype=torch.long)
            out = strat.forward_loss(TrainBatch(t, {"target_repr": "hidden_state"}))
            backend.backward(out.loss / len(seeds), is_boundary=i == len(seeds) - 1)
            pl.append(torch.stack(out.metrics["plosses"]).float())
            ac.append(torch.stack(out.metrics["acces"]).float())
        g = eagle.engine.flat.grad.float().clone()
        backend.step()
        return dict(plosses=pl, acces=ac, grad=g, params=eagle.engine.flat.data.clone())
    finally:
        _lib._inject_library_for_tests(None)


def _compare(tmp_path, world, sp, ref, seeds, bars):
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    for r in ranks[1:]:     # every rank applies the same WORLD-averaged gradient
        assert torch.equal(r["params"], ranks[0]["params"])
    diffs = {}
    for d in range(world // sp):
        grp = ranks[d * sp:(d + 1) * sp]
        mean_loss = sum(r["plosses"] for r in grp) / sp
        diffs["loss"] = max(diffs.get("loss", 0.0), float((mean_loss - ref["plosses"][d]).abs().max()))
        for r in grp:       # accuracy: global counts, the same on every SP rank, the unsharded value
            assert torch.equal(r["acces"], grp[0]["acces"])
            diffs["acc"] = max(diffs.get("acc", 0.0), float((r["acces"] - ref["acces"][d]).abs().max()))
    g = ranks[0]["grad"] / world              # the SUM-reduced flat gradient, averaged over WORLD as the optimizer does
    gs = float(ref["grad"].abs().max())
    diffs["grad"] = float((g - ref["grad"]).abs().max()) / gs
    # weights after AdamW: the first step moves a weight by ~lr * sign(g) whatever |g| is, so a weight whose gradient is within the
    # gradient difference of zero may legitimately land 2 lr away.  Where |g| clearly exceeds that difference the sign is shared and
    # the two updates must agree to the bf16 rounding of the weight.
    clear = ref["grad"].abs() > 4 * (g - ref["grad"]).abs().max()
    diffs["clear_frac"] = float(clear.float().mean())
    diffs["params"] = float((ranks[0]["params"].float() - ref["params"].float())[clear].abs().max())
    print("usp vs unsharded:", diffs)
    assert diffs["clear_frac"] > 0.25         # (measured 0.32 - 0.49: the rest are small or zero gradients)
    for k, bar in bars.items():
        assert diffs[k] <= bar, (k, diffs[k], bar)


# Bars: about twice the difference measured on the interpreter build (recorded beside each); the two sides differ in the
# summation order of the attention (sp * chunk keys on nh / sp heads vs S keys on nh heads, the same rows) and in where bf16
# rounding happens in the gradient sums (per rank vs whole sample).
# (params: the weights whose gradient clearly exceeds the gradient difference, see _compare)
BARS = {(2, None): dict(loss=2.5e-7, acc=0.0, grad=1.3e-2, params=3e-5),       # measured: loss 1.2e-7, acc 0, grad 6.5e-3, params 1.5e-5
        (2, "lambda"): dict(loss=2.5e-7, acc=0.0, grad=8.5e-3, params=3e-5),   # measured: loss 1.2e-7, acc 0, grad 4.2e-3, params 1.5e-5
        (4, None): dict(loss=2.5e-7, acc=0.0, grad=1.2e-2, params=1.25e-4)}    # measured: loss 1.2e-7, acc 0, grad 5.6e-3, params 6.1e-5


@pytest.mark.parametrize("world,lk", [(2, None), (2, "lambda"), (4, None)], ids=["world2-sp2", "world2-sp2-lambda", "world4-dp2-sp2"])
def test_usp_step_matches_unsharded_step(emu_lib_path, tmp_path, world, lk):
    """world 2 = one SP pair; world 4 = draft_dp 2 x sp 2 (make_sp_groups pairs ranks 0,1 and 2,3; each pair reads its own sample)
    against single-process accumulation of loss / 2 over the same two samples"""
    seeds = [11, 12][:world // 2]
    mp.spawn(_worker, args=(world, 2, _free_port(), emu_lib_path, lk, str(tmp_path), seeds), nprocs=world, join=True)
    _compare(tmp_path, world, 2, _single(emu_lib_path, lk, seeds), seeds, BARS[(world, lk)])


def test_usp_runs_are_bit_identical(emu_lib_path, tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / str(i)
        d.mkdir()
        mp.spawn(_worker, args=(2, 2, _free_port(), emu_lib_path, None, str(d), [11]), nprocs=2, join=True)
        runs.append([torch.load(d / f"rank{r}.pt") for r in range(2)])
    for a, b in zip(*runs):
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------ refusals
def _engine_error(cfg, B=1):
    """the ValueError of building a USP engine (SP size 2, a stand-in group: the checks read only its size) and running one forward;
    every check fires before a kernel launch"""
    from specforge_amd.engine import Eagle3Engine

    class _G:          # a process group stand-in of size 2 (the refusals read the size only)
        pass

    import specforge_amd.engine as E

    real = (E.dist.get_world_size, E.dist.get_rank, E.dist.get_backend)
    E.dist.get_world_size, E.dist.get_rank, E.dist.get_backend = (lambda g=None: 2), (lambda g=None: 0), (lambda g=None: "gloo")
    try:
        with pytest.raises(ValueError) as ei:
            eng = Eagle3Engine(_model(cfg), ttt_length=T, sp_group=_G())
            eng.forward(input_ids=torch.zeros(B, 8 + T, dtype=torch.long), attention_mask=None, loss_mask=torch.ones(B, 8 + T),
                        hidden_states=torch.zeros(B, 8 + T, 384, dtype=torch.bfloat16))
    finally:
        E.dist.get_world_size, E.dist.get_rank, E.dist.get_backend = real
    return str(ei.value)


def test_usp_refusals(emu_lib_path):
    from specforge_amd import _lib
    from specforge_amd.reference_plugin import check_training_topology
    from specforge_amd.training import HipDPTrainingBackend, ParallelConfig

    _lib._inject_library_for_tests(emu_lib_path)
    try:
        assert "num_key_value_heads" in _engine_error(_cfg(nkv=1))
        assert "mrope" in _engine_error(_cfg(rope_scaling={"rope_type": "mrope", "mrope_section": [16, 8, 8]}))
        assert "batch_size" in _engine_error(_cfg(), B=2)
    finally:
        _lib._inject_library_for_tests(None)
    with pytest.raises(ValueError, match="tp_size"):
        HipDPTrainingBackend(ParallelConfig(tp_size=2))

    class _T:
        sp_ring_size, tp_size, attention_backend, batch_size = 1, 1, "usp", 1

    for k, v in (("sp_ring_size", 2), ("tp_size", 2), ("batch_size", 2)):
        t = _T()
        setattr(t, k, v)
        with pytest.raises(ValueError, match=k):
            check_training_topology(t)


def test_reference_schema_usp_config_reaches_the_refusals():
    """YAML-level configs the reference schema accepts are refused by the plugin's model factory before any step (the factory checks
    the topology first thing, so no model, device or target head is needed to reach the refusal)"""
    from oracle import ref_harness

    if not ref_harness.available():
        pytest.skip("reference checkout not present")
    ref_harness.setup()
    from specforge.config.schema import TrainingConfig

    from specforge_amd.reference_plugin import check_training_topology

    from types import SimpleNamespace

    from specforge_amd.reference_plugin import _training_model_factory

    build = _training_model_factory()
    cases = [(dict(attention_backend="usp", sp_ulysses_size=1, sp_ring_size=2), None, "sp_ring_size"),
             (dict(attention_backend="usp", sp_ulysses_size=2), _cfg(nkv=1), "num_key_value_heads"),
             (dict(attention_backend="usp", sp_ulysses_size=2), _cfg(), "attention_backend 'usp'")]
    for kw, draft_cfg, key in cases:
        t = TrainingConfig(batch_size=1, **kw)           # accepted by the reference's own schema
        with pytest.raises(ValueError, match=key):
            build(SimpleNamespace(training=t), None, draft_cfg, None, None)
    with pytest.raises(ValueError, match="tp_size"):
        check_training_topology(SimpleNamespace(sp_ring_size=1, tp_size=2, attention_backend="sdpa"))


def test_ingest_streams_usp_shards_over_draft_dp(tmp_path):
    """HiddenStateIngest(sp_rank, sp_size): every batch is this rank's usp_shard of one sample; the sp peers of a draft-dp rank read
    the same sample index"""
    from specforge_amd.ingest import HiddenStateIngest, normalize_offline_sample, usp_shard

    files = []
    for i, S_ in enumerate((13, 20, 9, 16)):
        r = _raw(S_, 40 + i)
        p = str(tmp_path / f"s{i}.ckpt")
        torch.save(dict(input_ids=r["input_ids"][0], loss_mask=r["loss_mask"][0], hidden_state=r["hidden_state"].to(torch.bfloat16),
                        aux_hidden_state=r["aux_hidden_state"].to(torch.bfloat16)), p)
        files.append(p)
    for dp_rank in range(2):
        seen = []
        for sp_rank in range(2):
            ing = HiddenStateIngest(files, batch_size=1, max_len=64, device="cpu", dp_rank=dp_rank, dp_size=2, seed=3,
                                    sp_rank=sp_rank, sp_size=2, ttt_length=3)
            batches = list(ing.epoch(0))
            seen.append([b.metadata["sample_indices"] for b in batches])
            for b in batches:
                raw = torch.load(files[b.metadata["sample_indices"][0]], weights_only=True)
                want = usp_shard(normalize_offline_sample(raw, 64), ttt_length=3, sp_rank=sp_rank, sp_size=2)
                assert set(b.tensors) == set(want)
                for k in want:
                    assert torch.equal(b.tensors[k], want[k]), k
        assert seen[0] == seen[1]
    with pytest.raises(ValueError, match="batch_size"):
        HiddenStateIngest(files, batch_size=2, max_len=64, device="cpu", sp_size=2)
