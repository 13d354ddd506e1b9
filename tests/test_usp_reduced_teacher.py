"""The reduced teacher and loss-row compaction under USP (Ulysses, ring and Ulysses x ring), on CPU: gloo ranks drive the engine with
the kernels under the SIMT interpreter.  A rank's teacher covers its chunk plus the T rows of overlap from the next shard; with a
sparse, turn-like loss mask and host-known per-rank window counts (``eagle3.loss_mask_window_counts``) the teacher keeps only its
draft logits (``_soft[0] == "zt"``) and runs over the gathered positions (``_teacher_compacted``), lm_head / CE over the rows with a
loss.  Held to the same USP step in the dense, materialised form and to the unsharded step; wrong counts raise.  The host counts of
the ingest and the plugin loader equal the helper's on the reference collator's batch."""
import functools
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T = 3
HT = 512                # target hidden size: the interpreter's reduced head GEMM needs K >= 512 (sf_gemm_nt_teacher_reduces)
VT, VD = 640, 256       # roundup(Vd, 256) < Vt


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cfg():
    from specforge_amd.model import DraftConfig

    return DraftConfig(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2, vocab_size=VT,
                       draft_vocab_size=VD, head_dim=64, target_hidden_size=HT, max_position_embeddings=1024, rms_norm_eps=1e-5)


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
        t2d = torch.zeros(VT, dtype=torch.bool)
        t2d[:2 * VD:2] = True                   # an ascending injection: the permuted teacher head with its partials
        m.load_vocab_mapping_tensors(t2d, torch.arange(VD) * 2 - torch.arange(VD))
    return m


def turn_mask(S_):
    """a chat-like loss mask: 12-token prompts (no loss) between 52-token answers; the shard boundaries of the cases here fall inside an
    answer, so the overlap rows carry a loss"""
    p = torch.arange(S_)
    lm = (((p + 20) % 64) >= 12).long()[None]
    lm[0, -1] = 0
    return lm


def _sample(S_, seed=11):
    g = torch.Generator().manual_seed(seed)
    return dict(input_ids=torch.randint(0, VT, (1, S_), generator=g), loss_mask=turn_mask(S_),
                hidden_state=torch.randn(1, S_, 3 * HT, generator=g).to(torch.bfloat16),
                target=torch.randn(1, S_, HT, generator=g).to(torch.bfloat16))


def _trainer(backend_kw, attention_backend="hip"):
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    cfg = _cfg()
    eagle = OnlineEagle3Model(_model(cfg), length=T, attention_backend=attention_backend).train()
    head = TargetHead((0.2 * torch.randn(VT, HT, generator=torch.Generator().manual_seed(9))).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-2, total_steps=100, warmup_ratio=0.0),
                                   **backend_kw)
    backend.prepare_model(eagle)
    return eagle, strat, backend


def _step(strat, backend, eagle, tensors, md=None):
    from specforge_amd.eagle3 import TrainBatch

    out = strat.forward_loss(TrainBatch(dict(tensors), dict({"target_repr": "hidden_state"}, **(md or {}))))
    eng = eagle.engine
    state = dict(compacted=eng._teacher_compacted, soft=eng._soft[0], lm_compact=eng._lm_compact_K is not None)
    backend.backward(out.loss, is_boundary=True)
    backend.synchronize_gradients()
    g = eng.flat.grad.float().clone()
    m = out.metrics
    return dict(state, plosses=torch.stack(m["plosses"]).float(), acces=torch.stack(m["acces"]).float(),
                acceptance_rates=torch.stack(m["acceptance_rates"]).float(), acc_corrects=torch.stack(m["acc_corrects"]).float(),
                ids=eagle.last_artifacts["target_token_ids"].cpu().clone(), pm=eagle.last_artifacts["position_mask"].cpu().clone(), grad=g)


def _worker(rank, sp, r, S_, port, emu_path, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    os.environ["SFEMU_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=sp)
    from specforge_amd import _lib
    from specforge_amd.eagle3 import loss_mask_window_counts
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    _lib._inject_library_for_tests(emu_path)
    shard = usp_shard(_sample(S_), ttt_length=T, sp_rank=rank, sp_size=sp)
    res = {}
    pc = lambda: dict(parallel_config=ParallelConfig(world_size=sp, sp_size=sp, sp_ring_size=r, dp_size=1))
    # the default: host window counts from the CPU mask -> reduced teacher over the gathered positions + compact lm_head / CE
    eagle, strat, backend = _trainer(pc(), attention_backend="usp")
    res["compact"] = _step(strat, backend, eagle, shard)
    # the same step dense and materialised
    eagle, strat, backend = _trainer(pc(), attention_backend="usp")
    eagle.engine.compact_loss_rows = False
    eagle.engine.materialise_soft_targets = True
    res["dense"] = _step(strat, backend, eagle, shard)
    # wrong counts (one too many; a zero where rows carry a loss): the device check raises at the end of the backward sweep
    res["errors"] = []
    for k, how in ((1, "plus"), (0, "zero")):
        eagle, strat, backend = _trainer(pc(), attention_backend="usp")
        wrong = loss_mask_window_counts(shard["loss_mask"], T)
        wrong[k] = wrong[k] + 1 if how == "plus" else 0
        try:
            _step(strat, backend, eagle, shard, {"loss_mask_window_counts": wrong})
            res["errors"].append(None)
        except RuntimeError as e:
            res["errors"].append(str(e))
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _single(emu_path, S_):
    """the unsharded step (host suffix counts: the compact teacher and lm_head there too)"""
    from specforge_amd import _lib

    _lib._inject_library_for_tests(emu_path)
    try:
        eagle, strat, backend = _trainer({})
        t = _sample(S_)
        t["attention_mask"] = torch.ones(1, S_, dtype=torch.long)
        return _step(strat, backend, eagle, t)
    finally:
        _lib._inject_library_for_tests(None)


# Bars of the USP step against the unsharded one: tests/test_usp.py's (loss 2.5e-7 -- 5e-7 with four ranks --, accuracy exact, gradient
# 1.3e-2 of its largest element); measured on the interpreter build beside each.
BARS = {"u2": dict(loss=2.5e-7, grad=1.3e-2),         # measured: loss 1.2e-7, grad 3.7e-3
        "u1r2": dict(loss=2.5e-7, grad=1.3e-2),       # measured: loss 1.2e-7, grad 3.7e-3
        "u2r2": dict(loss=5e-7, grad=1.3e-2)}         # measured: loss 1.2e-7, grad 5.9e-3


@pytest.mark.parametrize("sp,r,key", [(2, 1, "u2"), (2, 2, "u1r2"), (4, 2, "u2r2")])
def test_usp_reduced_teacher_with_compaction(emu_lib_path, tmp_path, sp, r, key):
    S_ = 256 * sp           # chunks of 256 rows, ~80 % of them with a loss: >= 192 gathered teacher rows per rank
    mp.spawn(_worker, args=(sp, r, S_, _free_port(), emu_lib_path, str(tmp_path)), nprocs=sp, join=True)
    ranks = [torch.load(tmp_path / f"rank{i}.pt") for i in range(sp)]
    for i, rk in enumerate(ranks):
        c, d = rk["compact"], rk["dense"]
        assert c["compacted"] and c["soft"] == "zt" and c["lm_compact"], (i, c["compacted"], c["soft"])
        assert not d["compacted"] and d["soft"] == "tp" and not d["lm_compact"]
        # against the dense materialised USP step: position mask and (where the loss mask is set) target ids exact, metrics to the
        # last bits of sum(target_p) (sd * (1 / sd) in the reduced form), gradients to summation order (compact lm_head stash)
        on = turn_mask(S_)[:, i * 256:(i + 1) * 256].bool()
        assert torch.equal(c["pm"], d["pm"]) and torch.equal(c["ids"][on], d["ids"][on])
        for k in ("plosses", "acces", "acceptance_rates", "acc_corrects"):
            torch.testing.assert_close(c[k], d[k], rtol=2e-6, atol=1e-7, msg=k)
        torch.testing.assert_close(c["grad"], d["grad"], rtol=2e-2, atol=4e-3 * float(d["grad"].abs().max()))
        for e in rk["errors"]:
            assert e is not None and "loss_counts" in e, e
    for rk in ranks[1:]:
        assert torch.equal(rk["compact"]["grad"], ranks[0]["compact"]["grad"])
        assert torch.equal(rk["compact"]["acces"], ranks[0]["compact"]["acces"])
    ref = _single(emu_lib_path, S_)
    assert ref["compacted"] and ref["soft"] == "zt"
    mean_loss = sum(rk["compact"]["plosses"] for rk in ranks) / sp
    dl = float((mean_loss - ref["plosses"]).abs().max())
    da = float((ranks[0]["compact"]["acces"] - ref["acces"]).abs().max())
    dg = float((ranks[0]["compact"]["grad"] / sp - ref["grad"]).abs().max()) / float(ref["grad"].abs().max())
    print(f"usp {key} compact vs unsharded: loss {dl:.3g} acc {da:.3g} grad {dg:.3g}")
    assert dl <= BARS[key]["loss"] and da == 0.0 and dg <= BARS[key]["grad"], (dl, da, dg)


def test_window_counts_helper():
    from specforge_amd.eagle3 import loss_mask_window_counts

    g = torch.Generator().manual_seed(3)
    for L, t in ((40, 3), (11, 7), (9, 1)):
        lm = (torch.rand(1, L, generator=g) > 0.4).long()
        S_ = L - t
        want = [int((lm[:, k:k + S_] != 0).sum()) for k in range(t)]
        assert loss_mask_window_counts(lm, t) == want
        assert loss_mask_window_counts(lm[..., None], t) == want          # ([B, S, 1] as the strategy's preprocess leaves it)
    assert loss_mask_window_counts(torch.ones(1, 3, dtype=torch.long), 3) == [0, 0, 0]


def test_ingest_usp_shards_carry_window_counts(tmp_path):
    """HiddenStateIngest(sp_size > 1): every shard's metadata carries the window counts of the rows the engine takes (chunk +
    ttt_length; with the collator's layout the mask is longer and usp_unpad cuts it)"""
    from specforge_amd.eagle3 import loss_mask_window_counts, usp_unpad
    from specforge_amd.ingest import HiddenStateIngest

    files = []
    for i, n in enumerate((45, 20, 9, 64)):
        g = torch.Generator().manual_seed(60 + i)
        p = str(tmp_path / f"s{i}.ckpt")
        torch.save(dict(input_ids=torch.randint(0, 100, (n,), generator=g), loss_mask=(torch.rand(n, generator=g) > 0.3).long(),
                        hidden_state=torch.randn(1, n, 16, generator=g).to(torch.bfloat16),
                        aux_hidden_state=torch.randn(1, n, 48, generator=g).to(torch.bfloat16)), p)
        files.append(p)
    for collator in (False, True):
        for sp, u in ((2, 2), (4, 2)):
            for sp_rank in range(sp):
                ing = HiddenStateIngest(files, batch_size=1, max_len=48, device="cpu", sp_rank=sp_rank, sp_size=sp, ttt_length=T,
                                        collator_layout=collator, sp_ulysses_size=u, seed=1)
                n = 0
                for b in ing.epoch(0):
                    lm = usp_unpad(b.tensors)["loss_mask"]
                    assert lm.shape[1] == b.tensors["hidden_state"].shape[1]
                    assert b.metadata["loss_mask_window_counts"] == loss_mask_window_counts(lm, T)
                    n += 1
                assert n == len(files)


@pytest.fixture(scope="module")
def ref(emu_lib_path):
    from oracle import ref_harness as RH

    if not RH.available():
        pytest.skip("needs the reference checkout")
    RH.setup()
    RH.init_single_rank(29593)
    from specforge_amd import _lib
    from specforge_amd import reference_plugin as RP

    _lib._inject_library_for_tests(emu_lib_path)
    yield RP
    RP.uninstall()
    _lib._inject_library_for_tests(None)


@pytest.mark.parametrize("u,r", [(2, 1), (1, 2), (2, 2)])
def test_plugin_usp_batches_carry_window_counts(ref, tmp_path, u, r):
    """the plugin loader's USP batches (ranged reader) carry the per-rank window counts the helper gives on the reference's own batch
    (process_data_usp + collator, usp_unpad as the strategy applies it); the reference's metadata stays as it is"""
    from specforge.data.preprocessing import OfflineEagle3Dataset
    from specforge.data.utils import DataCollatorWithPadding
    from specforge.launch import _shard_offline_refs
    from specforge.runtime.data_plane import FeatureDataLoader, LocalFeatureStore

    from specforge_amd.eagle3 import loss_mask_window_counts, usp_unpad
    from test_plugin_usp import _write_run_dir

    sp, max_len = u * r, 40
    _, feat, _, _ = _write_run_dir(str(tmp_path), [33, 5, 40, 47, 17])
    alg = ref.registry().resolve(ref.ALGORITHM_NAME)
    source = alg.providers.offline_for("text").build_reader(feat, run_id="t", ttt_length=T, max_len=max_len).read()
    Hip = ref.feature_loader_class()
    for sp_rank in range(sp):
        transform = functools.partial(OfflineEagle3Dataset.process_data_usp, max_len=max_len, ttt_length=T, sp_rank=sp_rank, sp_size=sp,
                                      ring_rank=sp_rank // u, sp_ring_size=r)
        collate = DataCollatorWithPadding()
        collate.sp_degree, collate.ulysses_degree = sp, u
        refs = _shard_offline_refs(source, use_usp_preprocess=True, seed=3, epoch=0, dp_rank=0, dp_size=1)
        mk = lambda cls: cls(LocalFeatureStore("t"), refs=refs, batch_size=1, collate_fn=collate, per_sample_transform=transform,
                             strategy=alg.name)
        want = list(mk(FeatureDataLoader))
        got = list(mk(Hip))
        assert len(got) == len(want) == len(refs)
        for b, w in zip(got, want):
            assert b.metadata == w.metadata
            assert b.loss_mask_window_counts == loss_mask_window_counts(usp_unpad(w.tensors)["loss_mask"], T)
