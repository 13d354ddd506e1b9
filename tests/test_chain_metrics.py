"""Joint chain counts per TTT depth (Eagle3Engine.chain -> ``chain_denoms`` / ``chain_corrects``, ``OnlineEagle3Model.last_chain``,
``StepOutput.metrics["chain_top{k}_corrects"]``, ``Eagle3Engine.chain_lengths``, ``ChainAccumulator``) on the tiny golden configurations.
Counts are integers: every comparison is exact.

The yardstick is torch on the logits an EVAL forward leaves intact: per-row hits formed as tests/test_topk_metrics._torch_counts forms
them (rank = (z > z[t]).sum() + (z[:t] == z[t]).sum() < k, over the rows with a loss mask), then folded over the steps: a row is
eligible at depth k if it had a loss mask at every depth 0 .. k, alive in channel h if it also hit at every one of them.

With the goldens' own vocabulary map every chain is dead by depth 2 (most teacher tokens have no draft index), so every case here
first runs one eval forward, takes the distinct teacher ids and rebuilds the model with an ascending map that contains them all, and
uses topk = (1, Vd/2, 3Vd/4, Vd): then some chains of the wide channels survive to the deepest depth and some do not."""
import pytest
import torch

from specforge_amd.eagle3 import ChainAccumulator, loss_mask_suffix_counts
from test_engine_golden import _batch, _build
from test_topk_metrics import _load

GOLDENS = ["eagle3_tiny_fp32", "eagle31_gqa_fp32"]
_cache = {}


def _remapped(golden_dir, name, mask, dev):
    """the golden with an ascending vocabulary map that holds every teacher token of its batch (module docstring)"""
    blob = _load(golden_dir, name, mask)
    key = (name, str(dev))
    if key not in _cache:
        full = _load(golden_dir, name)
        cfg, model, eagle, strat = _build(full, dev)
        eagle.eval()
        with torch.no_grad():
            strat.forward_loss(_batch(full, dev))
        ids = torch.unique(eagle.last_artifacts["target_token_ids"].cpu())
        Vt, Vd = full["t2d"].numel(), full["d2t"].numel()
        assert ids.numel() <= Vd
        t2d = torch.zeros(Vt, dtype=torch.bool)
        t2d[ids] = True
        rest = (~t2d).nonzero().flatten()[:Vd - ids.numel()]        # fill up with the lowest other ids
        t2d[rest] = True
        d2t = t2d.nonzero().flatten() - torch.arange(Vd)
        _cache[key] = (t2d, d2t.to(full["d2t"].dtype))
    blob["t2d"], blob["d2t"] = _cache[key]
    return blob


def _topk_for(blob):
    Vd = blob["d2t"].numel()
    return (1, Vd // 2, 3 * Vd // 4, Vd)


def _torch_fold(eng, B, S, d2t, Vt, topk):
    """per-row hits with torch from the logits an eval forward left in the engine's buffers, folded over the steps"""
    b = eng._views[(B, S)]
    d2t = d2t.long()
    Vd = d2t.numel()
    inv = torch.full((Vt,), -1, dtype=torch.long)
    inv[torch.arange(Vd) + d2t] = torch.arange(Vd)
    ks = (1,) + tuple(topk)
    elig = torch.ones(B * S, dtype=torch.bool)
    alive = torch.ones(len(ks), B * S, dtype=torch.bool)
    want = dict(denoms=[], corrects=[], marginal=[], depth=torch.zeros(B * S, dtype=torch.int32),
                length=torch.zeros(len(ks), B * S, dtype=torch.int32))
    for k in range(eng.T):
        z = b["logits"][k].float().cpu()                                  # [B * S, Vd]
        lm = b["lm"][:, k:k + S].reshape(-1).cpu()
        t = inv[b["tids"][:, k:k + S].reshape(-1).cpu()]
        zt = z.gather(1, t.clamp_min(0)[:, None])
        below = torch.arange(Vd)[None, :] < t[:, None]
        rank = (z > zt).sum(1) + ((z == zt) & below).sum(1)
        ok = (lm != 0) & (t >= 0)
        hit = torch.stack([ok & (rank < kk) for kk in ks])
        elig = elig & (lm != 0)
        alive = alive & elig[None] & hit
        want["denoms"].append(elig.float().sum())
        want["corrects"].append(alive.float().sum(1))
        want["marginal"].append(hit.float().sum(1))
        want["depth"] += elig.int()
        want["length"] += alive.int()
    return want


def _eval(blob, dev, topk, chain=True):
    cfg, model, eagle, strat = _build(blob, dev)
    eagle.topk, eagle.chain = topk, chain
    eagle.eval()
    with torch.no_grad():
        out = strat.forward_loss(_batch(blob, dev))
    B, S = blob["batch"]["input_ids"].shape
    want = _torch_fold(eagle.engine, B, S, blob["d2t"], blob["t2d"].numel(), topk)
    return out, want, eagle


def _assert_counts(eagle, want, what=""):
    den, cor = eagle.last_chain
    assert len(den) == len(cor) == eagle.engine.T
    for k in range(eagle.engine.T):
        assert den[k].dim() == 0 and torch.equal(den[k].cpu(), want["denoms"][k]), (what, k, den[k], want["denoms"][k])
        assert torch.equal(cor[k].cpu(), want["corrects"][k]), (what, k, cor[k], want["corrects"][k])


@pytest.mark.parametrize("name", GOLDENS)
def test_eval_forward_counts_match_torch(backend, golden_dir, name):
    blob = _remapped(golden_dir, name, None, backend)
    topk = _topk_for(blob)
    out, want, eagle = _eval(blob, backend, topk)
    T, m = eagle.engine.T, out.metrics
    den, cor = [float(x) for x in eagle.last_chain[0]], torch.stack([c.cpu() for c in eagle.last_chain[1]])
    print("chain_denoms", den, "chain_corrects", cor.tolist(), "marginal", torch.stack(want["marginal"]).tolist())
    _assert_counts(eagle, want)
    assert cor.shape == (T, 1 + len(topk))
    # depth 0 is the marginal count
    assert float(m["chain_top1_corrects"][0]) == float(m["acc_corrects"][0]) and float(m["chain_denoms"][0]) == float(m["acc_denoms"][0])
    for kk in topk:
        assert float(m[f"chain_top{kk}_corrects"][0]) == float(m[f"top{kk}_corrects"][0])
    for k in range(T):
        assert float(m["chain_denoms"][k]) == float(m["acc_denoms"][k])      # the goldens' loss mask is full: nothing is censored
        assert m["chain_denoms"][k].dim() == 0 and m["chain_top1_corrects"][k].dim() == 0
        assert float(cor[k, -1]) == den[k]                                   # the Vd channel: every scored target has a draft index
        assert bool((cor[k, 1:] >= cor[k, :-1]).all())                       # monotone in k
        for j, kk in enumerate(topk):
            assert float(m[f"chain_top{kk}_corrects"][k]) == float(cor[k, 1 + j])
    assert bool((cor[1:] <= cor[:-1]).all()) and all(a >= b for a, b in zip(den, den[1:]))       # monotone in depth
    # non-vacuity: at the deepest depth some chains of a channel are alive and some are dead; the joint count is not the marginal one
    assert any(0 < float(cor[T - 1, h]) < den[T - 1] for h in range(1 + len(topk)))
    marg = torch.stack(want["marginal"])
    assert float(marg[:, 3].min()) >= 32                                     # (the 3Vd/4 channel's marginal hits stay high ...)
    assert bool((cor[1:] != marg[1:]).any())                                 # (... and the joint counts fall below them)


def test_denominators_with_a_gap(backend, golden_dir):
    """the ``half`` mask on the 7-step golden: the eligible rows thin out to none at the last depth"""
    blob = _remapped(golden_dir, "eagle31_gqa_fp32", "half", backend)
    out, want, eagle = _eval(blob, backend, _topk_for(blob))
    _assert_counts(eagle, want)
    assert [float(x) for x in eagle.last_chain[0]] == [19, 9, 4, 3, 2, 1, 0]
    assert float(out.metrics["acc_denoms"][1]) > 9                           # censoring: fewer rows than the step's own loss mask


@pytest.mark.parametrize("name,mask", [("eagle31_gqa_fp32", "half"), ("eagle31_gqa_fp32", "head_only"), ("eagle3_tiny_fp32", "half"),
                                       ("eagle3_lk_lambda_fp32", "half")])
def test_counts_agree_across_variants(backend, golden_dir, name, mask):
    """eval (checked against torch) == training dense == training with loss-row compaction forced on; a loss mask with half the rows
    out; a step whose compact row count is 0; an LK objective"""
    blob = _remapped(golden_dir, name, mask, backend)
    topk = _topk_for(blob)
    out, want, eagle = _eval(blob, backend, topk)
    _assert_counts(eagle, want, "eval")
    got = eagle.engine.chain_lengths()
    B, S = blob["batch"]["input_ids"].shape
    assert got["depth"].dtype == torch.int32 and got["depth"].shape == (B, S) and got["length"].shape == (1 + len(topk), B, S)
    assert torch.equal(got["depth"].cpu().view(-1), want["depth"]) and torch.equal(got["length"].cpu().view(1 + len(topk), -1), want["length"])
    for compact in (False, True):
        cfg, model, eagle, strat = _build(blob, backend)
        eagle.topk, eagle.chain = topk, True
        eagle.train()
        eagle.engine.compact_loss_rows = compact
        batch = _batch(blob, backend)
        batch.metadata["loss_mask_suffix_counts"] = loss_mask_suffix_counts(blob["batch"]["loss_mask"])
        o = strat.forward_loss(batch)
        assert (eagle.engine._lm_compact_K is not None) == (compact and (eagle.engine.lk_loss_type is None or eagle.engine._soft[0] == "zt"))
        _assert_counts(eagle, want, f"train compact={compact}")
        got = eagle.engine.chain_lengths()
        assert torch.equal(got["depth"].cpu().view(-1), want["depth"]) and torch.equal(got["length"].cpu().view(1 + len(topk), -1), want["length"])
        o.loss.backward()
        for k in range(eagle.engine.T):
            assert float(o.metrics["chain_top1_corrects"][k]) == float(want["corrects"][k][0])
    if mask == "head_only":     # the mask ends at position 2: no chain is scorable at depth 3 or beyond
        assert all(float(d) == 0.0 for d in want["denoms"][3:]) and float(want["denoms"][2]) == B


@pytest.mark.parametrize("topk", [(), (1, 2, 4, 8)], ids=["top1_only", "topk"])
@pytest.mark.parametrize("name", GOLDENS + ["eagle3_lk_lambda_fp32"])
def test_training_step_is_bit_identical_with_and_without_chain(backend, golden_dir, name, topk):
    """the fold runs after the fused CE on buffers of its own and disturbs nothing"""
    blob = _load(golden_dir, name)
    runs = []
    for chain in (False, True):
        cfg, model, eagle, strat = _build(blob, backend)
        eagle.topk, eagle.chain = topk, chain
        eagle.train()
        out = strat.forward_loss(_batch(blob, backend))
        out.loss.backward()
        runs.append((out, eagle.engine.flat.grad.clone().cpu(), eagle))
        for nm in ("chain_state", "chain_rows", "chain_met"):
            assert (nm in eagle.engine.arena_names()) == chain
    (a, ga, ea), (b, gb, eb) = runs
    assert ea.last_chain is None and not any(k.startswith("chain") for k in a.metrics)
    assert torch.equal(a.loss.detach().cpu(), b.loss.detach().cpu()) and torch.equal(ga, gb)
    for key in a.metrics:
        assert torch.equal(torch.stack(a.metrics[key]).cpu(), torch.stack(b.metrics[key]).cpu()), key
    assert sorted(set(b.metrics) - set(a.metrics)) == sorted(["chain_denoms"] + [f"chain_top{k}_corrects" for k in {1, *topk}])
    assert float(b.metrics["chain_top1_corrects"][0]) == float(b.metrics["acc_corrects"][0])
    with pytest.raises(RuntimeError, match="chain_lengths"):
        ea.engine.chain_lengths()


def test_switching_chain_on_an_engine_rebuilds_and_frees(backend, golden_dir):
    blob = _remapped(golden_dir, "eagle3_tiny_fp32", None, backend)
    topk = _topk_for(blob)
    out, want, eagle = _eval(blob, backend, topk, chain=False)
    assert eagle.last_chain is None and "chain_met" not in eagle.engine.arena_names()
    cfg, model, eagle2, strat = _build(blob, backend)
    eagle2.topk = topk
    eagle2.eval()
    with torch.no_grad():
        strat.forward_loss(_batch(blob, backend))
        assert eagle2.last_chain is None
        eagle2.chain = True
        strat.forward_loss(_batch(blob, backend))
        _assert_counts(eagle2, want, "switched on")
        strat.forward_loss(_batch(blob, backend))                      # the state is zeroed at the start of every forward
        _assert_counts(eagle2, want, "second forward")
        eagle2.chain = False
        strat.forward_loss(_batch(blob, backend))
    assert eagle2.last_chain is None and not any(n.startswith("chain") for n in eagle2.engine.arena_names())


def test_a_one_in_topk_is_named_once(backend, golden_dir):
    blob = _remapped(golden_dir, "eagle3_tiny_fp32", None, backend)
    out, want, eagle = _eval(blob, backend, (1, 2))
    _assert_counts(eagle, want)
    cor = torch.stack([c.cpu() for c in eagle.last_chain[1]])
    assert cor.shape[1] == 3 and torch.equal(cor[:, 0], cor[:, 1])
    assert sorted(k for k in out.metrics if k.startswith("chain")) == ["chain_denoms", "chain_top1_corrects", "chain_top2_corrects"]
    assert torch.equal(torch.stack(out.metrics["chain_top1_corrects"]).cpu(), cor[:, 0])


def test_accumulator_sums_before_the_ratio(backend, golden_dir):
    """two batches of different size equal one concatenated count; a depth without an eligible row reports 0.0"""
    blob = _remapped(golden_dir, "eagle3_tiny_fp32", "head_only", backend)
    topk = _topk_for(blob)
    ks = (1,) + topk[1:]
    cfg, model, eagle, strat = _build(blob, backend)
    eagle.topk, eagle.chain = topk, True
    eagle.eval()
    full = _batch(blob, backend)
    assert full.tensors["input_ids"].shape[0] >= 2
    one = type(full)(tensors={k: v[:1] for k, v in full.tensors.items()}, metadata=dict(full.metadata))
    acc = ChainAccumulator(ks)
    assert acc.summary() == {}
    sums = {k: torch.zeros(eagle.length, dtype=torch.float64) for k in ks}
    den = torch.zeros(eagle.length, dtype=torch.float64)
    with torch.no_grad():
        for batch in (full, one):
            m = strat.forward_loss(batch).metrics
            acc.update(m)
            for k in ks:
                sums[k] += torch.stack(m[f"chain_top{k}_corrects"]).double().cpu()
            den += torch.stack(m["chain_denoms"]).double().cpu()
    s = acc.summary()
    assert sorted(s) == sorted([f"chain_top{k}_acc_{i}" for k in ks for i in range(eagle.length)] + [f"chain_acc_len_top{k}" for k in ks])
    assert den.tolist() == [9.0, 6.0, 3.0, 0.0]                            # (2 + 1 samples, the mask on positions 0 .. 2)
    for k in ks:
        rates = [float(c / d) if d > 0 else 0.0 for c, d in zip(sums[k].tolist(), den.tolist())]
        for i, a in enumerate(rates):
            assert s[f"chain_top{k}_acc_{i}"] == a
        assert s[f"chain_acc_len_top{k}"] == sum(rates)
        assert s[f"chain_top{k}_acc_3"] == 0.0
    assert s[f"chain_acc_len_top{topk[-1]}"] == 3.0 and s["chain_acc_len_top1"] <= s[f"chain_acc_len_top{topk[1]}"]
    with pytest.raises(ValueError, match="ChainAccumulator"):
        ChainAccumulator((1, 1))
