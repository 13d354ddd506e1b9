"""Top-k hit counts per TTT step (Eagle3Engine.topk -> ``topk_corrects``, ``OnlineEagle3Model.last_topk``, ``StepOutput.metrics["top{k}_corrects"]``,
``TopKAccumulator``) on the tiny golden configurations.  Counts are integers: every comparison is exact.

The yardstick is torch on the logits an EVAL forward leaves intact: rank = (z > z[t]).sum() + (z[:t] == z[t]).sum() with t the draft index
of the teacher's token, counted over the rows with a loss mask.  Training forwards (whose CE overwrites the logits with their gradient) must
give the same counts -- dense and with loss-row compaction, with an LK objective -- and must not move a bit of the losses, metrics or
gradients of a run without the metric."""
import os

import pytest
import torch

from specforge_amd.eagle3 import TopKAccumulator, loss_mask_suffix_counts
from test_engine_golden import _batch, _build

GOLDENS = ["eagle3_tiny_fp32", "eagle31_gqa_fp32"]


def _load(golden_dir, name, mask=None):
    blob = torch.load(os.path.join(golden_dir, f"{name}.pt"), weights_only=False)
    lm = blob["batch"]["loss_mask"].clone()
    if mask == "half":          # half the rows out
        lm = (torch.rand(lm.shape, generator=torch.Generator().manual_seed(5)) < 0.5).to(lm.dtype)
    elif mask == "head_only":   # the mask ends at position 2: TTT steps 3.. compact to zero rows
        lm.zero_()
        lm[:, :3] = 1
    blob["batch"] = dict(blob["batch"], loss_mask=lm)
    return blob


def _torch_counts(eng, B, S, d2t, Vt, topk):
    """the hit counts and the position-mask counts per TTT step, with torch, from the logits an eval forward left in the engine's buffers"""
    b = eng._views[(B, S)]
    d2t = d2t.long()
    Vd = d2t.numel()
    inv = torch.full((Vt,), -1, dtype=torch.long)
    inv[torch.arange(Vd) + d2t] = torch.arange(Vd)
    want, pmc = [], []
    for k in range(eng.T):
        z = b["logits"][k].float().cpu()                                  # [B * S, Vd]
        lm = b["lm"][:, k:k + S].reshape(-1).cpu()
        t = inv[b["tids"][:, k:k + S].reshape(-1).cpu()]
        zt = z.gather(1, t.clamp_min(0)[:, None])
        below = torch.arange(Vd)[None, :] < t[:, None]
        rank = (z > zt).sum(1) + ((z == zt) & below).sum(1)
        ok = (lm != 0) & (t >= 0)
        want.append(torch.stack([(ok & (rank < kk)).float().sum() for kk in topk]))
        pmc.append(float(b["pm"][:, k:k + S].sum()))
    return want, pmc


def _eval_counts(blob, dev, topk):
    """an eval forward with ``topk`` -> (metrics, the counts recomputed with torch from the logits it left, the position-mask counts)"""
    cfg, model, eagle, strat = _build(blob, dev)
    eagle.topk = topk
    eagle.eval()
    with torch.no_grad():
        out = strat.forward_loss(_batch(blob, dev))
    B, S = blob["batch"]["input_ids"].shape
    want, pmc = _torch_counts(eagle.engine, B, S, blob["d2t"], blob["t2d"].numel(), topk)
    assert len(eagle.last_topk) == eagle.engine.T
    return out, want, pmc, eagle


@pytest.mark.parametrize("name", GOLDENS)
def test_eval_forward_counts_match_torch(backend, golden_dir, name):
    blob = _load(golden_dir, name)
    Vd = blob["d2t"].numel()
    topk = (1, 2, 4, Vd)
    out, want, pmc, eagle = _eval_counts(blob, backend, topk)
    got = [t.cpu() for t in eagle.last_topk]
    print("topk_corrects", [g.tolist() for g in got])
    for k, g in enumerate(got):
        assert g.shape == (len(topk),) and torch.equal(g, want[k])
        assert float(g[0]) == float(out.metrics["acc_corrects"][k])                # rank 0 == the fused CE's correct rows
        assert float(g[-1]) == pmc[k]                                                # every scored target inside the draft vocabulary
        assert bool((g[1:] >= g[:-1]).all())
        for j, kk in enumerate(topk):
            assert float(out.metrics[f"top{kk}_corrects"][k]) == float(g[j]) and out.metrics[f"top{kk}_corrects"][k].dim() == 0
    assert sum(float(g[1]) > float(g[0]) for g in got) > 0                          # the case does tell top-2 from top-1


@pytest.mark.parametrize("name", GOLDENS + ["eagle3_lk_lambda_fp32"])
def test_training_step_is_bit_identical_with_and_without_topk(backend, golden_dir, name):
    """the rank kernel runs before the in-place gradient and disturbs nothing"""
    blob = _load(golden_dir, name)
    runs = []
    for topk in ((), (1, 2, 4, 8)):
        cfg, model, eagle, strat = _build(blob, backend)
        eagle.topk = topk
        eagle.train()
        out = strat.forward_loss(_batch(blob, backend))
        out.loss.backward()
        runs.append((out, eagle.engine.flat.grad.clone().cpu(), eagle))
        assert ("topk_met" in eagle.engine.arena_names()) == bool(topk) and ("topk_hit" in eagle.engine.arena_names()) == bool(topk)
    (a, ga, ea), (b, gb, eb) = runs
    assert ea.last_topk is None and not any(k.startswith("top") for k in a.metrics)
    assert torch.equal(a.loss.detach().cpu(), b.loss.detach().cpu()) and torch.equal(ga, gb)
    for key in a.metrics:
        assert torch.equal(torch.stack(a.metrics[key]).cpu(), torch.stack(b.metrics[key]).cpu()), key
    for k, g in enumerate(eb.last_topk):
        assert float(g[0]) == float(b.metrics["acc_corrects"][k])


@pytest.mark.parametrize("name,mask", [("eagle31_gqa_fp32", None), ("eagle31_gqa_fp32", "half"), ("eagle31_gqa_fp32", "head_only"),
                                       ("eagle3_tiny_fp32", "half"), ("eagle3_lk_lambda_fp32", "half")])
def test_counts_agree_across_variants(backend, golden_dir, name, mask):
    """eval (checked against torch) == training dense == training with loss-row compaction forced on; a loss mask with half the rows
    out; a step whose compact row count is 0; an LK objective"""
    blob = _load(golden_dir, name, mask)
    topk = (1, 2, 4, 8)
    out, want, pmc, eagle = _eval_counts(blob, backend, topk)
    for k, g in enumerate(eagle.last_topk):
        assert torch.equal(g.cpu(), want[k])
    for compact in (False, True):
        cfg, model, eagle, strat = _build(blob, backend)
        eagle.topk = topk
        eagle.train()
        eagle.engine.compact_loss_rows = compact
        batch = _batch(blob, backend)
        batch.metadata["loss_mask_suffix_counts"] = loss_mask_suffix_counts(blob["batch"]["loss_mask"])
        o = strat.forward_loss(batch)
        if mask is not None:       # the compact path did run (an LK objective compacts only on the stored-draft-logits form of the teacher)
            assert (eagle.engine._lm_compact_K is not None) == (compact and (eagle.engine.lk_loss_type is None or eagle.engine._soft[0] == "zt"))
        o.loss.backward()
        for k, g in enumerate(eagle.last_topk):
            assert torch.equal(g.cpu(), want[k]), (compact, k, g, want[k])
            assert float(g[0]) == float(o.metrics["acc_corrects"][k])
    if mask == "head_only":
        assert all(float(w.sum()) == 0.0 for w in want[3:])


@pytest.mark.parametrize("lk", [None, "lambda"])
def test_counts_with_the_reduced_teacher_and_compact_lk_rows(backend, lk):
    """a shape whose teacher takes the reduced head GEMM (stored draft logits; under the interpreter always): the training step with the
    defaults -- compact lm_head / CE / LK gradient rows, a teacher over the loss-mask positions only -- counts what the eval forward's
    logits give with torch"""
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead, TrainBatch
    from test_lk_reduced_teacher import KW, LK_KW, _case, _small_model

    B, S, T = 2, 288, 3
    topk = (1, 2, 4, 8)
    case = _case(B, S, 28, [S, 251])
    lm = (torch.rand(B, S, generator=torch.Generator().manual_seed(5)) < 0.4).to(case["batch"]["loss_mask"].dtype)
    counts = {}
    for train in (False, True):
        eagle = OnlineEagle3Model(_small_model(case, backend), length=T, lk_loss_type=lk, topk=topk, **LK_KW).train(train)
        strat = Eagle3TrainStrategy(eagle, target_head=TargetHead(case["head_w"].to(backend)))
        b = case["batch"]
        batch = TrainBatch(dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], loss_mask=lm, hidden_state=b["hidden_state"].to(backend),
                                target=b["target"].to(backend)), {"target_repr": "hidden_state", "loss_mask_suffix_counts": loss_mask_suffix_counts(lm)})
        with torch.set_grad_enabled(train):
            out = strat.forward_loss(batch)
        if train:
            if str(backend) == "cpu":
                assert eagle.engine._soft[0] == "zt" and eagle.engine._lm_compact_K is not None and eagle.engine._teacher_compacted
            out.loss.backward()
        else:
            want, _ = _torch_counts(eagle.engine, B, S, case["d2t"], KW["vocab_size"], topk)
        counts[train] = [g.cpu() for g in eagle.last_topk]
        for k, g in enumerate(counts[train]):
            assert torch.equal(g, want[k]), (train, k, g, want[k])
            assert float(g[0]) == float(out.metrics["acc_corrects"][k])
    assert float(sum(w.sum() for w in want)) > 0


def test_topk_setting_is_validated(golden_dir):
    from specforge_amd.engine import Eagle3Engine
    for bad in ((0, 1), (2, 1), (1, 1), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="topk"):
            Eagle3Engine._check_topk(bad)
    assert Eagle3Engine._check_topk([1, 2, 8]) == (1, 2, 8) and Eagle3Engine._check_topk(None) == ()


def test_accumulator_sums_before_the_ratio(backend, golden_dir):
    """two batches of different size: the rates are the ratio of the summed counts; simulated_acc_len_top1 is the reference
    Evaluator's a0 + a0*a1 + ... on the same rates"""
    blob = _load(golden_dir, "eagle3_tiny_fp32", "half")
    topk = (1, 2, 4)
    cfg, model, eagle, strat = _build(blob, backend)
    eagle.topk = topk
    eagle.eval()
    full = _batch(blob, backend)
    B = full.tensors["input_ids"].shape[0]
    assert B >= 2
    one = type(full)(tensors={k: v[:1] for k, v in full.tensors.items()}, metadata=dict(full.metadata))
    acc = TopKAccumulator(topk)
    assert acc.summary() == {}
    sums = {k: torch.zeros(eagle.length, dtype=torch.float64) for k in topk}
    den = torch.zeros(eagle.length, dtype=torch.float64)
    with torch.no_grad():
        for batch in (full, one):
            m = strat.forward_loss(batch).metrics
            acc.update(m)
            for k in topk:
                sums[k] += torch.stack(m[f"top{k}_corrects"]).double().cpu()
            den += torch.stack(m["acc_denoms"]).double().cpu()
    s = acc.summary()
    for k in topk:
        rates = (sums[k] / den.clamp_min(1.0)).tolist()
        for i, a in enumerate(rates):
            assert s[f"top{k}_acc_{i}"] == a
        cumulative, total = 1.0, 0.0
        for a in rates:                                  # eval/evaluator.py: _simulated_acc_len
            cumulative *= a
            total += cumulative
        assert s[f"simulated_acc_len_top{k}"] == total
    top1 = (sums[1] / den.clamp_min(1.0)).tolist()
    assert s["simulated_acc_len_top1"] <= s["simulated_acc_len_top2"] <= s["simulated_acc_len_top4"] and top1[0] > 0
