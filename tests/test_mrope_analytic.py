"""Analytic multimodal RoPE (``sf_rope_mrope`` / ``ops.rope_mrope`` / ``Eagle3Engine.mrope_analytic``): the angles are computed on the device
from the three-axis ids -- fp32 ``inv_freq * id``, accurate cos / sin, cast -- instead of gathered from a cos / sin table.

Kernel: the cos / sin it rotates with against float64 on the same fp32 angles, bit-for-bit agreement with ``sf_rope`` on per-token tables
holding those values, the backward as the transpose, negative ids, argument checks -- under the SIMT interpreter and on the GPU
(``backend``).  Engine: a tiny mrope draft against the pinned fp32 oracle, next to the table path; ids the table path refuses."""
import ctypes

import pytest
import torch

from oracle import eagle3_oracle as O
from specforge_amd import _lib, ops
from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead, TrainBatch
from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3, rope_inv_freq

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _lib._inject_library_for_tests(None)
    _lib.lib()
    return "cuda"


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------ kernel
SHAPES = [(4, 64), (2, 128), (1, 256), (3, 32)]          # (nheads, hd)
ROWS = [1, 3, 64, 257]
ID_SETS = ["small", "2^20", "2^24+1"]


def _axis(hd):
    """mrope_section [16, 24, 24] at hd 128, scaled alike for the others: which id axis channel pair d reads"""
    sec = [hd // 8, 3 * hd // 16, 3 * hd // 16]
    assert sum(sec) == hd // 2
    return torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(sec)])


def _inv_freq(hd):
    return 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))


def _ids(kind, R, seed):
    """[3, R] int64, the three axes different.  small: 1 .. 299; around 2^20; 2^24 + 1 and the odd and even ids above it, where the
    int64 -> fp32 conversion has to round (to nearest even)"""
    g = torch.Generator().manual_seed(seed)
    if kind == "small":
        return torch.randint(1, 300, (3, R), generator=g)
    if kind == "2^20":
        return (1 << 20) + torch.randint(-1000, 1000, (3, R), generator=g)
    p = (1 << 24) + 1 + torch.randint(0, 64, (3, R), generator=g)
    p[0, 0] = (1 << 24) + 1
    return p


def _reference(pos3, axis, inv, pos_off):
    """float64 cos / sin [R, hd/2] of the fp32 angle float(id + off) * inv_freq, and the worst absolute error of torch's own fp32
    cos / sin on those angles"""
    p = (pos3 + pos_off)[axis.long()].t()                     # [R, hd/2] int64
    ang = p.float() * inv[None, :]                            # .float(): round to nearest; one fp32 product
    c64, s64 = ang.double().cos(), ang.double().sin()
    err = max(float((ang.cos().double() - c64).abs().max()), float((ang.sin().double() - s64).abs().max()))
    return c64, s64, err


def _window(ref, E, dtype):
    """(lo, hi, near): the float64 values moved by 4 E either way and rounded to the dtype, and where the two differ -- the elements
    within the window of a rounding boundary"""
    lo, hi = (ref - 4 * E).float().to(dtype), (ref + 4 * E).float().to(dtype)
    return lo, hi, bits(lo) != bits(hi)


def _seeded_ids(kind, rows, hd, pos_off):
    """ids for case 1, the seed chosen FROM THE FLOAT64 REFERENCE ALONE (before any kernel runs) so that at most 1 % of the bf16
    elements lie within the window of a rounding boundary: with one row of 32 channels a single such element is 3 %"""
    axis, inv = _axis(hd), _inv_freq(hd)
    for seed in range(rows + hd, rows + hd + 64):
        pos3 = _ids(kind, rows, seed)
        c64, s64, E = _reference(pos3, axis, inv, pos_off)
        ref = torch.cat([c64, s64], -1)
        if float(_window(ref, E, BF)[2].float().mean()) <= 0.01:
            return pos3, ref, E
    raise AssertionError("no seed keeps the share of boundary elements under 1 %")


def _recover(dev, dtype, R, nheads, hd, pos3, pos_off, scale=1.0, backward=False, flag=None):
    """x = (1 | 0) per head: the forward leaves cos | sin of every channel in each head (backward: cos | -sin)"""
    x = torch.zeros(R, nheads, hd)
    x[..., :hd // 2] = 1.0
    x = x.view(R, nheads * hd).to(dtype).to(dev)
    ops.rope_mrope(x, nheads, hd, _inv_freq(hd).to(dev), _axis(hd).to(dev), pos3.to(dev), pos_off, scale, backward=backward, flag=flag)
    return x.cpu().view(R, nheads, hd)


@pytest.mark.parametrize("pos_off", [0, 6])
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("nheads,hd", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_cos_sin_recovered(backend, rows, nheads, hd, dtype, pos_off):
    """Case 1.  The cos / sin the kernel rotates with, against the float64 cos / sin of the fp32 product rounded to the dtype.  E = the
    worst error of torch's fp32 cos / sin against float64 on the same angles; window = 4 E (a GPU library a couple of ulps looser than
    the host's).  fp32: every element within the window.  bf16: equal bits, except where the float64 value lies within the window of a
    bf16 rounding boundary (then either neighbour) -- at most 1 % of the elements, asserted from the reference before the kernel runs.
    Every head holds the same values.
    Measured worst |kernel - float64| / E over the fp32 cases: interpreter 1.02 (the host's own sincosf), MI355X 2.37; bf16 elements off
    the rounded float64 value: interpreter 0, MI355X 2 of 936 000 (586 lie within the window)."""
    for kind in ID_SETS:
        pos3, ref, E = _seeded_ids(kind, rows, hd, pos_off)   # ref [R, hd] = cos | sin in float64
        assert 0 < E < 2.0 ** -22
        W = 4 * E
        lo, hi, near = _window(ref, E, dtype)
        if dtype == BF:
            share = float(near.float().mean())
            assert share <= 0.01, (kind, share)
        got = _recover(backend, dtype, rows, nheads, hd, pos3, pos_off)
        assert bool(torch.isfinite(got.float()).all())
        for h in range(1, nheads):
            assert torch.equal(bits(got[:, h]), bits(got[:, 0]))
        g = got[:, 0]
        worst = float((g.double() - ref).abs().max())
        if dtype == F32:
            print(f"mrope cos/sin fp32 {kind} rows={rows} hd={hd} off={pos_off}: worst error / E = {worst / E:.2f} (E = {E:.3e})")
            assert worst <= W, (kind, worst / E)
        else:
            exact = bits(g) == bits(ref.float().to(BF))
            nb = (bits(g) == bits(lo)) | (bits(g) == bits(hi))
            print(f"mrope cos/sin bf16 {kind} rows={rows} hd={hd} off={pos_off}: {int((~exact).sum())} of {exact.numel()} off the float64 "
                  f"rounding, {int(near.sum())} within 4 E of a boundary (E = {E:.3e})")
            assert bool((exact | (near & nb)).all()), (kind, int((~(exact | (near & nb))).sum()))


@pytest.mark.parametrize("dtype", [BF, F32])
def test_scale_multiplies_cos_and_sin(backend, dtype):
    """scale = 0.5 (an exact product): the recovered values are half those of scale 1, bit for bit after the cast"""
    R, nheads, hd = 5, 2, 64
    pos3 = _ids("2^20", R, 3)
    one = _recover(backend, dtype, R, nheads, hd, pos3, 2, 1.0)
    half = _recover(backend, dtype, R, nheads, hd, pos3, 2, 0.5)
    assert torch.equal(bits(half), bits((one.float() * 0.5).to(dtype)))


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("nheads,hd", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_same_bits_as_rope_on_per_token_tables(backend, rows, nheads, hd, dtype, backward):
    """Case 2.  Per-token tables built from the kernel's own cos / sin (case 1's recovery), handed to ``ops.rope_``: random x comes out
    with the same bits from both kernels, forward and backward, inside a wider buffer whose other columns stay untouched"""
    left, right = 16, 8
    for kind, pos_off in zip(ID_SETS, (0, 6, 6)):
        pos3 = _ids(kind, rows, seed=7 * rows + hd)
        rec = _recover(backend, dtype, rows, 1, hd, pos3, pos_off)[:, 0]                 # [R, hd] = cos | sin
        cos_rows = torch.cat([rec[:, :hd // 2]] * 2, -1).contiguous().to(backend)
        sin_rows = torch.cat([rec[:, hd // 2:]] * 2, -1).contiguous().to(backend)
        g = torch.Generator().manual_seed(rows + nheads)
        x = torch.randn(rows, left + nheads * hd + right, generator=g).to(dtype)
        a, b = x.clone().to(backend), x.clone().to(backend)
        va, vb = a[:, left:left + nheads * hd], b[:, left:left + nheads * hd]
        ops.rope_mrope(va, nheads, hd, _inv_freq(hd).to(backend), _axis(hd).to(backend), pos3.to(backend), pos_off, backward=backward)
        ops.rope_(vb, nheads, hd, cos_rows, sin_rows, torch.arange(rows).to(backend), 0, backward=backward)
        assert torch.equal(bits(a), bits(b)), (kind, int((bits(a) != bits(b)).sum()))
        assert torch.equal(bits(a[:, :left]), bits(x[:, :left])) and torch.equal(bits(a[:, left + nheads * hd:]), bits(x[:, left + nheads * hd:]))
        assert not torch.equal(bits(va), bits(x[:, left:left + nheads * hd]))


@pytest.mark.parametrize("nheads,hd", SHAPES)
@pytest.mark.parametrize("rows", [3, 257])
def test_backward_is_the_transpose(backend, rows, nheads, hd):
    """Case 3.  <y, R x> == <R^T y, x> in float64 from fp32 runs, to 1e-5 of the sum of the products' magnitudes (the bar of
    test_rope_backward_is_the_transpose_of_forward)"""
    pos3 = _ids("2^20", rows, seed=hd)
    g = torch.Generator().manual_seed(hd + rows)
    x, y = torch.randn(rows, nheads * hd, generator=g), torch.randn(rows, nheads * hd, generator=g)
    d = lambda t: t.to(backend)
    args = (nheads, hd, d(_inv_freq(hd)), d(_axis(hd)), d(pos3), 6)
    fx = ops.rope_mrope(d(x.clone()), *args).cpu().double()
    by = ops.rope_mrope(d(y.clone()), *args, backward=True).cpu().double()
    lhs, rhs = float((fx * y.double()).sum()), float((x.double() * by).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((fx * y.double()).abs().sum())


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("pos_off", [0, 6])
@pytest.mark.parametrize("nheads,hd", SHAPES)
def test_negative_id_row_is_flagged_not_rotated(backend, nheads, hd, dtype, pos_off, backward):
    """Case 4.  One row with id -1 - pos_off on one axis (negative after the offset; with pos_off 6 a second row holds -1, which the
    offset makes valid): the flag becomes 1, every output is finite, and every other row has the bits of a run without that row.
    Without a negative id the flag stays 0."""
    R, bad = 64, 37
    pos3 = _ids("small", R, seed=hd)
    pos3[1, bad] = -1 - pos_off
    if pos_off:
        pos3[2, 5] = -1
    g = torch.Generator().manual_seed(hd)
    x = torch.randn(R, nheads * hd, generator=g).to(dtype)
    d = lambda t: t.to(backend)
    inv, axis = d(_inv_freq(hd)), d(_axis(hd))
    flag = torch.zeros(1, device=backend)
    got = ops.rope_mrope(d(x.clone()), nheads, hd, inv, axis, d(pos3), pos_off, backward=backward, flag=flag).cpu()
    assert float(flag.cpu()) == 1.0
    assert bool(torch.isfinite(got.float()).all())
    keep = torch.arange(R) != bad
    flag2 = torch.zeros(1, device=backend)
    ref = ops.rope_mrope(d(x[keep].clone()), nheads, hd, inv, axis, d(pos3[:, keep].contiguous()), pos_off, backward=backward, flag=flag2).cpu()
    assert float(flag2.cpu()) == 0.0
    assert torch.equal(bits(got[keep]), bits(ref))
    assert not torch.equal(bits(ref), bits(x[keep]))
    # no flag pointer: the row is left finite all the same
    got3 = ops.rope_mrope(d(x.clone()), nheads, hd, inv, axis, d(pos3), pos_off, backward=backward).cpu()
    assert torch.equal(bits(got3), bits(got))


def test_argument_checks(backend):
    """Case 5.  rows == 0 returns 0 and writes nothing; a head_dim that is no multiple of 16 and a row stride that is no multiple of 8
    are refused by sf_rope_mrope as by sf_rope"""
    L = _lib.lib()
    hd, nheads, R = 64, 2, 4
    d = lambda t: t.to(backend)
    x = d(torch.full((R, nheads * hd), 7.5, dtype=BF))
    inv, axis, pos3 = d(_inv_freq(hd)), d(_axis(hd)), d(_ids("small", R, 1))
    flag = torch.zeros(1, device=backend)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda rows, hd_, ld: L.sf_rope_mrope(p(x), 0, ld, rows, nheads, hd_, p(inv), p(axis), p(pos3), 0, 1.0, 0, p(flag), ops._stream())
    assert call(0, hd, nheads * hd) == 0
    assert bool((x.cpu() == 7.5).all()) and float(flag.cpu()) == 0.0
    empty = ops.rope_mrope(x[:0], nheads, hd, inv, axis, pos3[:, :0].contiguous(), 0)
    assert empty.shape[0] == 0 and bool((x.cpu() == 7.5).all())
    cos = d(torch.ones(8, hd, dtype=BF))
    pos = d(torch.arange(R))
    rope = lambda hd_, ld: L.sf_rope(p(x), 0, ld, R, nheads, hd_, p(cos), p(cos), p(pos), 0, 8, 0, ops._stream())
    for hd_, ld in ((24, nheads * hd), (hd, nheads * hd + 4)):
        assert rope(hd_, ld) != 0
        assert call(R, hd_, ld) != 0 and b"sf_rope_mrope" in L.sf_last_error()
    assert bool((x.cpu() == 7.5).all())
    with pytest.raises(_lib.SfError, match="sf_rope_mrope"):
        ops.rope_mrope(d(torch.zeros(R, nheads * hd + 4, dtype=BF))[:, :nheads * hd], nheads, hd, inv, axis, pos3, 0)


# ------------------------------------------------------------------ engine
T_, B_, S_ = 3, 2, 48
LENGTHS = [48, 37]            # ragged attention mask


def _cfg_kw(hd=64, rope_scaling="mrope", lk=None):
    sec = [hd // 8, 3 * hd // 16, 3 * hd // 16]
    rs = {"rope_type": "mrope", "mrope_section": sec} if rope_scaling == "mrope" else rope_scaling
    return dict(hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=1, vocab_size=96, draft_vocab_size=32,
                head_dim=hd, target_hidden_size=64, max_position_embeddings=64, rms_norm_eps=1e-5, rope_scaling=rs)


def _pos3(shift=0):
    """[3, B, S] ids, the three axes different (temporal / height / width in the manner of an image span), all >= 0"""
    s = torch.arange(S_)
    t = torch.stack([s, s // 2 + 3, (s * 3) % 17 + 1])                                   # [3, S]
    return torch.stack([t, t.flip(0) + 2], 1).contiguous() + shift                       # [3, B, S]


_CASES = {}


def _case(hd=64, lk=None, rope_scaling="mrope"):
    """weights, batch and teacher head of the tiny draft (bf16-representable), built once per variant and never modified"""
    key = (hd, lk, str(rope_scaling))
    if key not in _CASES:
        kw = _cfg_kw(hd, rope_scaling)
        oc = O.DraftConfig(**kw)
        params = {k: v.to(BF) for k, v in O.init_params(oc, seed=3).items()}
        g = torch.Generator().manual_seed(4)
        embed = (torch.randn(96, 64, generator=g) * 0.05).to(BF)
        head_w = (torch.randn(96, 64, generator=g) * 0.3).to(BF)
        t2d, d2t = O.make_vocab_mapping(96, 32, seed=1)
        batch = O.make_batch(oc, B_, S_, seed=5, dtype=BF, lengths=LENGTHS)
        _CASES[key] = dict(kw=kw, oc=oc, params=params, embed=embed, head_w=head_w, t2d=t2d, d2t=d2t, batch=batch, lk=lk)
    return _CASES[key]


_ORACLE = {}


def _oracle(case, pos, tag):
    """the pinned oracle in fp32 on the same (bf16-representable) weights and inputs; computed once per (case, ids)"""
    key = (id(case), tag)
    if key not in _ORACLE:
        p = {k: v.float().clone().requires_grad_(True) for k, v in case["params"].items()}
        b = case["batch"]
        out = O.eagle3_forward(p, case["oc"], embed_weight=case["embed"].float(), target_head_weight=case["head_w"].float(),
                               t2d=case["t2d"], d2t=case["d2t"], input_ids=b["input_ids"], attention_mask=b["attention_mask"],
                               loss_mask=b["loss_mask"], hidden_state=b["hidden_state"].float(), target_hidden=b["target"].float(),
                               ttt_length=T_, position_ids=pos, lk_loss_type=case["lk"])
        out.loss.backward()
        _ORACLE[key] = dict(plosses=torch.stack([x.detach() for x in out.plosses]), acces=torch.stack(out.acces).float(),
                            denoms=torch.stack(out.acc_denoms).float(), grads={k: v.grad.detach() for k, v in p.items()})
    return _ORACLE[key]


def _build(case, dev, analytic):
    model = LlamaForCausalLMEagle3(DraftConfig(**case["kw"]), device=dev)
    sd = dict(case["params"])
    sd["embed_tokens.weight"], sd["t2d"], sd["d2t"] = case["embed"], case["t2d"], case["d2t"]
    model.load_state_dict(sd)
    eagle = OnlineEagle3Model(model, length=T_, lk_loss_type=case["lk"], mrope_analytic=analytic).train()
    return model, eagle, Eagle3TrainStrategy(eagle, target_head=TargetHead(case["head_w"].to(dev)))


def _tensors(case, dev, pos):
    b = case["batch"]
    t = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], loss_mask=b["loss_mask"],
             hidden_state=b["hidden_state"].to(dev), target=b["target"].to(dev))
    if pos is not None:
        t["position_ids"] = pos
    return TrainBatch(t, {"target_repr": "hidden_state"})


def _run(case, dev, analytic, pos):
    model, eagle, strat = _build(case, dev, analytic)
    out = strat.forward_loss(_tensors(case, dev, pos))
    out.loss.backward()
    res = dict(plosses=torch.stack(out.metrics["plosses"]).float().cpu(), acces=torch.stack(out.metrics["acces"]).float().cpu(),
               grads={k: p.grad.float().cpu() for k, p in model.named_parameters() if p.grad is not None},
               flat=eagle.engine.flat.grad.clone().cpu())
    return res, eagle


def _distances(res, ref):
    """to the oracle: plosses (max abs), accuracies (in tokens), every gradient (max abs over the tensor's largest oracle entry)"""
    d = {"plosses": float((res["plosses"] - ref["plosses"]).abs().max()),
         "acces": float(((res["acces"] - ref["acces"]).abs() * ref["denoms"]).max())}
    for k, g in ref["grads"].items():
        d[k] = float((res["grads"][k] - g).abs().max()) / float(g.abs().max().clamp_min(1e-8))
    return d


# the absolute floors of tests/test_engine_golden.py: 2e-2 on losses, one token on an accuracy (a bf16 near-tie of the draft's argmax),
# 4e-3 of a gradient's largest entry between two forms of the same computation
FLOORS = {"plosses": 2e-2, "acces": 1.0 + 1e-3}
GRAD_FLOOR = 4e-3


def _assert_no_farther(an, tb, what):
    """the analytic path's distance to the oracle <= 1.5 x the table path's + the floor: the two rotate with cos / sin that differ by one
    rounding on the small share of elements of case 1, everything else is the same computation"""
    da, dt = _distances(an, what), _distances(tb, what)
    for k in da:
        print(f"  {k}: analytic {da[k]:.3e}  table {dt[k]:.3e}")
    bad = {k: (da[k], dt[k]) for k in da if da[k] > 1.5 * dt[k] + FLOORS.get(k, GRAD_FLOOR)}
    assert not bad, bad
    assert all(bool(torch.isfinite(g).all()) for g in an["grads"].values())


@pytest.mark.parametrize("hd,lk", [(64, None), (32, None), (64, "alpha")])
def test_ids_inside_the_table_match_the_table_path(backend, hd, lk):
    """Case 6.  ids the table holds: both paths against the fp32 oracle on plosses, accuracies and every gradient; hd 32 runs the
    zero-padded heads, lk 'alpha' an LK objective"""
    case, pos = _case(hd, lk), _pos3()
    ref = _oracle(case, pos, "inside")
    an, _ = _run(case, backend, True, pos)
    tb, _ = _run(case, backend, False, pos)
    _assert_no_farther(an, tb, ref)


def test_device_ids_beyond_the_table_train(backend):
    """Case 7.  ids up to 5000: as a device tensor with no position_span the default engine refuses them in backward (they do not fit
    its table); the analytic engine trains, and agrees with a default engine given the same ids as a CPU tensor (its table grows)"""
    case, pos = _case(), _pos3(shift=4950)
    assert int(pos.max()) >= 5000 - 1
    ref = _oracle(case, pos, "5000")
    if backend != "cpu":         # (under the interpreter every tensor is host memory: ids are always host-known there)
        model, eagle, strat = _build(case, backend, False)
        with pytest.raises(RuntimeError, match="position_ids"):
            strat.forward_loss(_tensors(case, backend, pos.to(backend))).loss.backward()
    an, eagle = _run(case, backend, True, pos.to(backend))
    assert eagle.engine.cos.shape[0] == 64 + 20
    tb, eagle_t = _run(case, backend, False, pos)
    assert eagle_t.engine.cos.shape[0] > 5000
    _assert_no_farther(an, tb, ref)


def test_host_known_ids_beyond_the_cap_train(backend):
    """Case 8.  host-known ids past the table path's cap (the larger of 64 x (max_position_embeddings + 20) and
    Eagle3Engine.max_rope_positions): ValueError there; the analytic engine trains and its table is what it was"""
    case = _case()
    model, eagle, strat = _build(case, backend, False)
    eng = eagle.engine
    cap = max(eng.max_rope_positions, 64 * (64 + 20))
    pos = _pos3(shift=cap)
    with pytest.raises(ValueError, match="mrope"):
        strat.forward_loss(_tensors(case, backend, pos))
    an, eagle = _run(case, backend, True, pos)
    assert eagle.engine.cos.shape[0] == 64 + 20
    assert bool(torch.isfinite(an["plosses"]).all()) and bool(torch.isfinite(an["flat"].float()).all())
    assert float(an["flat"].float().abs().max()) > 0
    # the same ids on every axis shifted by a whole table: another rotation, another loss
    inside, _ = _run(case, backend, True, _pos3())
    assert not torch.equal(inside["plosses"], an["plosses"])


def test_host_known_negative_ids_are_refused(backend):
    """Case 9a.  a negative id in a CPU tensor, or announced through position_span: ValueError on both paths"""
    case = _case()
    neg = _pos3()
    neg[1, 0, 5] = -2
    for analytic in (False, True):
        model, eagle, strat = _build(case, backend, analytic)
        with pytest.raises(ValueError, match="mrope"):
            strat.forward_loss(_tensors(case, backend, neg))
        b = case["batch"]
        with pytest.raises(ValueError, match="mrope"):
            eagle(input_ids=b["input_ids"], attention_mask=b["attention_mask"], loss_mask=b["loss_mask"][..., None],
                  hidden_states=b["hidden_state"].to(backend), target_hidden_for_compact=b["target"].to(backend),
                  target_head_weight=case["head_w"].to(backend), position_ids=_pos3().to(backend), position_span=(-2, 60))


@pytest.mark.gpu
def test_device_only_negative_ids_fail_in_backward(gpu):
    """Case 9b.  a negative id that exists only on the device: the kernel zeroes the row and sets the flag, backward raises -- and
    nothing non-finite was written into the flat gradient before it"""
    case = _case()
    neg = _pos3()
    neg[1, 0, 5] = -2
    model, eagle, strat = _build(case, gpu, True)
    out = strat.forward_loss(_tensors(case, gpu, neg.to(gpu)))
    assert bool(torch.isfinite(torch.stack(out.metrics["plosses"]).float()).all())
    with pytest.raises(RuntimeError, match="position_ids"):
        out.loss.backward()
    assert bool(torch.isfinite(eagle.engine.flat.grad.float()).all())
    # the eval forward pays the read-back itself
    eagle.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="position_ids"):
        strat.forward_loss(_tensors(case, gpu, neg.to(gpu)))
    # and a clean batch afterwards trains: the flag does not stick
    eagle.train()
    strat.forward_loss(_tensors(case, gpu, _pos3().to(gpu))).loss.backward()


def test_arena_has_no_per_token_tables(backend):
    """Case 10.  after an analytic forward the arena holds the ids once ([3, N]) and none of the per-step cos / sin rows; it is smaller
    than the table engine's at the same shape.  Switching an engine over drops the other path's buffers."""
    case, pos = _case(), _pos3()
    _, ea = _run(case, backend, True, pos)
    _, et = _run(case, backend, False, pos)
    names_a, names_t = ea.engine.arena_names(), et.engine.arena_names()
    assert not [n for n in names_a if n.startswith(("cos_rows", "sin_rows"))] and "pos3" in names_a
    assert {f"cos_rows_{k}" for k in range(T_)} | {f"sin_rows_{k}" for k in range(T_)} <= set(names_t) and "pos3" not in names_t
    assert ea.engine.arena_bytes() < et.engine.arena_bytes()
    assert set(names_t) - set(names_a) == {f"{p}_rows_{k}" for p in ("cos", "sin") for k in range(T_)}
    et.engine.mrope_analytic = True
    assert not [n for n in et.engine.arena_names() if n.startswith(("cos_rows", "sin_rows"))]


def test_usp_with_mrope_is_still_refused(emu_lib_path, monkeypatch):
    """Case 11a.  attention_backend 'usp' refuses rope_type 'mrope' with the same message, whatever mrope_analytic says"""
    import specforge_amd.engine as E

    _lib._inject_library_for_tests(emu_lib_path)
    try:
        monkeypatch.setattr(E.dist, "get_world_size", lambda g=None: 2)
        monkeypatch.setattr(E.dist, "get_rank", lambda g=None: 0)
        monkeypatch.setattr(E.dist, "get_backend", lambda g=None: "gloo")
        msgs = []
        for analytic in (False, True):
            model = LlamaForCausalLMEagle3(DraftConfig(**dict(_cfg_kw(), num_key_value_heads=2)))     # (heads the SP size divides)
            with pytest.raises(ValueError, match="mrope") as ei:
                E.Eagle3Engine(model, ttt_length=T_, sp_group=object(), mrope_analytic=analytic)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1] and "not supported with attention_backend 'usp'" in msgs[0]
    finally:
        _lib._inject_library_for_tests(None)


@pytest.mark.parametrize("rope_scaling", [None, dict(rope_type="linear", factor=2.0)])
def test_switch_changes_nothing_without_mrope(backend, rope_scaling):
    """Case 11b.  mrope_analytic=True on a config that is not mrope: bit-equal losses and gradients, the same buffers"""
    case = _case(rope_scaling=rope_scaling)
    on, eo = _run(case, backend, True, None)
    off, ef = _run(case, backend, False, None)
    assert torch.equal(on["plosses"], off["plosses"]) and torch.equal(bits(on["flat"]), bits(off["flat"]))
    assert eo.engine.arena_names() == ef.engine.arena_names() and eo.engine.arena_bytes() == ef.engine.arena_bytes()


def test_both_paths_start_from_the_same_numbers():
    """inv_freq and the amplitude factor of the analytic path are those ``rope_tables`` builds the table from: the table's angles are
    float(position) * inv_freq, so its fp32 rows are cos / sin of exactly the products the kernel forms"""
    from specforge_amd.model import rope_tables

    cfg = DraftConfig(**_cfg_kw())
    inv, amp = rope_inv_freq(cfg)
    assert amp == 1.0 and inv.dtype == F32 and inv.numel() == 32
    cos, sin = rope_tables(cfg, F32)
    ang = torch.arange(cos.shape[0], dtype=F32)[:, None] * inv[None, :]
    assert torch.equal(cos[:, :32], ang.cos()) and torch.equal(sin[:, 32:], ang.sin())
