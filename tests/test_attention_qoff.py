"""TTT attention with a query offset (ring sequence parallelism; include/specforge_amd.h: sf_attn_fwd_off and friends).

A sequence is cut into contiguous "ranks".  A rank's launch takes its own query rows [q_off, q_off + Sq) and the step-0 keys
[0, q_off + Sq), and must give:
  * forward O / LSE and dQ = the rows [q_off, q_off + Sq) of the unsharded kernels -- bit for bit when q_off and Sq are multiples of
    the 128-query block (the same key tiles are visited in the same order by the same waves);
  * dK / dV summed over the ranks = the unsharded dK / dV up to fp32 summation order;
  * q_off = 0 through the new entry points = the existing entry points, bit for bit;
and the concatenated result matches the oracle's restatement (oracle/eagle3_oracle.py::ttt_attention) at test_attention.py's bars.

With an unaligned q_off the waves hold other query rows than in the unsharded launch.  A wave defers its softmax rescale until
some row's maximum grew by more than 2^8 (sf_attn.hip), so a row may be exponentiated against another running maximum; the
probabilities are rounded to bf16 for the PV / dS MFMAs, so the results move by bf16 rounding of P, not by more.
"""
import math

import pytest
import torch

from oracle import eagle3_oracle as O
from specforge_amd import ops

from test_attention import _mk, _oracle


def _flat(t, B, S):
    return t.reshape(B * S, -1)


def _unsharded(backend, q, ks, vs, do, B, S, nh, nkv, hd, kv_len):
    """the existing kernels over the whole sequence: o, lse, dq, dk0, dv0 (fp32), the diagonal branches' dk / dv"""
    d = lambda t: t.to(backend)
    scale = 1.0 / math.sqrt(hd)
    n = len(ks)
    qv, dout = d(_flat(q, B, S)), d(_flat(do, B, S))
    K, V = [d(_flat(k, B, S)) for k in ks], [d(_flat(v, B, S)) for v in vs]
    o = torch.empty(B * S, nh * hd, dtype=torch.bfloat16, device=backend)
    lse = torch.empty(B, nh, S, device=backend)
    ops.attn_fwd(qv, K[0], V[0], K[1:], V[1:], kv_len, o, lse, B=B, S=S, nh=nh, nkv=nkv, hd=hd, scale=scale)
    delta = torch.empty(B, nh, S, device=backend)
    dq_init = torch.zeros(B * S, nh * hd, device=backend) if n > 1 else None
    dk = [torch.zeros(B * S, nkv * hd, device=backend) for _ in range(n)]
    dv = [torch.zeros(B * S, nkv * hd, device=backend) for _ in range(n)]
    ops.attn_bwd_pre(qv, o, dout, K[1:], V[1:], dk[1:], dv[1:], lse, delta, dq_init, B=B, S=S, nh=nh, nkv=nkv, hd=hd, scale=scale)
    dq = torch.empty(B * S, nh * hd, dtype=torch.bfloat16, device=backend)
    ops.attn_bwd_dq(qv, dout, K[0], V[0], kv_len, lse, delta, dq_init, dq, B=B, S=S, nh=nh, nkv=nkv, hd=hd, scale=scale)
    ws = torch.empty(max(1, ops.attn_bwd_dkv_workspace_floats(B, S, nh, nkv, hd)), device=backend)
    ops.attn_bwd_dkv(qv, dout, K[0], V[0], kv_len, lse, delta, dk[0], dv[0], B=B, S=S, nh=nh, nkv=nkv, hd=hd, scale=scale,
                     workspace=ws)
    return dict(o=o.cpu(), lse=lse.cpu(), dq=dq.cpu(), dk=[t.cpu() for t in dk], dv=[t.cpu() for t in dv])


def _shard(backend, q, ks, vs, do, B, q_off, Sq, nh, nkv, hd, kv_len, *, entry="off"):
    """one rank: queries / diagonal branches / dO rows [q_off, q_off + Sq), step-0 keys [0, q_off + Sq).  entry "plain" runs the
    existing entry points (q_off must be 0)"""
    d = lambda t: t.to(backend)
    scale = 1.0 / math.sqrt(hd)
    n = len(ks)
    SK = q_off + Sq
    rows = lambda t: d(t[:, q_off:SK].reshape(B * Sq, -1))
    qv, dout = rows(q), rows(do)
    Kd, Vd = [rows(k) for k in ks[1:]], [rows(v) for v in vs[1:]]
    k0, v0 = d(ks[0][:, :SK].reshape(B * SK, -1)), d(vs[0][:, :SK].reshape(B * SK, -1))
    o = torch.empty(B * Sq, nh * hd, dtype=torch.bfloat16, device=backend)
    lse = torch.empty(B, nh, Sq, device=backend)
    kw = dict(B=B, nh=nh, nkv=nkv, hd=hd, scale=scale)
    if entry == "off":
        ops.attn_fwd_off(qv, k0, v0, Kd, Vd, kv_len, o, lse, S=Sq, q_off=q_off, **kw)
    else:
        assert q_off == 0
        ops.attn_fwd(qv, k0, v0, Kd, Vd, kv_len, o, lse, S=Sq, **kw)
    delta = torch.empty(B, nh, Sq, device=backend)
    dq_init = torch.zeros(B * Sq, nh * hd, device=backend) if n > 1 else None
    dkd = [torch.zeros(B * Sq, nkv * hd, device=backend) for _ in range(n - 1)]
    dvd = [torch.zeros(B * Sq, nkv * hd, device=backend) for _ in range(n - 1)]
    ops.attn_bwd_pre(qv, o, dout, Kd, Vd, dkd, dvd, lse, delta, dq_init, S=Sq, **kw)
    dq = torch.empty(B * Sq, nh * hd, dtype=torch.bfloat16, device=backend)
    dk0 = torch.zeros(B * SK, nkv * hd, device=backend)
    dv0 = torch.zeros(B * SK, nkv * hd, device=backend)
    if entry == "off":
        ops.attn_bwd_dq_off(qv, dout, k0, v0, kv_len, lse, delta, dq_init, dq, S=Sq, q_off=q_off, **kw)
        ws = torch.empty(max(1, ops.attn_bwd_dkv_off_workspace_floats(B, Sq, q_off, nh, nkv, hd)), device=backend)
        ops.attn_bwd_dkv_off(qv, dout, k0, v0, kv_len, lse, delta, dk0, dv0, S=Sq, q_off=q_off, workspace=ws, **kw)
    else:
        ops.attn_bwd_dq(qv, dout, k0, v0, kv_len, lse, delta, dq_init, dq, S=Sq, **kw)
        ws = torch.empty(max(1, ops.attn_bwd_dkv_workspace_floats(B, Sq, nh, nkv, hd)), device=backend)
        ops.attn_bwd_dkv(qv, dout, k0, v0, kv_len, lse, delta, dk0, dv0, S=Sq, workspace=ws, **kw)
    return dict(o=o.cpu(), lse=lse.cpu(), dq=dq.cpu(), dk0=dk0.cpu(), dv0=dv0.cpu(), dkd=[t.cpu() for t in dkd],
                dvd=[t.cpu() for t in dvd])


def _bf16_ulps(got, ref):
    """largest difference in units of the bf16 spacing at the reference's magnitude (0 = identical)"""
    got, ref = got.float(), ref.float()
    spacing = torch.where(ref == 0, torch.full_like(ref, 2.0 ** -133),
                          torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))) * 2.0 ** -7)
    return float(((got - ref).abs() / spacing).max())


def _run(backend, B, bounds, nh, nkv, hd, nsteps, lengths, seed, *, aligned, fp32_rel):
    """``bounds``: the ranks' first rows and the sequence length, e.g. [0, 128, 256]"""
    S = bounds[-1]
    q, ks, vs, do = _mk(B, S, nh, nkv, hd, nsteps, seed=seed)
    kv_len = torch.tensor(lengths, dtype=torch.int32).to(backend)
    full = _unsharded(backend, q, ks, vs, do, B, S, nh, nkv, hd, kv_len)
    row = lambda t, a, e: t.view(B, S, -1)[:, a:e].reshape(B * (e - a), -1)
    dk_sum = torch.zeros(B, S, nkv * hd)
    dv_sum = torch.zeros(B, S, nkv * hd)
    worst = dict(o=0.0, dq=0.0, lse=0.0)
    outs = []
    for a, e in zip(bounds[:-1], bounds[1:]):
        r = _shard(backend, q, ks, vs, do, B, a, e - a, nh, nkv, hd, kv_len)
        outs.append(r)
        for name in ("o", "dq"):
            ref = row(full[name], a, e)
            if aligned:
                assert torch.equal(r[name], ref), (name, a, e)
            worst[name] = max(worst[name], _bf16_ulps(r[name], ref))
        lse_ref = full["lse"][:, :, a:e]
        if aligned:
            assert torch.equal(r["lse"], lse_ref), ("lse", a, e)
        worst["lse"] = max(worst["lse"], float((r["lse"] - lse_ref).abs().max()))
        for i in range(nsteps - 1):         # the diagonal branches are per token: local rows of the unsharded sums
            if aligned:
                assert torch.equal(r["dkd"][i], row(full["dk"][i + 1], a, e)) and torch.equal(r["dvd"][i], row(full["dv"][i + 1], a, e))
        dk_sum[:, :e] += r["dk0"].view(B, e, -1)
        dv_sum[:, :e] += r["dv0"].view(B, e, -1)
    for got, ref, what in ((dk_sum, full["dk"][0].view(B, S, -1), "dk0"), (dv_sum, full["dv"][0].view(B, S, -1), "dv0")):
        err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        worst[what] = err
        assert err <= fp32_rel, (what, err, fp32_rel)
    for b, L in enumerate(lengths):       # keys at / after kv_len: exactly zero
        assert float(dk_sum[b, L:].abs().max() if L < S else 0.0) == 0.0
    return q, ks, vs, do, outs, worst


# ---- interpreter sizes (and the same on the GPU): 128-aligned ranks are bit-identical; the oracle on the concatenation ----------
@pytest.mark.parametrize("hd", [64, 128, 256])
@pytest.mark.parametrize("nh,nkv,nsteps,lengths", [
    (2, 2, 1, [256]),       # GQA 1, no diagonal branch, full length
    (4, 1, 4, [256]),       # GQA 4, 3 diagonal branches
    (2, 2, 4, [200]),       # kv_len inside the last rank's own block
    (4, 1, 1, [100]),       # kv_len inside an earlier block: the last rank's queries see only rank 0's keys
])
def test_qoff_aligned_ranks_equal_unsharded_rows(backend, hd, nh, nkv, nsteps, lengths):
    B, bounds = 1, [0, 128, 256]      # dK / dV summed over the ranks: measured <= 1.6e-7 of max |dK| on the interpreter (bar 4e-7)
    q, ks, vs, do, outs, worst = _run(backend, B, bounds, nh, nkv, hd, nsteps, lengths, seed=hd + 7 * nsteps + lengths[0],
                                      aligned=True, fp32_rel=4e-7)
    # the oracle on the concatenated sequence (test_attention.py's bars)
    S = bounds[-1]
    o_ref, dq_ref, dk_ref, dv_ref = _oracle(q, ks, vs, do, B, S, nh, nkv, hd, lengths)
    o = torch.cat([r["o"] for r in outs])
    dq = torch.cat([r["dq"] for r in outs])
    torch.testing.assert_close(o.float(), o_ref, rtol=2e-2, atol=2e-2)
    tol = lambda ref: 3e-2 * float(ref.abs().max()) + 1e-6
    assert float((dq.float() - dq_ref).abs().max()) <= tol(dq_ref)
    for i in range(1, nsteps):
        dki = torch.cat([r["dkd"][i - 1] for r in outs])
        assert float((dki - dk_ref[i]).abs().max()) <= tol(dk_ref[i])


@pytest.mark.parametrize("hd", [64, 128, 256])
def test_qoff_unaligned_ranks(backend, hd):
    """chunk = ceil(S / sp) is rarely a multiple of 128: three ranks of 100 rows, two samples of different lengths.  O / dQ move by bf16
    rounding of P only (module docstring); measured 0 ulp on the interpreter and on an MI355X at these sizes -- bound: 1 bf16 ulp of
    the reference's magnitude.  dK / dV summed over the ranks: measured <= 1.9e-7 of max |dK| on the interpreter (bar 4e-7)"""
    B, bounds, nh, nkv, nsteps = 2, [0, 100, 200, 300], 4, 2, 3
    _, _, _, _, _, worst = _run(backend, B, bounds, nh, nkv, hd, nsteps, [300, 170], seed=hd, aligned=False, fp32_rel=4e-7)
    assert worst["o"] <= 1.0 and worst["dq"] <= 1.0, worst


@pytest.mark.parametrize("hd", [64, 128, 256])
def test_qoff_zero_is_the_existing_entry_points(backend, hd):
    B, S, nh, nkv, nsteps = 2, 150, 8, 2, 3
    q, ks, vs, do = _mk(B, S, nh, nkv, hd, nsteps, seed=3 * hd)
    kv_len = torch.tensor([150, 97], dtype=torch.int32).to(backend)
    a = _shard(backend, q, ks, vs, do, B, 0, S, nh, nkv, hd, kv_len, entry="plain")
    b = _shard(backend, q, ks, vs, do, B, 0, S, nh, nkv, hd, kv_len, entry="off")
    for name in ("o", "lse", "dq", "dk0", "dv0"):
        assert torch.equal(a[name], b[name]), name
    assert ops.attn_bwd_dkv_off_workspace_floats(B, S, 0, nh, nkv, hd) == ops.attn_bwd_dkv_workspace_floats(B, S, nh, nkv, hd)
    assert ops.attn_bwd_dkv_off_workspace_floats(1, 100, 4000, 32, 8, 128) == ops.attn_bwd_dkv_workspace_floats(1, 4100, 32, 8, 128)


def test_qoff_argument_checks(emu_lib_path):
    import ctypes

    from specforge_amd import _lib

    _lib._inject_library_for_tests(emu_lib_path)
    try:
        L = _lib.lib()
        a = torch.zeros(8, 8, dtype=torch.bfloat16)
        p = ctypes.c_void_p(a.data_ptr())
        st = L.sf_attn_fwd_off(p, 128, p, 128, p, None, None, 0, None, p, 128, p, 1, 64, -1, 1, 1, 128, 1.0, None)
        assert st != 0 and b"q_off" in L.sf_last_error()
        st = L.sf_attn_bwd_dq_off(p, 128, p, 128, p, 128, p, 128, None, p, p, None, p, 128, 1, 64, -5, 1, 1, 128, 1.0, None)
        assert st != 0 and b"q_off" in L.sf_last_error()
        st = L.sf_attn_bwd_dkv_off(p, 128, p, 128, p, 128, p, 128, None, p, p, p, p, 128, 1, 64, -5, 1, 1, 128, 1.0, None, 0, None)
        assert st != 0 and b"q_off" in L.sf_last_error()
        # the key buffer holds q_off + Sq rows: its 2 GiB descriptor bound counts them all
        st = L.sf_attn_fwd_off(p, 1 << 12, p, 1 << 12, p, None, None, 0, None, p, 1 << 12, p, 1, 64, 1 << 18, 1, 1, 128, 1.0, None)
        assert st != 0 and b"2 GiB" in L.sf_last_error()
        st = L.sf_attn_bwd_dq_off(p, 1 << 12, p, 1 << 12, p, 1 << 12, p, 1 << 12, None, p, p, None, p, 1 << 12, 1, 64, 1 << 18, 1, 1,
                                  128, 1.0, None)
        assert st != 0 and b"2 GiB" in L.sf_last_error()
        assert L.sf_attn_bwd_dkv_off_workspace_floats(1, 64, -1, 4, 1, 128) == 0
    finally:
        _lib._inject_library_for_tests(None)


# ---- real sizes on the GPU: Sq 4096 behind 4096 / 12288 / 4176 keys of earlier ranks ------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nh,nkv,hd", [(32, 8, 128), (16, 2, 256), (64, 8, 64)])
@pytest.mark.parametrize("q_off", [4096, 12288, 4096 + 80])
def test_qoff_real_sizes_gpu(nh, nkv, hd, q_off):
    """two ranks: [0, q_off) and [q_off, q_off + 4096), 3 diagonal branches, kv_len inside the own block.  Measured on an MI355X:
    O / LSE / dQ identical to the unsharded rows at every q_off here (the unaligned 4176 included); dK / dV summed over the ranks
    <= 4.3e-6 of max |dK| (bar 9e-6)"""
    from specforge_amd import _lib

    _lib.lib()
    Sq = 4096
    bounds = [0, q_off, q_off + Sq]
    aligned = q_off % 128 == 0
    _, _, _, _, _, worst = _run("cuda", 1, bounds, nh, nkv, hd, 4, [q_off + Sq - 300], seed=q_off + hd, aligned=aligned,
                                fp32_rel=9e-6)
    print("measured", dict(nh=nh, nkv=nkv, hd=hd, q_off=q_off), worst)
    assert worst["o"] <= 1.0 and worst["dq"] <= 1.0, worst
