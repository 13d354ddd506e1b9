"""RMSNorm forward / backward (single and two-norm forms, the embedding gather), the column sum of the weight-gradient partials and the
row expansion against float64 references written from the definitions, at the hidden sizes on each side of the kernels' switches (one,
two and four 16-byte vectors per thread) and the row counts that leave every remainder of the backward's row groups (4 or 2 rows in
flight, 16 rows per workgroup).  Every operand is a view into a wider buffer with marked neighbours; outputs start as NaN.

The norm is defined with xhat = round_T(x * rstd).  The kernels form x * rstd as ONE fp32 product, so with the fp32 rstd in hand (the
forward's own output, the backward's input) xhat is known bit for bit: xhat = bf16(fp32(x * rstd)), and a bf16 y = bf16(w * xhat) -- an
exact product, one rounding -- is compared for equal bits with no exception.  rstd itself and every fp32 result are held to FACTOR x
max(error of the same formula in torch fp32, floor) against float64, as in tests/test_loss_kernels.py; a bf16 dx must have the bits of
bf16(float64 dx) except within FACTOR x floor of a rounding boundary, for at most 1 % of a case (asserted on the input too)."""
import pytest
import torch

from specforge_amd import ops
from f64_helpers import BF, F32, MARK, InputRejected, bf16_bits, gpu, outside_untouched, rbf, ulp, wide  # noqa: F401
from f64_helpers import held as _held

FACTOR = 6.0            # see profiles/kernel_tests_coverage.md for the measured ratios

EPS = 1e-5
NAN = float("nan")


def held(got, want, yard, floor, what):
    return _held(got, want, yard, floor, what, factor=FACTOR)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def rnd(x64, dtype):
    """round_T of a float64 tensor holding fp32 values"""
    return rbf(x64) if dtype == BF else x64


def xhat_of(x, rstd, dtype):
    """round_T(fp32(x * rstd)) as float64: x of the storage type, rstd fp32 (the double product of an 8- or 24-bit by a 24-bit significand is
    exact, .float() is the one fp32 rounding the kernel's multiply makes)"""
    return rnd((x.double() * rstd.double()[:, None]).float().double(), dtype)


def norm_inputs(dtype, R, H, seed, zero_row=True):
    """x rows: 1: zeros; w with a zero and negative entries"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, H, generator=g)
    if zero_row and R > 1:
        x[1] = 0.0
    w = 1.0 + 0.5 * torch.randn(H, generator=g)
    w[1 % H], w[2 % H], w[H - 1] = 0.0, -1.25, -0.5
    return g, x.to(dtype), w.to(dtype)


# ------------------------------------------------------------------ forward
def case_fwd(dev, dtype, R, H, seed=0, gather=None):
    """gather = (S, Spad, off): x is a table, row b * S + s reads table[ids_pad[b, s + off]] (an id repeated, the table's last row used)"""
    g, x, w = norm_inputs(dtype, R, H, seed)
    ids = None
    if gather:
        S, Spad, off = gather
        assert R % S == 0
        table = x[: max(R // 2, 2)] if R > 2 else x
        ids = torch.randint(0, table.shape[0], (R // S, Spad), generator=g)
        ids[0, off], ids[-1, off + S - 1] = table.shape[0] - 1, table.shape[0] - 1
        if S > 1:
            ids[0, off + 1] = ids[0, off]
        rows = torch.stack([table[ids[r // S, r % S + off]] for r in range(R)])
        bx, vx = wide(table, 8, 8, dev)
    else:
        rows = x
        bx, vx = wide(x, 8, 8, dev)
    by, vy = wide(torch.full((R, H), NAN, dtype=dtype), 16, 8, dev, rows_extra=1)
    rstd = torch.full((R + 2,), MARK, device=dev)
    ops.rmsnorm_fwd(vx, w.to(dev), EPS, vy, rstd, ids_pad=ids.to(dev) if gather else None, S=gather[0] if gather else 1,
                    Spad=gather[1] if gather else 1, off=gather[2] if gather else 0, rows=R)
    assert outside_untouched(by, R, 16, H) and bool((rstd[R:].cpu() == MARK).all())
    x64, w64 = rows.double(), w.double()
    rs64 = 1.0 / torch.sqrt((x64 * x64).mean(-1) + float(torch.tensor(EPS, dtype=F32)))
    rs32 = torch.rsqrt((rows.float() * rows.float()).mean(-1) + EPS)
    got_rs, y = rstd[:R].cpu(), vy.cpu()
    held(got_rs, rs64, rs32, ulp(rs64, F32), "rmsnorm_fwd rstd")
    if R > 1 and not gather:
        assert not bool(y[1].float().any())                     # the row of zeros: rstd = 1 / sqrt(eps), y = 0
    if dtype == BF:
        want = rbf(w64 * xhat_of(rows, got_rs, dtype))
        assert torch.equal(y.double(), want), int((y.double() != want).sum())
        # and against the float64 rstd: the neighbouring xhat only where x * rstd64 is within FACTOR fp32 ulps of a rounding boundary, < 1 %
        xh = x64 * rs64[:, None]
        win = FACTOR * ulp(xh, F32)
        lo, hi, mid = rbf(xh - win), rbf(xh + win), rbf(xh)
        boundary = lo != hi
        if float(boundary.double().mean()) >= 0.01:
            raise InputRejected("the input puts too many elements next to a rounding boundary")
        ok = (y.double() == rbf(w64 * mid)) | (boundary & ((y.double() == rbf(w64 * lo)) | (y.double() == rbf(w64 * hi))))
        assert bool(ok.all()), int((~ok).sum())
    else:
        want = w64 * x64 * rs64[:, None]
        held(y, want, w.float() * (rows.float() * rs32[:, None]), 2 * ulp(want, F32), "rmsnorm_fwd y fp32")
    return rows, w, got_rs


PAIRS = [(8, 1), (8, 5), (128, 3), (128, 17), (896, 4), (896, 33), (2040, 15), (2048, 16), (2048, 31), (2056, 5), (2056, 17), (4096, 3),
         (4096, 16), (4096, 33), (4104, 1), (4104, 4), (4104, 15), (7168, 3), (7168, 17), (8192, 5), (8192, 16), (8192, 31)]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,R", PAIRS)
def test_rmsnorm_fwd_against_float64(backend, dtype, H, R):
    case_fwd(backend, dtype, R, H, seed=H + R)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,off", [(128, 0), (2056, 2), (4104, 0), (8192, 2)])
def test_rmsnorm_fwd_gather(backend, dtype, H, off):
    case_fwd(backend, dtype, 6, H, seed=H + 1, gather=(3, 5, off))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H", [8, 2048, 4104, 8192])
def test_rmsnorm_fwd_scaled_rows_have_the_same_xhat(backend, dtype, H):
    """rows 1 and 2 are row 0 times 2^10 and 2^-10; with eps = 0 every fp32 operation of the norm scales exactly, so y has row 0's bits"""
    _, x, w = norm_inputs(dtype, 3, H, H, zero_row=False)
    x[1], x[2] = (x[0].float() * 1024.0).to(dtype), (x[0].float() / 1024.0).to(dtype)
    y = torch.full((3, H), NAN, dtype=dtype, device=backend)
    rstd = torch.zeros(3, device=backend)
    ops.rmsnorm_fwd(x.to(backend), w.to(backend), 0.0, y, rstd)
    assert torch.equal(bits(y[1]), bits(y[0])) and torch.equal(bits(y[2]), bits(y[0]))
    r = rstd.cpu()
    assert float(r[1]) * 1024.0 == float(r[0]) and float(r[2]) / 1024.0 == float(r[0])


# ------------------------------------------------------------------ backward
def bwd_reference(dtype, dys, ws, x, rs, add):
    """float64 dx, dw per norm and the floors; dys / ws: one or two (dy, w) pairs of the same x"""
    H = x.shape[1]
    xh = xhat_of(x, rs, dtype)
    g = sum(dy.double() * w.double()[None, :] for dy, w in zip(dys, ws))
    mean = (g * xh).mean(-1, keepdim=True)
    core = g - xh * mean
    rs64 = rs.double()[:, None]
    dx = rs64 * core + (add.double() if add is not None else 0.0)
    f_mean = ulp((g * xh).abs().sum(-1, keepdim=True) / H, F32)
    gmax = torch.stack([(dy.double() * w.double()[None, :]).abs() for dy, w in zip(dys, ws)]).max(0).values      # g1 + g2 may cancel: its unit is the larger product's
    floor = rs64 * (xh.abs() * f_mean + ulp(torch.maximum(gmax, (xh * mean).abs()), F32)) + ulp(torch.maximum((rs64 * core).abs(), dx.abs()), F32)
    dws = [(dy.double() * xh) for dy in dys]
    return dx, floor, dws, xh


def bwd_yardstick(dys, ws, x, rs, add, xh):
    g = sum(dy.float() * w.float()[None, :] for dy, w in zip(dys, ws))
    xh = xh.float()
    dx = rs[:, None] * (g - xh * ((g * xh).sum(-1, keepdim=True) / x.shape[1]))
    return dx + add.float() if add is not None else dx


def case_bwd(dev, dtype, R, H, two=False, add=True, dw_mode=0, want_dx=True, seed=0, gather=None):
    """dw_mode 0: dw = ...; 1: dw += ... (must equal the = result plus the previous content exactly); 2: only the per-block partials.
    Row 0: rstd = 1.5 and x with an odd last significand bit, so that every x * rstd is an exact bf16 round-to-even tie; row 1: zeros;
    row 2: dy = 0 (dx must be ``add`` bit for bit)."""
    g, x, w = norm_inputs(dtype, R, H, seed)
    w2 = (0.5 * torch.randn(H, generator=g)).to(dtype)
    dy, dy2 = torch.randn(R, H, generator=g).to(dtype), torch.randn(R, H, generator=g).to(dtype)
    if R > 2:
        dy[2], dy2[2] = 0.0, 0.0
    rs = (1.0 / torch.sqrt((x.double() ** 2).mean(-1) + EPS)).float()
    if dtype == BF:
        x[0] = ((torch.randint(0, 21, (H,), generator=g) * 2 + 1).float() / 128.0 + 1.0) * (torch.randint(0, 2, (H,), generator=g) * 2 - 1).float()
        rs[0] = 1.5
        assert bool((rbf(x[0].double() * 1.5 - 2.0 ** -9) != rbf(x[0].double() * 1.5 + 2.0 ** -9)).all())
    addt = torch.randn(R, H, generator=g).to(dtype) if add else None
    ids = None
    rows = x
    if gather:
        S, Spad, off = gather
        ids = torch.randint(0, R, (R // S, Spad), generator=g)
        ids[0, off], ids[0, off + 1] = R - 1, R - 1
        rows = torch.stack([x[ids[r // S, r % S + off]] for r in range(R)])
    dys, ws = ([dy, dy2], [w, w2]) if two else ([dy], [w])
    dx64, floor, dws, xh = bwd_reference(dtype, dys, ws, rows, rs, addt)
    d = lambda t: t.to(dev)
    bdy, vdy = wide(dy, 8, 8, dev)
    bdy2, vdy2 = wide(dy2, 16, 8, dev)
    bx, vx = wide(x, 8, 16, dev)
    vadd = wide(addt, 16, 16, dev)[1] if add else None
    bdx, vdx = wide(torch.full((R, H), NAN, dtype=dtype), 8, 8, dev, rows_extra=1)
    nb = (R + 15) // 16
    assert ops.rmsnorm_bwd_workspace(R, H) == nb * H
    ws_buf = torch.full((2 * nb * H + 8,), MARK, device=dev)
    prev = torch.randn(2, H, generator=g)

    def run(mode, acc):
        if two:
            ops.rmsnorm_bwd2(vdy, d(w), acc[0] if acc is not None else None, mode == 1, vdy2, d(w2), acc[1] if acc is not None else None, mode == 1,
                             vx, d(rs), dx=vdx, add=vadd, workspace=ws_buf, partial_only=mode == 2)
        else:
            ops.rmsnorm_bwd(vdy, vx, d(w), d(rs), dx=vdx if want_dx else None, add=vadd, dw_acc=acc[0] if acc is not None else None,
                            dw_accumulate=mode == 1, workspace=ws_buf, ids_pad=d(ids) if gather else None, S=gather[0] if gather else 1,
                            Spad=gather[1] if gather else 1, off=gather[2] if gather else 0, partial_only=mode == 2)

    tag = "rmsnorm_bwd2" if two else "rmsnorm_bwd"
    n = 2 if two else 1
    accbuf = torch.full((2, H + 16), MARK, device=dev)
    acc = accbuf[:, 8:8 + H]
    if dw_mode == 2:
        run(2, None)
        part = ws_buf.cpu()[: 2 * nb * H].view(2, nb, H)
        for i in range(n):
            for b in range(nb):
                blk = dws[i][16 * b: 16 * (b + 1)]
                held(part[i, b], blk.sum(0), blk.float().sum(0), ulp(blk.abs().sum(0), F32), tag + " dw partial")
        assert bool((ws_buf.cpu()[2 * nb * H:] == MARK).all()) and (two or bool((ws_buf.cpu()[nb * H:] == MARK).all()))
    else:
        run(0, acc)
        dw0 = acc.cpu().clone()
        for i in range(n):
            held(dw0[i], dws[i].sum(0), dws[i].float().sum(0), ulp(dws[i].abs().sum(0), F32), tag + " dw")
        if dw_mode == 1:
            acc[:n] = prev[:n].to(dev)
            vdx.fill_(NAN)
            run(1, acc)
            assert torch.equal(bits(acc[:n]), bits(prev[:n] + dw0[:n]))
        b = accbuf.cpu()
        assert bool((b[:, :8] == MARK).all()) and bool((b[:, 8 + H:] == MARK).all()) and (two or bool((b[1] == MARK).all()))
    assert outside_untouched(bdx, R, 8, H)
    assert torch.equal(bits(vx), bits(x)) and torch.equal(bits(vdy), bits(dy))
    if not (want_dx or two):
        assert bool(torch.isnan(vdx.cpu().float()).all())
        return
    got = vdx.cpu()
    assert not bool(torch.isnan(got.float()).any()), "a dx row was not stored"
    if R > 2 and add:
        assert torch.equal(bits(got[2]), bits(addt[2]))
    if R > 1 and not gather:
        # the row of zeros: xhat = 0, so dx = rstd * g (+ add) exactly as the formula gives -- fp32(rstd * g), add summed in fp32 and one
        # rounding to T; the compiler may fuse a product into the sum that follows it, so each fused form is a candidate too
        f = lambda t: t.float().double()
        rs1 = rs.double()[1]
        pr = [a.double()[1] * b.double() for a, b in zip(dys, ws)]                      # exact in float64 (24 x 24 bits)
        gs = [f(pr[0])] if not two else [f(f(pr[0]) + f(pr[1])), f(pr[0] + f(pr[1])), f(f(pr[0]) + pr[1])]
        cands = []
        for gv in gs:
            cands += [f(f(rs1 * gv) + addt.double()[1]), f(rs1 * gv + addt.double()[1])] if add else [f(rs1 * gv)]
        hit = torch.stack([got[1].double() == rnd(c, dtype) for c in cands]).any(0)
        assert bool(hit.all()), (tag + " zero row", int((~hit).sum()))
    if dtype == F32:
        held(got, dx64, bwd_yardstick(dys, ws, rows, rs, addt, xh), floor, tag + " dx fp32")
    else:
        bf16_bits(got, dx64, FACTOR * floor, tag + " dx", cap=0.01)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,R", PAIRS)
def test_rmsnorm_bwd_against_float64(backend, dtype, H, R):
    i = PAIRS.index((H, R))
    case_bwd(backend, dtype, R, H, add=i % 2 == 0, dw_mode=i % 3, want_dx=i % 5 != 4, seed=H + R)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,R", [p for p in PAIRS if p[0] <= 4096])
def test_rmsnorm_bwd2_against_float64(backend, dtype, H, R):
    i = PAIRS.index((H, R))
    case_bwd(backend, dtype, R, H, two=True, add=i % 2 == 1, dw_mode=(i + 1) % 3, seed=H + R + 1)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,off", [(128, 0), (4104, 2)])
def test_rmsnorm_bwd_gather(backend, dtype, H, off):
    case_bwd(backend, dtype, 6, H, seed=H, gather=(3, 5, off))


def test_rmsnorm_bwd2_is_refused_above_4096(backend):
    t = lambda *s: torch.zeros(*s, dtype=BF, device=backend)
    f = lambda *s: torch.zeros(*s, device=backend)
    with pytest.raises(Exception, match="4096"):
        ops.rmsnorm_bwd2(t(2, 4104), t(4104), f(4104), False, t(2, 4104), t(4104), f(4104), False, t(2, 4104), f(2), dx=t(2, 4104), workspace=f(2 * 4104))


# ------------------------------------------------------------------ column sum, row expansion
@pytest.mark.parametrize("nb", [1, 15, 16, 17, 2048, 2049, 2049 + 63])
def test_colsum_accum_against_float64(backend, nb):
    """small integers with a 2^20 among them: every fp32 sum is exact in any order, so a skipped or doubled row lane changes the result"""
    for H in (8, 63, 64, 65, 200):
        g = torch.Generator().manual_seed(nb + H)
        part = torch.randint(-9, 10, (nb, H), generator=g).float()
        part[nb // 2, H // 3], part[nb - 1, H - 1], part[0, 0] = 2.0 ** 20, -(2.0 ** 20), 2.0 ** 20
        want = part.double().sum(0)
        prev = torch.randint(-9, 10, (H,), generator=g).float()
        for accumulate in (False, True):
            buf = torch.full((H + 24,), MARK, device=backend)
            acc = buf[8:8 + H]
            acc[:] = prev.to(backend) if accumulate else NAN
            ops.colsum_accum(part.to(backend), nb, H, acc, accumulate)
            assert torch.equal(acc.cpu().double(), want + (prev.double() if accumulate else 0.0)), (nb, H, accumulate)
            assert bool((buf.cpu()[:8] == MARK).all()) and bool((buf.cpu()[8 + H:] == MARK).all())


def case_rows_expand(dev, dtype, rows, C, nsrc=5):
    g = torch.Generator().manual_seed(rows + C)
    src = torch.randn(nsrc, C, generator=g).to(dtype)
    inv = torch.randint(-1, nsrc, (rows,), generator=g).int()
    inv[:5] = torch.tensor([-1, 0, nsrc - 1, 2, 2], dtype=torch.int32)[:rows]
    bs, vs = wide(src, 8, 16, dev)
    bd, vd = wide(torch.full((rows, C), NAN, dtype=dtype), 16, 8, dev, rows_extra=1)
    ops.rows_expand(vs, inv.to(dev), vd)
    want = torch.where((inv >= 0)[:, None], src[inv.clamp_min(0).long()], torch.zeros(rows, C, dtype=dtype))
    assert torch.equal(bits(vd), bits(want)) and outside_untouched(bd, rows, 16, C) and torch.equal(bits(vs), bits(src))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [8, 24, 4096])
def test_rows_expand(backend, dtype, C):
    case_rows_expand(backend, dtype, 9, C)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_rows_expand_second_grid_stride_trip(gpu, dtype):
    """rows x C / 8 > 2048 blocks x 256 threads"""
    assert 1030 * (4096 // 8) > 2048 * 256
    case_rows_expand(gpu, dtype, 1030, 4096)
