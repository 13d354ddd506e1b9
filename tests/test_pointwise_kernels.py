"""RoPE, SwiGLU and the small movers (cast, bf16 split / add, shifted accumulate, transpose) against float64 references written from the
definition of each operation, at the sizes, strides and values where such kernels go wrong: head sizes that are not powers of two,
position ids that are not ``arange`` and leave the table at both ends, gates where the sigmoid's exponential saturates, exact
round-to-even ties, values that overflow bf16, views into wider buffers whose neighbours must come back untouched.  Every case
runs under the SIMT interpreter and on the GPU (``backend``); the sizes with a second grid-stride trip are GPU only."""
import pytest
import torch

from specforge_amd import _lib, ops

BF, F32 = torch.bfloat16, torch.float32
MARK = 7.5       # what the neighbours of a view hold (exact in bf16)


@pytest.fixture
def gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _lib._inject_library_for_tests(None)
    _lib.lib()
    return "cuda"


def ulp(x, dtype):
    """spacing of ``dtype`` at |x| (float64 in and out; normal range)"""
    _, e = torch.frexp(x.double().abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - (8 if dtype == BF else 24))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits_or_both_nan(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    nan = torch.isnan(a.float())
    return torch.equal(nan, torch.isnan(b.float())) and torch.equal(bits(a)[~nan], bits(b)[~nan])


def wide(vals, left, right, dev, rows_extra=0):
    """a 2-D tensor as a view into a wider buffer (``left`` / ``right`` columns of MARK on its sides); returns (buffer, view)"""
    R, C = vals.shape
    buf = torch.full((R + rows_extra, left + C + right), MARK, dtype=vals.dtype)
    buf[:R, left:left + C] = vals
    buf = buf.to(dev)
    return buf, buf[:R, left:left + C]


def outside_untouched(buf, R, left, C):
    b = buf.cpu()
    return bool((b[:, :left] == MARK).all()) and bool((b[:, left + C:] == MARK).all()) and bool((b[R:] == MARK).all())


# ------------------------------------------------------------------ RoPE
def _tables(hd, max_pos, dtype):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    emb = torch.cat([ang, ang], -1)
    return emb.cos().float().to(dtype), emb.sin().float().to(dtype)


def _rope64(x, nheads, hd, cos, sin, pos):
    """rotate-half in float64 from the same tables: y = x * cos + rotate_half(x) * sin, per head.  Returns (y, larger product)."""
    R = x.shape[0]
    xh = x.double().view(R, nheads, hd)
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    rot = torch.cat([-xh[..., hd // 2:], xh[..., :hd // 2]], -1)
    return (xh * c + rot * s).view(R, nheads * hd), torch.maximum((xh * c).abs(), (rot * s).abs()).view(R, nheads * hd)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("hd,nheads", [(64, 1), (64, 4), (80, 4), (96, 1), (96, 4), (128, 4), (128, 40), (256, 1), (256, 4)])
def test_rope_forward(backend, dtype, hd, nheads):
    """fp32: within 2 ulps of the larger of the two products (their difference may cancel).  bf16: the reference model multiplies and
    adds in bf16, so the expected value is bf16(bf16(x1 c) + bf16(-x2 s)) as torch computes it -- equal bits, except where the
    kernel is within one bf16 ulp of the larger product, for under 1 % of the elements (measured: none, under the interpreter
    and on MI355X: the kernel rounds both products to bf16 and adds them in fp32, which is what torch's bf16 add does)."""
    R, max_pos, left, right = 37, 50, 16, 24
    gen = torch.Generator().manual_seed(hd + nheads)
    cos, sin = _tables(hd, max_pos, dtype)
    pos = torch.randint(0, max_pos, (R,), generator=gen)
    pos[0], pos[1] = 0, max_pos - 1
    x = torch.randn(R, nheads * hd, generator=gen).to(dtype)
    buf, view = wide(x, left, right, backend)
    ops.rope_(view, nheads, hd, cos.to(backend), sin.to(backend), (pos - 3).to(backend), 3)
    assert outside_untouched(buf, R, left, nheads * hd)
    got = view.cpu()
    want, big = _rope64(x, nheads, hd, cos, sin, pos)
    if dtype == F32:
        assert bool(((got.double() - want).abs() <= 2 * ulp(torch.maximum(big, want.abs()), F32)).all())
        return
    xh = x.view(R, nheads, hd)
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    rot = torch.cat([-xh[..., hd // 2:], xh[..., :hd // 2]], -1)
    exp = (xh * c + rot * s).view(R, nheads * hd)            # bf16 tensors: every product and the sum rounded to bf16
    diff = bits(got) != bits(exp)
    share = float(diff.float().mean())
    print(f"rope bf16 hd={hd} nheads={nheads}: share of elements off the torch bf16 expression {share:.5f}")
    assert share < 0.01
    assert bool(((got.double() - exp.double()).abs()[diff] <= ulp(big, BF)[diff]).all())
    assert bool(((got.double() - want).abs() <= 1.5 * ulp(torch.maximum(big, want.abs()), BF)).all())      # three roundings, half an ulp each


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("backward", [False, True])
def test_rope_clamps_positions_to_the_table(backend, dtype, backward):
    """pos + off = -2 is computed at position 0 and pos + off = max_pos + 5 at max_pos - 1 (no read outside the table)"""
    hd, nheads, max_pos, R = 80, 3, 20, 6
    gen = torch.Generator().manual_seed(5)
    cos, sin = _tables(hd, max_pos, dtype)
    x = torch.randn(2, nheads * hd, generator=gen).to(dtype).repeat_interleave(3, 0)      # rows 0-2 equal, rows 3-5 equal
    pos = torch.tensor([0, -2, -1000, max_pos - 1, max_pos + 5, 10 ** 9])
    d = lambda t: t.to(backend)
    got = ops.rope_(d(x.clone()), nheads, hd, d(cos), d(sin), d(pos), 0, backward=backward).cpu()
    assert torch.equal(bits(got[0]), bits(got[1])) and torch.equal(bits(got[0]), bits(got[2]))
    assert torch.equal(bits(got[3]), bits(got[4])) and torch.equal(bits(got[3]), bits(got[5]))
    assert not torch.equal(bits(got[0]), bits(got[3]))
    off = ops.rope_(d(x.clone()), nheads, hd, d(cos), d(sin), d(pos - 4), 4, backward=backward).cpu()     # the same positions as id + offset
    assert torch.equal(bits(off), bits(got))
    want, big = _rope64(x, nheads, hd, cos, -sin if backward else sin, torch.tensor([0, 0, 0, max_pos - 1, max_pos - 1, max_pos - 1]))
    assert bool(((got.double() - want).abs() <= 2 * ulp(torch.maximum(big, want.abs()), dtype)).all())     # (bf16: 1.5 ulps, three roundings)


@pytest.mark.parametrize("hd,nheads", [(64, 4), (80, 1), (128, 40), (256, 4)])
def test_rope_backward_is_the_transpose_of_forward(backend, hd, nheads):
    """<rope(x), y> == <x, rope_bwd(y)> in fp32, to 1e-5 of the sum of the products' magnitudes"""
    R, max_pos = 19, 64
    gen = torch.Generator().manual_seed(hd)
    cos, sin = _tables(hd, max_pos, F32)
    pos = torch.randint(0, max_pos, (R,), generator=gen)
    x, y = torch.randn(R, nheads * hd, generator=gen), torch.randn(R, nheads * hd, generator=gen)
    d = lambda t: t.to(backend)
    fx = ops.rope_(d(x.clone()), nheads, hd, d(cos), d(sin), d(pos), 0).cpu().double()
    by = ops.rope_(d(y.clone()), nheads, hd, d(cos), d(sin), d(pos), 0, backward=True).cpu().double()
    lhs, rhs = float((fx * y.double()).sum()), float((x.double() * by).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((fx * y.double()).abs().sum())
    want, big = _rope64(y, nheads, hd, cos, -sin, pos)           # the transpose of a rotation is the rotation by the opposite angle
    assert bool(((by - want).abs() <= 2 * ulp(torch.maximum(big, want.abs()), F32)).all())


# ------------------------------------------------------------------ SwiGLU
GATES = [0.0, 2.0 ** -20, 1.0, 10.0, 30.0, 87.0, 89.0, 100.0, 127.0, 3e4]


def _swiglu_inputs(dtype, seed, rows_randn=5):
    """rows 0-3: the gate grid (both signs) crossed with up / dact of both signs; then randn rows"""
    gates = torch.tensor([s * g for g in GATES for s in (1.0, -1.0)])
    I = 8 * ((gates.numel() + 7) // 8)
    gates = torch.cat([gates, torch.zeros(I - gates.numel())])
    gen = torch.Generator().manual_seed(seed)
    gu, da = [], []
    for su, sd in ((1.5, 0.75), (-1.5, 0.75), (0.37, -1.25), (-0.37, -1.25)):
        gu.append(torch.cat([gates, torch.full((I,), su)]))
        da.append(torch.full((I,), sd))
    gu = torch.stack(gu + [torch.randn(2 * I, generator=gen) * 3 for _ in range(rows_randn)])
    da = torch.stack(da + [torch.randn(I, generator=gen) for _ in range(rows_randn)])
    return gu.to(dtype), da.to(dtype), I


def _swiglu64(gu, da, I, dtype):
    g, u, da = gu[:, :I].double(), gu[:, I:].double(), da.double()
    sg = torch.sigmoid(g)
    silu_t = (g * sg).to(dtype).double()          # the model's act_fn output is a tensor of the storage type before the product
    return silu_t * u, da * u * (sg * (1 + g * (1 - sg))), da * silu_t


def _swiglu_bf16_exact(act, dgu, gu, da, I, tag):
    """bf16: T(silu) times a bf16 value is exact in fp32, so act and dup are ONE rounding of an exact product and are compared bit for
    bit: act == bf16(T(silu) * up), dup == bf16(dact * T(silu)), T(silu) = bf16 of the float64 silu.  Two exceptions, each tested
    as a condition on the input, not on the result:
    - boundary: the fp32 silu of the kernel (as of torch's own bf16 silu) is within (4 + |g|) * 2^-24 of the float64 one -- exp2, rcp,
      an add and a multiply at an ulp each, and the rounding of g * log2(e), which moves the exponential by |g| * 2^-24.  Where the
      float64 silu moved by twice that either way rounds to two different bf16 values, the neighbouring T(silu) is accepted too.
      Under 1 % of the elements may take it (expected 2e-4; measured: 0 of 216 on the grid, 4.2 M random gates on MI355X 1.2e-4).
    - underflow: where the float64 sigmoid is under 2^-125 the fp32 one is a denormal or its exponential overflows (g < -86.6); silu
      is then below 1e-35 and the result is only required to be within 1e-6 x |up| (|dact|) of it, as the issue allows in fp32.
    dgate = dact * up * silu'(g) is not an exact product: one bf16 ulp of the float64 value (underflow as above; where
    |silu'(g)| < 2^-10, next to its zero at g = -1.278, the fp32 bound 1e-6 x |dact up|)."""
    g, u, d = gu[:, :I], gu[:, I:], da
    g64 = g.double()
    sg = torch.sigmoid(g64)
    s64 = g64 * sg
    w = 2.0 ** -21 * (1.0 + g64.abs() / 4)
    t_mid, t_lo, t_hi = s64.to(BF), (s64 * (1 - w)).to(BF), (s64 * (1 + w)).to(BF)
    boundary = bits(t_lo) != bits(t_hi)
    under = sg < 2.0 ** -125
    for got, other, absleg, what in ((act, u, u.double().abs(), "act"), (dgu[:, I:], d, d.double().abs(), "dup")):
        exact = lambda t: bits((t.float() * other.float()).to(BF))
        b = bits(got)
        eq_mid = b == exact(t_mid)
        eq_nb = (b == exact(t_lo)) | (b == exact(t_hi))
        und_ok = under & ((got.double() - t_mid.double() * other.double()).abs() <= 1e-6 * absleg)
        taken = ~eq_mid & ~under
        share = float(taken.float().mean())
        print(f"swiglu {tag} {what}: share of elements on the neighbouring T(silu) {share:.2e}, boundary elements {int(boundary.sum())}")
        assert bool((eq_mid | (boundary & eq_nb) | und_ok).all()), (what, int((~(eq_mid | (boundary & eq_nb) | und_ok)).sum()))
        assert share < 0.01, (what, share)
    dsilu = sg * (1 + g64 * (1 - sg))
    want = d.double() * u.double() * dsilu
    err = (dgu[:, :I].double() - want).abs()
    loose = under | (dsilu.abs() < 2.0 ** -10)
    tol = torch.where(loose, torch.maximum(ulp(want, BF), 1e-6 * (d.double() * u.double()).abs()), ulp(want, BF))
    print(f"swiglu {tag} dgate: worst error {float((err / ulp(want, BF))[~loose].max()):.2f} bf16 ulps")
    assert bool((err <= tol).all()), "dgate"


def _swiglu_check(dev, gu, da, I, dtype, tag):
    """fp32: 4 ulps of the result, or 1e-6 x |up| (x |dact| for the gradients): v_exp_f32 and v_rcp_f32 are about an ulp each, and
    where the sigmoid underflows the result is below any such ulp (measured worst case where the ulp leg decides: act 0.50 ulps
    under the interpreter, 4.55 on MI355X over 4.2 M random gates -- the bound stays as the issue states it).  bf16: see
    _swiglu_bf16_exact.  No NaN or inf where the float64 value is finite."""
    R = gu.shape[0]
    bgu, vgu = wide(gu, 8, 16, dev)
    bda, vda = wide(da, 16, 8, dev)
    bact, vact = wide(torch.zeros(R, I, dtype=dtype), 24, 8, dev)
    bdgu, vdgu = wide(torch.zeros(R, 2 * I, dtype=dtype), 8, 8, dev)
    ops.swiglu_fwd(vgu, vact)
    ops.swiglu_bwd(vda, vgu, vdgu)
    assert outside_untouched(bact, R, 24, I) and outside_untouched(bdgu, R, 8, 2 * I)
    assert torch.equal(bits(vgu), bits(gu)) and torch.equal(bits(vda), bits(da))
    refs = _swiglu64(gu, da, I, dtype)
    u, d = gu[:, I:].double().abs(), da.double().abs()
    act, dgu = vact.cpu(), vdgu.cpu()
    for got, want in zip((act, dgu[:, :I], dgu[:, I:]), refs):
        assert bool(torch.isfinite(got.float()[torch.isfinite(want)]).all())
    if dtype == BF:
        _swiglu_bf16_exact(act, dgu, gu, da, I, tag)
        return
    for got, want, absleg, what in ((act, refs[0], u, "act"), (dgu[:, :I], refs[1], d * u, "dgate"), (dgu[:, I:], refs[2], d, "dup")):
        err = (got.double() - want).abs()
        decides = err > 1e-6 * absleg
        in_ulps = float((err / ulp(want, F32))[want.abs() > 1e-3 * absleg].max())
        print(f"swiglu {tag} {what}: worst error {in_ulps:.2f} ulps ({int(decides.sum())} elements past the 1e-6 leg)")
        assert bool((err <= torch.maximum(4 * ulp(want, F32), 1e-6 * absleg)).all()), (what, in_ulps)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_swiglu_saturating_gates_and_strides(backend, dtype):
    gu, da, I = _swiglu_inputs(dtype, 1)
    _swiglu_check(backend, gu, da, I, dtype, str(dtype)[6:])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, F32])
def test_swiglu_second_grid_stride_trip(gpu, dtype):
    """rows x I / 8 > 2048 blocks x 256 threads"""
    gu, da, I = _swiglu_inputs(dtype, 2, rows_randn=2048 * 256 // 3 + 40)
    assert gu.shape[0] * (I // 8) > 2048 * 256
    _swiglu_check(gpu, gu, da, I, dtype, str(dtype)[6:] + "-large")


def _fused_shape(dev):
    """a shape whose gate|up and down-projection GEMMs take the FUSED SwiGLU epilogues (include/specforge_amd.h: more than half a tile
    per CU on the GPU, K >= 512; the interpreter build fuses any whole-tile shape with K >= 512)"""
    return (512, 256, 512) if dev == "cpu" else (4096, 2560, 512)


def test_swiglu_fused_gemm_epilogues_on_the_saturating_gates(backend):
    """The fused epilogues of gemm_nt_swiglu_fwd / _bwd share sf_swiglu_{fwd,bwd}_elem with the standalone kernels.  One-hot rows of A
    make the GEMM exact (row r of the product is column r % K of the weight), so gate|up and dact are the chosen values and the
    fused launch must give the bits of the standalone kernel on them -- on the gate grid where exp2 saturates and on randn."""
    dev = backend
    M, I, K = _fused_shape(dev)
    gen = torch.Generator().manual_seed(11)
    gates = torch.tensor([s * g for g in GATES for s in (1.0, -1.0)])
    gm = torch.randn(K, 2 * I, generator=gen) * 3                     # row k of gate|up (rows repeat with period K)
    gm[:, :I][:, ::3] = gates[torch.arange(K)[:, None] % gates.numel()].expand(K, (I + 2) // 3)    # every third gate column: the grid
    gm[: K // 2, I::2] = 1.5
    gm[K // 2:, I::2] = -0.37
    gm = (gm + 0.0).to(BF)                 # (a GEMM sums its zeros to +0: no -0 gate)
    dm = torch.randn(K, I, generator=gen).to(BF)
    dm[:, ::2] = torch.where(torch.arange(K)[:, None] % 2 == 0, 0.75, -1.25).to(BF)
    a = torch.zeros(M, K, dtype=BF)
    a[torch.arange(M), torch.arange(M) % K] = 1.0
    rows = torch.arange(M) % K
    d = lambda t: t.to(dev)
    # forward: gate|up = A . Wgu^T with Wgu = gm^T
    gu = torch.full((M, 2 * I), 7.0, dtype=BF, device=dev)
    act = torch.full((M, I), 5.0, dtype=BF, device=dev)
    ops.gemm_nt_swiglu_fwd(d(a), d(gm.t().contiguous()), gu, act)
    assert torch.equal(bits(gu), bits(gm[rows]))
    act_ref = torch.empty((M, I), dtype=BF, device=dev)
    ops.swiglu_fwd(d(gm[rows]), act_ref)
    assert torch.equal(bits(act), bits(act_ref))
    # backward: dact = A . Wdown^T with Wdown = dm^T
    dgu = torch.full((M, 2 * I), 7.0, dtype=BF, device=dev)
    scratch = torch.empty((M, I), dtype=BF, device=dev)
    ops.gemm_nt_swiglu_bwd(d(a), d(dm.t().contiguous()), d(gm[rows]), dgu, scratch)
    dgu_ref = torch.empty((M, 2 * I), dtype=BF, device=dev)
    ops.swiglu_bwd(d(dm[rows]), d(gm[rows]), dgu_ref)
    same = bits(dgu) == bits(dgu_ref)
    print(f"fused swiglu bwd: {int((~same).sum())} of {same.numel()} elements differ from the standalone kernel")
    assert bool(same.all())
    assert bool(torch.isfinite(dgu.float().cpu()).all()) and bool(torch.isfinite(act.float().cpu()).all())


# ------------------------------------------------------------------ casts and movers
def _special(rows, C, seed):
    """fp32 values with exact bf16 round-to-even ties, the largest finite fp32 (overflows bf16), both zeros, an inf and a NaN"""
    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(seed))
    sp = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 3.4028234663852886e38, -3.4028234663852886e38,
                       0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1 + 2.0 ** -8 + 2.0 ** -23, 2.0 ** -100, 65280.0 + 128.0])
    x.view(-1)[:sp.numel()] = sp
    x.view(-1)[-sp.numel():] = sp
    return x


def _movers(dev, rows, C):
    x = _special(rows, C, 1)
    finite = torch.isfinite(x)
    # cast (scale 1 and a power of two: the product is exact, the rounding is the cast's)
    for dtype in (BF, F32):
        for scale in (1.0, 0.5):
            buf, out = wide(torch.zeros(rows, C, dtype=dtype), 8, 16, dev)
            bin_, vin = wide(x, 16, 8, dev)
            ops.cast_from_f32(vin, out, scale)
            assert same_bits_or_both_nan(out, (x * scale).to(dtype)) and outside_untouched(buf, rows, 8, C)
    # split: hi = bf16(x) exactly, hi + lo reproduces x to 2^-16
    bhi, hi = wide(torch.zeros(rows, C, dtype=BF), 8, 8, dev)
    blo, lo = wide(torch.zeros(rows, C, dtype=BF), 8, 8, dev)
    ops.split_bf16(wide(x, 8, 8, dev)[1], hi, lo)
    assert same_bits_or_both_nan(hi, x.to(BF)) and outside_untouched(bhi, rows, 8, C) and outside_untouched(blo, rows, 8, C)
    ok = finite & torch.isfinite(x.to(BF).float()) & (x.abs() > 1e-30)
    rec = hi.cpu().double() + lo.cpu().double()
    assert bool(((rec - x.double()).abs()[ok] <= 2.0 ** -16 * x.double().abs()[ok]).all())
    # add: bf16 operands, fp32 sum, one rounding (1 + 2^-8 and 1 + 2^-7 + 2^-8 are ties of the sum)
    a = x.to(BF)
    b = torch.randn(rows, C, generator=torch.Generator().manual_seed(2)).to(BF)
    a.view(-1)[20:24] = torch.tensor([1.0, 1 + 2.0 ** -7, -1.0, 3.3895313892515355e38]).to(BF)
    b.view(-1)[20:24] = torch.tensor([2.0 ** -8, 2.0 ** -8, -2.0 ** -8, 3.3895313892515355e38]).to(BF)
    out = torch.full((rows * C + 16,), MARK, dtype=BF, device=dev)
    ops.add_bf16(a.to(dev), b.to(dev), out[:rows * C])
    assert same_bits_or_both_nan(out[:rows * C].view(rows, C), (a.float() + b.float()).to(BF)) and bool((out[rows * C:].cpu() == MARK).all())
    # shifted accumulate: dst[b * Spad + s + off] += src[b * S + s] in fp32, every other row untouched
    B = 2 if rows % 2 == 0 else 1
    S = rows // B
    Spad, off = S + 3, 2
    d0 = torch.randn(B * Spad, C, generator=torch.Generator().manual_seed(3))
    bd, dst = wide(d0, 8, 8, dev)
    ops.shift_accum(wide(a, 8, 8, dev)[1], dst, B=B, S=S, Spad=Spad, off=off)
    want = d0.clone().view(B, Spad, C)
    want[:, off:off + S] += a.float().view(B, S, C)
    assert same_bits_or_both_nan(dst, want.view(B * Spad, C)) and outside_untouched(bd, B * Spad, 8, C)
    # shift + sum + split with one step: the sum is the source itself, so hi is the source and lo is zero (NaN / inf: NaN)
    bh2, h2 = wide(torch.zeros(B * Spad, C, dtype=BF), 8, 8, dev)
    bl2, l2 = wide(torch.zeros(B * Spad, C, dtype=BF), 8, 8, dev)
    ops.shift_sum_split(wide(a, 8, 8, dev)[1], h2, l2, T=1, B=B, S=S, Spad=Spad)
    wh = torch.zeros(B, Spad, C, dtype=BF)
    wh[:, :S] = (0.0 + a.float()).to(BF).view(B, S, C)      # (a sum that starts at +0: -0 comes out as +0)
    assert same_bits_or_both_nan(h2, wh.view(B * Spad, C)) and outside_untouched(bh2, B * Spad, 8, C) and outside_untouched(bl2, B * Spad, 8, C)
    fin = torch.isfinite(wh.float()).view(B * Spad, C)
    assert not bool(l2.cpu()[fin].float().any())


@pytest.mark.parametrize("rows,C", [(1, 32), (6, 40), (14, 264)])
def test_casts_and_movers_round_like_torch(backend, rows, C):
    _movers(backend, rows, C)


@pytest.mark.gpu
def test_casts_and_movers_second_grid_stride_trip(gpu):
    _movers(gpu, 2100, 2048)         # 2100 x 256 units of 8 > 2048 blocks x 256 threads


# ------------------------------------------------------------------ transpose
def _transpose(inp, out, in_b1, in_b2, out_b1, out_b2, nb1, nb2, R, C, in_ld, out_ld):
    _lib.check(_lib.lib().sf_transpose(ops._p(inp), ops._dt(inp), in_b1, in_b2, in_ld, ops._p(out), out_b1, out_b2, out_ld, nb1, nb2, R, C,
                                       ops._stream()), "sf_transpose")


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("nb1,nb2", [(1, 1), (2, 3), (3, 1)])
@pytest.mark.parametrize("R", [8, 72, 200, 264])
@pytest.mark.parametrize("C", [8, 72, 200, 264])
def test_transpose_batches_strides_and_padding(backend, dtype, nb1, nb2, R, C):
    """out[b1][b2][c][r] = in[b1][b2][r][c], exact; both sides have padded rows and padding between the batches, which stays"""
    in_ld, out_ld = C + 8, R + 16
    in_b2, out_b2 = R * in_ld + 24, C * out_ld + 8
    in_b1, out_b1 = nb2 * in_b2 + 16, nb2 * out_b2 + 40
    gen = torch.Generator().manual_seed(R + C)
    src = (torch.randn(nb1 * in_b1, generator=gen) * 4).to(dtype)
    dst = torch.full((nb1 * out_b1,), MARK, dtype=dtype)
    want = dst.clone()
    for i in range(nb1):
        for j in range(nb2):
            blk = src[i * in_b1 + j * in_b2:][:R * in_ld].view(R, in_ld)[:, :C]
            want[i * out_b1 + j * out_b2:][:C * out_ld].view(C, out_ld)[:, :R] = blk.t()
    s, d = src.to(backend), dst.to(backend)
    _transpose(s, d, in_b1, in_b2, out_b1, out_b2, nb1, nb2, R, C, in_ld, out_ld)
    assert torch.equal(bits(d), bits(want)) and torch.equal(bits(s), bits(src))


def test_transpose_refuses_more_batches_than_a_grid_holds(backend):
    t = torch.zeros(64, dtype=BF, device=backend)
    with pytest.raises(Exception, match="too many batches"):
        _transpose(t, t.clone(), 0, 0, 0, 0, 256, 256, 8, 8, 8, 8)
