"""sf_row_conf (the draft's top-1 softmax probability per row, conf = 1 / sum_j exp(z_j - max z)) against float64.

Vocabulary sizes: the loop-boundary sizes of test_topk_rank_kernel (the two kernels stream a row the same way).  Rows are planted: a
unique maximum 200 above the rest (conf exactly 1), all logits equal (1 / V), the maximum duplicated in another region, the maximum
planted alone, a randn row, a grid row and the same row shifted by +-3000, three comparable terms near 3000 over a negligible rest (a
kernel that scales z and max z separately before it subtracts loses ~3000 * 1.44 * 2^-24 per term there; on the grid row's thousands
of terms such errors average out, on three they miss the bound), a row without a loss mask whose logits are NaN (-1, nothing read);
the maximum's column visits every region of the stream (test_loss_kernels.region_cols).  The logits are a view into a wider marked
buffer and must come back untouched; conf_tok is indexed by token row, has guard entries, and token rows a row_map leaves out keep
their fill.

Bound: FACTOR x max(error of torch.softmax(z.float()).max() on the CPU, floor), both against the float64 softmax maximum.  The floor is
conf x 2^-24 x the number of fp32 roundings on the longest dependency path of the kernel's own summation order (``roundings``): the
first term that enters lane 0's running sum (subtract, scale, exponential, three pairwise adds), a multiply and an add per chunk of
that lane, five per (max, sum) merge -- the tail element, six wave levels, the other waves -- and the final division.
The measured ratios are in profiles/kernel_tests_coverage.md."""
import pytest
import torch

from specforge_amd import _lib, ops
from f64_helpers import BF, F32, MARK, gpu, held, outside_untouched, wide  # noqa: F401
from test_loss_kernels import FACTOR, region_cols
from test_topk_rank_kernel import KEEP, TOPK_V

B, S, T = 2, 5, 3
SPAD, ROWS = S + T, B * S
NT, NW = 256, 4                  # the launch geometry of row_conf_kernel
VARIANTS = [(0, False), (2, True), (2, False), (0, True)]      # (off, row_map?)
NO_MASK = 7


def roundings(V, nt=NT, nw=NW):
    chunks = -(-(V // 8) // nt)                    # lane 0 folds the most chunks
    stream = 6 + 2 * chunks if chunks else 0
    merges = (1 if V % 8 else 0) + 6 + (nw - 1)
    return stream + 5 * merges + 1


def planted_rows(dtype, V, tc, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, V, generator=g) * 2
    x[0] = x[0].clamp(max=8.0)
    x[0, tc] = 208.0                                           # the unique maximum, >= 200 above the rest: conf exactly 1
    x[1] = 0.5                                                 # all equal: 1 / V
    others = [c for c in region_cols(V) if c != tc] or [c for c in (0, V - 1) if c != tc]
    x[2, tc] = 12.0                                            # the maximum, duplicated in another region
    x[2, others[-1]] = 12.0
    grid, kmax = (16.0, 3) if dtype == BF else (2.0 ** -8, 2048)     # a grid that survives a shift by 3000 in ``dtype``
    k = torch.randint(0, kmax + 1, (V,), generator=g).double()
    base = -grid * k - (8.0 if dtype == BF else 0.0)                 # (bf16 near 3000 holds multiples of 16: 3000 - 8 - 16 k)
    x[4], x[5], x[6] = base, base + 3000.0, base - 3000.0
    x[8, tc] = 12.0                                            # the maximum planted alone
    # three terms of comparable weight near 3000 and nothing else (the rest lies 104 below): rounding errors of the terms cannot
    # average out over the row, as they do on the grid row's thousands of terms (fp32; bf16 near 3000 holds multiples of 16 only)
    x[9] = 2896.0
    near = [c for c in (tc, (tc + 9) % V, (tc + 2 * NT * 8 + 3) % V) if c < V]
    for c, v in zip(dict.fromkeys(near), (3008.0, 2992.0, 2976.0) if dtype == BF else (3000.0, 2999.6875, 2999.3125)):
        x[9, c] = v
    x = x.to(dtype)
    assert torch.equal(x[5].double() - 3000.0, x[4].double()) and torch.equal(x[6].double() + 3000.0, x[4].double())
    x[NO_MASK] = float("nan")                                  # no loss mask: never read
    return x


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def run_case(dev, dtype, V, tc, variant, seed):
    off, use_map = variant
    x = planted_rows(dtype, V, tc, seed)
    pr = lambda r: (r // S, r % S + off)
    lm = torch.zeros(B, SPAD, dtype=torch.int32)               # (whatever a wrong address would read is no loss mask)
    for r in range(ROWS):
        lm[pr(r)] = 1
    lm[pr(NO_MASK)] = 0
    keep = KEEP if use_map else list(range(ROWS))
    n = len(keep)
    xk = x[keep]
    scored = [r != NO_MASK for r in keep]
    z = xk[scored]
    want = torch.softmax(z.double(), -1).max(-1).values
    yard = torch.softmax(z.float(), -1).max(-1).values
    floor = want * 2.0 ** -24 * roundings(V)
    bx, vx = wide(xk, 8, 16 + (-V) % 8, dev, rows_extra=2)
    buf = torch.full((ROWS + 3,), MARK, device=dev)
    conf = buf[:ROWS]
    ops.row_conf(vx, S=S, Spad=SPAD, off=off, loss_mask_pad=lm.to(dev), conf_tok=conf,
                 row_map=torch.tensor(keep).to(dev) if use_map else None)
    assert outside_untouched(bx, n, 8, V) and torch.equal(bits(vx), bits(xk))
    out = buf.cpu()
    assert bool((out[ROWS:] == MARK).all())
    assert all(float(out[r]) == MARK for r in range(ROWS) if r not in keep)
    got = out[torch.tensor([r for r in keep if r != NO_MASK])]
    if NO_MASK in keep:
        assert float(out[NO_MASK]) == -1.0
    ratio = held(got, want, yard, floor, f"row_conf V={V} tc={tc} off={off} map={use_map}", FACTOR)
    where = {r: i for i, r in enumerate(r for r in keep if r != NO_MASK)}
    assert float(got[where[0]]) == 1.0                          # exp(-200) is 0 in fp32
    if 5 in where and 4 in where:
        assert float(want[where[4]]) == float(want[where[5]]) == float(want[where[6]])
    # bitwise repeatable
    again = torch.full((ROWS,), MARK, device=dev)
    ops.row_conf(vx, S=S, Spad=SPAD, off=off, loss_mask_pad=lm.to(dev), conf_tok=again,
                 row_map=torch.tensor(keep).to(dev) if use_map else None)
    assert torch.equal(again.cpu(), out[:ROWS])
    return ratio


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", TOPK_V)
def test_row_conf_against_float64(backend, dtype, V):
    """every region of the stream as the maximum's column, every variant (offset 0 / 2, dense / row_map) at least once"""
    cols = region_cols(V)
    worst = 0.0
    for i in range(max(len(cols), len(VARIANTS))):
        worst = max(worst, run_case(backend, dtype, V, cols[i % len(cols)], VARIANTS[i % len(VARIANTS)], seed=V % 89 + i))
    print(f"worst ratio V={V}: {worst:.3f}")


def test_row_conf_map_entry_out_of_range_and_no_rows(backend):
    """a row_map entry outside [0, ntok) writes nothing; rows == 0 launches nothing"""
    dev, V = backend, 2059
    x = (torch.randn(4, V, generator=torch.Generator().manual_seed(5)) * 2).to(BF)
    lm = torch.ones(B, SPAD, dtype=torch.int32, device=dev)
    buf = torch.full((ROWS + 3,), MARK, device=dev)
    _, vx = wide(x, 8, 16 + (-V) % 8, dev)
    ops.row_conf(vx, S=S, Spad=SPAD, off=1, loss_mask_pad=lm, conf_tok=buf[:ROWS], row_map=torch.tensor([ROWS, 4, -1, ROWS + 2]).to(dev))
    out = buf.cpu()
    assert bool((out[:4] == MARK).all()) and bool((out[5:] == MARK).all())
    want = torch.softmax(x[1].double(), -1).max()
    assert abs(float(out[4]) - float(want)) <= FACTOR * roundings(V) * 2.0 ** -24 * float(want)
    ops.row_conf(vx[:0], S=S, Spad=SPAD, off=1, loss_mask_pad=lm, conf_tok=buf[:ROWS], row_map=torch.tensor([1]).to(dev))
    assert torch.equal(buf.cpu(), out)


def test_row_conf_bad_arguments(backend):
    """off + S > Spad, a leading dimension that is no multiple of 8: the ABI's error, nothing launched"""
    dev = backend
    x = torch.randn(ROWS, 64).to(BF).to(dev)
    lm = torch.ones(B, SPAD, dtype=torch.int32, device=dev)
    conf = torch.full((ROWS,), MARK, device=dev)
    with pytest.raises(_lib.SfError, match="sf_row_conf"):
        ops.row_conf(x, S=S, Spad=SPAD, off=T + 1, loss_mask_pad=lm, conf_tok=conf)
    with pytest.raises(_lib.SfError, match="sf_row_conf"):
        ops.row_conf(torch.randn(ROWS, 68).to(BF).to(dev)[:, :60], S=S, Spad=SPAD, off=0, loss_mask_pad=lm, conf_tok=conf)
    assert bool((conf.cpu() == MARK).all())
    ops.row_conf(x, S=S, Spad=SPAD, off=T, loss_mask_pad=lm, conf_tok=conf)
    assert bool(((conf.cpu() > 0) & (conf.cpu() <= 1)).all())
