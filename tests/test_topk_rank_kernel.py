"""sf_topk_rank (the rank of the target token in a row of draft logits, and the per-row top-k hits) against torch:

    rank = (z > z[t]).sum() + (z[:t] == z[t]).sum()

Everything is an integer and compared exactly.  Vocabulary sizes: idle lanes with a tail only (7), exactly one trip of 256 lanes x 8
(2048), one trip + one chunk + a tail of 3 (2059), the four-chunk unrolled loop entered by lane 0 alone (6152), by every lane (8192),
once + one chunk + a tail of 5 (8205), twice by lane 0 (16392), and 32000 (three unrolled trips, a fourth that only 160 lanes enter, the
one-chunk loop for the rest).  Rows are planted: the target the unique maximum, the unique minimum, all logits equal, a grid row full of
ties and the same row shifted by +-3000, the target's value duplicated at a lower and at a higher index of another region, a randn row,
a target the draft vocabulary lacks, a target id past the target vocabulary, a row without a loss mask; the target's column visits every
region of the stream (test_loss_kernels.region_cols).  The logits are a view into a wider marked buffer and must come back untouched."""
import pytest
import torch

from specforge_amd import _lib, ops
from f64_helpers import BF, F32, MARK, gpu, outside_untouched, wide  # noqa: F401
from test_loss_kernels import region_cols

B, S, T = 2, 5, 3
SPAD, ROWS = S + T, B * S
KEEP = [8, 3, 0, 5]          # the row_map variant: 4 of the 10 rows, out of order
TOPK_V = [7, 2048, 2059, 6152, 8192, 8205, 16392, 32000]


def thresholds(V):
    return [(1, 2, 4, 8), (1, V), (V + 1,)]


# (off, which thresholds, row_map?, identity vocabulary map?)
VARIANTS = [(0, 0, False, False), (2, 1, True, False), (0, 2, False, False), (2, 0, False, True), (0, 1, True, True), (2, 2, True, False)]


def planted_rows(dtype, V, tc, seed):
    """ten rows of logits whose target column is ``tc`` (rows 8 and 9: no valid target), see the module docstring"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, V, generator=g) * 2
    x[0, tc] = 50.0                                            # the unique maximum: rank 0
    x[1, tc] = -50.0                                           # the unique minimum: rank V - 1
    x[2] = 0.5                                                 # all equal: rank tc
    cols = region_cols(V)
    lower, higher = [c for c in cols if c < tc], [c for c in cols if c > tc]
    x[3, tc] = 1.25                                            # a duplicate at a lower and at a higher index, in other regions
    if lower:
        x[3, lower[0]] = 1.25
    if higher:
        x[3, higher[-1]] = 1.25
    grid, kmax = (16.0, 3) if dtype == BF else (2.0 ** -8, 2048)     # a grid that survives a shift by 3000 in ``dtype``
    k = torch.randint(0, kmax + 1, (V,), generator=g).double()
    base = -grid * k - (8.0 if dtype == BF else 0.0)                 # (bf16 near 3000 holds multiples of 16: 3000 - 8 - 16 k)
    x[4], x[5], x[6] = base, base + 3000.0, base - 3000.0
    x = x.to(dtype)
    assert torch.equal(x[5].double() - 3000.0, x[4].double()) and torch.equal(x[6].double() + 3000.0, x[4].double())
    return x


def reference_rank(z, t):
    z = z.float()
    return int((z > z[t]).sum()) + int((z[:t] == z[t]).sum())


def run_case(dev, dtype, V, tc, variant, seed):
    off, ki, use_map, identity = variant
    kk = thresholds(V)[ki]
    J = len(kk)
    g = torch.Generator().manual_seed(seed + 77)
    x = planted_rows(dtype, V, tc, seed)
    # a non-identity ascending vocabulary map: draft j <-> target j + d2t[j]
    if identity:
        d2t, Vt, t2d_index = torch.zeros(V, dtype=torch.int64), V, None
    else:
        step = torch.randint(0, 3, (V,), generator=g)
        step[min(1, V - 1)] = 1                                 # at least one target id has no draft index
        d2t = torch.cumsum(step, 0)
        Vt = V + int(d2t[-1]) + 3
        t2d_index = torch.full((Vt,), -1, dtype=torch.int32)
        t2d_index[torch.arange(V) + d2t] = torch.arange(V, dtype=torch.int32)
    pr = lambda r: (r // S, r % S + off)
    tgt = torch.full((B, SPAD), -7, dtype=torch.int64)          # (whatever a wrong address would read is no valid id)
    lm = torch.ones(B, SPAD, dtype=torch.int32)
    draft_t = [tc] * ROWS
    for r in range(ROWS):
        tgt[pr(r)] = tc + int(d2t[tc])
    if identity:
        tgt[pr(8)] = -1
        tgt[pr(9)] = V
    else:
        absent = int((t2d_index == -1).nonzero()[0])
        tgt[pr(8)] = absent                                     # a target the draft vocabulary lacks
        tgt[pr(9)] = Vt + 5                                     # an id past the target vocabulary
    draft_t[8] = draft_t[9] = None
    lm[pr(7)] = 0                                               # a randn row without a loss mask
    keep = KEEP if use_map else list(range(ROWS))
    n = len(keep)
    xk = x[keep]
    want = torch.tensor([V if (draft_t[r] is None or int(lm[pr(r)]) == 0) else reference_rank(x[r], draft_t[r]) for r in keep])
    want_hit = torch.stack([((want < k) & (want < V)).float() * torch.tensor([float(lm[pr(r)]) for r in keep]) for k in kk])
    planted = {0: 0, 1: V - 1, 2: tc}
    for i, r in enumerate(keep):
        if r in planted:
            assert int(want[i]) == planted[r]
    if not use_map:
        assert int(want[4]) == int(want[5]) == int(want[6])     # the shift by +-3000 moves no rank
    d = lambda t: None if t is None else t.to(dev)
    bx, vx = wide(xk, 8, 16 + (-V) % 8, dev, rows_extra=2)
    row_rank = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    row_hit = torch.full((J * n + 2,), MARK, device=dev)
    kw = dict(S=S, Spad=SPAD, off=off, loss_mask_pad=d(lm), tgt_ids_pad=d(tgt), row_map=d(torch.tensor(keep)) if use_map else None)
    ops.topk_rank(vx, t2d_index=d(t2d_index), kk=kk, row_rank=row_rank, row_hit=row_hit, **kw)
    assert outside_untouched(bx, n, 8, V) and torch.equal(vx.cpu(), xk)
    got, hit = row_rank.cpu(), row_hit.cpu()
    print(f"V={V} tc={tc} variant={variant}: ranks {got[:n].tolist()}")
    assert bool((got[n:] == -7).all()) and bool((hit[J * n:] == MARK).all())
    assert torch.equal(got[:n].long(), want)
    hit = hit[:J * n].view(J, n)
    assert torch.equal(hit, want_hit)
    assert bool((hit[1:] >= hit[:-1]).all())                    # monotone in k
    sentinel = want == V
    assert not bool(hit[:, sentinel].any())                     # no hit at any threshold, V + 1 included
    if kk == (V + 1,):
        assert torch.equal(hit[0], (~sentinel).float())
    if V % 8 == 0 and kk[0] == 1:
        # threshold 1 == the fused CE's row_correct for the same inputs, bit for bit
        outs = [torch.full((n,), MARK, device=dev) for _ in range(3)]
        bx2, vx2 = wide(xk, 8, 16, dev)
        ops.ce_fused(vx2, torch.zeros(B, SPAD, V, device=dev), pos_mask_pad=d(torch.ones(B, SPAD, dtype=torch.int32)), tsum_pad=d(torch.ones(B, SPAD)),
                     d2t=d(d2t), write_grad=False, row_loss=outs[0], row_correct=outs[1], row_accept=outs[2], **kw)
        assert torch.equal(outs[1].cpu(), hit[0])
        assert torch.equal(outs[1].cpu(), (want == 0).float())
    # rank only (no thresholds)
    rr = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ops.topk_rank(vx, t2d_index=d(t2d_index), row_rank=rr, **kw)
    assert torch.equal(rr.cpu().long(), want)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", TOPK_V)
def test_topk_rank_against_torch(backend, dtype, V):
    """every region of the stream as the target's column, every variant (offset 0 / 2, the three threshold sets, dense / row_map, a
    non-identity ascending d2t / the identity) at least once"""
    cols = region_cols(V)
    for i in range(max(len(cols), len(VARIANTS))):
        run_case(backend, dtype, V, cols[i % len(cols)], VARIANTS[i % len(VARIANTS)], seed=V % 89 + i)


def test_topk_rank_bad_arguments(backend):
    """nine thresholds, off + S > Spad: the ABI's error, nothing launched"""
    dev, V = backend, 64
    x = torch.randn(ROWS, V).to(BF).to(dev)
    lm = torch.ones(B, SPAD, dtype=torch.int32, device=dev)
    tgt = torch.zeros(B, SPAD, dtype=torch.int64, device=dev)
    row_rank = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)
    row_hit = torch.full((9 * ROWS,), MARK, device=dev)
    kw = dict(loss_mask_pad=lm, tgt_ids_pad=tgt, row_rank=row_rank, row_hit=row_hit)
    with pytest.raises(_lib.SfError, match="sf_topk_rank"):
        ops.topk_rank(x, S=S, Spad=SPAD, off=0, kk=(1,) * 9, **kw)
    with pytest.raises(_lib.SfError, match="sf_topk_rank"):
        ops.topk_rank(x, S=S, Spad=SPAD, off=T + 1, kk=(1, 2), **kw)
    with pytest.raises(_lib.SfError, match="sf_topk_rank"):
        ops.topk_rank(x, S=S, Spad=SPAD, off=0, kk=(0,), **kw)
    assert bool((row_rank.cpu() == -7).all()) and bool((row_hit.cpu() == MARK).all())
    ops.topk_rank(x, S=S, Spad=SPAD, off=T, kk=(1, 2, 3, 4, 5, 6, 7, 8), **kw)      # the limits themselves are fine
    assert bool((row_rank.cpu() >= 0).all()) and bool((row_hit.cpu()[:8 * ROWS] != MARK).all()) and bool((row_hit.cpu()[8 * ROWS:] == MARK).all())
