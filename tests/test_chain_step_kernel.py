"""sf_chain_step (the per-row carrier of the joint chain fold across the TTT steps) against a plain Python fold.

    eligible = loss_mask[b, s + off] != 0 and depth[rt] == off          -> depth[rt] = off + 1
    alive_h  = eligible and length[h][rt] == off and hit_h               -> length[h][rt] = off + 1

Everything is an integer and compared exactly.  The base shape B=2, S=5, T=3 (Spad = S + T) exercises the b*Spad addressing and the last
row at off = T - 1; it runs dense, with an out-of-order row_map, and with a different row_map per step in which a row skips step 1 and
returns at step 2 (it must stay dead).  Planted rows: all hit, all miss, a miss at depth 1 followed by hits (no revival), a loss mask of
0 at depth 1 followed by 1 (censored for good, and no miss), a channel that outlives channel 0.  State, inputs and outputs are views
into wider marked buffers."""
import pytest
import torch

from specforge_amd import _lib, ops
from f64_helpers import MARK

B, S, T = 2, 5, 3
SPAD, NTOK = S + T, B * S
KEEP = [8, 3, 0, 5]
IMARK = -7
# planted token rows (see the module docstring); row 9 = (b 1, s 4) reads lm[1, 5] at depth 1, which no planted row reads at depth 0
ALL_HIT, ALL_MISS, MISS_AT_1, OUTLIVES, CENSORED = 0, 5, 3, 8, 9


def fold_step(depth, length, lm, S_, Spad, off, rmap, correct, hit):
    """the reference: one step over the compact rows ``rmap`` (token rows); depth [ntok], length [1+J, ntok] are updated in place"""
    J, ntok, n = length.shape[0] - 1, depth.numel(), len(rmap)
    out = torch.zeros(2 + J, n)
    for r, rt in enumerate(rmap):
        if not 0 <= rt < ntok:
            continue
        b, s = divmod(rt, S_)
        if int(lm[b * Spad + s + off]) == 0 or int(depth[rt]) != off:
            continue
        depth[rt] = off + 1
        out[0, r] = 1.0
        for h in range(1 + J):
            x = correct[r] if h == 0 else hit[h - 1, r]
            if int(length[h, rt]) == off and float(x) != 0.0:
                length[h, rt] = off + 1
                out[1 + h, r] = 1.0
    return out


def margins(vals, dev, mark):
    """``vals`` as a contiguous view into a wider buffer filled with ``mark`` -> (buffer, view, left margin)"""
    left, n = 5, vals.numel()
    buf = torch.full((left + n + 7,), mark, dtype=vals.dtype)
    buf[left:left + n] = vals.reshape(-1)
    buf = buf.to(dev)
    return buf, buf[left:left + n].view(vals.shape), left


def margins_kept(buf, left, n, mark):
    b = buf.cpu()
    return bool((b[:left] == mark).all()) and bool((b[left + n:] == mark).all())


def run_steps(dev, B_, S_, T_, J, lm, hits, maps):
    """T_ steps of the kernel beside the reference; ``hits`` [T_, 1+J, ntok] per TOKEN row, ``maps[k]`` = the step's row_map or None.
    Returns the per-step outputs of the kernel (checked equal to the reference's) and the final (depth, length)."""
    Spad, ntok = S_ + T_, B_ * S_
    state = torch.zeros(2 + J, ntok, dtype=torch.int32)
    sbuf, sview, sleft = margins(state, dev, IMARK)
    want_depth, want_len = torch.zeros(ntok, dtype=torch.int32), torch.zeros(1 + J, ntok, dtype=torch.int32)
    lm_d = lm.reshape(-1).to(dev)
    outs = []
    for k in range(T_):
        rmap = list(range(ntok)) if maps[k] is None else list(maps[k])
        n = len(rmap)
        src = torch.tensor([rt if 0 <= rt < ntok else 0 for rt in rmap])
        correct, hit = hits[k, 0][src].contiguous(), hits[k, 1:][:, src].contiguous()
        want = fold_step(want_depth, want_len, lm.reshape(-1), S_, Spad, k, rmap, correct, hit)
        cbuf, cview, cleft = margins(correct, dev, MARK)
        hbuf, hview, hleft = margins(hit, dev, MARK) if J else (None, None, 0)
        obuf, oview, oleft = margins(torch.full((2 + J, n), MARK), dev, MARK)
        ops.chain_step(rows=n, S=S_, Spad=Spad, off=k, loss_mask_pad=lm_d, row_correct=cview, row_hit=hview, chain_depth=sview[0],
                       chain_len=sview[1:], row_out=oview, row_map=None if maps[k] is None else torch.tensor(rmap, dtype=torch.int64).to(dev))
        assert margins_kept(obuf, oleft, (2 + J) * n, MARK) and margins_kept(sbuf, sleft, (2 + J) * ntok, IMARK)
        assert torch.equal(cview.cpu(), correct) and margins_kept(cbuf, cleft, n, MARK)
        if J:
            assert torch.equal(hview.cpu(), hit) and margins_kept(hbuf, hleft, J * n, MARK)
        got = oview.cpu()
        assert torch.equal(got, want), (k, got, want)
        assert torch.equal(sview[0].cpu(), want_depth) and torch.equal(sview[1:].cpu(), want_len), k
        # the counts as the engine forms them
        cnt = torch.full((2 + J,), MARK, device=dev)
        ops.reduce_sum(oview, n, 2 + J, cnt, 1.0)
        assert torch.equal(cnt.cpu(), want.sum(1))
        outs.append(got)
    return outs, want_depth, want_len


def planted(J, seed):
    g = torch.Generator().manual_seed(seed)
    hits = (torch.rand(T, 1 + J, NTOK, generator=g) < 0.6).float()
    lm = torch.ones(B, SPAD, dtype=torch.int32)
    hits[:, :, ALL_HIT] = 1.0
    hits[:, :, ALL_MISS] = 0.0
    hits[:, :, MISS_AT_1] = 1.0
    hits[1, :, MISS_AT_1] = 0.0
    hits[:, :, OUTLIVES] = 1.0
    hits[1:, 0, OUTLIVES] = 0.0                     # channel 0 misses from depth 1 on, the others go on
    hits[:, :, CENSORED] = 1.0
    lm[CENSORED // S, CENSORED % S + 1] = 0         # depth 1 of row 9 (and depth 2 of row 8, which channel 0 does not reach)
    return lm, hits


FORMS = {"dense": [None] * T, "row_map": [KEEP] * T, "row_map_per_step": [KEEP, [0, 8, 5], [3, 5, 0, 8]]}


@pytest.mark.parametrize("J", [0, 3, 8])
@pytest.mark.parametrize("form", list(FORMS))
def test_chain_step_base_shape(backend, form, J):
    lm, hits = planted(J, seed=11 + J)
    outs, depth, length = run_steps(backend, B, S, T, J, lm, hits, FORMS[form])
    print(form, J, "depth", depth.tolist(), "length", length.tolist())
    assert int(depth[ALL_HIT]) == T and bool((length[:, ALL_HIT] == T).all())
    assert int(depth[MISS_AT_1]) == (1 if form == "row_map_per_step" else T)     # the row that skips step 1 never comes back
    assert bool((length[:, MISS_AT_1] == 1).all())                               # a miss (or a skipped step) at depth 1: no revival at 2
    if form == "row_map_per_step":
        assert not bool(outs[2][:, 0].any())                                     # (row 3 is compact row 0 of step 2: not eligible, not alive)
    assert int(length[0, OUTLIVES]) == 1 and int(depth[OUTLIVES]) == 2          # (its depth 2 reads the censoring position)
    if J:
        assert bool((length[1:, OUTLIVES] == 2).all())                           # channels that outlive channel 0
    if form == "dense":
        assert int(depth[ALL_MISS]) == T and bool((length[:, ALL_MISS] == 0).all())
        # censored at depth 1 for good -- the mask is 1 again at depth 2 -- and not counted as a miss: out of the denominator
        assert int(depth[CENSORED]) == 1 and bool((length[:, CENSORED] == 1).all())
        assert float(outs[1][0, CENSORED]) == 0.0 and float(outs[2][0, CENSORED]) == 0.0
    else:
        assert int(depth[CENSORED]) == 0 and int(depth[1]) == 0                  # rows no map names keep the zero state


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 256, 257])
def test_chain_step_grid_tail(backend, rows):
    """B = 1, S = rows: the last block's idle lanes; dense, then every row through a reversed row_map"""
    J, T_ = 3, 2
    g = torch.Generator().manual_seed(rows)
    hits = (torch.rand(T_, 1 + J, rows, generator=g) < 0.7).float()
    lm = (torch.rand(1, rows + T_, generator=g) < 0.8).to(torch.int32)
    _, d0, l0 = run_steps(backend, 1, rows, T_, J, lm, hits, [None] * T_)
    _, d1, l1 = run_steps(backend, 1, rows, T_, J, lm, hits, [list(range(rows))[::-1]] * T_)
    assert torch.equal(d0, d1) and torch.equal(l0, l1)
    assert bool((l0 <= d0[None]).all())


def test_chain_step_row_map_outside_the_token_rows(backend):
    """an entry of -1 and one of ntok: zeros in their outputs, no state touched (run_steps compares the whole state and the margins)"""
    J = 3
    lm, hits = planted(J, seed=3)
    outs, depth, length = run_steps(backend, B, S, T, J, lm, hits, [[8, -1, 0, NTOK]] * T)
    for o in outs:
        assert not bool(o[:, 1].any()) and not bool(o[:, 3].any())
    assert float(outs[0][0, 0]) == 1.0 and float(outs[0][0, 2]) == 1.0
    assert int(depth[NTOK - 1]) == 0 and int(depth[0]) == T


def test_chain_step_no_rows_and_bad_arguments(backend):
    dev, J = backend, 2
    lm = torch.ones(B, SPAD, dtype=torch.int32, device=dev)
    state = torch.full((2 + J, NTOK), IMARK, dtype=torch.int32, device=dev)
    correct = torch.ones(NTOK, device=dev)
    hit = torch.ones(J, NTOK, device=dev)
    out = torch.full((2 + J, NTOK), MARK, device=dev)
    kw = dict(S=S, Spad=SPAD, loss_mask_pad=lm, row_correct=correct, row_hit=hit, row_out=out)
    L = _lib.lib()
    p = lambda t: None if t is None else t.data_ptr()
    assert L.sf_chain_step(0, S, SPAD, 0, NTOK, p(lm), None, p(correct), p(hit), J, p(state[0]), p(state[1:]), p(out), None) == 0
    ops.chain_step(rows=0, off=0, chain_depth=state[0], chain_len=state[1:], **kw)                  # rows == 0: nothing launched
    with pytest.raises(_lib.SfError, match="sf_chain_step"):
        ops.chain_step(rows=NTOK, off=T + 1, chain_depth=state[0], chain_len=state[1:], **kw)       # off + S > Spad
    with pytest.raises(_lib.SfError, match="sf_chain_step"):
        ops.chain_step(rows=NTOK, off=-1, chain_depth=state[0], chain_len=state[1:], **kw)
    with pytest.raises(_lib.SfError, match="sf_chain_step"):                                        # nine top-k channels
        wide_len = torch.full((10, NTOK), IMARK, dtype=torch.int32, device=dev)
        ops.chain_step(rows=NTOK, off=0, chain_depth=state[0], chain_len=wide_len, **dict(kw, row_hit=torch.ones(9, NTOK, device=dev),
                                                                                          row_out=torch.full((11, NTOK), MARK, device=dev)))
    with pytest.raises(_lib.SfError, match="sf_chain_step"):                                        # ntok no multiple of S
        odd = torch.full((3, 7), IMARK, dtype=torch.int32, device=dev)
        ops.chain_step(rows=4, off=0, chain_depth=odd[0], chain_len=odd[1:], **kw)
    assert L.sf_chain_step(-1, S, SPAD, 0, NTOK, p(lm), None, p(correct), p(hit), J, p(state[0]), p(state[1:]), p(out), None) != 0
    with pytest.raises(ValueError, match="chain_step"):                                             # fp32 counts are exact below 2^24 rows
        ops.chain_step(rows=1 << 24, off=0, chain_depth=state[0], chain_len=state[1:], **kw)
    assert bool((state.cpu() == IMARK).all()) and bool((out.cpu() == MARK).all())
    ops.chain_step(rows=NTOK, off=T, chain_depth=state[0], chain_len=state[1:], **kw)               # the limits themselves are fine
    assert bool((out.cpu() == 0).all()) and bool((state.cpu() == IMARK).all())                     # (depth -7 != off: nobody eligible)
