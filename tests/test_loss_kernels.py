"""The loss rows (fused CE in its three forms, the two LK gradients) and the two teacher reductions against float64 references written
from the definitions in include/specforge_amd.h, at the vocabulary sizes where each kernel changes path (idle lanes, one full trip of
256 lanes, the four-chunk unrolled loop entered by lane 0 alone / by every lane / twice, its one-chunk remainder loop, the scalar tail,
the LK kernel's 256 ... 1024 lanes, its register chunks and its streamed columns) and on rows whose values are planted: a dominant
logit, equal logits, a row shifted by +-3000, maxima with a duplicate at a higher index in another region, exact s == q ties,
pod_scale 0 and 1, tsum 1/2, a one-hot target.  Every operand is a view into a wider buffer whose neighbours must come back untouched.

Bounds.  Integers are compared exactly.  An fp32 output is held to FACTOR x max(error of the same formula in torch fp32 on the CPU,
floor), both errors taken against float64; the floor is the rounding unit of the formula's larger terms, worked out from the float64
reference alone (exp(a - b) moves by ulp32(max(|a|, |b|)) relative and by one ulp32 of itself; a sum by the ulp32 of its larger term),
so that a yardstick which is exact by luck does not make the bound zero.  A bf16 gradient must have the bits of bf16(float64
reference); where the float64 value lies within FACTOR x floor of a bf16 rounding boundary the neighbouring value is accepted too, for
at most 2 % of a case -- and that at most 2 % of the elements of an input lie that close is asserted from the reference alone.
The measured ratios are in profiles/kernel_tests_coverage.md."""
import pytest
import torch

from specforge_amd import ops
from f64_helpers import BF, F32, MARK, InputRejected, bf16_bits, gpu, outside_untouched, ulp, wide  # noqa: F401
from f64_helpers import held as _held

B, S, T = 2, 5, 3
SPAD, ROWS = S + T, B * S
BIG = -30000.0
FACTOR = 5.0            # see profiles/kernel_tests_coverage.md for the measured ratios


def held(got, want, yard, floor, what):
    return _held(got, want, yard, floor, what, factor=FACTOR)


# ------------------------------------------------------------------ inputs
def region_cols(V, nt=256):
    """one column in each region of a 256-lane streaming kernel that this V has: the first chunk, lane 0's fourth chunk of the first
    unrolled trip, a middle chunk, the last whole chunk (the remainder loop unless the trips divide V), the scalar tail"""
    V8 = V // 8
    cols = [min(3, V - 1)]
    if V8 > 3 * nt:
        cols.append(3 * nt * 8 + 1)
    if V8 > 300:
        cols.append(300 * 8 + 6)
    if V8 > 1:
        cols.append((V8 - 1) * 8 + 2)
    if V % 8:
        cols.append(V - 1)
    return sorted(set(cols))


def logits_rows(dtype, V, seed, scale=2.0, shift=3000.0):
    """rows 0-2: a row on a grid that survives a shift by 3000 in ``dtype`` (eight columns share the maximum), the row + 3000, the
    row - 3000; 3: one logit 120 above the rest; 4: all equal; 5-8: the maximum planted in each region in turn with a duplicate at a
    higher index in another region; 9: randn"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, V, generator=g) * scale
    grid, kmax = (16.0, 3) if dtype == BF else (2.0 ** -8, 2048)
    k = torch.randint(1, kmax + 1, (V,), generator=g).double()
    k[torch.randperm(V, generator=g)[:8 if V >= 64 else 1]] = 0
    base = -grid * k - (8.0 if dtype == BF and shift == 3000.0 else 0.0)           # (bf16 near 3000 holds multiples of 16: 3000 - 8 - 16 k)
    x[0], x[1], x[2] = base, base + shift, base - shift
    x[3, V // 2] = 125.0
    x[4] = 0.5
    cols = region_cols(V)
    for i in range(4):
        c = cols[i % len(cols)]
        higher = [h for h in cols if h > c] or ([V - 1] if V - 1 > c else [])
        x[5 + i, c] = 12.0
        if higher:
            x[5 + i, higher[i % len(higher)]] = 12.0
    x = x.to(dtype)
    assert torch.equal(x[1].double() - shift, x[0].double()) and torch.equal(x[2].double() + shift, x[0].double())
    return x


def first_argmax(x):
    m = x.max(-1, keepdim=True).values
    idx = torch.arange(x.shape[-1]).expand_as(x).clone()
    idx[x != m] = x.shape[-1]
    return idx.min(-1).values


def teacher_side(V, seed):
    """the generator, random teacher draft logits zt [B, SPAD, V] bf16 and pod_scale [B, SPAD]; the case plants its rows, then finish_teacher"""
    g = torch.Generator().manual_seed(seed + 1000)
    zt = (torch.randn(B, SPAD, V, generator=g) * 2).to(BF)
    pod = torch.rand(B, SPAD, generator=g)
    return g, zt, pod


def finish_teacher(zt, pod, halves=(), ties=()):
    """zmd / zinv per padded position (``halves``: zinv halved, so tsum = 1/2; ``ties``: zmd = 0, zinv = 1/4, pod = 1), the float64 target
    p = exp(zt - zmd) * zinv the kernels re-form and its fp32 rounding unit"""
    zmd = zt.float().max(-1).values
    zinv = (1.0 / torch.exp(zt.float() - zmd[..., None]).sum(-1)).float()
    for b, s in halves:
        zinv[b, s] *= 0.5
    for b, s in ties:
        zmd[b, s], zinv[b, s], pod[b, s] = 0.0, 0.25, 1.0
    p = torch.exp(zt.double() - zmd.double()[..., None]) * zinv.double()[..., None]
    fp = p * ulp(torch.maximum(zt.double().abs(), zmd.double().abs()[..., None]), F32) + 2 * ulp(p, F32)
    return zmd, zinv, p, fp


# ------------------------------------------------------------------ fused CE
def case_ce(dev, dtype, V, form, off, seed=0):
    """form 'p': sf_ce_fused on fp32 probabilities, dense rows; 'zt': sf_ce_fused_zt, compact rows (row_map), St = S, so rows with
    s + off >= S are masked by the kernel whatever pos_mask says; 'zt_rows': sf_ce_fused_zt_rows with St = S + T, dense rows"""
    x = logits_rows(dtype, V, seed)
    St = S if form == "zt" else SPAD
    g, zt, pod = teacher_side(V, seed)
    pr = lambda r: (r // S, r % S + off)
    zt[pr(5)] = BIG
    zt[pr(5)][V // 3] = 0.0                                    # row 5: a one-hot target
    pod[pr(3)], pod[pr(4)] = 1.0, 0.0
    zmd, zinv, p, fp = finish_teacher(zt, pod, halves=[pr(6)])    # row 6: tsum = 1/2
    if form == "p":
        target = p.float()
        p, fp = target.double(), torch.zeros_like(p)
    tsum = p.sum(-1).float()
    pos = torch.ones(B, SPAD, dtype=torch.int32)
    pos[pr(9)] = 0
    lm = torch.randint(0, 2, (B, SPAD), generator=g, dtype=torch.int32)
    d2t = torch.cumsum(torch.randint(0, 3, (V,), generator=g), 0)
    pred = first_argmax(x.double())
    tgt = torch.full((B, SPAD), -1, dtype=torch.int64)
    for r in range(0, ROWS, 2):
        tgt[pr(r)] = pred[r] + d2t[pred[r]]
    tgt[pr(1)] = pred[1] + d2t[pred[1]] + 1                      # a miss by one
    keep = torch.tensor([0, 1, 2, 3, 5, 6, 7, 9]) if form == "zt" else torch.arange(ROWS)
    n = keep.numel()
    sl = lambda t: torch.stack([t[pr(int(r))] for r in keep])
    pm = sl(pos).double() * torch.tensor([float(int(r) % S + off < St) for r in keep], dtype=torch.float64)
    assert 0 < int(pm.sum()) < n
    gs = 0.37
    gs32 = float(torch.tensor(gs, dtype=F32))
    # float64 reference
    xk = x[keep]
    x64 = xk.double()
    lse = torch.logsumexp(x64, -1, keepdim=True)
    s = torch.exp(x64 - lse)
    pk, fpk, podk, tsk = sl(p), sl(fp), sl(pod).double()[:, None], sl(tsum).double()[:, None]
    loss = -(pk * (x64 - lse)).sum(-1) * pm
    accept = torch.minimum(pk * podk, s).sum(-1) * pm
    grad = gs32 * pm[:, None] * (s * tsk - pk)
    # the same formulas in fp32
    x32 = xk.float()
    lse32 = torch.logsumexp(x32, -1, keepdim=True)
    lp32 = x32 - lse32
    s32 = torch.exp(lp32)
    p32 = sl(target) if form == "p" else torch.exp(sl(zt).float() - sl(zmd)[:, None]) * sl(zinv)[:, None]
    pm32, pod32, ts32 = pm.float(), sl(pod)[:, None], sl(tsum)[:, None]
    loss32 = -(p32 * lp32).sum(-1) * pm32
    accept32 = torch.minimum(p32 * pod32, s32).sum(-1) * pm32
    grad32 = (s32 * ts32 - p32) * (gs32 * pm32)[:, None]
    # floors
    eL = ulp(torch.maximum(x64.abs().max(-1, keepdim=True).values, lse.abs()), F32)
    fs = s * eL + ulp(s, F32)
    f_loss = (fpk * (x64 - lse).abs() + pk * eL).sum(-1) + ulp(torch.maximum((pk * x64.abs()).sum(-1), tsk[:, 0] * lse[:, 0].abs()), F32)
    f_acc = torch.where(s < pk * podk, fs, fpk * podk).sum(-1) + ulp(accept, F32)
    f_grad = gs32 * pm[:, None] * (tsk * fs + fpk + ulp(torch.maximum(s * tsk, pk), F32))
    # run
    d = lambda t: t.to(dev)
    bx, vx = wide(xk, 8, 16 + (-V) % 8, dev, rows_extra=2)
    outs = [torch.full((n + 2,), MARK, device=dev) for _ in range(3)]
    row_pred = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    kw = dict(S=S, Spad=SPAD, off=off, pos_mask_pad=d(pos), loss_mask_pad=d(lm), tgt_ids_pad=d(tgt), pod_scale_pad=d(pod), tsum_pad=d(tsum),
              d2t=d(d2t), grad_scale=gs, row_loss=outs[0], row_correct=outs[1], row_accept=outs[2], row_pred=row_pred,
              row_map=d(keep) if form == "zt" else None)
    if form == "p":
        ops.ce_fused(vx, d(target), **kw)
    else:
        bz, vz = wide(zt[:, :St].reshape(B * St, V), 16, 8, dev, rows_extra=1)
        if form == "zt":
            ops.ce_fused_zt(vx, vz, d(zmd), d(zinv), **kw)
        else:
            ops.ce_fused_zt_rows(vx, vz, d(zmd), d(zinv), St=St, **kw)
        assert outside_untouched(bz, B * St, 16, V) and torch.equal(vz.cpu(), zt[:, :St].reshape(B * St, V))
    tag = f"ce[{form}]"
    assert outside_untouched(bx, n, 8, V)
    assert all(bool((o[n:].cpu() == MARK).all()) for o in outs) and bool((row_pred[n:].cpu() == -7).all())
    assert torch.equal(row_pred[:n].cpu().long(), pred[keep])
    hit = (pred[keep] + d2t[pred[keep]]) == sl(tgt)
    assert torch.equal(outs[1][:n].cpu(), torch.where(hit, sl(lm).float(), torch.zeros(n)))
    held(outs[0][:n], loss, loss32, f_loss, tag + " row_loss")
    held(outs[2][:n], accept, accept32, f_acc, tag + " row_accept")
    got = vx.cpu()
    masked = pm == 0
    assert not bool(got[masked].float().any()) and not bool(outs[0][:n].cpu()[masked].any()) and not bool(outs[2][:n].cpu()[masked].any())
    if dtype == F32:
        held(got, grad, grad32, f_grad, tag + " grad fp32")
    else:
        bf16_bits(got, grad, FACTOR * f_grad, tag + " grad")


CE_V = [8, 2040, 2056, 6152, 8192, 8200, 16392]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("form", ["p", "zt", "zt_rows"])
@pytest.mark.parametrize("V", CE_V)
def test_ce_fused_against_float64(backend, dtype, form, V):
    """offsets 0, 2 and T in turn (the 'zt' form, whose rows past S - off are masked by the kernel, only 0 and 2)"""
    i = CE_V.index(V)
    off = [0, 2][i % 2] if form == "zt" else [0, 2, T][(i + (form == "p")) % 3]
    case_ce(backend, dtype, V, form, off, seed=i + 10 + (3 if V == 8 else 0))      # (V = 8: a seed whose 80 elements meet the 2 % cap)


# ------------------------------------------------------------------ LK gradients
def lk_lanes(V):
    nt = ((V // 8 + 3) // 4 + 63) // 64 * 64
    return min(max(nt, 256), 1024)


def _lk(x, p, pod, tsum, m, mode, kl_scale, kl_decay, step, kl_row_scale, accept_sum, mask_sum):
    """the LK gradient as the comment above ce_lk_grad_kernel defines it, in the dtype of its arguments; softmax as exp(x - max) / sum
    (exact on the planted tie rows in either precision)"""
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    s = e / e.sum(-1, keepdim=True)
    q = p * pod
    a = torch.minimum(q, s).sum(-1, keepdim=True)
    ind = (s < q).to(x.dtype) + 0.5 * (s == q).to(x.dtype)
    c = (ind * s).sum(-1, keepdim=True)
    D = mask_sum.clamp_min(1e-8)
    if mode == "alpha":
        ka, kb = torch.zeros_like(a), torch.where(a > 0, -step / (D * a), torch.zeros_like(a))
    else:
        w = kl_scale * torch.exp(-kl_decay * accept_sum / D)
        ka, kb = (step * kl_row_scale * w).expand_as(a), (-step * (1 - w) / D).expand_as(a)
    return m[:, None] * (ka * (s * tsum - p) + kb * s * (ind - c)), dict(s=s, q=q, a=a, ind=ind, c=c, ka=ka * m[:, None], kb=kb * m[:, None])


def case_lk(dev, dtype, V, form, compact=False, St=S, off=1, seed=0):
    """form 'zt': sf_ce_lk_grad_zt_rows (dense or row_map, St teacher rows); 'p': sf_ce_lk_grad on fp32 probabilities.  Both objectives.
    Rows 7 and 8 carry exact ties s == q == 1/4 (s = 1/4 on four columns, q = 1/4 on three): in a register chunk with u >= 1, in a
    streamed chunk and in the tail where this V has them.  Rows 1 and 2 are row 0 shifted by +-3000 for fp32 logits and by +-32 for bf16
    logits.  Every element of an LK gradient row scales with a_r and c_r, which carry the relative error ulp32(lse) of the softmax --
    2.4e-4 at 3000: half the bf16 elements of such a row would lie inside the rounding window (the 2 % cap is on the input), so the
    bf16 +-3000 rows are in the CE and teacher cases only.  An fp32 gradient is held by a ratio, and fp32 cannot tell s < q from s > q
    within that error, so the targets of the fp32 rows 1 and 2 are built from row 0 itself: zt = x0 +- 1 with pod_scale = 1 puts every
    q a factor of about 1.8 above or 4 below its s (no near-tie, asserted below for every input)."""
    nt = lk_lanes(V) if form == "zt" else 256
    St = St if form == "zt" else SPAD                         # (the fp32-target form has a target row at every padded position)
    x = logits_rows(dtype, V, seed, scale=1.5, shift=3000.0 if dtype == F32 else 32.0)
    g, zt, pod = teacher_side(V, seed)
    pr = lambda r: (r // S, r % S + off)
    if dtype == F32:
        sign = torch.randint(0, 2, (V,), generator=torch.Generator().manual_seed(seed + 5)).float() * 2 - 1
        for r in (1, 2):
            zt[pr(r)] = (x[0] + sign).to(BF)
            pod[pr(r)] = 1.0
    V8 = V // 8
    t1 = (5 + nt) * 8 + 3 if 5 + nt < V8 else 9
    t2 = V - 1 if V % 8 else (32768 + 8 * 7 + 1 if V > 32768 + 64 else (V8 - 1) * 8 + 6)
    if V > 32768 + 8 and V - 1 != t2:
        t2b = 32768 + 2                                         # lane 0's first streamed chunk
    else:
        t2b = 40
    tie_cols = sorted({t1, t2, t2b})
    others = [c for c in (0, 17, 70, 100, 120) if c not in tie_cols]
    ties = []
    for r in (7, 8):           # s = 1/4 on four columns, q = 1/4 on three: ties on tie_cols, s > q on the rest of the four, s < q where only zt is 0
        x[r] = BIG
        x[r, tie_cols + others[:4 - len(tie_cols)]] = 0.0
        zt[pr(r)] = BIG
        zt[pr(r)][tie_cols + others[3:3 + 3 - len(tie_cols)]] = 0.0
        ties.append(pr(r))
    pod[pr(3)], pod[pr(4)] = 1.0, 0.0
    zmd, zinv, p, fp = finish_teacher(zt, pod, halves=[pr(6)], ties=ties)
    if form == "p":
        target = p.float()
        p, fp = target.double(), torch.zeros_like(p)
    tsum = p.sum(-1).float()
    pos = torch.ones(B, SPAD, dtype=torch.int32)
    pos[pr(9)] = 0
    keep = torch.tensor([0, 1, 2, 3, 4, 6, 7, 8, 9]) if compact else torch.arange(ROWS)
    n = keep.numel()
    sl = lambda t: torch.stack([t[pr(int(r))] for r in keep])
    m = sl(pos).double() * torch.tensor([float(int(r) % S + off < St) for r in keep], dtype=torch.float64)
    xk = x[keep]
    x64, pk, fpk, podk, tsk = xk.double(), sl(p), sl(fp), sl(pod).double()[:, None], sl(tsum).double()[:, None]
    hyper = dict(kl_scale=0.7, kl_decay=1.5, step=0.64, kl_row_scale=1.0 / 7)
    f32 = lambda v: torch.tensor(v, dtype=F32)
    d = lambda t: t.to(dev)
    for mode in ("alpha", "lambda"):
        _, parts = _lk(x64, pk, podk, tsk, m, mode, accept_sum=torch.tensor(1.0).double(), mask_sum=m.sum(), **hyper)
        accept_sum, mask_sum = f32(float((m * parts["a"][:, 0]).sum())), f32(float(m.sum()))
        h64 = {k: float(f32(v)) for k, v in hyper.items()}
        grad, q = _lk(x64, pk, podk, tsk, m, mode, accept_sum=accept_sum.double(), mask_sum=mask_sum.double(), **h64)
        p32 = sl(target) if form == "p" else torch.exp(sl(zt).float() - sl(zmd)[:, None]) * sl(zinv)[:, None]
        grad32, _ = _lk(xk.float(), p32, sl(pod)[:, None], sl(tsum)[:, None], m.float(), mode, accept_sum=accept_sum, mask_sum=mask_sum,
                        **{k: f32(v) for k, v in hyper.items()})
        # floors; and no element but the planted ties may sit where fp32 cannot tell s < q from s > q
        lse = torch.logsumexp(x64, -1, keepdim=True)
        eL = ulp(torch.maximum(x64.abs().max(-1, keepdim=True).values, lse.abs()), F32)
        sv, qv, ind, c = q["s"], q["q"], q["ind"], q["c"]
        fs = sv * eL + ulp(sv, F32)
        fq = fpk * podk + ulp(qv, F32)
        close = ((sv - qv).abs() <= 2 * FACTOR * (fs + fq)) & (sv != qv) & (torch.maximum(sv, qv) > 1e-30) & (m[:, None] > 0)
        if bool(close.any()):
            raise InputRejected(("near-tie in the input: pick another seed", int(close.sum())))
        fa = torch.where(sv < qv, fs, fq).sum(-1, keepdim=True) + ulp(q["a"], F32)
        fc = (ind * fs).sum(-1, keepdim=True) + ulp(c, F32)
        ka, kb = q["ka"].abs(), q["kb"].abs()
        rel_kb = (torch.where(q["a"] > 0, fa / q["a"].clamp_min(1e-300), torch.zeros_like(fa)) if mode == "alpha" else 0.0) + 2.0 ** -22
        floor = (ka * (tsk * fs + fpk + ulp(torch.maximum(sv * tsk, pk), F32))
                 + kb * (fs * (ind - c).abs() + sv * fc + ulp(sv * torch.maximum(ind, c), F32) + sv * (ind - c).abs() * rel_kb))
        assert int(((sv == qv) & (sv > 0) & (m[:, None] > 0)).sum()) >= len(tie_cols)
        bx, vx = wide(xk, 8, 16 + (-V) % 8, dev, rows_extra=2)
        kw = dict(S=S, Spad=SPAD, off=off, pos_mask_pad=d(pos), pod_scale_pad=d(pod), tsum_pad=d(tsum), lk_loss_type=mode,
                  kl_scale=hyper["kl_scale"], kl_decay=hyper["kl_decay"], step_scale=hyper["step"], kl_row_scale=hyper["kl_row_scale"],
                  accept_sum=d(accept_sum.view(1)), mask_sum=d(mask_sum.view(1)))
        if form == "p":
            ops.ce_lk_grad(vx, d(target), **kw)
        else:
            bz, vz = wide(zt[:, :St].reshape(B * St, V), 16, 8 + (-V) % 8, dev, rows_extra=1)
            ops.ce_lk_grad_zt(vx, vz, d(zmd), d(zinv), St=St, row_map=d(keep) if compact else None, **kw)
            assert outside_untouched(bz, B * St, 16, V)
        assert outside_untouched(bx, n, 8, V)
        got = vx.cpu()
        assert not bool(got[m == 0].float().any())
        tag = f"lk[{form},{mode}]"
        if dtype == F32:
            held(got, grad, grad32, floor, tag + " grad fp32")
        else:
            bf16_bits(got, grad, FACTOR * floor, tag + " grad")


LK_V = [136, 8192, 8200, 8197, 16392, 32768, 32776, 32779, 40968]
LK_VARIANTS = [(False, S), (True, SPAD), (False, SPAD), (True, S)]
# seeds whose inputs meet the two conditions case_lk asserts from the float64 reference alone (no near-tie; <= 2 % of the bf16 elements
# next to a rounding boundary -- the bf16 grid rows hold four distinct logits, so their gradients come in clusters of equal values)
LK_SEED_SHIFT = {(136, 0): 1, (8192, 0): 1, (16392, 1): 1, (32768, 0): 1, (40968, 0): 9}


def lk_zt_args(V, variant):
    compact, St = LK_VARIANTS[(LK_V.index(V) + 2 * variant) % 4]
    return dict(compact=compact, St=St, off=[1, 2][variant], seed=V % 97 + LK_SEED_SHIFT.get((V, variant), 0))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V,variant", [(V, v) for V in LK_V for v in ((0, 1) if V < 32768 else (0,))])
def test_ce_lk_grad_zt_rows_against_float64(backend, dtype, variant, V):
    """256 lanes (136, 8192), 320 lanes (8200; 8197 with a tail), more than one register chunk per lane (16392), 1024 lanes with every
    chunk in registers (32768), the first streamed chunk without and with a tail (32776, 32779), a lane with two streamed chunks
    (40968); dense and row_map, St = S and S + T, paired so that each V below 32768 meets both layouts and both St.  (The interpreter
    runs the largest in under a second, so none is GPU only.)"""
    case_lk(backend, dtype, V, "zt", **lk_zt_args(V, variant))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [136, 2061])
def test_ce_lk_grad_against_float64(backend, dtype, V):
    case_lk(backend, dtype, V, "p", off=2, seed=V % 97)


# ------------------------------------------------------------------ teacher reductions
def draft_columns(Vt, Vd, g, first=None):
    cols = torch.sort(torch.randperm(first or Vt, generator=g)[:Vd]).values
    if Vt % 8 and first is None and Vt - 2 not in cols:
        cols[-1] = Vt - 2                                       # a draft column inside the scalar tail
    return cols


def teacher_reference(z, cols, lm):
    """float64 and fp32 values of the teacher reduction of natural-layout rows z (storage dtype), draft columns ``cols``"""
    out = {}
    for name, dt in (("ref", torch.float64), ("yard", F32)):
        zz = z.to(dt)
        zd = zz[:, cols]
        md = zd.max(-1, keepdim=True).values
        e = torch.exp(zd - md)
        sd = e.sum(-1, keepdim=True)
        p = e / sd
        out[name] = dict(p=p, pod=torch.exp(md[:, 0] + torch.log(sd[:, 0]) - torch.logsumexp(zz, -1)), tsum=p.sum(-1), zmd=md[:, 0], zinv=1.0 / sd[:, 0])
    r, z64 = out["ref"], z.double()
    md, lse = r["zmd"], torch.logsumexp(z64, -1)
    eD = ulp(torch.maximum(z64[:, cols].abs().max(-1).values, md.abs()), F32)
    fp = r["p"] * ulp(torch.maximum(z64[:, cols].abs(), md.abs()[:, None]), F32) + 2 * ulp(r["p"], F32) + r["p"] * eD[:, None]
    out["floor"] = dict(p=fp, tsum=fp.sum(-1), zinv=r["zinv"] * (eD + 2.0 ** -23),
                        pod=r["pod"] * (eD + ulp(torch.maximum(md.abs(), lse.abs()), F32) + ulp(lse, F32)) + ulp(r["pod"], F32) + 2.0 ** -126)     # (a denormal result may flush to 0)
    ids = first_argmax(z64)
    t2d = torch.zeros(z.shape[1], dtype=torch.uint8)
    t2d[cols] = 1
    out["ids"], out["t2d"] = ids, t2d
    out["pos"] = t2d[ids].int() * lm
    return out


def check_teacher(o, ref, tag, tp=True):
    rows = lambda t: t.cpu()[:, :S].reshape(ROWS, *t.shape[2:])
    for t in o.values():
        if t is not None:
            assert bool((t.cpu()[:, S:] == (MARK if t.dtype == F32 else -7)).all()), "padded positions were written"
    assert torch.equal(rows(o["ids"]), ref["ids"]) and torch.equal(rows(o["pos"]), ref["pos"])
    names = ["pod", "tsum"] + (["p"] if tp else []) + (["zinv"] if o.get("zinv") is not None else [])
    for k in names:
        held(rows(o[k]), ref["ref"][k], ref["yard"][k], ref["floor"][k], f"{tag} {k}")
    if o.get("zmd") is not None:
        assert torch.equal(rows(o["zmd"]).double(), ref["ref"]["zmd"])


def teacher_outputs(dev, Vd, tp=True, zmd=False):
    f = lambda *s: torch.full(s, MARK, device=dev)
    i = lambda dt: torch.full((B, SPAD), -7, dtype=dt, device=dev)
    return dict(p=f(B, SPAD, Vd) if tp else None, pod=f(B, SPAD), tsum=f(B, SPAD), ids=i(torch.int64), pos=i(torch.int32),
                zmd=f(B, SPAD) if zmd else None, zinv=f(B, SPAD) if zmd else None)


def case_teacher(dev, dtype, Vt, Vd, first=None, seed=0):
    """sf_teacher_reduce (natural layout, d2t gather, t2d mask words)"""
    g = torch.Generator().manual_seed(seed + 50)
    cols = draft_columns(Vt, Vd, g, first)
    z = logits_rows(dtype, Vt, seed)
    lm = torch.randint(0, 2, (B, SPAD), generator=g, dtype=torch.int32)
    ref = teacher_reference(z, cols, lm[:, :S].reshape(ROWS))
    d2t = cols - torch.arange(Vd)
    bz, vz = wide(z, 8, 8 + (-Vt) % 8, dev, rows_extra=1)
    o = teacher_outputs(dev, Vd)
    ops.teacher_reduce(vz, Vd=Vd, d2t=d2t.to(dev), t2d_u8=ref["t2d"].to(dev), loss_mask_pad=lm.to(dev), S=S, Spad=SPAD, target_p_pad=o["p"],
                       pod_scale_pad=o["pod"], tsum_pad=o["tsum"], ids_pad=o["ids"], pos_mask_pad=o["pos"])
    assert outside_untouched(bz, ROWS, 8, Vt) and torch.equal(vz.cpu(), z)
    check_teacher(o, ref, "teacher_reduce")


TEACHER = [(8, 3, None), (2040, 96, None), (2056, 100, 512), (6152, 2048, None), (8192, 2056, None), (8200, 2048, None), (16392, 2056, None),
           (8197, 2048, None), (6157, 1801, None)]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("Vt,Vd,first", TEACHER)
def test_teacher_reduce_against_float64(backend, dtype, Vt, Vd, first):
    """Vt on each side of every loop of the streaming pass (8197 and 6157: a scalar tail that holds a draft column); Vd on each side of
    the batched gather (8 x 256 = 2048); Vt = 2056 with every draft column in the first 512 columns: waves 1-3 hold none"""
    case_teacher(backend, dtype, Vt, Vd, first, seed=Vt % 89)


def case_teacher_perm(dev, dtype, Vt, Vd, nparts, tp=True, seed=0):
    """sf_teacher_reduce_perm: draft columns first; the last 128 * nparts permuted columns arrive as hand-written (max, sum-exp, argmax
    column) records computed in float64 from the full row.  Rows 3-6: the draft maximum 59, 61, 95 and 200 below the row maximum (the
    switch between the shared-term sum and the exact re-sum is at 60); 7: the row maximum at a draft column AND in the last column
    block (a record, with nparts); 8: the maximum only there; 9: the maximum in lane 0's fourth unrolled chunk and at a draft column"""
    g = torch.Generator().manual_seed(seed + 70)
    cols = draft_columns(Vt, Vd, g, first=Vt - 1)
    rest = torch.tensor(sorted(set(range(Vt)) - set(cols.tolist())), dtype=torch.long)
    perm = torch.cat([cols, rest])
    z = logits_rows(dtype, Vt, seed).float()
    top = int(rest[len(rest) // 2])
    for r, gap in ((3, 59.0), (4, 61.0), (5, 95.0), (6, 200.0)):
        z[r] = torch.randn(Vt, generator=g)
        z[r, top] = 10.0
        z[r, cols] = 10.0 - gap - torch.randn(Vd, generator=g).abs() * 2
        z[r, cols[7 % Vd]] = 10.0 - gap
    last = int(perm[Vt - 3])
    z[7] = torch.randn(Vt, generator=g)
    z[7, cols[5 % Vd]] = z[7, last] = 12.0
    z[8] = torch.randn(Vt, generator=g)
    z[8, last] = 12.0
    z[9] = torch.randn(Vt, generator=g)
    z[9, cols[2 % Vd]] = 12.0
    if Vt - 128 * nparts > 769 * 8:
        z[9, perm[768 * 8 + 1]] = 12.0
    z = z.to(dtype)
    lm = torch.randint(0, 2, (B, SPAD), generator=g, dtype=torch.int32)
    ref = teacher_reference(z, cols, lm[:, :S].reshape(ROWS))
    Vz = Vt - 128 * nparts
    assert Vz >= Vd
    zp = z[:, perm]
    part = None
    if nparts:
        part = torch.full((ROWS + 1, nparts + 2, 4), MARK)
        for q in range(nparts):
            blk = zp[:, Vz + 128 * q: Vz + 128 * (q + 1)].double()
            bm = blk.max(-1).values
            part[:ROWS, q, 0], part[:ROWS, q, 1] = bm.float(), torch.exp(blk - bm[:, None]).sum(-1).float()
            part[:ROWS, q, 2], part[:ROWS, q, 3] = (Vz + 128 * q + first_argmax(blk)).float(), 0.0
        part = part.to(dev)
    bz, vz = wide(zp[:, :Vz].contiguous(), 8, 8 + (-Vz) % 8, dev, rows_extra=1)
    o = teacher_outputs(dev, Vd, tp=tp, zmd=True)
    ops.teacher_reduce_perm(vz, Vt=Vt, Vd=Vd, perm=perm.int().to(dev), t2d_u8=ref["t2d"].to(dev), loss_mask_pad=lm.to(dev), S=S, Spad=SPAD,
                            target_p_pad=o["p"], pod_scale_pad=o["pod"], tsum_pad=o["tsum"], ids_pad=o["ids"], pos_mask_pad=o["pos"],
                            part=part, nparts=nparts, zmd_pad=o["zmd"], zinv_pad=o["zinv"])
    assert outside_untouched(bz, ROWS, 8, Vz)
    check_teacher(o, ref, "teacher_reduce_perm", tp=tp)


PERM = [(16, 8, 0, True), (2040, 96, 0, True), (2056, 104, 0, False), (6152, 2048, 0, True), (8192, 2056, 0, True), (8200, 2048, 0, False),
        (16392, 2056, 0, True), (8197, 2048, 0, True), (6157, 1800, 0, True), (2056 + 256, 104, 2, True), (8200 + 384, 2048, 3, True),
        (8197 + 128, 2048, 1, False)]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("Vt,Vd,nparts,tp", PERM)
def test_teacher_reduce_perm_against_float64(backend, dtype, Vt, Vd, nparts, tp):
    """the Vt set of the streaming loops, Vz % 8 != 0, column blocks past Vz as ``part`` records, with and without target_p"""
    case_teacher_perm(backend, dtype, Vt, Vd, nparts, tp, seed=Vt % 83)
