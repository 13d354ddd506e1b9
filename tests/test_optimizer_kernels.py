"""The kernels that write every weight and every logged number, against float64 references written from the definition of the
operation: sf_grad_norm, sf_adamw_step (BF16Optimizer.step of the reference, optimizer.py:85-168: fp32 norm of the gradients,
clamp(max_norm / (norm + 1e-6), max=1), torch.optim.AdamW on fp32 masters, params = T(master)), sf_eagle3_metrics, sf_axpy_f32 and
sf_reduce_sum.  The C-ABI carries the hyperparameters as fp32: they are rounded to fp32 ONCE here and the float64 recurrence, the
yardstick (torch.optim.AdamW, fp32, CPU) and the kernel all get those values (fp32(0.999) differs from 0.999 by 1.3e-8, which is a
1.3e-5 relative difference in 1 - beta2: a different hyperparameter, not an arithmetic error of anybody).

Every case runs under the SIMT interpreter and on the GPU (``backend``); the sizes with a second grid-stride trip are GPU only."""
import json
import math
import os
import random

import pytest
import torch

from specforge_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 16            # guard elements on both sides of every stream (16 elements keep a 2- or 4-byte stream 16-byte aligned)
GUARD = 7.5       # exact in bf16


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def ulp32(x):
    """spacing of fp32 at |x| (float64 in, float64 out)"""
    a = x.detach().double().abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def guarded(vals, off, dev):
    """vals inside a larger allocation, ``off`` elements past a 16-byte boundary, G guard elements before and after"""
    n = vals.numel()
    buf = torch.full((G + off + n + G,), GUARD, dtype=vals.dtype)
    buf[G + off:G + off + n] = vals
    buf = buf.to(dev)
    return buf, buf[G + off:G + off + n]


def guards_intact(buf, off, n):
    b = buf.cpu()
    return bool((b[:G + off] == GUARD).all()) and bool((b[G + off + n:] == GUARD).all())


@pytest.fixture
def gpu():
    from specforge_amd import _lib

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _lib._inject_library_for_tests(None)
    _lib.lib()
    return "cuda"


@pytest.fixture
def emu(emu_lib_path):
    from specforge_amd import _lib

    _lib._inject_library_for_tests(emu_lib_path)
    yield "cpu"
    _lib._inject_library_for_tests(None)


# ------------------------------------------------------------------ float64 definitions
def adamw64(g, p, m, v, norm, *, max_norm, lr, betas, eps, wd, step, prescale):
    """one BF16Optimizer.step on flat buffers in float64 (max_norm <= 0: no clipping, the kernel's contract)"""
    g, p, m, v = g.double(), p.double(), m.double(), v.double()
    clip = min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 else 1.0
    g = g * (clip * prescale)
    b1, b2 = betas
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    return p, m, v


def adamw_torch(g, p, m, v, norm, *, max_norm, lr, betas, eps, wd, step, prescale):
    """the yardstick: the reference's inner optimizer (torch.optim.AdamW, fp32, CPU) on the same inputs, the gradient clipped the
    way optimizer.py:92,154 does it"""
    g32 = g.float() * prescale
    if max_norm > 0:
        g32 = g32 * torch.clamp(max_norm / (norm.float().cpu() + 1e-6), max=1.0)
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([q], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    q.grad = g32.reshape(q.shape)
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


def max_rel(x, ref):
    nz = ref != 0
    assert bool((x.double()[~nz] == 0).all())
    return float(((x.double()[nz] - ref[nz]).abs() / ref[nz].abs()).max()) if bool(nz.any()) else 0.0


def check_norm(norm, g, prescale, tag=""):
    """|kernel - fp64| <= max(2 x the error of the reference's fp32 expression, 2^-22 relative).  Returns (kernel, yardstick) errors."""
    want = float(g.double().square().sum().sqrt()) * prescale
    yard = float(g.float().square().sum().sqrt()) * prescale
    got = float(norm.cpu()[0])
    ek, ey = abs(got - want), abs(yard - want)
    print(f"norm{tag}: n={g.numel()} kernel_rel={ek / max(want, 1e-300):.3e} yardstick_rel={ey / max(want, 1e-300):.3e}")
    assert ek <= max(2 * ey, 2.0 ** -22 * want), (got, want, yard)
    return ek / max(want, 1e-300), ey / max(want, 1e-300)


def case_adamw(dev, *, n, gdtype, wd, prescale, max_norm, step0, betas, eps, offs, nsteps, seed, lr=1e-2):
    """``nsteps`` chained steps on two copies of the same values: every stream 16-byte aligned (8 parameters per trip) and every
    stream ``offs[i]`` elements past a 16-byte boundary (one parameter per trip).  Returns the largest kernel / yardstick error
    ratio seen (max relative error per tensor, both against float64)."""
    gen = torch.Generator().manual_seed(seed)
    lr, wd, eps, max_norm, prescale = f32(lr), f32(wd), f32(eps), f32(max_norm), f32(prescale)
    betas = (f32(betas[0]), f32(betas[1]))
    p0 = torch.randn(n, generator=gen)
    fresh = step0 == 1
    m0 = torch.zeros(n) if fresh else 0.1 * torch.randn(n, generator=gen)
    v0 = torch.zeros(n) if fresh else 0.01 * torch.rand(n, generator=gen) + 1e-6
    streams = {}
    for name, o in (("A", (0,) * 5), ("B", offs)):
        streams[name] = [guarded(t, off, dev) for t, off in zip(
            (torch.zeros(n, dtype=gdtype), p0, m0, v0, p0.to(gdtype)), o)]
    assert all(v.data_ptr() % 16 == 0 for _, v in streams["A"]) or n == 0
    assert any(v.data_ptr() % 16 for _, v in streams["B"]) or n == 0
    norm = torch.empty(1, device=dev)
    worst = 0.0
    for s in range(nsteps):
        step = step0 + s
        g = torch.randn(n, generator=gen).to(gdtype)
        for name in "AB":
            streams[name][0][1].copy_(g)
        ws = torch.full((1024,), float("nan"), device=dev)          # the workspace may hold anything on entry
        ops.grad_norm(streams["A"][0][1], norm, ws, prescale)
        check_norm(norm, g, prescale)
        pre = [streams["A"][i][1].cpu().clone() for i in (1, 2, 3)]
        kw = dict(max_norm=max_norm, lr=lr, eps=eps, wd=wd, step=step)
        for name in "AB":
            (_, gv), (_, pv), (_, mv), (_, vv), (_, qv) = streams[name]
            ops.adamw_step(gv, pv, mv, vv, qv, norm, beta1=betas[0], beta2=betas[1], grad_prescale=prescale, **kw)
        got = {name: [streams[name][i][1].cpu().clone() for i in (1, 2, 3, 4)] for name in "AB"}
        for name, o in (("A", (0,) * 5), ("B", offs)):
            for (buf, _), off in zip(streams[name], o):
                assert guards_intact(buf, off, n), (name, off)
            # the kernel rounds the master once: the stored parameter is T(master), bit for bit
            assert torch.equal(bits(got[name][3]), bits(got[name][0].to(gdtype))), name
        # the aligned (8 per trip) and the one-per-trip launch: the same bits (the kernel leaves no contraction to the compiler)
        for a, b, what in zip(got["A"], got["B"], ("master", "exp_avg", "exp_avg_sq", "param")):
            assert torch.equal(bits(a), bits(b)), f"aligned and one-per-trip launches differ in {what} at step {step}"
        ref = adamw64(g, *pre, norm.cpu()[0], betas=betas, prescale=prescale, **kw)
        yard = adamw_torch(g, *pre, norm, betas=betas, prescale=prescale, **kw)
        # exp_avg = beta1 * m + (1 - beta1) * g' and master = p' - update are sums whose terms can cancel: where they do, ANY fp32
        # evaluation is off by up to half an ulp of each rounded TERM, a large relative error of a small result, and whether the
        # kernel or torch (exp_avg by lerp, m + w * (g' - m): another expression) comes out nearer at one such element is chance.
        # "2 ulps of the element" is therefore taken at the element's largest fp32 quantity: the result or a term of its last sum
        # (exp_avg_sq sums positive terms: there it is the result).
        clip = min(1.0, max_norm / (float(norm.cpu()[0]) + 1e-6)) if max_norm > 0 else 1.0
        decayed = pre[0].double() * (1.0 - lr * wd)
        terms = dict(master=torch.maximum(decayed.abs(), (ref[0] - decayed).abs()), exp_avg_sq=ref[2].abs(),
                     exp_avg=torch.maximum(betas[0] * pre[1].double().abs(), (1.0 - betas[0]) * (g.double() * (clip * prescale)).abs()))
        for k, y, r, what in zip(got["A"], yard, ref, ("master", "exp_avg", "exp_avg_sq")):
            assert bool(torch.isfinite(k).all()), what
            ek, ey = max_rel(k, r), max_rel(y, r)
            ratio = ek / max(ey, 2.0 ** -24)
            print(f"adamw n={n} step={step} {what}: kernel_rel={ek:.3e} yardstick_rel={ey:.3e} ratio={ratio:.2f}")
            scale = torch.maximum(r.abs(), terms[what])
            bad = (k.double() - r).abs() > torch.maximum(4 * ey * r.abs(), 2 * ulp32(scale))
            assert not bool(bad.any()), (what, step, int(bad.sum()), ek, ey)
            worst = max(worst, float(((k.double() - r).abs() / torch.maximum(4 * ey * r.abs(), 2 * ulp32(scale))).max()))
    return worst


NS = [1, 7, 8, 9, 2047, 2048 + 5, 256 * 8 * 3 + 1]
AXES = dict(gdtype=[torch.bfloat16, torch.float32], wd=[0.0, 0.01, 0.5], prescale=[1.0, 1 / 8], max_norm=[0.5, 1e6, 0.0, -1.0],
            step0=[1, 2, 1000, 10 ** 6], betas=[(0.9, 0.999), (0.8, 0.95)], eps=[1e-8, 1e-5],
            offs=[(1, 1, 1, 1, 1), (2, 3, 1, 2, 3), (3, 2, 3, 1, 2), (0, 0, 0, 0, 1), (1, 0, 0, 0, 0), (0, 2, 0, 0, 0)])


def draw_adamw(rng, n=None):
    """one point of the grid of the issue: ``n`` given or drawn, every other axis drawn"""
    c = {k: rng.choice(v) for k, v in AXES.items()}
    c.update(n=rng.choice(NS) if n is None else n, nsteps=rng.choice([1, 2, 3]), seed=rng.randrange(1 << 30), lr=rng.choice([1e-2, 1e-4]))
    return c


def _cases():
    rng = random.Random(1234)
    out = [draw_adamw(rng, n) for _ in range(4) for n in NS]
    for i, (k, vals) in enumerate(AXES.items()):       # every value of every axis at least once, whatever the draws gave
        for j, val in enumerate(vals):
            out[(5 * i + j) % len(out)][k] = val
    return out


CASES = _cases()


def _id(c):
    return "n{n}-{d}-wd{wd}-ps{prescale:g}-mn{max_norm:g}-s{step0}-b{b}-e{eps:g}-o{o}".format(
        d=str(c["gdtype"])[6:], b=c["betas"][0], o="".join(map(str, c["offs"])), **{k: c[k] for k in ("n", "wd", "prescale", "max_norm", "step0", "eps")})


def test_adamw_cases_cover_every_value_of_every_axis():
    for k, vals in AXES.items():
        assert {repr(c[k]) for c in CASES} == {repr(v) for v in vals}, k
    assert {c["n"] for c in CASES} == set(NS)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_adamw_and_grad_norm_against_float64(backend, case):
    """Bit-exact: param == T(master); guards; aligned launch == one-per-trip launch.  Against the float64 recurrence on the same fp32
    inputs: the max relative error of master / exp_avg / exp_avg_sq is at most 4 x that of torch.optim.AdamW (fp32, CPU), floor 2 ulps.

    "2 ulps of the element" is taken at the largest fp32 quantity of the element's last sum (see case_adamw): measured raw ratios
    kernel error / max(yardstick error, 2^-24) are 1.39 for exp_avg_sq (interpreter and MI355X), but up to 49 (interpreter) and
    20 (MI355X) for exp_avg and 11 / 12 for the master, each at an element where the two terms of the sum cancel; against the
    bound as asserted the kernel stays under 1.  Gradient norm: kernel error <= 7.3e-8 relative throughout (its block sums end
    in a double reduction), the fp32 yardstick reaches 3e-7 at n = 6145."""
    case_adamw(backend, **case)


@pytest.mark.gpu
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_adamw_second_grid_stride_trip(gpu, gdtype):
    """n just past 4096 blocks x 256 threads x 8 parameters: the vector loop takes a second trip and the tail follows it"""
    case_adamw(gpu, n=4096 * 256 * 8 + 8 * 300 + 5, gdtype=gdtype, wd=0.01, prescale=1 / 8, max_norm=0.5, step0=2, betas=(0.9, 0.999),
               eps=1e-8, offs=(1, 1, 1, 1, 1), nsteps=1, seed=5)


@pytest.mark.gpu
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_grad_norm_second_grid_stride_trip(gpu, gdtype):
    n = 1024 * 256 * 8 + 8 * 700 + 3
    g = (torch.randn(n, generator=torch.Generator().manual_seed(3)) * 3).to(gdtype)
    norm = torch.empty(1, device=gpu)
    ops.grad_norm(g.to(gpu), norm, torch.full((1024,), float("nan"), device=gpu), 0.125)
    check_norm(norm, g, 0.125)


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 256 * 8 * 3 + 1])
def test_grad_norm_sizes_and_tail(backend, gdtype, n):
    """the tail n % 8 belongs to block 0 alone; values differ per element so a tail summed twice or not at all shows"""
    g = (torch.arange(1, n + 1, dtype=torch.float32) % 37 - 11.5).to(gdtype)
    norm = torch.empty(1, device=backend)
    for prescale in (1.0, 0.125):
        ops.grad_norm(g.to(backend), norm, torch.full((1024,), float("nan"), device=backend), prescale)
        check_norm(norm, g, prescale)


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [5, 2048 + 5])
def test_zero_gradient_gives_norm_zero_and_a_finite_step(backend, gdtype, n):
    dev = backend
    g = torch.zeros(n, dtype=gdtype, device=dev)
    norm = torch.full((1,), float("nan"), device=dev)
    ops.grad_norm(g, norm, torch.full((1024,), float("nan"), device=dev))
    assert float(norm.cpu()[0]) == 0.0
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    master, m, v, q = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), p0.to(gdtype).clone().to(dev)
    lr, wd = f32(1e-2), f32(0.5)
    ops.adamw_step(g, master, m, v, q, norm, max_norm=0.5, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=wd, step=1)
    assert bool(torch.isfinite(master).all()) and bool(torch.isfinite(q.float()).all())
    # weight decay is decoupled and comes first: with no gradient and no state the step IS the decay
    want = p0.double() * (1.0 - lr * wd)
    assert bool(((master.cpu().double() - want).abs() <= ulp32(want)).all())
    assert not bool(m.cpu().any()) and not bool(v.cpu().any())
    assert torch.equal(bits(q), bits(master.cpu().to(gdtype)))


def test_n_zero_touches_nothing(backend):
    dev = backend
    bufs = [torch.full((2 * G,), GUARD, dtype=dt, device=dev) for dt in (torch.bfloat16, torch.float32, torch.float32, torch.float32, torch.bfloat16)]
    g, p, m, v, q = (b[G:G] for b in bufs)
    norm = torch.full((1,), float("nan"), device=dev)
    ops.grad_norm(g, norm, torch.full((1024,), float("nan"), device=dev))
    assert float(norm.cpu()[0]) == 0.0
    ops.adamw_step(g, p, m, v, q, norm, max_norm=0.5, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.1, step=1)
    assert all(bool((b.cpu() == GUARD).all()) for b in bufs)


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_non_finite_gradient_gives_the_classes_of_the_reference(backend, gdtype):
    """one inf in the gradient: the reference's norm is inf, its clip coefficient 0, the clipped gradient NaN at that element and 0
    elsewhere.  The kernel must give finite / inf / NaN in the same places -- no tolerance involved."""
    n, bad = 2048 + 5, 1029
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(n, generator=gen).to(gdtype)
    g[bad] = float("inf")
    p0, m0, v0 = torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen), 0.01 * torch.rand(n, generator=gen)
    kw = dict(max_norm=0.5, lr=f32(1e-2), eps=f32(1e-8), wd=f32(0.01), step=3)
    betas = (f32(0.9), f32(0.999))
    ref_norm = g.float().square().sum().sqrt()
    clip = torch.clamp(0.5 / (ref_norm + 1e-6), max=1.0)
    assert math.isinf(float(ref_norm)) and float(clip) == 0.0
    yard = adamw_torch(g, p0, m0, v0, ref_norm.reshape(1), betas=betas, prescale=1.0, **kw)
    dev = backend
    norm = torch.empty(1, device=dev)
    ops.grad_norm(g.to(dev), norm, torch.empty(1024, device=dev))
    assert math.isinf(float(norm.cpu()[0])) and float(norm.cpu()[0]) > 0
    master, m, v, q = p0.clone().to(dev), m0.clone().to(dev), v0.clone().to(dev), p0.to(gdtype).clone().to(dev)
    ops.adamw_step(g.to(dev), master, m, v, q, norm, beta1=betas[0], beta2=betas[1], **kw)
    cls = lambda t: torch.isnan(t.float().cpu()) * 2 + torch.isinf(t.float().cpu()) * 1
    for k, y, what in zip((master, m, v), yard, ("master", "exp_avg", "exp_avg_sq")):
        assert torch.equal(cls(k), cls(y)), what
        assert int(cls(y)[bad]) == 2 and int((cls(y) != 0).sum()) == 1, what      # what the reference does, recorded
    assert torch.equal(cls(q), cls(yard[0]))


# ------------------------------------------------------------------ BF16Optimizer on the flat buffer (interpreter)
def _tiny_opt(norm_output=True, **kw):
    from specforge_amd.eagle3 import OnlineEagle3Model
    from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3
    from specforge_amd.training import BF16Optimizer

    with open(os.path.join(ROOT, "examples", "tiny_draft_config.json")) as fh:
        cfg = DraftConfig.from_hf(json.load(fh))
    cfg.norm_output = norm_output
    torch.manual_seed(0)
    eagle = OnlineEagle3Model(LlamaForCausalLMEagle3(cfg), length=2).train()
    return eagle, BF16Optimizer(eagle, lr=1e-2, total_steps=100, warmup_ratio=0.0, **kw)


@pytest.mark.parametrize("norm_output", [True, False])
def test_bf16_optimizer_weight_decay_and_prescale_on_the_flat_buffer(emu, norm_output):
    """3 steps of training.BF16Optimizer with weight_decay = 0.1 and grad_prescale = 0.5 against the float64 recurrence on the flat
    buffer.  norm_output = False: the trailing norm.weight slice has no gradient; master, state and parameter keep their bits
    (no decay either).  Bounds from counting roundings, half an ulp each: the update lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps) passes
    about ten fp32 roundings from the gradient to the master, so the master is within 8 ulps of max(|p|, |update|) (the update taken at
    the magnitude of exp_avg's two terms, which may cancel); exp_avg and
    exp_avg_sq are a scaled (and squared) gradient, two or three products and a sum: 8 ulps of the sum of the two terms' magnitudes
    as well (measured under the interpreter: 5.4, 2.7 and 4.3 ulps).  A dropped decay or prescale is an error of 1e-3 and more."""
    eagle, opt = _tiny_opt(norm_output, weight_decay=0.1, max_grad_norm=0.5, betas=(0.8, 0.95), eps=1e-5)
    opt.grad_prescale = 0.5
    f = eagle.engine.flat
    n = opt.n_active
    lo, hi = f.slices["norm.weight"]
    assert hi == f.numel and (n == lo if not norm_output else n == f.numel)
    tail0 = [t[n:].clone() for t in (opt.master, opt.exp_avg, opt.exp_avg_sq, f.data)]
    gen = torch.Generator().manual_seed(4)
    wd, eps, b1, b2 = f32(0.1), f32(1e-5), f32(0.8), f32(0.95)
    for step in range(1, 4):
        f.grad.copy_((torch.randn(f.numel, generator=gen) * 0.05).to(torch.bfloat16))
        pre = [t[:n].clone() for t in (opt.master, opt.exp_avg, opt.exp_avg_sq)]
        lr = f32(opt.get_learning_rate())
        g = f.grad[:n].clone()
        norm = opt.step()
        want_norm = float(g.double().square().sum().sqrt()) * 0.5
        assert abs(float(norm) - want_norm) <= 2.0 ** -22 * want_norm
        ref = adamw64(g, *pre, norm, max_norm=0.5, lr=lr, betas=(b1, b2), eps=eps, wd=wd, step=step, prescale=0.5)
        gs = g.double() * 0.5 * min(1.0, 0.5 / (float(norm) + 1e-6))
        mterms = b1 * pre[1].double().abs() + (1 - b1) * gs.abs()          # the update at the magnitude of exp_avg's terms
        upd = lr / (1 - b1 ** step) * mterms / (ref[2].sqrt() / math.sqrt(1 - b2 ** step) + eps)
        scale = (torch.maximum(pre[0].double().abs(), upd), b1 * pre[1].double().abs() + (1 - b1) * gs.abs(),
                 b2 * pre[2].double().abs() + (1 - b2) * gs * gs)
        for k, r, sc, what in zip((opt.master, opt.exp_avg, opt.exp_avg_sq), ref, scale, ("master", "exp_avg", "exp_avg_sq")):
            assert bool(((k[:n].double() - r).abs() <= 8 * ulp32(sc)).all()), (what, step)
        assert torch.equal(bits(f.data[:n]), bits(opt.master[:n].to(torch.bfloat16)))
    for t, t0 in zip((opt.master, opt.exp_avg, opt.exp_avg_sq, f.data), tail0):
        assert torch.equal(bits(t[n:]), bits(t0))


@pytest.mark.parametrize("max_grad_norm", [0.0, -1.0])
def test_bf16_optimizer_refuses_a_max_grad_norm_that_is_not_positive(emu, max_grad_norm):
    """The reference scales every gradient by clamp(max_grad_norm / (norm + 1e-6), max=1): 0 freezes training, a negative value
    turns the step around.  The kernel does not clip for max_norm <= 0.  BF16Optimizer takes neither reading silently."""
    with pytest.raises(ValueError, match="max_grad_norm"):
        _tiny_opt(max_grad_norm=max_grad_norm)


# ------------------------------------------------------------------ sf_eagle3_metrics
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 5, 300])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("pad", [0, 4])
def test_eagle3_metrics(backend, B, S, T, pad):
    """out[k] = {ploss, correct, acc denominator, acc, acceptance, position denominator, B*S, ploss} of TTT step k; the masks of
    step k are the window [b, k : k + S] of the padded arrays (eagle3/model.py:161-190; clamp_min 1e-6 / 1e-8)."""
    Spad = S + T - 1 + pad
    gen = torch.Generator().manual_seed(100 * B + 10 * T + S + pad)
    lm = torch.randint(-1, 3, (B, Spad), generator=gen, dtype=torch.int32)       # anything non-zero counts
    pm = torch.randint(0, 4, (B, Spad), generator=gen, dtype=torch.int32) * torch.randint(0, 2, (B, Spad), generator=gen, dtype=torch.int32)
    if T > 1:
        lm[:, 1:1 + S], pm[:, 1:1 + S] = 0, 0        # the window of step 1 is all zero
        if pad:
            lm[:, S + T - 1:], pm[:, S + T - 1:] = 5, 5   # past every window: must not be counted
    met = torch.rand(3 * T, generator=gen) * 50
    out = torch.full((8 * T + 8,), -77.0, device=backend)
    ops.eagle3_metrics(met.to(backend), lm.to(backend), pm.to(backend), out[:8 * T], B=B, S=S, Spad=Spad, T=T)
    out = out.cpu()
    assert bool((out[8 * T:] == -77.0).all())
    near = lambda got, want: abs(float(got) - want) <= float(ulp32(torch.tensor(want)))
    for k in range(T):
        nl = sum(1 for b in range(B) for s in range(S) if int(lm[b, s + k]) != 0)
        npos = sum(1 for b in range(B) for s in range(S) if int(pm[b, s + k]) != 0)
        o = out[8 * k:8 * k + 8]
        dl, dp = max(float(nl), f32(1e-6)), max(float(npos), f32(1e-8))
        loss, correct, accept = (float(met[3 * k + i]) for i in range(3))
        assert float(o[2]) == dl and float(o[5]) == dp and float(o[6]) == float(B * S) and float(o[1]) == correct, (k, o)
        assert near(o[0], loss / (B * S)) and near(o[3], correct / dl) and near(o[4], accept / dp), (k, o)
        assert torch.equal(bits(o[7:8]), bits(o[0:1]))
        if T > 1 and k == 1:
            assert nl == 0 and npos == 0 and float(o[2]) == f32(1e-6) and float(o[5]) == f32(1e-8)


# ------------------------------------------------------------------ sf_axpy_f32 / sf_reduce_sum
def _axpy_case(dev, n):
    gen = torch.Generator().manual_seed(n)
    x, y0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3
    alpha = f32(0.37)
    y = torch.full((n + 2 * G,), float("nan"), device=dev)      # the engine's first micro-batch: y is not initialised
    ops.axpy_f32(alpha, x.to(dev), y[G:G + n], accumulate=False)
    assert bool(torch.isnan(y[:G].cpu()).all()) and bool(torch.isnan(y[G + n:].cpu()).all())
    assert torch.equal(bits(y[G:G + n]), bits((x.double() * alpha).float()))       # one fp32 product: the rounded fp64 product
    buf, yv = guarded(y0, 0, dev)
    ops.axpy_f32(alpha, x.to(dev), yv, accumulate=True)
    want = y0.double() + alpha * x.double()
    two = (y0 + (x.double() * alpha).float()).double()       # two roundings; or one (fma): within an ulp of the fp64 value
    got = yv.cpu().double()
    assert bool((((got - want).abs() <= ulp32(want)) | (got == two)).all()) and guards_intact(buf, 0, n)


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_axpy_f32(backend, n):
    _axpy_case(backend, n)


@pytest.mark.gpu
def test_axpy_f32_second_grid_stride_trip(gpu):
    _axpy_case(gpu, 2048 * 256 + 4097)


@pytest.mark.parametrize("nseg", [1, 5])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 100003])
def test_reduce_sum(backend, nseg, n):
    """out[b] = float32(sum of segment b in float64 * scale), to an ulp (the kernel accumulates in double)"""
    gen = torch.Generator().manual_seed(n + nseg)
    x = torch.randn(nseg * n, generator=gen) * torch.exp2(torch.randint(-20, 20, (nseg * n,), generator=gen).float())
    scale = f32(1 / 3)
    out = torch.full((nseg + 4,), -77.0, device=backend)
    inp = x.to(backend) if n else torch.zeros(1, device=backend)
    ops.reduce_sum(inp, n, nseg, out[:nseg], scale)
    out = out.cpu()
    assert bool((out[nseg:] == -77.0).all())
    want = x.double().view(nseg, n).sum(1) * scale
    assert bool(((out[:nseg].double() - want).abs() <= ulp32(want)).all()), (out[:nseg], want)
