"""What tests/test_loss_kernels.py and tests/test_norm_kernels.py share: views into wider marked buffers, the spacing of a number format,
one-rounding bf16, the bound "FACTOR x max(error of the same formula in torch fp32, floor)" and the bit-for-bit bf16 comparison."""
import pytest
import torch

from specforge_amd import _lib

BF, F32 = torch.bfloat16, torch.float32
MARK = 7.5


class InputRejected(AssertionError):
    """a case's INPUT misses a property the case asserts from the float64 reference alone (a near-tie, too many elements next to a
    rounding boundary): a test fails on it, tools/kernel_fuzz.py draws the next seed"""


@pytest.fixture
def gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _lib._inject_library_for_tests(None)
    _lib.lib()
    return "cuda"


def ulp(x, dtype):
    """spacing of ``dtype`` at |x| (float64 in and out; normal range)"""
    _, e = torch.frexp(x.double().abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e.clamp_min(-125) - (8 if dtype == BF else 24))


def rbf(x):
    """float64 -> the nearest bf16 value (ties to even), as float64: ONE rounding (torch's double -> bfloat16 goes through float)"""
    q = ulp(x, BF)
    return torch.round(x / q) * q


def wide(vals, left, right, dev, rows_extra=0):
    R, C = vals.shape
    buf = torch.full((R + rows_extra, left + C + right), MARK, dtype=vals.dtype)
    buf[:R, left:left + C] = vals
    buf = buf.to(dev)
    return buf, buf[:R, left:left + C]


def outside_untouched(buf, R, left, C):
    b = buf.cpu()
    return bool((b[:, :left] == MARK).all()) and bool((b[:, left + C:] == MARK).all()) and bool((b[R:] == MARK).all())


def held(got, want, yard, floor, what, factor):
    """|got - want| <= factor x max(|yard - want|, floor) elementwise; prints and returns the worst ratio"""
    err = (got.detach().cpu().double() - want).abs()
    unit = torch.maximum((yard.double() - want).abs(), floor).clamp_min(1e-300)
    ratio = float((err / unit).max()) if err.numel() else 0.0
    print(f"ratio {what}: {ratio:.3f}")
    assert ratio <= factor, (what, ratio)
    return ratio


def bf16_bits(got, want, window, what, cap=0.02):
    """got (bf16) has the bits of bf16(want); another value only where want +- window straddles a rounding boundary -- then any bf16 value
    from bf16(want - window) to bf16(want + window), more than one step apart where the terms of a difference cancel -- for <= cap of the case"""
    g = got.detach().cpu().double()
    lo, hi, mid = rbf(want - window), rbf(want + window), rbf(want)
    under = want.abs() + window < 2.0 ** -126            # below the normal range a result may flush to zero (sf_exp_fast): only its size is held
    assert bool((g.abs()[under] <= 2.0 ** -126).all()), what
    near = (lo != hi) & ~under
    if float(near.double().mean()) > cap:
        raise InputRejected((what, "the input puts too many elements next to a rounding boundary", float(near.double().mean())))
    off = (g != mid) & ~under
    print(f"bf16 {what}: {int(off.sum())} of {off.numel()} elements on the neighbouring value, {int(near.sum())} within the window")
    assert bool((~off | (near & (g >= lo) & (g <= hi))).all()), (what, int((off & ~(near & (g >= lo) & (g <= hi))).sum()))
    assert float(off.double().mean()) <= cap, what
