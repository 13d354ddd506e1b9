"""Randomised sweep of the HBM-bound kernels against their references: fused CE (loss, in-place gradient, argmax / accuracy /
acceptance artefacts), RMSNorm forward / backward (+ residual gradient, weight-gradient column sums), the teacher reduction on permuted
logits and the teacher-head GEMM with its reduction epilogue -- the bodies of tests/test_kernels.py over seeded random shapes
(row counts that are not multiples of anything, vocabularies that are multiples of 8 only, every TTT offset, hidden sizes 8 ... 8192);
the clip + AdamW step with its gradient norm (tests/test_optimizer_kernels.py: any size, alignment, hyperparameter of its grid), the
pointwise kernels (tests/test_pointwise_kernels.py: RoPE head sizes / head counts, SwiGLU and the casts at random sizes) and the float64
cases of the loss, teacher and norm kernels (tests/test_loss_kernels.py, tests/test_norm_kernels.py) at random sizes.

    python tools/kernel_fuzz.py [--cases 300] [--seed 0]          (GPU box; one JSON line per failure, a summary line last)
    python tools/kernel_fuzz.py --emu --cases 20                  (this container: the SIMT interpreter, small shapes)
"""
import argparse
import json
import os
import random
import sys
import time
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_kernels as TK  # noqa: E402


def draw(rng, emu, more=False):
    """``more``: the optimizer and pointwise kinds too; ``more == 2``: the float64 loss and norm kinds as well (off: the draws of a seed stay
    what they were before those kinds existed)"""
    kind = rng.choice(["ce", "ce", "norm", "norm", "teacher_reduce", "teacher_gemm"] + (["adamw", "adamw", "pointwise"] if more else [])
                      + (["loss", "loss", "norm64"] if more == 2 else []))
    if kind == "loss":       # tests/test_loss_kernels.py; the interpreter draws V past 8200, where the unrolled loops and their remainders run
        op = rng.choice(["ce", "lk", "teacher", "teacher_perm"])
        V = 8 * rng.randint(2, 1100 if emu else 5200) + (rng.randint(1, 7) if op in ("lk", "teacher") and rng.random() < 0.3 else 0)
        return kind, dict(op=op, dtype=rng.choice([torch.bfloat16, torch.float32]), V=V, seed=rng.randrange(1 << 20), pick=rng.randrange(1 << 10))
    if kind == "norm64":     # tests/test_norm_kernels.py
        op = rng.choice(["fwd", "bwd", "bwd2"])
        return kind, dict(op=op, dtype=rng.choice([torch.bfloat16, torch.float32]), H=8 * rng.randint(1, 512 if op == "bwd2" else 1024),
                          R=rng.randint(1, 40 if emu else 600), seed=rng.randrange(1 << 20), pick=rng.randrange(1 << 10))
    if kind == "adamw":
        import test_optimizer_kernels as TO
        return kind, TO.draw_adamw(rng, n=rng.randint(1, 3000 if emu else 3_000_000))
    if kind == "pointwise":
        op = rng.choice(["rope", "swiglu", "movers"])
        if op == "rope":
            return kind, dict(op=op, dtype=rng.choice([torch.bfloat16, torch.float32]), hd=16 * rng.randint(1, 16), nheads=rng.randint(1, 8 if emu else 48))
        if op == "swiglu":
            return kind, dict(op=op, dtype=rng.choice([torch.bfloat16, torch.float32]), seed=rng.randrange(1 << 30), rows=rng.randint(0, 20 if emu else 5000))
        return kind, dict(op=op, rows=rng.randint(1, 12 if emu else 700), C=8 * rng.randint(4, 20 if emu else 300))
    f32 = rng.random() < 0.35
    dtype, = (torch.float32,) if f32 else (torch.bfloat16,)
    if kind == "ce":
        B, S = rng.choice([1, 2, 3]), rng.randint(5, 40 if emu else 300)
        V = 8 * rng.randint(2, 64 if emu else 5000)
        T = rng.randint(1, 7)
        return kind, dict(dtype=dtype, tol=1e-4 if f32 else 2e-2, B=B, S=S, V=V, T=T, off=rng.randint(0, T))
    if kind == "norm":
        H = 8 * rng.randint(1, 1024)
        R = rng.randint(1, 20 if emu else 600)
        return kind, dict(dtype=dtype, tol=1e-5 if f32 else 2e-2, R=R, H=H)
    if kind == "teacher_reduce":
        Vd = 8 * rng.randint(6, 40 if emu else 400)          # (the test plants ties at draft columns 2, 3, 7 and rest columns 0 ... 40)
        Vt = Vd + 8 * rng.randint(6, 60 if emu else 2000)
        return kind, dict(dtype=dtype, Vt=Vt, Vd=Vd)
    # (the test asserts WHICH kernel the interpreter build dispatches to: there only shapes its 4-wave kernel takes, M >= 192 and K >= 512)
    M = rng.randint(192, 300) if emu else rng.randint(8, 2200)
    Vd = 8 * rng.randint(4, 40 if emu else 300)
    Vt = Vd + (0 if rng.random() < 0.1 else 8 * rng.randint(40, 100 if emu else 3000))
    K = 64 * (rng.randint(8, 9) if emu else rng.randint(1, 16))
    return kind, dict(M=M, Vt=Vt, Vd=Vd, K=K)


def case_pointwise(dev, op, **kw):
    import test_pointwise_kernels as TP
    if op == "rope":
        TP.test_rope_forward(dev, kw["dtype"], kw["hd"], kw["nheads"])
    elif op == "swiglu":
        gu, da, I = TP._swiglu_inputs(kw["dtype"], kw["seed"], rows_randn=kw["rows"])
        TP._swiglu_check(dev, gu, da, I, kw["dtype"], "fuzz")
    else:
        TP._movers(dev, kw["rows"], kw["C"])


def case_adamw(dev, **kw):
    import test_optimizer_kernels as TO
    TO.case_adamw(dev, **kw)


def _retry_inputs(fn, seed):
    """the float64 cases assert two properties of their INPUT from the reference alone (no near-tie, few elements next to a rounding
    boundary); a drawn seed that misses one is replaced by the next"""
    from f64_helpers import InputRejected
    for k in range(8):
        try:
            return fn(seed + k)
        except InputRejected:
            pass
    raise AssertionError("no seed in eight gave an input the case accepts")


def case_loss(dev, op, dtype, V, seed, pick):
    import test_loss_kernels as TL
    if op == "ce":
        form = ["p", "zt", "zt_rows"][pick % 3]
        _retry_inputs(lambda s: TL.case_ce(dev, dtype, V, form, [0, 2][pick % 2] if form == "zt" else [0, 2, TL.T][pick % 3], seed=s), seed)
    elif op == "lk":
        compact, St = TL.LK_VARIANTS[pick % 4]
        _retry_inputs(lambda s: TL.case_lk(dev, dtype, max(V, 136), "zt", compact=compact, St=St, off=1 + pick % 2, seed=s), seed)
    elif op == "teacher":
        V = max(V, 64)
        TL.case_teacher(dev, dtype, V, max(3, min(V // 3, 2000 + pick % 100)), seed=seed)
    else:
        V = max(V, 64)
        nparts = pick % 3
        TL.case_teacher_perm(dev, dtype, V + 128 * nparts, 8 * max(1, min(V // 24, 250 + pick % 10)), nparts, tp=pick % 2 == 0, seed=seed)


def case_norm64(dev, op, dtype, H, R, seed, pick):
    import test_norm_kernels as TN
    if op == "fwd":
        _retry_inputs(lambda s: TN.case_fwd(dev, dtype, R, H, seed=s), seed)
    else:
        _retry_inputs(lambda s: TN.case_bwd(dev, dtype, R, H, two=op == "bwd2", add=pick % 2 == 0, dw_mode=pick % 3,
                                            want_dx=op == "bwd2" or pick % 5 != 4, seed=s), seed)


FNS = dict(loss=case_loss, norm64=case_norm64, ce=TK.test_ce_fused, norm=TK.test_rmsnorm_fwd_bwd, teacher_reduce=TK.test_teacher_reduce_perm,
           teacher_gemm=TK.test_gemm_nt_teacher_matches_the_stored_logits, adamw=case_adamw, pointwise=case_pointwise)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--emu", action="store_true")
    args = ap.parse_args()
    rng = random.Random(args.seed)
    from specforge_amd import _lib
    if args.emu:
        from specforge_amd import build
        _lib._inject_library_for_tests(build.build_emu())
        dev = "cpu"
    else:
        _lib.lib()
        dev = "cuda"
    fns = FNS
    t0 = time.time()
    fails, count = 0, {}
    for i in range(args.cases):
        kind, kw = draw(rng, args.emu, 2)
        count[kind] = count.get(kind, 0) + 1
        try:
            fns[kind](dev, **kw)
        except Exception as e:
            fails += 1
            tb = traceback.format_exc().strip().splitlines()
            print(json.dumps(dict(i=i, kind=kind, case={k: str(v) for k, v in kw.items()}, error=f"{type(e).__name__}: {e}"[:700],
                                  where=[x.strip()[:160] for x in tb[-5:-1]])), flush=True)
    print(json.dumps(dict(summary=True, cases=args.cases, seed=args.seed, failures=fails, by_kind=count, seconds=round(time.time() - t0, 1))), flush=True)
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
