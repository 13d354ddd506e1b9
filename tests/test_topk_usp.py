"""Top-k hit counts under USP: two SP ranks (tests/_topk_usp_worker.py, gloo) against the unsharded step of the same model and sample in
the pytest process.  The counts of a rank are sums over the SP group: both ranks report the same numbers, and they are the
single-process counts -- integers, compared exactly.  Under the interpreter, and once on the GPU (both ranks share cuda:0: three
processes hold the device; each rank runs under a time limit)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ranks(tmp_path, emu, lk):
    port = _free_port()
    outs = [str(tmp_path / f"rank{r}.pt") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_topk_usp_worker.py"), "--rank", str(r), "--port", str(port),
                               "--emu", emu, "--lk", lk or "", "--out", outs[r]], cwd=ROOT) for r in range(2)]
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(timeout=CHILD_TIMEOUT))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail(f"USP rank did not finish within {CHILD_TIMEOUT} s")
    assert rcs == [0, 0], rcs
    return [torch.load(o) for o in outs]


def _check(ref, ranks):
    print("unsharded topk_corrects", ref["topk"].tolist(), "rank 0", ranks[0]["topk"].tolist())
    for r in ranks:
        assert torch.equal(r["topk"], ref["topk"])
        assert torch.equal(r["acc_denoms"], ref["acc_denoms"]) and torch.equal(r["acc_corrects"], ref["acc_corrects"])
        assert torch.equal(r["topk"][:, 0], r["acc_corrects"])
        for j, k in enumerate(_worker().TOPK):
            assert torch.equal(r["named"][k], r["topk"][:, j])
    assert float(ref["topk"].sum()) > 0 and bool((ref["topk"][:, 1:] >= ref["topk"][:, :-1]).all())


def _worker():
    import _topk_usp_worker as W

    return W


@pytest.mark.parametrize("lk", [None, "lambda"])
def test_usp_counts_equal_the_unsharded_counts(emu_lib_path, tmp_path, lk):
    from specforge_amd import _lib

    W = _worker()
    _lib._inject_library_for_tests(emu_lib_path)
    try:
        eagle, strat, backend = W.setup(torch.device("cpu"), lk=lk)
        ref = W.step(eagle, strat, backend, W.sample(torch.device("cpu")))
    finally:
        _lib._inject_library_for_tests(None)
    _check(ref, _ranks(tmp_path, emu_lib_path, lk))


@pytest.mark.gpu
def test_usp_counts_equal_the_unsharded_counts_on_the_gpu(tmp_path):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from specforge_amd import _lib

    W = _worker()
    _lib._inject_library_for_tests(None)
    dev = torch.device("cuda", 0)
    eagle, strat, backend = W.setup(dev)
    ref = W.step(eagle, strat, backend, W.sample(dev))
    torch.cuda.synchronize()
    del eagle, strat, backend
    torch.cuda.empty_cache()
    _check(ref, _ranks(tmp_path, "", None))
