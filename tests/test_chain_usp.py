"""Joint chain counts under USP: two SP ranks (tests/_chain_usp_worker.py, gloo) against the unsharded step of the same model and sample
in the pytest process.  A rank's loss mask covers its chunk + T overlap positions, so a chain never crosses ranks; the counts of a rank
are sums over the SP group, carried by the collective that already sums the accuracy counts: both ranks report the same numbers, and
they are the single-process counts -- integers, compared exactly.  Plain and LK objective under the interpreter, and once on the GPU
(both ranks share cuda:0: three processes hold the device; each rank runs under a time limit)."""
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
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_chain_usp_worker.py"), "--rank", str(r), "--port", str(port),
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
    print("unsharded chain_denoms", ref["denoms"].tolist(), "chain_corrects", ref["corrects"].tolist(), "rank 0", ranks[0]["corrects"].tolist())
    for r in ranks:
        assert torch.equal(r["denoms"], ref["denoms"]) and torch.equal(r["corrects"], ref["corrects"])
        assert torch.equal(r["topk"], ref["topk"])                 # (the chain columns ride behind the top-k ones: those stay where they were)
        assert torch.equal(r["acc_denoms"], ref["acc_denoms"]) and torch.equal(r["acc_corrects"], ref["acc_corrects"])
        assert torch.equal(r["named_denoms"], r["denoms"])
        for j, k in enumerate(_worker().TOPK):
            assert torch.equal(r["named"][k], r["corrects"][:, 0 if k == 1 else 1 + j])
    den, cor, T = ref["denoms"], ref["corrects"], ref["denoms"].numel()
    assert float(cor[0, 0]) == float(ref["acc_corrects"][0]) and float(den[0]) == float(ref["acc_denoms"][0])
    assert torch.equal(cor[0, 1:], ref["topk"][0])                 # depth 0 is the marginal count
    assert bool((den[1:] < ref["acc_denoms"][1:]).all())           # the sample's loss mask has holes: chains are censored
    assert float(den[T - 1]) > 0 and 0 < float(cor[T - 1, -1]) < float(den[T - 1])      # chains alive and dead at the deepest depth
    assert bool((cor[:, 1:] >= cor[:, :-1]).all()) and bool((cor[1:] <= cor[:-1]).all())


def _worker():
    import _chain_usp_worker as W

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
