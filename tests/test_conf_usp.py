"""Draft-confidence counts under USP: two SP ranks (tests/_conf_usp_worker.py, gloo, under the interpreter) against the unsharded step of
the same model and sample in the pytest process.  A rank's loss mask covers its chunk + T overlap positions, so a gated chain never
crosses ranks; the counts of a rank are sums over the SP group, carried BEHIND the top-k and chain columns by the collective that already
sums the accuracy counts.  Both ranks report the same numbers and they are the single-process counts -- integers, compared exactly; the
top-k and chain counts are the unsharded ones too.  A bin's confidence sum is each rank's fp32 sum (one rounding of its float64 sum)
added once more in fp32: held to two fp32 spacings of the unsharded sum.  Plain and LK objective.  No GPU leg: the counts ride the
collective that tests/test_chain_usp.py exercises on the device."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from f64_helpers import F32, ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ranks(tmp_path, emu, lk, sample):
    port = _free_port()
    outs = [str(tmp_path / f"rank{r}.pt") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_conf_usp_worker.py"), "--rank", str(r), "--port", str(port),
                               "--emu", emu, "--lk", lk or "", "--sample", sample, "--out", outs[r]], cwd=ROOT) for r in range(2)]
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
    import _conf_usp_worker as W

    NB, J = W.BINS, len(W.TAU)
    print("unsharded bins", ref["bins"][:, 0].tolist(), "hits", ref["bins"][:, 1].sum(1).tolist(), "denoms", ref["denoms"].tolist(),
          "gate", ref["gate"].tolist())
    for r in ranks:
        assert r["bins"].shape == (W.T, 3, NB) and r["gate"].shape == (W.T, J, 2)
        assert torch.equal(r["bins"][:, :2], ref["bins"][:, :2]) and torch.equal(r["denoms"], ref["denoms"]) and torch.equal(r["gate"], ref["gate"])
        assert bool(((r["bins"][:, 2].double() - ref["bins"][:, 2].double()).abs() <= 2 * ulp(ref["bins"][:, 2].double(), F32)).all())
        # the top-k and chain columns stay where they are
        assert torch.equal(r["topk"], ref["topk"]) and torch.equal(r["chain_denoms"], ref["chain_denoms"])
        assert torch.equal(r["chain_corrects"], ref["chain_corrects"])
        assert torch.equal(r["acc_denoms"], ref["acc_denoms"]) and torch.equal(r["acc_corrects"], ref["acc_corrects"])
        n = r["named"]
        assert torch.equal(n["conf_bin_counts"], r["bins"][:, 0]) and torch.equal(n["conf_bin_corrects"], r["bins"][:, 1])
        assert torch.equal(n["conf_bin_sums"], r["bins"][:, 2]) and torch.equal(n["conf_denoms"], r["denoms"])
        assert torch.equal(n["conf_gate_drafted"], r["gate"][:, :, 0]) and torch.equal(n["conf_gate_accepted"], r["gate"][:, :, 1])
    bins, den, gate = ref["bins"], ref["denoms"], ref["gate"]
    assert torch.equal(den, ref["chain_denoms"])                                      # the gated fold censors as the chain fold does
    assert torch.equal(gate[:, 0, 1], ref["chain_corrects"][:, 0])                   # a threshold of 0 is the top-1 chain
    assert torch.equal(bins[:, 0].sum(1), ref["acc_denoms"]) and torch.equal(bins[:, 1].sum(1), ref["acc_corrects"])
    assert float(gate[0, 0, 0]) == float(den[0]) and bool((den[1:] < ref["acc_denoms"][1:]).all())     # holes in the loss mask censor chains
    assert 0 < float(ref["acc_corrects"][0]) < float(den[0]) and 0 < float(gate[0, -1, 1]) < float(gate[0, 0, 1])   # hits, misses, a gate that bites
    assert int((bins[0, 0] > 0).sum()) >= 3 and float(gate[0, -1, 0]) < float(gate[0, 0, 0])           # spread confidences; the gates thin out
    assert bool((gate[:, 1:] <= gate[:, :-1]).all()) and bool((gate[1:, :, 1] <= gate[:-1, :, 1]).all()) and bool((gate[..., 1] <= gate[..., 0]).all())


@pytest.mark.parametrize("lk", [None, "lambda"])
def test_usp_counts_equal_the_unsharded_counts(emu_lib_path, tmp_path, lk):
    from specforge_amd import _lib
    import _conf_usp_worker as W

    _lib._inject_library_for_tests(emu_lib_path)
    try:
        eagle, strat, backend = W.setup(torch.device("cpu"), lk=lk)
        smp = W.hit_sample(torch.device("cpu"), eagle, strat)
        ref = W.step(eagle, strat, backend, smp)
    finally:
        _lib._inject_library_for_tests(None)
    torch.save(smp, str(tmp_path / "sample.pt"))
    _check(ref, _ranks(tmp_path, emu_lib_path, lk, str(tmp_path / "sample.pt")))
