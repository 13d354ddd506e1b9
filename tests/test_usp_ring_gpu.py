"""Ring attention inside USP on the MI355X: u x r SP ranks against the unsharded step of the same model and sample in the pytest process.
gloo: every rank shares cuda:0 and exchanges through pinned host buffers (at most five processes hold the device: pytest + four
ranks); RCCL: rank x on cuda:x (skipped without enough devices).  Each rank runs under a time limit.  Bars: about twice the difference
measured on the MI355X (recorded beside each)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900

# (config, seq, u, r): cfg 1 real dims 1 x 4096, Llama-3-8B dims 1 x 2048, the head_dim-256 draft 1 x 4000 (chunk 2000 / 1000: the
# ring offsets are not multiples of the 128-query block)
CASES = [("cfg1", 4096, 1, 2), ("cfg1", 4096, 2, 2), ("llama3-8b", 2048, 1, 2), ("llama3-8b", 2048, 2, 2), ("hd256", 4000, 1, 2),
         ("hd256", 4000, 2, 2)]
# (loss: an fp32 ulp of the loss where the measurement was exact; params: weights whose gradient clearly exceeds the gradient
#  difference -- 0.5 % of them at cfg 1, 2 - 13 % at the other dims)
BARS = {("cfg1", 4096, 1, 2): dict(loss=1e-6, acc=0.0, grad=1.1e-2, params=1e-6),        # measured: loss 0, acc 0, grad 5.3e-3, params 4.8e-7
        ("cfg1", 4096, 2, 2): dict(loss=1e-6, acc=0.0, grad=1.1e-2, params=2e-6),        # measured: loss 3.0e-8, acc 0, grad 5.3e-3, params 9.5e-7
        ("llama3-8b", 2048, 1, 2): dict(loss=8e-6, acc=0.0, grad=9e-3, params=2e-6),     # measured: loss 3.8e-6, acc 0, grad 4.3e-3, params 9.5e-7
        ("llama3-8b", 2048, 2, 2): dict(loss=6e-6, acc=0.0, grad=1.75e-2, params=2e-6),  # measured: loss 2.9e-6, acc 0, grad 8.7e-3, params 9.5e-7
        ("hd256", 4000, 1, 2): dict(loss=2.5e-6, acc=0.0, grad=1.1e-2, params=2e-6),     # measured: loss 1.3e-6, acc 0, grad 5.3e-3, params 9.5e-7
        ("hd256", 4000, 2, 2): dict(loss=2e-6, acc=0.0, grad=1.1e-2, params=2e-6)}       # measured: loss 8.6e-7, acc 0, grad 5.3e-3, params 9.5e-7


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _unsharded(config, seq):
    import _usp_gpu as W
    import _usp_ring_gpu as R
    from specforge_amd import _lib

    _lib._inject_library_for_tests(None)
    real, W.dims = W.dims, R.dims
    try:
        eagle, strat, backend, batch = W.setup(config, seq, torch.device("cuda", 0))
        res = W.step(eagle, strat, backend, batch)
    finally:
        W.dims = real
    del eagle, strat, backend, batch
    torch.cuda.empty_cache()
    return res


def _ranks(tmp_path, config, seq, u, r, backend):
    port, world = _free_port(), u * r
    outs = [str(tmp_path / f"{backend}_rank{x}.pt") for x in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_usp_ring_gpu.py"), "--rank", str(x), "--ulysses", str(u),
                               "--ring", str(r), "--port", str(port), "--backend", backend, "--config", config, "--seq", str(seq),
                               "--out", outs[x]], cwd=ROOT)
             for x in range(world)]
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(timeout=CHILD_TIMEOUT))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail(f"ring rank did not finish within {CHILD_TIMEOUT} s")
    assert rcs == [0] * world, rcs
    return [torch.load(o) for o in outs]


def _compare(ref, ranks, bars):
    n = len(ranks)
    diffs = {}
    mean_loss = sum(x["plosses"] for x in ranks) / n
    diffs["loss"] = float((mean_loss - ref["plosses"]).abs().max())
    for x in ranks[1:]:
        assert torch.equal(ranks[0]["acces"], x["acces"])     # global counts: the same on every rank
    diffs["acc"] = float((ranks[0]["acces"] - ref["acces"]).abs().max())
    g = ranks[0]["grad"] / n
    diffs["grad"] = float((g - ref["grad"]).abs().max()) / float(ref["grad"].abs().max())
    clear = ref["grad"].abs() > 4 * (g - ref["grad"]).abs().max()   # (see tests/test_usp.py::_compare)
    diffs["clear_frac"] = float(clear.float().mean())
    diffs["params"] = float((ranks[0]["params"].float() - ref["params"].float())[clear].abs().max()) if clear.any() else 0.0
    print("ring vs unsharded:", diffs)
    for k, bar in bars.items():
        assert diffs[k] <= bar, (k, diffs[k], bar)


@pytest.mark.gpu
@pytest.mark.parametrize("config,seq,u,r", CASES, ids=[f"{c}-1x{s}-u{u}r{r}" for c, s, u, r in CASES])
def test_ring_ranks_share_one_device_over_gloo(tmp_path, config, seq, u, r):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    ref = _unsharded(config, seq)
    _compare(ref, _ranks(tmp_path, config, seq, u, r, "gloo"), BARS[(config, seq, u, r)])


@pytest.mark.gpu
@pytest.mark.parametrize("u,r", [(1, 2), (2, 2)])
def test_ring_ranks_over_rccl(tmp_path, u, r):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    if torch.cuda.device_count() < u * r:
        pytest.skip(f"RCCL u{u} x r{r} needs {u * r} devices")
    config, seq = "llama3-8b", 2048
    ref = _unsharded(config, seq)
    _compare(ref, _ranks(tmp_path, config, seq, u, r, "nccl"), BARS[(config, seq, u, r)])
