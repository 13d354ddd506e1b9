"""USP (attention_backend "usp") on the MI355X: two SP ranks against the unsharded step of the same model and sample in the pytest
process.  gloo: both ranks share cuda:0 and exchange through pinned host buffers; RCCL: rank r on cuda:r (skipped on a one-device
box).  At most three processes hold a device (pytest + two ranks); each rank runs under a time limit.  Bars: about twice the
difference measured on the MI355X (recorded beside each)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900

# (config, seq): cfg 1 (Qwen2.5-0.5B draft) real dims 1 x 4096, Llama-3-8B dims 1 x 2048
CASES = [("cfg1", 4096), ("llama3-8b", 2048)]
# (loss: an fp32 ulp of the loss where the measurement was exact; params: weights whose gradient clearly exceeds the gradient
#  difference -- 0.5 % of them at cfg 1, 13 % at Llama-3-8B dims)
BARS = {("cfg1", 4096): dict(loss=1e-6, acc=0.0, grad=1.1e-2, params=1e-6),          # measured: loss 0, acc 0, grad 5.3e-3, params 4.8e-7
        ("llama3-8b", 2048): dict(loss=8e-6, acc=0.0, grad=9e-3, params=2e-6)}      # measured: loss 3.8e-6, acc 0, grad 4.3e-3, params 9.5e-7


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _unsharded(config, seq):
    import _usp_gpu as W
    from specforge_amd import _lib

    _lib._inject_library_for_tests(None)
    eagle, strat, backend, batch = W.setup(config, seq, torch.device("cuda", 0))
    res = W.step(eagle, strat, backend, batch)
    del eagle, strat, backend, batch
    torch.cuda.empty_cache()
    return res


def _ranks(tmp_path, config, seq, backend):
    port = _free_port()
    outs = [str(tmp_path / f"{backend}_rank{r}.pt") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_usp_gpu.py"), "--rank", str(r), "--port", str(port),
                               "--backend", backend, "--config", config, "--seq", str(seq), "--out", outs[r]], cwd=ROOT)
             for r in range(2)]
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


def _compare(ref, ranks, bars):
    diffs = {}
    mean_loss = (ranks[0]["plosses"] + ranks[1]["plosses"]) / 2
    diffs["loss"] = float((mean_loss - ref["plosses"]).abs().max())
    assert torch.equal(ranks[0]["acces"], ranks[1]["acces"])     # global counts: the same on both ranks
    diffs["acc"] = float((ranks[0]["acces"] - ref["acces"]).abs().max())
    g = ranks[0]["grad"] / 2
    diffs["grad"] = float((g - ref["grad"]).abs().max()) / float(ref["grad"].abs().max())
    clear = ref["grad"].abs() > 4 * (g - ref["grad"]).abs().max()   # (see tests/test_usp.py::_compare)
    diffs["clear_frac"] = float(clear.float().mean())
    diffs["params"] = float((ranks[0]["params"].float() - ref["params"].float())[clear].abs().max()) if clear.any() else 0.0
    print("usp vs unsharded:", diffs)
    for k, bar in bars.items():
        assert diffs[k] <= bar, (k, diffs[k], bar)


@pytest.mark.gpu
@pytest.mark.parametrize("config,seq", CASES, ids=[f"{c}-1x{s}" for c, s in CASES])
def test_two_ranks_share_one_device_over_gloo(tmp_path, config, seq):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    ref = _unsharded(config, seq)
    _compare(ref, _ranks(tmp_path, config, seq, "gloo"), BARS[(config, seq)])


@pytest.mark.gpu
def test_two_ranks_over_rccl(tmp_path):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    if torch.cuda.device_count() < 2:
        pytest.skip("RCCL SP 2 needs two devices")
    config, seq = CASES[1]
    ref = _unsharded(config, seq)
    _compare(ref, _ranks(tmp_path, config, seq, "nccl"), BARS[(config, seq)])
