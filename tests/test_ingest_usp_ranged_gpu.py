"""The ranged USP ingest on the MI355X (no reference needed): the device batches it stages for sp 2 and 4 are bit-identical to a full
read staged to the device and sharded there, and a 2-rank gloo USP step on one device fed by it gives the loss, accuracy and
gradients of the same step fed by full reads.  At most three processes hold the device (pytest + two ranks); each rank runs under a
time limit."""
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900
T = 7

pytestmark = pytest.mark.gpu


def _sample(path, S, Ht, V, seed):
    g = torch.Generator().manual_seed(seed)
    torch.save(dict(input_ids=torch.randint(0, V, (S,), generator=g), loss_mask=(torch.rand(S, generator=g) > 0.5).long(),
                    hidden_state=torch.randn(1, S, Ht, generator=g).to(torch.bfloat16),
                    aux_hidden_state=torch.randn(1, S, 3 * Ht, generator=g).to(torch.bfloat16)), path)
    return path


@pytest.mark.parametrize("sp", [2, 4])
def test_ranged_device_batches_equal_full_read(tmp_path, sp):
    from specforge_amd import _lib
    from specforge_amd.ingest import HiddenStateIngest, usp_shard

    _lib._inject_library_for_tests(None)
    dev = torch.device("cuda", 0)
    files = [_sample(str(tmp_path / f"{i}.ckpt"), S, 512, 1000, i) for i, S in enumerate((4096, 4093, 9, 5000))]
    full = HiddenStateIngest(files, batch_size=1, max_len=4096, device=dev, shuffle=False)
    want = []
    for b in full.epoch(0):
        want.append([{k: v.cpu() for k, v in usp_shard(b.tensors, ttt_length=T, sp_rank=r, sp_size=sp).items()} for r in range(sp)])
    for r in range(sp):
        ing = HiddenStateIngest(files, batch_size=1, max_len=4096, device=dev, shuffle=False, sp_rank=r, sp_size=sp, ttt_length=T)
        n = 0
        for b in ing.epoch(0):
            assert all(v.is_cuda for v in b.tensors.values())
            w = want[n][r]
            assert set(b.tensors) == set(w)
            for k, v in w.items():
                assert torch.equal(b.tensors[k].cpu(), v), (r, n, k)
            n += 1
        assert n == len(files)


def test_usp_step_fed_by_ranged_ingest_equals_full_reads(tmp_path):
    S = 4096
    f = _sample(str(tmp_path / "s.ckpt"), S, 896, 151936, 11)       # cfg 1 dims (tests/_usp_gpu.py)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    outs = [str(tmp_path / f"rank{r}.pt") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_ingest_usp_ranged_gpu.py"), "--rank", str(r), "--port", str(port),
                               "--file", f, "--seq", str(S), "--out", outs[r]], cwd=ROOT) for r in range(2)]
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(timeout=CHILD_TIMEOUT))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail(f"USP rank did not finish within {CHILD_TIMEOUT} s")
    assert rcs == [0, 0], rcs
    for o in outs:
        res = torch.load(o)
        for k in ("plosses", "acces", "grad", "params"):
            assert torch.equal(res["ranged"][k], res["full"][k]), k
        assert res["ranged"]["grad"].abs().max() > 0
