"""The reduced teacher and loss-row compaction under USP on the MI355X: gloo ranks sharing cuda:0 (at most three processes hold the
device: pytest + two ranks), each under a time limit.  A sparse chat-like loss mask (bench.make_loss_mask, density 0.5) in host
memory: every rank passes its window counts, so the teacher keeps only its draft logits and runs over the gathered positions, lm_head
/ CE over the rows with a loss.  Held to the unsharded sparse step of the same model and sample (bars: about twice the difference
measured on the MI355X, recorded beside each); each rank's peak allocation against the same USP step with the dense teacher (the
[St, Vt] bf16 logits scratch and target_p [St, Vd] fp32, St = chunk + T teacher rows) by the arithmetic of those arrays."""
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900

# (config, seq, u, r): Llama-3-8B dims 1 x 8192 at Ulysses 2 and at ring 2; the head_dim-256 draft 1 x 8000 at ring 2 (chunk 4000: the
# ring offset is not a multiple of the 128-query block)
CASES = [("llama3-8b", 8192, 2, 1), ("llama3-8b", 8192, 1, 2), ("hd256", 8000, 1, 2)]
# (loss: about an fp32 ulp of the loss where the measurement was exact)
BARS = {("llama3-8b", 8192, 2, 1): dict(loss=1e-6, acc=0.0, grad=1e-2),      # measured: loss 0, acc 0, grad 4.9e-3
        ("llama3-8b", 8192, 1, 2): dict(loss=1e-6, acc=0.0, grad=1e-2),      # measured: loss 0, acc 0, grad 4.9e-3
        ("hd256", 8000, 1, 2): dict(loss=1.2e-6, acc=0.0, grad=1.1e-2)}      # measured: loss 5.7e-7, acc 0, grad 5.4e-3
# Memory (measured, per rank, GB of peak allocation saved against the dense teacher / the arithmetic scratch + target_p - zd):
# Llama-3-8B dims u2 and u1r2: reduced 1.315 / compact 1.178 - 1.189 / 1.315; hd256 u1r2: reduced 1.345 / compact 1.276 - 1.281 / 1.345


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dims(config):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _usp_ring_gpu as R

    return R.dims(config)


def _ranks(tmp_path, config, seq, u, r):
    port, world = _free_port(), u * r
    outs = [str(tmp_path / f"rank{x}.pt") for x in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_usp_reduced_teacher_gpu.py"), "--rank", str(x), "--ulysses",
                               str(u), "--ring", str(r), "--port", str(port), "--config", config, "--seq", str(seq), "--out", outs[x]],
                              cwd=ROOT) for x in range(world)]
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(timeout=CHILD_TIMEOUT))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail(f"USP rank did not finish within {CHILD_TIMEOUT} s")
    assert rcs == [0] * world, rcs
    return [torch.load(o) for o in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("config,seq,u,r", CASES, ids=[f"{c}-1x{s}-u{u}r{r}" for c, s, u, r in CASES])
def test_usp_reduced_teacher_and_compaction_on_device(tmp_path, config, seq, u, r):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _usp_reduced_teacher_gpu as G

    ref = G.run_mode("compact", config, seq, torch.device("cuda", 0))          # the unsharded sparse step (suffix counts)
    assert ref["compacted"] and ref["soft"] == "zt"
    ranks = _ranks(tmp_path, config, seq, u, r)
    world, T = u * r, G.W.T
    d = _dims(config)
    St = seq // world + T
    Vt, Vd = d["vocab_size"], d["draft_vocab_size"]
    scratch, tp, zd = St * Vt * 2, St * Vd * 4, St * ((Vd + 255) // 256 * 256) * 2
    diffs = {}
    for x, rk in enumerate(ranks):
        c, m, dn = rk["compact"], rk["reduced"], rk["dense"]
        assert c["compacted"] and c["soft"] == "zt" and c["lm_compact"], x
        assert not m["compacted"] and m["soft"] == "zt" and not m["lm_compact"]
        assert not dn["compacted"] and dn["soft"] == "tp" and not dn["lm_compact"]
        for mode in ("reduced", "dense"):       # the three forms of the same USP step
            torch.testing.assert_close(rk[mode]["plosses"], c["plosses"], rtol=1e-4, atol=1e-5)
            assert torch.equal(rk[mode]["acces"], c["acces"])
        # memory: the reduced teacher drops the logits scratch and target_p for zd; the gathered form adds its own scratch (the head GEMM's
        # output for <= teacher_compact_rows gathered rows, [rows, roundup(Vd, 256)] bf16, and their hidden rows [rows, Ht] bf16)
        gathered = 4096 * ((Vd + 255) // 256 * 256) * 2 + St * d["target_hidden_size"] * 2
        diffs[f"rank{x}_saved_gb"] = dict(reduced=(dn["peak_delta"] - m["peak_delta"]) / 1e9, compact=(dn["peak_delta"] - c["peak_delta"]) / 1e9,
                                          arithmetic=(scratch + tp - zd) / 1e9)
        # (slack: the caching allocator rounds each block up to 2 MiB -- zd's rounding is the only one against the saving)
        slack = 2 << 20
        assert dn["peak_delta"] - m["peak_delta"] >= scratch + tp - zd - slack, diffs
        assert dn["peak_delta"] - c["peak_delta"] >= scratch + tp - zd - gathered - slack, diffs
    mean_loss = sum(rk["compact"]["plosses"] for rk in ranks) / world
    diffs["loss"] = float((mean_loss - ref["plosses"]).abs().max())
    diffs["acc"] = float((ranks[0]["compact"]["acces"] - ref["acces"]).abs().max())
    g = ranks[0]["compact"]["grad"] / world
    diffs["grad"] = float((g - ref["grad"]).abs().max()) / float(ref["grad"].abs().max())
    print("usp compact vs unsharded:", diffs)
    for k, bar in BARS[(config, seq, u, r)].items():
        assert diffs[k] <= bar, (k, diffs[k], bar)
