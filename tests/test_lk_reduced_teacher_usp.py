"""An LK objective under USP on the reduced teacher and compacted loss rows: two gloo ranks (kernels under the SIMT interpreter), SP 2 as
Ulysses 2 and as ring 2, LK lambda, a turn-like loss mask of density 0.5, a shape the reduced head GEMM takes.  Every rank keeps only
the teacher's draft logits and compacts; losses, accuracies, gradients and updated weights against the unsharded single-process step
at the bars tests/test_usp.py holds its lambda case to (read from that module)."""
import pytest
import torch
import torch.multiprocessing as mp

import _lk_usp_worker as W
import test_usp as U


@pytest.mark.parametrize("ring", [1, 2], ids=["ulysses2", "ring2"])
def test_lk_usp_step_on_the_reduced_teacher_matches_unsharded_step(emu_lib_path, tmp_path, ring):
    sp, S_ = 2, 2 * W.CHUNK
    mp.spawn(W.worker, args=(sp, ring, S_, U._free_port(), emu_lib_path, "lambda", str(tmp_path)), nprocs=sp, join=True)
    for r in range(sp):
        rk = torch.load(tmp_path / f"rank{r}.pt")
        assert rk["soft"] == "zt" and rk["compacted"] and rk["lm_compact"], (r, rk["soft"], rk["compacted"], rk["lm_compact"])
        assert "tp" not in rk["names"] and "teacher_z" not in rk["names"]
    ref = W.single(emu_lib_path, "lambda", S_)
    assert ref["soft"] == "zt" and ref["compacted"] and ref["lm_compact"]
    U._compare(tmp_path, sp, sp, dict(plosses=[ref["plosses"]], acces=[ref["acces"]], grad=ref["grad"], params=ref["params"]), [11],
               U.BARS[(2, "lambda")])
