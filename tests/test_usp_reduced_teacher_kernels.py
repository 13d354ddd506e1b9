"""sf_ce_fused_zt_rows: the fused CE on the teacher's stored draft logits with St teacher rows per sample.  Under USP a rank's teacher
covers its chunk of S rows plus the T rows of overlap from the next shard (real targets, not constant tails), so TTT step `off` of row
(b, s) reads teacher row b * St + s + off, St = S + T.  Held bit for bit to sf_ce_fused on the target_p array the same teacher kernel
materialises (losses, in-place gradients, accuracy, acceptance, with and without a row_map), and with St == S to sf_ce_fused_zt."""
import pytest
import torch

from oracle import eagle3_oracle as O
from specforge_amd import _lib, ops


def _teacher(backend, B, S, T, Vt, Vd, seed):
    """teacher draft logits of B samples with St = S + T rows each (the overlap rows carry a loss mask), reduced by sf_teacher_reduce_perm
    into the materialised target_p and the (zmd, zinv) row scalars"""
    St = Spad = S + T
    g = torch.Generator().manual_seed(seed)
    zfull = (torch.randn(B * St, Vt, generator=g) * 3).to(torch.bfloat16)
    t2d, d2t = O.make_vocab_mapping(Vt, Vd, seed=seed + 1)
    perm = torch.cat([torch.arange(Vd) + d2t, torch.nonzero(~t2d.bool()).flatten()])
    zp = zfull[:, perm].contiguous()
    d = lambda t: t.to(backend)
    lm = (torch.rand(B, Spad, generator=g) > 0.3).int()
    lm[:, S:] = 1                                  # the next shard's first positions: real targets
    lm[:, Spad - 1] = 0
    tp = torch.full((B, Spad, Vd), 1.0 / Vd, device=backend)
    o = dict(pod_scale_pad=torch.zeros(B, Spad, device=backend), tsum_pad=torch.zeros(B, Spad, device=backend),
             ids_pad=torch.zeros(B, Spad, dtype=torch.int64, device=backend), pos_mask_pad=torch.zeros(B, Spad, dtype=torch.int32, device=backend))
    zmd, zinv = torch.zeros(B, Spad, device=backend), torch.zeros(B, Spad, device=backend)
    ops.teacher_reduce_perm(d(zp), Vt=Vt, Vd=Vd, perm=d(perm.to(torch.int32)), t2d_u8=d(t2d.to(torch.uint8)), loss_mask_pad=d(lm),
                            S=St, Spad=Spad, target_p_pad=tp, zmd_pad=zmd, zinv_pad=zinv, **o)
    zd = torch.zeros(B * St, Vd + 8, dtype=torch.bfloat16)          # the stored draft logits (wider rows, as the engine's roundup(Vd, 256))
    zd[:, :Vd] = zp[:, :Vd]
    return dict(St=St, Spad=Spad, tp=tp, zd=d(zd), zmd=zmd, zinv=zinv, lm=d(lm), d2t=d(d2t), **o)


def _ce(backend, x, t, *, form, S, off, row_map=None):
    n = x.shape[0]
    rows = [torch.zeros(n, device=backend) for _ in range(3)]
    pred = torch.zeros(n, dtype=torch.int32, device=backend)
    common = dict(S=S, Spad=t["Spad"], off=off, pos_mask_pad=t["pos_mask_pad"], loss_mask_pad=t["lm"], tgt_ids_pad=t["ids_pad"],
                  pod_scale_pad=t["pod_scale_pad"], tsum_pad=t["tsum_pad"], d2t=t["d2t"], grad_scale=0.37, write_grad=True,
                  row_loss=rows[0], row_correct=rows[1], row_accept=rows[2], row_pred=pred, row_map=row_map)
    if form == "tp":
        ops.ce_fused(x, t["tp"], **common)
    elif form == "zt":
        ops.ce_fused_zt(x, t["zd"], t["zmd"], t["zinv"], **common)
    else:
        ops.ce_fused_zt_rows(x, t["zd"], t["zmd"], t["zinv"], St=t["St"], **common)
    return [x.cpu()] + [r.cpu() for r in rows] + [pred.cpu()]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ce_on_overlap_teacher_rows_equals_materialised_targets(backend, dtype):
    B, S, T, Vt, Vd = 2, 12, 3, 640, 384
    t = _teacher(backend, B, S, T, Vt, Vd, seed=31)
    g = torch.Generator().manual_seed(32)
    pm = t["pos_mask_pad"].cpu()
    for off in range(T):
        if off > 0:                                 # the rows that read the overlap carry a position mask: the overlap is exercised
            assert int(pm[:, S:S + off].sum()) > 0
        logits = (torch.randn(B * S, Vd, generator=g) * 2).to(dtype)
        dense = _ce(backend, logits.clone().to(backend), t, form="tp", S=S, off=off)
        rows = _ce(backend, logits.clone().to(backend), t, form="zt_rows", S=S, off=off)
        for a, b_ in zip(dense, rows):
            assert torch.equal(a, b_)
        assert float(dense[1].abs().sum()) > 0
        # row_map (loss-row compaction): a compact copy of the rows with loss_mask[b, s + off] != 0 -- the window, overlap included
        keep = torch.nonzero(t["lm"].cpu()[:, off:off + S].reshape(-1)).view(-1)
        for form in ("tp", "zt_rows"):
            comp = _ce(backend, logits[keep].clone().to(backend), t, form=form, S=S, off=off, row_map=keep.to(backend))
            for i, a in enumerate(comp):
                assert torch.equal(a, dense[i][keep]), (form, off, i)
        left = torch.ones(B * S, dtype=torch.bool)
        left[keep] = False
        assert float(dense[0][left].float().abs().max()) == 0


def test_ce_rows_with_natural_teacher_rows_equals_ce_fused_zt(backend):
    """St == S (no sequence parallelism): the new entry gives the bits of sf_ce_fused_zt, which forces the mask to 0 for s + off >= S"""
    B, S, T, Vt, Vd = 2, 12, 3, 640, 256
    t = _teacher(backend, B, S, 0, Vt, Vd, seed=41)         # S teacher rows per sample ...
    Spad = S + T                                            # ... laid into arrays padded for the TTT shift
    for k in ("pod_scale_pad", "tsum_pad", "ids_pad", "pos_mask_pad", "zmd", "zinv", "lm"):
        v = t[k]
        pad = torch.zeros(B, Spad, dtype=v.dtype, device=v.device)
        pad[:, :S] = v
        t[k] = pad
    t["lm"][:, S:] = 1              # (a mask past the sample's end must not be read: sf_ce_fused_zt forces position mask 0 there)
    t["pos_mask_pad"][:, S:] = 1
    t["Spad"] = Spad
    g = torch.Generator().manual_seed(42)
    for off in range(T):
        logits = (torch.randn(B * S, Vd, generator=g) * 2).to(torch.bfloat16)
        a = _ce(backend, logits.clone().to(backend), t, form="zt", S=S, off=off)
        b_ = _ce(backend, logits.clone().to(backend), t, form="zt_rows", S=S, off=off)
        for x, y in zip(a, b_):
            assert torch.equal(x, y)
        keep = torch.arange(0, B * S, 3)
        a = _ce(backend, logits[keep].clone().to(backend), t, form="zt", S=S, off=off, row_map=keep.to(backend))
        b_ = _ce(backend, logits[keep].clone().to(backend), t, form="zt_rows", S=S, off=off, row_map=keep.to(backend))
        for x, y in zip(a, b_):
            assert torch.equal(x, y)


def test_ce_rows_refuses_bad_teacher_row_counts(backend):
    B, S, T, Vd = 1, 8, 3, 256
    t = _teacher(backend, B, S, T, 640, Vd, seed=51)
    x = torch.zeros(B * S, Vd, dtype=torch.bfloat16, device=backend)
    t["zd"] = torch.zeros(B * (S + T + 1), Vd, dtype=torch.bfloat16, device=backend)
    for St in (S - 1, S + T + 1):      # fewer teacher rows than chunk rows, or more than the padded arrays hold
        t["St"] = St
        with pytest.raises(_lib.SfError, match="sf_ce_fused_zt_rows"):
            _ce(backend, x, t, form="zt_rows", S=S, off=0)
