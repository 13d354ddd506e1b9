"""sf_conf_fold (per-row reliability bins, gated hits and drafted rows of one TTT step) with sf_chain_step as the gating fold, against
a torch fold written like tests/test_chain_metrics._torch_fold.  Inputs are synthetic and every comparison is exact: torch forms the bin
with the same fp32 multiply and truncation and compares the same fp32 values with the same fp32 thresholds.

conf_tok holds -1, 0, 1.0, values exactly on bin edges and on thresholds and the float just below each, and random values; row_correct
is random 0/1 (0 where conf is -1, as a row that was not scored has no hit); the loss mask has holes.  All T steps are folded.  Cases:
NB in {0, 1, 10, 32}, J in {0, 1, 8}, thresholds including 0 and 1, dense rows / a row_map / a row_map with entries out of range."""
import pytest
import torch

from specforge_amd import _lib, ops
from f64_helpers import MARK, gpu  # noqa: F401
from test_topk_rank_kernel import KEEP

B, S, T = 2, 5, 3
SPAD, NTOK = S + T, B * S
TAUS = {0: (), 1: None, 8: (0.0, 0.1, 0.25, 0.3, 0.5, 0.75, 0.9, 1.0)}
MAPS = [None, KEEP, [8, 3, NTOK + 2, 0, -1, 5]]
F32 = torch.float32


def _taus(NB, J):
    return {0: (0.0,), 1: (1.0,), 10: (0.3,), 32: (0.5,)}[NB] if J == 1 else TAUS[J]


def specials(NB, tau):
    """the values that decide a comparison: 0, 1, every bin edge b / NB and every threshold as fp32, and the float just below each"""
    edges = [torch.tensor(b, dtype=F32) / NB for b in range(1, NB)] + [torch.tensor(t, dtype=F32) for t in tau if t > 0]
    vals = [torch.tensor(0.0), torch.tensor(1.0)]
    for e in edges:
        vals += [e, torch.nextafter(e, torch.tensor(0.0))]
    return torch.unique(torch.stack(vals))


def inputs(NB, tau, seed):
    """rounds of (conf [T, NTOK], row_correct [T, NTOK], loss mask [B, SPAD]) that together hold every special value under a loss mask"""
    g = torch.Generator().manual_seed(seed)
    sp = specials(NB, tau)
    sp = sp[torch.randperm(sp.numel(), generator=g)]
    rounds, used = [], 0
    while used < sp.numel() or len(rounds) < 2:
        lm = (torch.rand(B, SPAD, generator=g) < 0.85).to(torch.int32)
        mask = torch.stack([lm[:, k:k + S].reshape(-1) for k in range(T)])      # [T, NTOK]
        conf = torch.rand(T, NTOK, generator=g)
        conf[mask == 0] = -1.0                                   # what the engine's fill and sf_row_conf leave on a row without a loss mask
        idx = mask.view(-1).nonzero().flatten()
        idx = idx[torch.randperm(idx.numel(), generator=g)]
        part = sp[used:used + idx.numel() // 2]                  # half of the scored values are special, the rest random
        used += part.numel()
        conf.view(-1)[idx[:part.numel()]] = part
        deep = [int(i) for i in idx[part.numel():] if int(i) >= NTOK]
        conf.view(-1)[deep[0]] = -1.0                            # one row with a loss mask and no confidence (never at depth 0)
        rc = (torch.rand(T, NTOK, generator=g) < 0.7).float()
        rc[conf < 0] = 0.0                                       # a row that was not scored has no hit
        rounds.append((conf, rc, lm))
    return rounds, sp


def compact_rc(rc, k, maps):
    """row_correct of step k in the order of the step's rows (an entry out of range: 1, which must not count)"""
    if maps is None:
        return rc[k].clone()
    return torch.tensor([float(rc[k, rt]) if 0 <= rt < NTOK else 1.0 for rt in maps])


def torch_fold(conf, rc, lm, NB, tau, maps):
    """per step the expected row outputs of conf_fold and chain_step, and the final state"""
    J = len(tau)
    tau32 = torch.tensor(tau, dtype=F32)
    depth, length = torch.zeros(NTOK, dtype=torch.int32), torch.zeros(1 + J, NTOK, dtype=torch.int32)
    steps = []
    for k in range(T):
        rows = list(range(NTOK)) if maps is None else maps
        n = len(rows)
        rck = compact_rc(rc, k, maps)
        bins, gate, draft, chain = torch.zeros(3 * NB, n), torch.zeros(J, n), torch.zeros(J, n), torch.zeros(2 + J, n)
        for r, rt in enumerate(rows):
            if not 0 <= rt < NTOK:
                continue
            has = bool(lm[rt // S, rt % S + k])
            c = conf[k, rt]
            hit = bool(rck[r] != 0)
            scored = has and bool(c >= 0)
            if NB and scored:
                q = min(NB - 1, int((c * torch.tensor(float(NB), dtype=F32)).to(torch.int32)))
                bins[q, r], bins[NB + q, r], bins[2 * NB + q, r] = 1.0, float(hit), c
            over = c >= tau32
            for j in range(J):
                gate[j, r] = float(scored and hit and bool(over[j]))
                draft[j, r] = float(has and int(depth[rt]) == k and int(length[1 + j, rt]) == k and bool(over[j]))
            eligible = has and int(depth[rt]) == k
            if eligible:
                depth[rt] = k + 1
            chain[0, r] = float(eligible)
            for h in range(1 + J):
                alive = eligible and int(length[h, rt]) == k and bool(hit if h == 0 else gate[h - 1, r] != 0)
                if alive:
                    length[h, rt] = k + 1
                chain[1 + h, r] = float(alive)
        steps.append(dict(bins=bins, gate=gate, draft=draft, chain=chain))
    return steps, depth, length


def run_round(dev, conf, rc, lm, NB, tau, maps):
    J = len(tau)
    want, wdepth, wlen = torch_fold(conf, rc, lm, NB, tau, maps)
    n = NTOK if maps is None else len(maps)
    d = lambda t: t.to(dev)
    state = torch.zeros(2 + J, NTOK, dtype=torch.int32, device=dev)
    row_map = None if maps is None else d(torch.tensor(maps))
    conf_d, lm_d = d(conf.contiguous()), d(lm)
    totals = dict(drafted=torch.zeros(T, J), accepted=torch.zeros(T, 1 + J), eligible=torch.zeros(T))
    for k in range(T):
        bins = torch.full((3 * NB * n + 2,), MARK, device=dev)
        gate, draft = torch.full((J * n + 2,), MARK, device=dev), torch.full((J * n + 2,), MARK, device=dev)
        chain = torch.full(((2 + J) * n + 2,), MARK, device=dev)
        rck = d(compact_rc(rc, k, maps))
        kw = dict(rows=n, S=S, Spad=SPAD, off=k, loss_mask_pad=lm_d, row_correct=rck, row_map=row_map)
        before = state.clone()
        ops.conf_fold(conf_tok=conf_d[k], bins=NB, tau=tau, gate_depth=state[0] if J else None, gate_len=state[1:] if J else None,
                      row_bins=bins if NB else None, row_gate=gate if J else None, row_draft=draft if J else None, **kw)
        assert torch.equal(state, before)                      # the fold reads the state
        ops.chain_step(row_hit=gate[:J * n].view(J, n) if J else None, chain_depth=state[0], chain_len=state[1:], row_out=chain, **kw)
        w = want[k]
        for got, exp, C in ((bins, w["bins"], 3 * NB), (gate, w["gate"], J), (draft, w["draft"], J), (chain, w["chain"], 2 + J)):
            g = got.cpu()
            assert bool((g[C * n:] == MARK).all())
            assert torch.equal(g[:C * n].view(C, n), exp), (k, C, g[:C * n].view(C, n), exp)
        if NB:      # laid out for sf_reduce_sum: counts exact, the conf sum is the float64 sum rounded once
            out = torch.full((3 * NB + 1,), MARK, device=dev)
            ops.reduce_sum(bins, n, 3 * NB, out, 1.0)
            assert torch.equal(out.cpu()[:3 * NB], w["bins"].double().sum(1).float()) and float(out[3 * NB]) == MARK
        totals["drafted"][k], totals["accepted"][k], totals["eligible"][k] = w["draft"].sum(1), w["chain"][1:].sum(1), w["chain"][0].sum()
    assert torch.equal(state[0].cpu(), wdepth) and torch.equal(state[1:].cpu(), wlen)
    return totals


@pytest.mark.parametrize("NB,J", [(nb, j) for nb in (0, 1, 10, 32) for j in (0, 1, 8) if nb or j])
def test_conf_fold_against_torch(backend, NB, J):
    tau = _taus(NB, J)
    rounds, sp = inputs(NB, tau, seed=NB * 10 + J)
    seen = torch.cat([conf[conf >= 0] for conf, _, _ in rounds])
    assert all(bool((seen == v).any()) for v in sp)             # every special value is scored somewhere
    for i, (conf, rc, lm) in enumerate(rounds):
        for maps in MAPS:
            tot = run_round(backend, conf, rc, lm, NB, tau, maps)
            acc, drafted = tot["accepted"], tot["drafted"]
            assert bool((acc[1:] <= acc[:-1]).all())                            # monotone in depth
            if J:
                assert bool((acc[:, 2:] <= acc[:, 1:-1]).all())                 # monotone in the threshold (ascending)
                assert bool((acc[:, 1:] <= drafted).all())                      # an accepted token was drafted
                for j, t in enumerate(tau):
                    if t == 0.0:
                        assert torch.equal(acc[:, 1 + j], acc[:, 0])            # no gate: the top-1 chain
                        assert float(drafted[0, j]) == float(tot["eligible"][0])    # and every eligible row drafts at depth 0
            if maps is None:
                assert float(tot["eligible"][0]) > 0 and float(acc[0, 0]) > 0


def test_conf_fold_bad_arguments(backend):
    """33 bins, nine thresholds, a threshold over 1, no output at all: the ABI's error, nothing launched"""
    dev = backend
    conf = torch.rand(NTOK).to(dev)
    lm = torch.ones(B, SPAD, dtype=torch.int32, device=dev)
    rc = torch.ones(NTOK, device=dev)
    state = torch.zeros(10, NTOK, dtype=torch.int32, device=dev)
    bins = torch.full((3 * 33 * NTOK,), MARK, device=dev)
    gate, draft = torch.full((9 * NTOK,), MARK, device=dev), torch.full((9 * NTOK,), MARK, device=dev)
    kw = dict(rows=NTOK, S=S, Spad=SPAD, off=0, loss_mask_pad=lm, conf_tok=conf, row_correct=rc)
    with pytest.raises(_lib.SfError, match="sf_conf_fold"):
        ops.conf_fold(bins=33, row_bins=bins, **kw)
    with pytest.raises(_lib.SfError, match="sf_conf_fold"):
        ops.conf_fold(tau=(0.1,) * 9, gate_depth=state[0], gate_len=state, row_gate=gate, row_draft=draft, **kw)
    with pytest.raises(_lib.SfError, match="sf_conf_fold"):
        ops.conf_fold(tau=(0.5, 1.5), gate_depth=state[0], gate_len=state[1:4], row_gate=gate, row_draft=draft, **kw)
    with pytest.raises(_lib.SfError, match="sf_conf_fold"):
        ops.conf_fold(**kw)
    assert all(bool((t.cpu() == MARK).all()) for t in (bins, gate, draft))
    ops.conf_fold(bins=32, row_bins=bins, tau=(0.0,) * 8, gate_depth=state[0], gate_len=state[1:], row_gate=gate, row_draft=draft, **kw)
    assert bool((bins.cpu()[:96 * NTOK] != MARK).all()) and bool((gate.cpu()[:8 * NTOK] == 1.0).all()) and bool((draft.cpu()[:8 * NTOK] == 1.0).all())
