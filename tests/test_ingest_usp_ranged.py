"""The ranged USP reader of ``HiddenStateIngest(sp_rank=, sp_size=)`` on CPU (no reference needed): each rank reads only its shard's
``ceil(S / sp) + ttt_length`` rows of every tensor from the file, and its batches are ``torch.equal`` to ``usp_shard`` of the whole
sample read and normalised -- for sp 2 and 4 (the ring layouts u x r = 1 x 2, 2 x 2, 1 x 4 shard by the same sp_rank = ring_rank * u +
ulysses_rank), uneven lengths, samples shorter than sp * (ttt_length + 1) and samples truncated at max_len; in ``usp_shard``'s layout
and in the reference collator's padded one."""
import os

import pytest
import torch

from specforge_amd.ingest import HiddenStateIngest, normalize_offline_sample, usp_shard

T = 3
MAX_LEN = 40
LENGTHS = [33, 5, 2, 17, 40, 47, 9, 3, 28, 1]
H = 64


def _files(tmp_path, lengths=LENGTHS):
    out = []
    for i, n in enumerate(lengths):
        g = torch.Generator().manual_seed(i)
        p = str(tmp_path / f"{i:04d}.ckpt")
        torch.save(dict(input_ids=torch.randint(0, 1000, (n,), generator=g), loss_mask=(torch.rand(n, generator=g) > 0.3).long(),
                        hidden_state=torch.randn(1, n, H, generator=g).to(torch.bfloat16),
                        aux_hidden_state=torch.randn(1, n, 3 * H, generator=g).to(torch.bfloat16)), p)
        out.append(p)
    return out


def _want(path, sp_rank, sp, collator_u=None):
    s = usp_shard(normalize_offline_sample(torch.load(path, weights_only=True), MAX_LEN), ttt_length=T, sp_rank=sp_rank, sp_size=sp)
    if collator_u is None:
        return s
    # the reference collator under SP (data/utils.py:122-196): ids / masks / target zero-padded to a multiple of sp, hidden_state not,
    # position ids zero-padded to that length times the Ulysses degree
    local = s["input_ids"].shape[1]
    L = -(-local // sp) * sp
    pad = lambda t, n: torch.cat([t, t.new_zeros((1, n - t.shape[1]) + tuple(t.shape[2:]))], dim=1)
    return dict(s, input_ids=pad(s["input_ids"], L), attention_mask=pad(s["attention_mask"], L), loss_mask=pad(s["loss_mask"], L),
                target=pad(s["target"], L), position_ids=pad(s["position_ids"], L * collator_u))


@pytest.mark.parametrize("sp,u", [(2, 2), (2, 1), (4, 4), (4, 2), (4, 1)], ids=["sp2", "ring2", "sp4", "u2xr2", "ring4"])
@pytest.mark.parametrize("collator", [False, True], ids=["usp_shard", "collator"])
@pytest.mark.parametrize("direct", [True, False], ids=["ranged", "generic"])
def test_ranged_shards_equal_usp_shard_of_a_full_read(tmp_path, sp, u, collator, direct):
    files = _files(tmp_path)
    for sp_rank in range(sp):
        ing = HiddenStateIngest(files, batch_size=1, max_len=MAX_LEN, device="cpu", shuffle=False, sp_rank=sp_rank, sp_size=sp,
                                ttt_length=T, direct=direct, collator_layout=collator, sp_ulysses_size=u)
        n = 0
        for b in ing.epoch(0):
            want = _want(files[b.metadata["sample_indices"][0]], sp_rank, sp, u if collator else None)
            assert set(b.tensors) == set(want)
            for k, v in want.items():
                assert b.tensors[k].dtype == v.dtype and torch.equal(b.tensors[k], v), (sp_rank, n, k)
            n += 1
        assert n == len(files)


def test_draft_dp_sampling_and_epochs(tmp_path):
    """the SP peers of a draft-dp rank get the same samples, in the same order, every epoch"""
    files = _files(tmp_path)
    for dp_rank in range(2):
        for epoch in (0, 1):
            seen = [[b.metadata["sample_indices"] for b in HiddenStateIngest(files, batch_size=1, max_len=MAX_LEN, device="cpu", seed=5,
                                                                            dp_rank=dp_rank, dp_size=2, sp_rank=r, sp_size=2,
                                                                            ttt_length=T).epoch(epoch)]
                    for r in range(2)]
            assert seen[0] == seen[1] and len(seen[0]) == len(files) // 2


def _rchar():
    with open("/proc/self/io") as f:
        return int(next(line for line in f if line.startswith("rchar")).split()[1])


@pytest.mark.parametrize("sp", [2, 4])
def test_ranged_reader_reads_only_the_shard(tmp_path, monkeypatch, sp):
    """payload bytes (counted at os.preadv) are exactly this rank's rows; everything the process read (/proc/self/io rchar, headers
    included) stays within those rows plus 64 KiB of zip / pickle headers per file"""
    S = 4096
    files = _files(tmp_path, [S, S])
    row = 4 * H * 2 + 2 * 8                       # hidden_state + target (bf16), input_ids + loss_mask (int64)
    counted = [0]
    real = os.preadv

    def preadv(fd, bufs, off):
        got = real(fd, bufs, off)
        counted[0] += got
        return got

    monkeypatch.setattr(os, "preadv", preadv)
    for sp_rank in range(sp):
        ing = HiddenStateIngest(files, batch_size=1, max_len=S, device="cpu", shuffle=False, sp_rank=sp_rank, sp_size=sp, ttt_length=T,
                                reader_threads=1)
        counted[0] = 0
        r0 = _rchar()
        n = sum(1 for _ in ing.epoch(0))
        read = _rchar() - r0
        rows = min(-(-S // sp) + T, S - sp_rank * -(-S // sp))
        assert n == 2 and counted[0] == 2 * rows * row, (sp_rank, counted[0])
        assert read <= 2 * (rows * row + 64 * 1024), (sp_rank, read, 2 * rows * row)
        assert read < 2 * S * row / sp * 1.1          # vs a full read of 2 * S rows
