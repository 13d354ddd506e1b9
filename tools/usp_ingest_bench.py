"""Ranged vs full read of USP shards (``HiddenStateIngest(sp_rank=, sp_size=)``): bytes read from the files per rank and files -> HBM
time per sample, at Llama-3-8B target dims (Ht 4096: 4 * Ht bf16 = 32 KiB of hidden states per token), one sample of S tokens.

    python tools/usp_ingest_bench.py [--seq 32768] [--sp 2] [--files 2] [--device cuda|cpu] > usp_ingest_bench.json

* ranged: what the ingest does under SP -- every rank reads only its ``ceil(S / sp) + ttt_length`` rows of each tensor into the
  pinned slot and sends that to the device;
* full: what it did before -- the whole sample read into the pinned slot and sent to the device, then ``usp_shard`` there.
Bytes are counted at ``os.preadv`` (the tensor payload; the zip headers are parsed once per file and cached).  Times are
the mean over the files of the second pass (page cache warm), per rank; the ranks run one after the other in this process."""
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, ".")
from specforge_amd import ingest as I  # noqa: E402


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


S, sp, nfiles, T = arg("--seq", 32768), arg("--sp", 2), arg("--files", 2), 7
Ht = arg("--hidden", 4096)
dev = torch.device(arg("--device", "cuda" if torch.cuda.is_available() else "cpu", str))
d = tempfile.mkdtemp(prefix="usp_ingest_")
g = torch.Generator().manual_seed(0)
files = []
for i in range(nfiles):
    p = os.path.join(d, f"{i:05d}.ckpt")
    torch.save({"input_ids": torch.randint(0, 128256, (S,), generator=g), "loss_mask": torch.ones(S, dtype=torch.long),
                "hidden_state": torch.randn(1, S, Ht, generator=g).to(torch.bfloat16),
                "aux_hidden_state": torch.randn(1, S, 3 * Ht, generator=g).to(torch.bfloat16)}, p)
    files.append(p)

counted = [0]
_preadv = os.preadv


def preadv(fd, bufs, off):
    n = _preadv(fd, bufs, off)
    counted[0] += max(n, 0)
    return n


os.preadv = preadv


def sync():
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def run(kind, sp_rank):
    if kind == "ranged":
        ing = I.HiddenStateIngest(files, batch_size=1, max_len=S, target_hidden_size=Ht, device=dev, shuffle=False, sp_rank=sp_rank,
                                  sp_size=sp, ttt_length=T)
    else:
        ing = I.HiddenStateIngest(files, batch_size=1, max_len=S, target_hidden_size=Ht, device=dev, shuffle=False)
    out = None
    for rep in range(2):          # rep 0 warms the page cache and the pinned slots
        counted[0] = 0
        sync()
        t0 = time.perf_counter()
        n = 0
        for b in ing.stream([[f] for f in files]):
            if kind == "full":
                I.usp_shard(b.tensors, ttt_length=T, sp_rank=sp_rank, sp_size=sp)
            n += 1
        sync()
        dt = time.perf_counter() - t0
        out = dict(bytes_read_per_sample=counted[0] // n, ms_per_sample=round(1e3 * dt / n, 2))
    return out


res = dict(seq=S, sp=sp, ttt_length=T, target_hidden_size=Ht, files=nfiles, device=str(dev),
           shard_rows=-(-S // sp) + T, full_sample_bytes=S * (4 * Ht * 2 + 2 * 8))
for r in range(sp):
    res[f"rank{r}"] = dict(ranged=run("ranged", r), full=run("full", r))
res["bytes_ratio_rank0"] = round(res["rank0"]["ranged"]["bytes_read_per_sample"] / res["rank0"]["full"]["bytes_read_per_sample"], 4)
res["time_ratio_rank0"] = round(res["rank0"]["ranged"]["ms_per_sample"] / res["rank0"]["full"]["ms_per_sample"], 3)
for f in files:
    os.remove(f)
os.rmdir(d)
print(json.dumps(res))
