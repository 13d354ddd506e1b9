"""Ulysses (attention_backend "usp") exchange layouts: sf_ulysses_pack_qkv / sf_ulysses_pack_o / sf_ulysses_unpack_o against a torch
restatement of the all-to-all images of LlamaUSPFlashAttention (reference llama3_eagle.py:1363-1505).  The RoPE fused into the qkv
pack is held bit for bit to ops.rope_ followed by the permutation; on the GPU the kernels give the bits of the interpreter build."""
import pytest
import torch

from specforge_amd import _lib, ops
from specforge_amd.model import DraftConfig, rope_tables

CASES = [  # (sp, nh, nkv, hd, chunk, pos_off, rope_type)
    (2, 4, 2, 64, 24, 0, None),
    (2, 8, 2, 128, 19, 3, "dynamic"),
    (4, 8, 4, 64, 13, 6, None),
    (4, 4, 4, 256, 9, 1, "dynamic"),
    (2, 2, 2, 256, 40, 2, None),
]


def _tables(hd, rope_type, device):
    rs = {"rope_type": "dynamic", "factor": 2.0} if rope_type == "dynamic" else None
    cfg = DraftConfig(hidden_size=4 * hd, intermediate_size=64, num_attention_heads=4, num_key_value_heads=2, vocab_size=64,
                      draft_vocab_size=32, head_dim=hd, max_position_embeddings=128, rope_scaling=rs)
    cos, sin = rope_tables(cfg, torch.bfloat16, n_pos=300 if rope_type == "dynamic" else None)
    return cos.to(device), sin.to(device)


def _to_blocks(tok, sp, nh, nkv, hd):
    """token rows [chunk, (nh+2nkv)*hd] -> [sp*chunk, (nh+2nkv)*hd/sp]: block j = rank j's q | k | v heads"""
    chunk = tok.shape[0]
    q = tok[:, :nh * hd].reshape(chunk, sp, nh // sp * hd)
    k = tok[:, nh * hd:(nh + nkv) * hd].reshape(chunk, sp, nkv // sp * hd)
    v = tok[:, (nh + nkv) * hd:(nh + 2 * nkv) * hd].reshape(chunk, sp, nkv // sp * hd)
    return torch.cat([q, k, v], dim=2).transpose(0, 1).reshape(sp * chunk, -1)


def _from_blocks(sh, sp, nh, nkv, hd):
    chunk = sh.shape[0] // sp
    x = sh.reshape(sp, chunk, -1).transpose(0, 1)
    gq, gk = nh // sp * hd, nkv // sp * hd
    return torch.cat([x[:, :, :gq].reshape(chunk, -1), x[:, :, gq:gq + gk].reshape(chunk, -1),
                      x[:, :, gq + gk:].reshape(chunk, -1)], dim=1)


def _run_case(dev, sp, nh, nkv, hd, chunk, off, rope_type, seed=0):
    """-> (packed forward, unpacked backward, their restatements) on ``dev``"""
    g = torch.Generator().manual_seed(seed)
    W = (nh + 2 * nkv) * hd
    ld = W + 16                                  # a token-row stride wider than the row (the qkv GEMM output is a view)
    tok = torch.randn(chunk, ld, generator=g).to(torch.bfloat16).to(dev)[:, :W]
    dsh = torch.randn(sp * chunk, W // sp, generator=g).to(torch.bfloat16).to(dev)
    pos = (torch.arange(chunk) + 5 * chunk).to(dev)          # global positions of a later rank
    cos, sin = _tables(hd, rope_type, dev)
    kw = dict(sp=sp, nh=nh, nkv=nkv, hd=hd, cos_t=cos, sin_t=sin, pos_ids=pos, pos_off=off)
    send = torch.empty(sp * chunk, W // sp, dtype=torch.bfloat16, device=dev)
    ops.ulysses_pack_qkv(tok, send, **kw)
    ref = tok.clone()
    ops.rope_(ref, nh + nkv, hd, cos, sin, pos, off)
    ref_send = _to_blocks(ref, sp, nh, nkv, hd)
    dtok = torch.zeros(chunk, ld, dtype=torch.bfloat16, device=dev)[:, :W]
    ops.ulysses_pack_qkv(dsh, dtok, backward=True, **kw)
    ref_tok = _from_blocks(dsh, sp, nh, nkv, hd).contiguous()
    ops.rope_(ref_tok, nh + nkv, hd, cos, sin, pos, off, backward=True)
    return send, dtok, ref_send, ref_tok


@pytest.mark.parametrize("case", CASES, ids=lambda c: "sp%d-nh%d-nkv%d-hd%d-chunk%d-off%d-%s" % c)
def test_pack_qkv_matches_rope_then_permutation(backend, case):
    send, dtok, ref_send, ref_tok = _run_case(backend, *case)
    assert torch.equal(send.view(torch.int16), ref_send.view(torch.int16))
    assert torch.equal(dtok.view(torch.int16), ref_tok.view(torch.int16))


@pytest.mark.parametrize("sp,nh,nkv,hd,chunk", [(2, 4, 2, 64, 24), (4, 8, 4, 128, 11), (2, 2, 2, 256, 7)])
def test_pack_unpack_identity(backend, sp, nh, nkv, hd, chunk):
    dev = backend
    g = torch.Generator().manual_seed(1)
    W = (nh + 2 * nkv) * hd
    tok = torch.randn(chunk, W, generator=g).to(torch.bfloat16).to(dev)
    # cos 1 / sin 0: the rotation is the identity in both directions, what remains is the permutation and its inverse
    cos = torch.ones(8, hd, dtype=torch.bfloat16, device=dev)
    sin = torch.zeros(8, hd, dtype=torch.bfloat16, device=dev)
    pos = torch.zeros(chunk, dtype=torch.int64, device=dev)
    kw = dict(sp=sp, nh=nh, nkv=nkv, hd=hd, cos_t=cos, sin_t=sin, pos_ids=pos, pos_off=0)
    sh = torch.empty(sp * chunk, W // sp, dtype=torch.bfloat16, device=dev)
    back = torch.empty_like(tok)
    ops.ulysses_pack_qkv(tok, sh, **kw)
    assert torch.equal(sh.view(torch.int16), _to_blocks(tok, sp, nh, nkv, hd).view(torch.int16))
    ops.ulysses_pack_qkv(sh, back, backward=True, **kw)
    assert torch.equal(back.view(torch.int16), tok.view(torch.int16))
    # O / dO: [chunk, nh*hd] <-> [sp*chunk, nh/sp*hd]
    w = nh // sp * hd
    o_tok = torch.randn(chunk, nh * hd + 8, generator=g).to(torch.bfloat16).to(dev)[:, :nh * hd]
    o_sh = torch.empty(sp * chunk, w, dtype=torch.bfloat16, device=dev)
    ops.ulysses_pack_o(o_tok, o_sh, sp=sp)
    assert torch.equal(o_sh, o_tok.reshape(chunk, sp, w).transpose(0, 1).reshape(sp * chunk, w))
    o_back = torch.zeros(chunk, nh * hd, dtype=torch.bfloat16, device=dev)
    ops.ulysses_unpack_o(o_sh, o_back, sp=sp)
    assert torch.equal(o_back, o_tok)


def test_pack_qkv_refuses_uneven_heads(backend):
    dev = backend
    x = torch.zeros(4, 4 * 64, dtype=torch.bfloat16, device=dev)
    y = torch.zeros(8, 2 * 64, dtype=torch.bfloat16, device=dev)
    cos = torch.ones(8, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(_lib.SfError, match="split evenly"):   # nkv = 1 over 2 ranks
        _lib.check(_lib.lib().sf_ulysses_pack_qkv(ops._p(x), 4 * 64, ops._p(y), 2 * 64, 4, 2, 2, 1, 64, ops._p(cos), ops._p(cos),
                                                   ops._p(torch.zeros(4, dtype=torch.int64, device=dev)), 0, 8, 0, ops._stream()),
                   "sf_ulysses_pack_qkv")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "sp%d-nh%d-nkv%d-hd%d-chunk%d-off%d-%s" % c)
def test_device_bits_equal_interpreter_bits(emu_lib_path, case):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    try:
        _lib._inject_library_for_tests(emu_lib_path)
        emu = [t.clone() for t in _run_case("cpu", *case, seed=7)]
    finally:
        _lib._inject_library_for_tests(None)
    dev = [t.cpu() for t in _run_case("cuda", *case, seed=7)]
    for a, b in zip(emu, dev):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
