"""One step of a tiny draft with the draft-confidence metrics on (tests/test_conf_usp.py), the same model and sample in every process
(those of tests/_topk_usp_worker.py, with lm_head scaled so that the confidences spread over the bins, and a teacher that names the
draft's own step-0 prediction at even positions and its neighbour at odd ones, so that depth 0 has hits and misses; top-k and chain
counts on as well, to show their columns stay where they are): as a module, the step the pytest process runs unsharded; as a script, one SP rank of a
two-rank world that exchanges over gloo under the SIMT interpreter (``--emu LIB``, CPU tensors) and writes its counts to ``--out``."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _topk_usp_worker as W  # noqa: E402

T, S = W.T, W.S
TOPK = (1, 64, 128)
BINS, TAU = 10, (0.0, 0.1, 0.2, 0.4)
LM_SCALE = 6.0      # the worker's step-0 logits have a standard deviation near 0.5; sqrt(2 ln 128) = 3.1 spreads the top-1 probability


def setup(dev, attention_backend="hip", backend_kw=None, lk=None):
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    cfg = DraftConfig(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2, vocab_size=256,
                      draft_vocab_size=128, head_dim=64, target_hidden_size=128, max_position_embeddings=128, rms_norm_eps=1e-5)
    m = LlamaForCausalLMEagle3(cfg, device=dev)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in m.named_parameters():       # (the parameters of W.setup, lm_head scaled)
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g) if "norm" in n else 0.05 * torch.randn(p.shape, generator=g)
            p.copy_((v * (LM_SCALE if n.startswith("lm_head") else 1.0)).to(p.device))
        t2d = torch.zeros(cfg.vocab_size, dtype=torch.bool)
        t2d[::2] = True
        m.load_vocab_mapping_tensors(t2d, torch.arange(cfg.draft_vocab_size) * 2 - torch.arange(cfg.draft_vocab_size))
    eagle = OnlineEagle3Model(m, length=T, attention_backend=attention_backend, lk_loss_type=lk, topk=TOPK, chain=True, conf_bins=BINS,
                              conf_thresholds=TAU).train()
    hw = torch.zeros(cfg.vocab_size, 128)       # the teacher's head reads a one-hot hidden state e_i as target token 2 i (draft index i)
    hw[torch.arange(cfg.vocab_size), torch.arange(cfg.vocab_size) // 2] = torch.where(torch.arange(cfg.vocab_size) % 2 == 0, 1.0, 0.5)
    head = TargetHead(hw.to(torch.bfloat16).to(dev))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda mod: BF16Optimizer(mod, lr=1e-2, total_steps=100, warmup_ratio=0.0), **(backend_kw or {}))
    backend.prepare_model(eagle)
    return eagle, strat, backend


def hit_sample(dev, eagle, strat):
    """W.sample with a target whose teacher token (after the strategy's left shift by one) is the unsharded draft's own step-0
    prediction at even positions and the next draft index at odd ones"""
    from specforge_amd.eagle3 import TrainBatch

    full = W.sample(dev)
    eagle.eval()
    with torch.no_grad():
        strat.forward_loss(TrainBatch(dict(full), {"target_repr": "hidden_state"}))
    eagle.train()
    pred = eagle.engine._views[(1, S)]["logits"][0].float().cpu().argmax(-1)
    tok = torch.where(torch.arange(S) % 2 == 0, pred, (pred + 1) % 128)
    target = torch.zeros(1, S, 128)
    target[0, torch.arange(1, S), tok[:-1]] = 8.0
    full["target"] = target.to(torch.bfloat16).to(dev)
    return full


def step(eagle, strat, backend, tensors):
    from specforge_amd.eagle3 import TrainBatch

    out = strat.forward_loss(TrainBatch(dict(tensors), {"target_repr": "hidden_state"}))
    backend.backward(out.loss, is_boundary=True)
    m = out.metrics
    bins, den, gate = eagle.last_conf
    st = lambda xs: torch.stack([t.float().cpu() for t in xs])
    return dict(bins=st(bins), denoms=st(den), gate=st(gate), topk=st(eagle.last_topk), chain_denoms=st(eagle.last_chain[0]),
                chain_corrects=st(eagle.last_chain[1]), acc_corrects=st(m["acc_corrects"]), acc_denoms=st(m["acc_denoms"]),
                named={k: st(m[k]) for k in ("conf_bin_counts", "conf_bin_corrects", "conf_bin_sums", "conf_denoms", "conf_gate_drafted",
                                             "conf_gate_accepted")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--emu", required=True)
    ap.add_argument("--lk", default="")
    ap.add_argument("--sample", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as dist

    from specforge_amd import _lib
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    torch.set_num_threads(1)
    os.environ["SFEMU_THREADS"] = "2"
    _lib._inject_library_for_tests(a.emu)
    dev = torch.device("cpu")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group("gloo", rank=a.rank, world_size=2)
    eagle, strat, backend = setup(dev, "usp", dict(parallel_config=ParallelConfig(world_size=2, sp_size=2, dp_size=1)), lk=a.lk or None)
    full = torch.load(a.sample)
    full.pop("attention_mask")
    res = step(eagle, strat, backend, usp_shard(full, ttt_length=T, sp_rank=a.rank, sp_size=2))
    torch.save(res, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
