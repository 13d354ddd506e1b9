"""One step of a tiny draft with the top-k hit counts on (tests/test_topk_usp.py), the same model and sample in every process: as a
module, the model / sample / step the pytest process runs unsharded; as a script, one SP rank of a two-rank world that exchanges over
gloo -- under the SIMT interpreter (``--emu LIB``, CPU tensors) or on cuda:0 (both ranks share the device, host-staged exchanges) --
and writes its counts to ``--out``."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T, S = 3, 64
TOPK = (1, 2, 4, 8)


def setup(dev, attention_backend="hip", backend_kw=None, lk=None):
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    cfg = DraftConfig(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2, vocab_size=256,
                      draft_vocab_size=128, head_dim=64, target_hidden_size=128, max_position_embeddings=128, rms_norm_eps=1e-5)
    m = LlamaForCausalLMEagle3(cfg, device=dev)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((1.0 + 0.1 * torch.randn(p.shape, generator=g) if "norm" in n else 0.05 * torch.randn(p.shape, generator=g)).to(p.device))
        t2d = torch.zeros(cfg.vocab_size, dtype=torch.bool)
        t2d[::2] = True
        m.load_vocab_mapping_tensors(t2d, torch.arange(cfg.draft_vocab_size) * 2 - torch.arange(cfg.draft_vocab_size))
    eagle = OnlineEagle3Model(m, length=T, attention_backend=attention_backend, lk_loss_type=lk, topk=TOPK).train()
    head = TargetHead((0.05 * torch.randn(cfg.vocab_size, 128, generator=torch.Generator().manual_seed(9))).to(torch.bfloat16).to(dev))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda mod: BF16Optimizer(mod, lr=1e-2, total_steps=100, warmup_ratio=0.0), **(backend_kw or {}))
    backend.prepare_model(eagle)
    return eagle, strat, backend


def sample(dev, seed=11):
    """one normalised sample: [1, S] ids / masks, [1, S, 3 * 128] hidden states, [1, S, 128] target"""
    g = torch.Generator().manual_seed(seed)
    lm = (torch.rand(1, S, generator=g) > 0.25).long()
    lm[0, -1] = 0
    return dict(input_ids=torch.randint(0, 256, (1, S), generator=g), loss_mask=lm, attention_mask=torch.ones(1, S, dtype=torch.long),
                hidden_state=torch.randn(1, S, 384, generator=g).to(torch.bfloat16).to(dev),
                target=torch.randn(1, S, 128, generator=g).to(torch.bfloat16).to(dev))


def step(eagle, strat, backend, tensors):
    from specforge_amd.eagle3 import TrainBatch

    out = strat.forward_loss(TrainBatch(dict(tensors), {"target_repr": "hidden_state"}))
    backend.backward(out.loss, is_boundary=True)
    m = out.metrics
    return dict(topk=torch.stack([t.float().cpu() for t in eagle.last_topk]), acc_corrects=torch.stack(m["acc_corrects"]).float().cpu(),
                acc_denoms=torch.stack(m["acc_denoms"]).float().cpu(),
                named={k: torch.stack(m[f"top{k}_corrects"]).float().cpu() for k in TOPK})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--emu", default="")
    ap.add_argument("--lk", default="")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as dist

    from specforge_amd import _lib
    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    if a.emu:
        torch.set_num_threads(1)
        os.environ["SFEMU_THREADS"] = "2"
        _lib._inject_library_for_tests(a.emu)
        dev = torch.device("cpu")
    else:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group("gloo", rank=a.rank, world_size=2)
    eagle, strat, backend = setup(dev, "usp", dict(parallel_config=ParallelConfig(world_size=2, sp_size=2, dp_size=1)), lk=a.lk or None)
    full = sample(dev)
    full.pop("attention_mask")
    res = step(eagle, strat, backend, usp_shard(full, ttt_length=T, sp_rank=a.rank, sp_size=2))
    if not a.emu:
        torch.cuda.synchronize()
    torch.save(res, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
