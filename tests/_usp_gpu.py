"""GPU half of the USP tests (tests/test_usp_gpu.py): one training step of a real-dimension draft, the same model / data in every
process (device generators with fixed seeds).  Run as a script it is one SP rank of a world that exchanges over gloo (both ranks
on cuda:0, host-staged) or RCCL (rank r on cuda:r) and writes its results to ``--out``."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T = 7
CFG1 = dict(hidden_size=896, intermediate_size=4864, num_attention_heads=14, num_key_value_heads=2, vocab_size=151936,
            draft_vocab_size=16000, head_dim=64, target_hidden_size=896, max_position_embeddings=32768, rms_norm_eps=1e-6,
            rope_theta=1000000.0)


def dims(name):
    from bench import LLAMA3_8B

    return {"cfg1": CFG1, "llama3-8b": LLAMA3_8B}[name]


def setup(name, S, dev, attention_backend="hip", backend_kw=None):
    from bench import make_batch, make_loss_mask
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend

    cfg = dict(dims(name))
    cfg["max_position_embeddings"] = max(cfg["max_position_embeddings"], S + T)
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    model = LlamaForCausalLMEagle3(DraftConfig(**cfg), device=dev)
    t2d = torch.zeros(cfg["vocab_size"], dtype=torch.bool)
    ids = torch.randperm(cfg["vocab_size"], generator=torch.Generator().manual_seed(0))[:cfg["draft_vocab_size"]].sort().values
    t2d[ids] = True
    model.load_vocab_mapping_tensors(t2d, ids - torch.arange(cfg["draft_vocab_size"]))
    eagle = OnlineEagle3Model(model, length=T, attention_backend=attention_backend).train()
    g = torch.Generator(device=dev).manual_seed(3)
    head = TargetHead((torch.randn(cfg["vocab_size"], cfg["target_hidden_size"], device=dev, generator=g) * 0.02).to(torch.bfloat16))
    strat = Eagle3TrainStrategy(eagle, target_head=head)
    backend = HipDPTrainingBackend(optimizer_factory=lambda m: BF16Optimizer(m, lr=1e-4, total_steps=100, warmup_ratio=0.0),
                                   **(backend_kw or {}))
    backend.prepare_model(eagle)
    batch = make_batch(cfg, 1, S, dev, seed=1, loss_mask=make_loss_mask(1, S, 0.5, seed=5))
    batch["loss_mask"][0, -1] = 0                       # a normalised sample (ingest.normalize_offline_sample)
    return eagle, strat, backend, batch


def step(eagle, strat, backend, tensors):
    from specforge_amd.eagle3 import TrainBatch

    out = strat.forward_loss(TrainBatch(dict(tensors), {"target_repr": "hidden_state"}))
    backend.backward(out.loss, is_boundary=True)
    backend.synchronize_gradients()
    g = eagle.engine.flat.grad.float().cpu()
    backend.step()
    torch.cuda.synchronize()
    m = out.metrics
    return dict(plosses=torch.stack(m["plosses"]).float().cpu(), acces=torch.stack(m["acces"]).float().cpu(), grad=g,
                params=eagle.engine.flat.data.cpu())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--config", default="cfg1")
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as dist

    from specforge_amd.ingest import usp_shard
    from specforge_amd.training import ParallelConfig

    dev = torch.device("cuda", a.rank if a.backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    dist.init_process_group(a.backend, rank=a.rank, world_size=a.world)
    eagle, strat, backend, batch = setup(a.config, a.seq, dev, "usp",
                                         dict(parallel_config=ParallelConfig(world_size=a.world, sp_size=a.world, dp_size=1)))
    res = step(eagle, strat, backend, usp_shard(batch, ttt_length=T, sp_rank=a.rank, sp_size=a.world))
    if a.rank != 0:          # (every rank holds the same reduced gradient and weights: rank 0 writes them)
        res = dict(plosses=res["plosses"], acces=res["acces"])
    torch.save(res, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
