"""TEST HARNESS process entry for the USP runs of tests/test_plugin_usp.py.

``python tests/_plugin_usp_worker.py train -c run.yaml`` = ``python -m specforge_amd.reference_plugin train -c run.yaml`` (``specforge
train`` on the HIP path) with the reference checkout present, like tests/_plugin_worker.py, with two differences:

* ``yunchang.globals.set_seq_parallel_pg`` builds REAL Ulysses / ring groups (yunchang's layout with ``use_ulysses_low=True``: the
  Ulysses peers of an SP group are consecutive ranks, the ring peers ``sp_ulysses_size`` apart), so the reference's
  ``init_distributed`` hands the backend, the USP transform and the collator working groups.  (oracle/ref_harness.py stubs them as
  None: enough for runs without sequence parallelism.)
* with ``SF_TEST_PROBE_DIR`` set, every trainer rank records ``probe_rank{r}.pt``: each micro-step's loss and metrics, each optimizer
  step's grad norm and learning rate, the flat gradient (averaged as the optimizer applies it) and weights after the first step, the
  final weights, and -- rank 0 -- the initial draft state, the teacher head and the optimizer's settings (what the Python-API replay
  of the same run starts from).

``run_api(rank, world, ...)`` is that replay: the same files, initial weights and topology through the Python API
(``HipDPTrainingBackend(ParallelConfig(sp_size=, sp_ring_size=))``, ``HiddenStateIngest(sp_rank=, sp_size=)``, ``TrainerCore``).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _install_yunchang_groups():
    import types

    import torch.distributed as dist

    yc = types.ModuleType("yunchang")
    g = types.ModuleType("yunchang.globals")

    class PROCESS_GROUP:
        ULYSSES_PG = None
        RING_PG = None

    def set_seq_parallel_pg(sp_ulysses_degree, sp_ring_degree, rank, world_size, use_ulysses_low=True):
        assert use_ulysses_low
        u, r = sp_ulysses_degree, sp_ring_degree
        sp = u * r
        for base in range(0, world_size, sp):
            for t in range(r):
                ranks = [base + t * u + j for j in range(u)]
                grp = dist.new_group(ranks)
                if rank in ranks:
                    PROCESS_GROUP.ULYSSES_PG = grp
            for j in range(u):
                ranks = [base + t * u + j for t in range(r)]
                grp = dist.new_group(ranks)
                if rank in ranks:
                    PROCESS_GROUP.RING_PG = grp

    g.PROCESS_GROUP = PROCESS_GROUP
    g.set_seq_parallel_pg = set_seq_parallel_pg
    yc.globals = g
    yc.set_seq_parallel_pg = set_seq_parallel_pg
    sys.modules["yunchang"] = yc
    sys.modules["yunchang.globals"] = g


def _probe_hooks(probe_dir, rank):
    """wraps the strategy's forward and the backend's step to record what the run computed"""
    import torch

    from specforge_amd import eagle3 as E
    from specforge_amd import training as T

    rec = dict(micro=[], steps=[], rank=rank)
    fwd0, step0, prep0 = E.Eagle3TrainStrategy.forward_loss, T.HipDPTrainingBackend.step, T.HipDPTrainingBackend.prepare_model

    def forward_loss(self, batch, ctx=None):
        out = fwd0(self, batch, ctx)
        m = out.metrics
        rec["micro"].append(dict(loss=out.loss.detach().float().cpu().clone(), plosses=torch.stack(m["plosses"]).float().cpu(),
                                 acces=torch.stack(m["acces"]).float().cpu()))
        rec.setdefault("strategy", self)
        return out

    def step(self):
        eng = self.module.engine
        if not rec["steps"]:
            self.synchronize_gradients()
            rec["grad1"] = (eng.flat.grad.float() / self.world).cpu().clone()
        gn = step0(self)
        rec["steps"].append(dict(grad_norm=float(gn), lr=float(self.optimizer.get_learning_rate())))
        if len(rec["steps"]) == 1:
            rec["params1"] = eng.flat.data.cpu().clone()
        rec["backend"] = self
        return gn

    def prepare_model(self, model, **kw):
        if rank == 0 and "init_state" not in rec:
            rec["init_state"] = {k: v.detach().cpu().clone() for k, v in model.draft_model.state_dict().items()}
        out = prep0(self, model, **kw)
        rec["groups"] = {k: (dist_ranks(getattr(self, k)) if getattr(self, k) is not None else None)
                         for k in ("sp_group", "sp_ulysses_group", "sp_ring_group", "draft_dp_group")}
        return out

    E.Eagle3TrainStrategy.forward_loss = forward_loss
    T.HipDPTrainingBackend.step = step
    T.HipDPTrainingBackend.prepare_model = prepare_model

    def dump():
        be = rec.pop("backend", None)
        strat = rec.pop("strategy", None)
        out = dict(rec)
        if be is not None:
            out["final"] = be.module.engine.flat.data.cpu().clone()
            o = be.optimizer
            out["world"], out["sp_size"] = be.world, be.sp_size
            out["optimizer"] = dict(lr=o.scheduler.base_lr, total_steps=o.scheduler.total_steps, warmup_steps=o.scheduler.warmup_steps,
                                    kind=o.scheduler.kind, max_grad_norm=o.max_grad_norm, weight_decay=o.weight_decay,
                                    betas=tuple(o.betas), eps=o.eps, last_epoch=o.scheduler.last_epoch)
        if strat is not None and rank == 0:
            out["head_w"] = strat.target_head.fc.weight.detach().cpu().clone()
        torch.save(out, os.path.join(probe_dir, f"probe_rank{rank}.pt"))

    return dump


def dist_ranks(group):
    import torch.distributed as dist

    return tuple(dist.get_process_group_ranks(group))


def main() -> int:
    _install_yunchang_groups()
    from oracle import ref_harness as RH

    RH.setup()
    from specforge_amd import _lib, build
    from specforge_amd import reference_plugin as RP

    _lib._inject_library_for_tests(build.build_emu())
    probe_dir = os.environ.get("SF_TEST_PROBE_DIR")
    dump = _probe_hooks(probe_dir, int(os.environ.get("RANK", "0"))) if probe_dir else None
    rc = RP.main(sys.argv[1:], worker_prefix=(sys.executable, os.path.abspath(__file__)))
    if dump is not None and "RANK" in os.environ:
        dump()
    return rc


# ------------------------------------------------------------------------------------------------------------- the Python-API replay
def run_api(rank, world, port, emu_path, feat_files, draft_json, probe0, out_dir, sp, ring, acc, steps, seed, max_len, ttt):
    """one rank of the Python-API run: world = draft_dp x sp (sp = 1: one unsharded process)"""
    import json

    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from specforge_amd import _lib
    from specforge_amd.eagle3 import Eagle3TrainStrategy, OnlineEagle3Model, TargetHead
    from specforge_amd.ingest import HiddenStateIngest
    from specforge_amd.model import DraftConfig, LlamaForCausalLMEagle3
    from specforge_amd.training import BF16Optimizer, HipDPTrainingBackend, ParallelConfig, TrainerCore, _WarmupSchedule

    _lib._inject_library_for_tests(emu_path)
    try:
        p0 = torch.load(probe0, weights_only=False)
        cfg = DraftConfig.from_hf(json.load(open(draft_json)))
        model = LlamaForCausalLMEagle3(cfg).to(torch.bfloat16)
        model.load_state_dict(p0["init_state"], strict=True)
        model.embed_tokens.weight.requires_grad_(False)
        eagle = OnlineEagle3Model(model, length=ttt, attention_backend="usp" if sp > 1 else "sdpa").train()
        strat = Eagle3TrainStrategy(eagle, target_head=TargetHead(p0["head_w"]))
        o = p0["optimizer"]

        def make_opt(m):
            opt = BF16Optimizer(m, lr=o["lr"], max_grad_norm=o["max_grad_norm"], weight_decay=o["weight_decay"], betas=o["betas"],
                                eps=o["eps"], lr_scheduler=o["kind"], total_steps=o["total_steps"], warmup_ratio=0.0)
            opt.scheduler = _WarmupSchedule(o["kind"], o["lr"], o["total_steps"], o["warmup_steps"])
            return opt

        pc = ParallelConfig(world_size=world, sp_size=sp, sp_ring_size=ring, dp_size=world // sp) if sp > 1 else None
        backend = HipDPTrainingBackend(pc, optimizer_factory=make_opt)
        backend.prepare_model(eagle, optimizer_target=model)
        dump = _probe_hooks(out_dir, rank)
        # (the hooks were installed after prepare_model: record the starting point the same way the launch did)
        core = TrainerCore(strat, backend, accumulation_steps=acc)
        ing = HiddenStateIngest(feat_files, batch_size=1, max_len=max_len, device="cpu", dp_rank=rank // sp, dp_size=world // sp,
                                seed=seed, shuffle=True, sp_rank=rank % sp, sp_size=sp, ttt_length=ttt)
        n = 0
        for b in ing.epoch(0):
            b.metadata["target_repr"] = "hidden_state"
            r = core.train_step(b)
            n += r.stepped
            if n == steps:
                break
        dump()
    finally:
        _lib._inject_library_for_tests(None)
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    raise SystemExit(main())
