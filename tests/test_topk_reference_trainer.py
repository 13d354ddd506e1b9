"""The top-k metric keys under the REFERENCE's own trainer (build container only: needs the reference checkout; skipped elsewhere), driven
the way tests/test_reference_trainer.py drives it, kernels under the SIMT interpreter:

* ``Trainer.fit()`` with ``OnlineEagle3Model(topk=...)``: ``StepOutput.metrics`` carries ``top{k}_corrects`` (T 0-dim counts each) and
  the reference's ``TrainerCore`` metric reduction (``_reduce_eagle3_metrics`` + the scalar pass, which skips list values) logs what it
  logs without them; the reference's ``Evaluator`` runs over the same strategy and returns the same eval/* keys.
* ``install(topk=...)`` reaches the model that the algorithm's own factory builds on the ``specforge train`` path."""
import os

import pytest
import torch

from oracle import ref_harness as RH
from test_reference_trainer import _write_run_dir

pytestmark = pytest.mark.skipif(not RH.available(), reason="needs the reference checkout (/root/reference): build container only")

TOPK = (1, 2, 4)


@pytest.fixture(scope="module")
def ref(emu_lib_path):
    RH.setup()
    RH.init_single_rank(29593)
    from specforge_amd import _lib
    from specforge_amd import reference_plugin as RP

    _lib._inject_library_for_tests(emu_lib_path)
    RP.draft_class()
    yield RP
    RP.uninstall()
    _lib._inject_library_for_tests(None)


@pytest.fixture
def seen(monkeypatch):
    """every StepOutput.metrics the HIP strategy hands to the reference's trainer / evaluator"""
    from specforge_amd.eagle3 import Eagle3TrainStrategy

    outs = []
    orig = Eagle3TrainStrategy.forward_loss

    def recording(self, batch, ctx=None):
        out = orig(self, batch, ctx)
        outs.append(out.metrics)
        return out

    monkeypatch.setattr(Eagle3TrainStrategy, "forward_loss", recording)
    return outs


def _check_keys(metrics, T, topk):
    for k in topk:
        v = metrics[f"top{k}_corrects"]
        assert isinstance(v, list) and len(v) == T and all(x.dim() == 0 for x in v)
    assert [float(x) for x in metrics["top1_corrects"]] == [float(x) for x in metrics["acc_corrects"]]
    for a, b in zip(topk, topk[1:]):
        assert all(float(x) <= float(y) for x, y in zip(metrics[f"top{a}_corrects"], metrics[f"top{b}_corrects"]))


def test_reference_trainer_and_evaluator_run_with_the_topk_keys(ref, seen, golden_dir, tmp_path):
    from specforge.launch import build_offline_runtime
    from specforge.modeling.auto import AutoDraftModel, AutoDraftModelConfig
    from specforge.modeling.target.target_head import TargetHead
    from specforge_amd.eagle3 import OnlineEagle3Model, TopKAccumulator
    from specforge_amd.training import BF16Optimizer

    blob = torch.load(os.path.join(golden_dir, "loss_curve_tiny.pt"), weights_only=False)
    c = blob["cfg"]
    dj, feat, td, vp = _write_run_dir(str(tmp_path), blob, ref.DRAFT_ARCHITECTURE)
    logged = {}
    for topk in ((), TOPK):
        ref.install()
        try:
            draft = AutoDraftModel.from_config(AutoDraftModelConfig.from_file(dj), attention_backend="sdpa", torch_dtype=torch.bfloat16)
            draft.load_state_dict(blob["init_state"], strict=True)
            draft.freeze_embedding()
            head = TargetHead.from_pretrained(td, lm_head_key="lm_head.weight")
            model = OnlineEagle3Model(draft_model=draft, length=c["ttt"], attention_backend="sdpa", topk=topk)
            log = logged[topk] = []
            del seen[:]
            trainer = build_offline_runtime(
                algorithm=ref.registry().resolve(ref.ALGORITHM_NAME), hidden_states_path=feat, eval_hidden_states_path=feat, eval_interval=1000,
                draft_model=model, target_head=head,
                optimizer_factory=lambda m: BF16Optimizer(m, lr=c["lr"], max_grad_norm=c["max_grad_norm"], warmup_ratio=c["warmup_ratio"],
                                                          total_steps=c["steps"]),
                run_id=f"topk-{len(topk)}", output_dir=os.path.join(str(tmp_path), f"out{len(topk)}"), ttt_length=c["ttt"], max_len=c["max_len"],
                batch_size=c["batch_size"], max_steps=2, total_steps=c["steps"], num_epochs=1, seed=c["seed"],
                logger=lambda m, s: log.append((s, dict(m))), log_interval=1)
            assert trainer.fit() == 2
            assert len(seen) == 2
            for m in seen:
                if topk:
                    _check_keys(m, c["ttt"], topk)
                else:
                    assert not any(k.startswith("top") for k in m)
            n_train = len(seen)
            ev = trainer._controller.evaluate_configured()        # the reference's Evaluator.run over the same strategy
            assert ev and "eval/simulated_acc_len" in ev and len(seen) > n_train
            if topk:
                acc = TopKAccumulator(topk)
                for m in seen[n_train:]:
                    _check_keys(m, c["ttt"], topk)
                    acc.update(m)
                s = acc.summary()
                # top-1 through the accumulator == the Evaluator's own per-position accuracy and simulated length (both: sums, then ratios)
                for i, a in enumerate(ev["eval/per_position_acc"]):
                    assert abs(s[f"top1_acc_{i}"] - a) <= 1e-12
                assert abs(s["simulated_acc_len_top1"] - ev["eval/simulated_acc_len"]) <= 1e-12
            logged[topk].append(("eval", ev))
        finally:
            ref.uninstall()
    # what the reference's reducer logged does not depend on the extra keys
    plain, with_topk = logged[()], logged[TOPK]
    assert [s for s, _ in plain] == [s for s, _ in with_topk]
    for (s, a), (_, b) in zip(plain, with_topk):
        assert set(a) == set(b), (s, set(a) ^ set(b))
        assert {"loss", "acc_0", "ploss_0"} <= set(a) or s == "eval"
        for k in a:
            if not k.startswith("perf/"):        # (wall-clock rates)
                assert a[k] == b[k], (s, k, a[k], b[k])


def test_install_topk_reaches_the_factory_built_model(ref, seen, golden_dir, tmp_path):
    """``specforge train``'s path (load_config -> resolve_run -> cli._train) with ``install(override=True, topk=...)``: the run YAML has
    no key for the setting and needs none"""
    import yaml

    from specforge import cli
    from specforge.application.composition import resolve_run
    from specforge.config import load_config

    blob = torch.load(os.path.join(golden_dir, "loss_curve_tiny.pt"), weights_only=False)
    work = str(tmp_path)
    dj, feat, td, vp = _write_run_dir(work, blob, "LlamaForCausalLMEagle3")
    run = dict(model=dict(target_model_path=td, draft_model_config=dj, embedding_key="model.embed_tokens.weight",
                          vocab_mapping_path=vp, torch_dtype="bfloat16"),
               data=dict(hidden_states_path=feat, max_length=24),
               training=dict(strategy="eagle3", num_epochs=1, batch_size=2, learning_rate=1e-3, max_grad_norm=0.5, ttt_length=3,
                             attention_backend="sdpa", save_interval=0, log_interval=1, dist_timeout=5, seed=0, max_steps=1),
               run_id="hiptopk", output_dir=os.path.join(work, "out"),
               deployment=dict(mode="local_colocated", trainer=dict(nnodes=1, nproc_per_node=1)))
    yp = os.path.join(work, "run.yaml")
    yaml.safe_dump(run, open(yp, "w"))
    ref.install(override=True, topk=(1, 2))
    try:
        assert ref._options["topk"] == (1, 2)
        resolved = resolve_run(load_config(yp), registry=ref.registry(override=True))
        import torch.distributed as dist

        if dist.is_initialized():          # cli._train owns init/destroy of the process group
            dist.destroy_process_group()
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            os.environ.pop(k, None)
        assert cli._train(resolved) == 1
    finally:
        ref.uninstall()
        RH.init_single_rank(29595)
    assert ref._options == {}
    assert len(seen) == 1
    _check_keys(seen[0], 3, (1, 2))
    with pytest.raises(ValueError, match="topk"):
        ref.install(topk=(2, 1))
    ref.uninstall()
