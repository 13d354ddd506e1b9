"""The chain metric keys under the REFERENCE's own trainer (build container only: needs the reference checkout; skipped elsewhere), driven
the way tests/test_topk_reference_trainer.py drives it, kernels under the SIMT interpreter:

* ``Trainer.fit()`` with ``OnlineEagle3Model(topk=..., chain=True)``: ``StepOutput.metrics`` carries ``chain_denoms`` and
  ``chain_top{k}_corrects`` (T 0-dim counts each) and the reference's ``TrainerCore`` metric reduction (which skips list values it does
  not know) logs what it logs without them; the reference's ``Evaluator`` runs over the same strategy and returns the same eval/* keys
  and values.
* ``install(chain=True, topk=...)`` reaches the model that the algorithm's own factory builds on the ``specforge train`` path, and
  ``uninstall()`` clears the option."""
import os

import pytest
import torch

from oracle import ref_harness as RH
from test_reference_trainer import _write_run_dir
from test_topk_reference_trainer import seen  # noqa: F401  (the fixture that records every StepOutput.metrics)

pytestmark = pytest.mark.skipif(not RH.available(), reason="needs the reference checkout: build container only")

TOPK = (1, 2, 4)


@pytest.fixture(scope="module")
def ref(emu_lib_path):
    RH.setup()
    RH.init_single_rank(29597)
    from specforge_amd import _lib
    from specforge_amd import reference_plugin as RP

    _lib._inject_library_for_tests(emu_lib_path)
    RP.draft_class()
    yield RP
    RP.uninstall()
    _lib._inject_library_for_tests(None)


def _check_keys(metrics, T, topk):
    ks = sorted({1, *topk})
    assert sorted(k for k in metrics if k.startswith("chain")) == sorted(["chain_denoms"] + [f"chain_top{k}_corrects" for k in ks])
    for key in ["chain_denoms"] + [f"chain_top{k}_corrects" for k in ks]:
        v = metrics[key]
        assert isinstance(v, list) and len(v) == T and all(x.dim() == 0 for x in v)
    assert float(metrics["chain_top1_corrects"][0]) == float(metrics["acc_corrects"][0])
    assert float(metrics["chain_denoms"][0]) == float(metrics["acc_denoms"][0])
    for i in range(T):
        assert float(metrics["chain_denoms"][i]) <= float(metrics["acc_denoms"][i])
        for a, b in zip(ks, ks[1:]):
            assert float(metrics[f"chain_top{a}_corrects"][i]) <= float(metrics[f"chain_top{b}_corrects"][i])
        assert float(metrics[f"chain_top{ks[-1]}_corrects"][i]) <= float(metrics["chain_denoms"][i])
        for k in topk:      # a joint count never exceeds the marginal one
            assert float(metrics[f"chain_top{k}_corrects"][i]) <= float(metrics[f"top{k}_corrects"][i])
        if i:
            assert float(metrics["chain_top1_corrects"][i]) <= float(metrics["chain_top1_corrects"][i - 1])


def test_reference_trainer_and_evaluator_run_with_the_chain_keys(ref, seen, golden_dir, tmp_path):  # noqa: F811
    from specforge.launch import build_offline_runtime
    from specforge.modeling.auto import AutoDraftModel, AutoDraftModelConfig
    from specforge.modeling.target.target_head import TargetHead
    from specforge_amd.eagle3 import ChainAccumulator, OnlineEagle3Model
    from specforge_amd.training import BF16Optimizer

    blob = torch.load(os.path.join(golden_dir, "loss_curve_tiny.pt"), weights_only=False)
    c = blob["cfg"]
    dj, feat, td, vp = _write_run_dir(str(tmp_path), blob, ref.DRAFT_ARCHITECTURE)
    logged = {}
    for chain in (False, True):
        ref.install()
        try:
            draft = AutoDraftModel.from_config(AutoDraftModelConfig.from_file(dj), attention_backend="sdpa", torch_dtype=torch.bfloat16)
            draft.load_state_dict(blob["init_state"], strict=True)
            draft.freeze_embedding()
            head = TargetHead.from_pretrained(td, lm_head_key="lm_head.weight")
            model = OnlineEagle3Model(draft_model=draft, length=c["ttt"], attention_backend="sdpa", topk=TOPK, chain=chain)
            log = logged[chain] = []
            del seen[:]
            trainer = build_offline_runtime(
                algorithm=ref.registry().resolve(ref.ALGORITHM_NAME), hidden_states_path=feat, eval_hidden_states_path=feat, eval_interval=1000,
                draft_model=model, target_head=head,
                optimizer_factory=lambda m: BF16Optimizer(m, lr=c["lr"], max_grad_norm=c["max_grad_norm"], warmup_ratio=c["warmup_ratio"],
                                                          total_steps=c["steps"]),
                run_id=f"chain-{int(chain)}", output_dir=os.path.join(str(tmp_path), f"out{int(chain)}"), ttt_length=c["ttt"], max_len=c["max_len"],
                batch_size=c["batch_size"], max_steps=2, total_steps=c["steps"], num_epochs=1, seed=c["seed"],
                logger=lambda m, s: log.append((s, dict(m))), log_interval=1)
            assert trainer.fit() == 2
            assert len(seen) == 2
            for m in seen:
                if chain:
                    _check_keys(m, c["ttt"], TOPK)
                else:
                    assert not any(k.startswith("chain") for k in m)
            n_train = len(seen)
            ev = trainer._controller.evaluate_configured()        # the reference's Evaluator.run over the same strategy
            assert ev and "eval/simulated_acc_len" in ev and len(seen) > n_train
            if chain:
                acc = ChainAccumulator(TOPK)
                for m in seen[n_train:]:
                    _check_keys(m, c["ttt"], TOPK)
                    acc.update(m)
                s = acc.summary()
                print("eval", {k: v for k, v in ev.items() if "acc" in k}, "chain", s)
                # depth 0 of the chain is the Evaluator's own position-0 accuracy (both: sums, then ratios) ...
                assert abs(s["chain_top1_acc_0"] - ev["eval/per_position_acc"][0]) <= 1e-12
                # ... and every chain rate lies in [0, 1], so the accepted length is bounded by the number of depths
                assert all(0.0 <= s[f"chain_top{k}_acc_{i}"] <= 1.0 for k in TOPK for i in range(c["ttt"]))
                assert 0.0 <= s["chain_acc_len_top1"] <= s["chain_acc_len_top2"] <= s["chain_acc_len_top4"] <= c["ttt"]
            logged[chain].append(("eval", ev))
        finally:
            ref.uninstall()
    # what the reference's reducer and evaluator report does not depend on the extra keys
    plain, with_chain = logged[False], logged[True]
    assert [s for s, _ in plain] == [s for s, _ in with_chain]
    for (s, a), (_, b) in zip(plain, with_chain):
        assert set(a) == set(b), (s, set(a) ^ set(b))
        assert {"loss", "acc_0", "ploss_0"} <= set(a) or s == "eval"
        for k in a:
            if not k.startswith("perf/"):        # (wall-clock rates)
                assert a[k] == b[k], (s, k, a[k], b[k])


def test_install_chain_reaches_the_factory_built_model(ref, seen, golden_dir, tmp_path, monkeypatch):  # noqa: F811
    """``specforge train``'s path (load_config -> resolve_run -> cli._train) with ``install(override=True, chain=True, topk=...)``: the
    run YAML has no key for the setting and needs none"""
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
               run_id="hipchain", output_dir=os.path.join(work, "out"),
               deployment=dict(mode="local_colocated", trainer=dict(nnodes=1, nproc_per_node=1)))
    yp = os.path.join(work, "run.yaml")
    yaml.safe_dump(run, open(yp, "w"))
    ref.install(override=True, chain=True, topk=(2, 4))
    try:
        assert ref._options == {"chain": True, "topk": (2, 4)}
        ref.install(override=True)                                  # None leaves both settings as they are
        assert ref._options == {"chain": True, "topk": (2, 4)}
        resolved = resolve_run(load_config(yp), registry=ref.registry(override=True))
        import torch.distributed as dist

        if dist.is_initialized():          # cli._train owns init/destroy of the process group
            dist.destroy_process_group()
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            os.environ.pop(k, None)
        # cli._train exports the run's FSDP sharding strategy; modules that run after this one (the pure reference runs of
        # tests/test_reference_trainer.py) need the harness's setting back
        monkeypatch.setenv("FSDP_SHARDING", os.environ.get("FSDP_SHARDING", "NO_SHARD"))
        assert cli._train(resolved) == 1
    finally:
        ref.uninstall()
        RH.init_single_rank(29599)
    assert ref._options == {}
    assert len(seen) == 1
    _check_keys(seen[0], 3, (2, 4))
    ref.install(chain=False)
    assert ref._options == {"chain": False}
    ref.uninstall()
    assert ref._options == {}
