"""The draft-confidence metric keys under the REFERENCE's own trainer (build container only: needs the reference checkout; skipped
elsewhere), driven the way tests/test_chain_reference_trainer.py drives it, kernels under the SIMT interpreter:

* ``Trainer.fit()`` with ``OnlineEagle3Model(conf_bins=..., conf_thresholds=...)``: ``StepOutput.metrics`` carries the six ``conf_*`` keys
  (lists over the T steps of [NB] / 0-dim / [J] counts) and the reference's ``TrainerCore`` metric reduction (which skips list values it
  does not know) logs what it logs without them; the reference's ``Evaluator`` runs over the same strategy and returns the same eval/*
  keys and values.
* ``install(conf_bins=..., conf_thresholds=...)`` reaches the model that the algorithm's own factory builds on the ``specforge train``
  path, and ``uninstall()`` clears the options."""
import os

import pytest
import torch

from oracle import ref_harness as RH
from test_reference_trainer import _write_run_dir
from test_topk_reference_trainer import seen  # noqa: F401  (the fixture that records every StepOutput.metrics)

pytestmark = pytest.mark.skipif(not RH.available(), reason="needs the reference checkout: build container only")

NB, TAU = 8, (0.0, 0.05, 0.5)
KEYS = ("conf_bin_counts", "conf_bin_corrects", "conf_bin_sums", "conf_denoms", "conf_gate_drafted", "conf_gate_accepted")


@pytest.fixture(scope="module")
def ref(emu_lib_path):
    RH.setup()
    RH.init_single_rank(29601)
    from specforge_amd import _lib
    from specforge_amd import reference_plugin as RP

    _lib._inject_library_for_tests(emu_lib_path)
    RP.draft_class()
    yield RP
    RP.uninstall()
    _lib._inject_library_for_tests(None)


def _check_keys(metrics, T, nb, tau):
    assert sorted(k for k in metrics if k.startswith("conf")) == sorted(KEYS)
    shapes = dict(conf_bin_counts=(nb,), conf_bin_corrects=(nb,), conf_bin_sums=(nb,), conf_denoms=(), conf_gate_drafted=(len(tau),),
                  conf_gate_accepted=(len(tau),))
    for key in KEYS:
        v = metrics[key]
        assert isinstance(v, list) and len(v) == T and all(tuple(x.shape) == shapes[key] for x in v), key
    assert float(metrics["conf_denoms"][0]) == float(metrics["acc_denoms"][0])
    for i in range(T):
        cnt, hit, cs = metrics["conf_bin_counts"][i], metrics["conf_bin_corrects"][i], metrics["conf_bin_sums"][i]
        dr, acc = metrics["conf_gate_drafted"][i], metrics["conf_gate_accepted"][i]
        if nb:      # every scored row lies in one bin, every top-1 hit too; a bin's confidence sum is at most its count
            assert float(cnt.sum()) == float(metrics["acc_denoms"][i]) and float(hit.sum()) == float(metrics["acc_corrects"][i])
            assert bool((hit <= cnt).all()) and bool((cs <= cnt).all()) and bool((cs >= 0).all())
        assert float(metrics["conf_denoms"][i]) <= float(metrics["acc_denoms"][i])
        assert bool((acc <= dr).all()) and bool((dr <= metrics["conf_denoms"][i]).all())
        assert bool((dr[1:] <= dr[:-1]).all()) and bool((acc[1:] <= acc[:-1]).all())         # ascending thresholds
        if i:
            assert bool((acc <= metrics["conf_gate_accepted"][i - 1]).all())
    if tau and tau[0] == 0.0:
        assert float(metrics["conf_gate_drafted"][0][0]) == float(metrics["conf_denoms"][0])
        assert float(metrics["conf_gate_accepted"][0][0]) == float(metrics["acc_corrects"][0])


def test_reference_trainer_and_evaluator_run_with_the_conf_keys(ref, seen, golden_dir, tmp_path):  # noqa: F811
    from specforge.launch import build_offline_runtime
    from specforge.modeling.auto import AutoDraftModel, AutoDraftModelConfig
    from specforge.modeling.target.target_head import TargetHead
    from specforge_amd.eagle3 import ConfidenceAccumulator, OnlineEagle3Model
    from specforge_amd.training import BF16Optimizer

    blob = torch.load(os.path.join(golden_dir, "loss_curve_tiny.pt"), weights_only=False)
    c = blob["cfg"]
    dj, feat, td, vp = _write_run_dir(str(tmp_path), blob, ref.DRAFT_ARCHITECTURE)
    logged = {}
    for on in (False, True):
        ref.install()
        try:
            draft = AutoDraftModel.from_config(AutoDraftModelConfig.from_file(dj), attention_backend="sdpa", torch_dtype=torch.bfloat16)
            draft.load_state_dict(blob["init_state"], strict=True)
            draft.freeze_embedding()
            head = TargetHead.from_pretrained(td, lm_head_key="lm_head.weight")
            model = OnlineEagle3Model(draft_model=draft, length=c["ttt"], attention_backend="sdpa", conf_bins=NB if on else 0,
                                      conf_thresholds=TAU if on else ())
            log = logged[on] = []
            del seen[:]
            trainer = build_offline_runtime(
                algorithm=ref.registry().resolve(ref.ALGORITHM_NAME), hidden_states_path=feat, eval_hidden_states_path=feat, eval_interval=1000,
                draft_model=model, target_head=head,
                optimizer_factory=lambda m: BF16Optimizer(m, lr=c["lr"], max_grad_norm=c["max_grad_norm"], warmup_ratio=c["warmup_ratio"],
                                                          total_steps=c["steps"]),
                run_id=f"conf-{int(on)}", output_dir=os.path.join(str(tmp_path), f"out{int(on)}"), ttt_length=c["ttt"], max_len=c["max_len"],
                batch_size=c["batch_size"], max_steps=2, total_steps=c["steps"], num_epochs=1, seed=c["seed"],
                logger=lambda m, s: log.append((s, dict(m))), log_interval=1)
            assert trainer.fit() == 2
            assert len(seen) == 2
            for m in seen:
                if on:
                    _check_keys(m, c["ttt"], NB, TAU)
                else:
                    assert not any(k.startswith("conf") for k in m)
            n_train = len(seen)
            ev = trainer._controller.evaluate_configured()        # the reference's Evaluator.run over the same strategy
            assert ev and "eval/simulated_acc_len" in ev and len(seen) > n_train
            if on:
                acc = ConfidenceAccumulator(NB, TAU)
                for m in seen[n_train:]:
                    _check_keys(m, c["ttt"], NB, TAU)
                    acc.update(m)
                s = acc.summary()
                print("eval", {k: v for k, v in ev.items() if "acc" in k}, "conf", {k: v for k, v in s.items() if "reliability" not in k})
                # depth 0's hit rate is the Evaluator's own position-0 accuracy (both: sums, then ratios) ...
                assert abs(s["conf_acc_0"] - ev["eval/per_position_acc"][0]) <= 1e-12
                # ... a calibration error is a mean of |accuracy - confidence|, and a gated chain accepts at most what it drafts
                assert all(0.0 <= s[f"conf_ece_{i}"] <= 1.0 and 0.0 < s[f"conf_mean_{i}"] <= 1.0 for i in range(c["ttt"]))
                names = [ConfidenceAccumulator.tau_name(t) for t in TAU]
                assert all(0.0 <= s[f"gated_acc_len_tau{n}"] <= s[f"gated_draft_len_tau{n}"] <= c["ttt"] for n in names)
                assert s[f"gated_draft_len_tau{names[0]}"] >= 1.0 or s["conf_acc_0"] == 0.0
            logged[on].append(("eval", ev))
        finally:
            ref.uninstall()
    # what the reference's reducer and evaluator report does not depend on the extra keys
    plain, with_conf = logged[False], logged[True]
    assert [s for s, _ in plain] == [s for s, _ in with_conf]
    for (s, a), (_, b) in zip(plain, with_conf):
        assert set(a) == set(b), (s, set(a) ^ set(b))
        assert {"loss", "acc_0", "ploss_0"} <= set(a) or s == "eval"
        for k in a:
            if not k.startswith("perf/"):        # (wall-clock rates)
                assert a[k] == b[k], (s, k, a[k], b[k])


def test_install_conf_reaches_the_factory_built_model(ref, seen, golden_dir, tmp_path, monkeypatch):  # noqa: F811
    """``specforge train``'s path (load_config -> resolve_run -> cli._train) with ``install(override=True, conf_bins=..., conf_thresholds=...)``:
    the run YAML has no key for the setting and needs none"""
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
               run_id="hipconf", output_dir=os.path.join(work, "out"),
               deployment=dict(mode="local_colocated", trainer=dict(nnodes=1, nproc_per_node=1)))
    yp = os.path.join(work, "run.yaml")
    yaml.safe_dump(run, open(yp, "w"))
    ref.install(override=True, conf_bins=4)
    ref.install(override=True, conf_thresholds=(0.0, 0.25))        # None leaves the other setting as it is
    try:
        assert ref._options == {"conf_bins": 4, "conf_thresholds": (0.0, 0.25)}
        ref.install(override=True)
        assert ref._options == {"conf_bins": 4, "conf_thresholds": (0.0, 0.25)}
        with pytest.raises(ValueError, match="conf_thresholds"):
            ref.install(conf_thresholds=(0.5, 0.25))
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
        RH.init_single_rank(29603)
    assert ref._options == {}
    assert len(seen) == 1
    _check_keys(seen[0], 3, 4, (0.0, 0.25))


def test_command_line_options_reach_install_and_the_spawned_workers(ref, golden_dir, tmp_path, capsys, monkeypatch):
    """``--conf-bins`` / ``--conf-thresholds`` in front of or behind ``train``: ``install()`` gets them and a two-process launch plan hands
    them to its workers on their command line"""
    import yaml

    blob = torch.load(os.path.join(golden_dir, "loss_curve_tiny.pt"), weights_only=False)
    work = str(tmp_path)
    dj, feat, td, vp = _write_run_dir(work, blob, "LlamaForCausalLMEagle3")
    run = dict(model=dict(target_model_path=td, draft_model_config=dj, embedding_key="model.embed_tokens.weight",
                          vocab_mapping_path=vp, torch_dtype="bfloat16"),
               data=dict(hidden_states_path=feat, max_length=24),
               training=dict(strategy="eagle3", num_epochs=1, batch_size=2, learning_rate=1e-3, max_grad_norm=0.5, ttt_length=3,
                             attention_backend="sdpa", save_interval=0, log_interval=1, dist_timeout=5, seed=0, max_steps=1),
               run_id="hipconfplan", output_dir=os.path.join(work, "out"),
               deployment=dict(mode="local_colocated", trainer=dict(nnodes=1, nproc_per_node=2)))
    yp = os.path.join(work, "run.yaml")
    yaml.safe_dump(run, open(yp, "w"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):     # (the harness's single-rank group: this process is the launcher here)
        monkeypatch.delenv(k, raising=False)
    try:
        for argv in (["--conf-bins", "4", "--conf-thresholds", "0.25,0.5", "train", "-c", yp, "--plan"],
                     ["train", "-c", yp, "--plan", "--conf-bins", "4", "--conf-thresholds", "0.25,0.5"]):
            ref.uninstall()
            assert ref.main(argv, worker_prefix=("WORKER",)) == 0
            assert ref._options["conf_bins"] == 4 and ref._options["conf_thresholds"] == (0.25, 0.5)
            import json

            argv_out = json.loads(capsys.readouterr().out)["commands"][0]["argv"]
            at = argv_out.index("WORKER")
            assert argv_out[at:at + 6] == ["WORKER", "--conf-bins", "4", "--conf-thresholds", "0.25,0.5", "train"], argv_out
    finally:
        ref.uninstall()
