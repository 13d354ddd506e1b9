"""``attention_backend: usp`` through ``specforge train`` on the HIP path (needs the reference checkout; skipped without it).

* the reference schema + ``check_training_topology`` accept offline USP (Ulysses, ring, Ulysses x ring) and keep every refusal;
* the plugin loader's per-rank USP batches are the reference's own ``process_data_usp`` + collator, tensor for tensor;
* ``specforge train`` really launched (gloo, SIMT interpreter) at world 2 (Ulysses 2), world 2 (ring 2) and world 4 (draft_dp 2 x
  Ulysses 2): per micro-step loss / accuracy, per step grad norm and the final weights equal, bit for bit, the Python-API USP run on
  the same files, initial weights and topology; the first step matches the unsharded single-process run within tests/test_usp.py's
  bars; a mid-epoch resume continues bit-identically and the checkpoint exports to sglang.
The ``specforge train`` launch needs the reference, so it runs on CPU only.
"""
import functools
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from oracle import ref_harness as RH

pytestmark = pytest.mark.skipif(not RH.available(), reason="needs the reference checkout")

T = 3                   # ttt_length
S = 32                  # tokens per sample of the launched runs (S % sp == 0: the unsharded comparison's chunks are equal)
N_FILES = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAFT = {"architectures": ["LlamaForCausalLMEagle3"], "model_type": "llama", "hidden_act": "silu", "hidden_size": 128,
         "intermediate_size": 256, "num_attention_heads": 4, "num_key_value_heads": 2, "head_dim": 64, "num_hidden_layers": 1,
         "max_position_embeddings": 512, "rms_norm_eps": 1e-05, "vocab_size": 256, "draft_vocab_size": 128, "pad_token_id": 0,
         "bos_token_id": 1, "eos_token_id": 2, "tie_word_embeddings": False, "torch_dtype": "bfloat16", "initializer_range": 0.02}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _raw(n, seed, H=128):
    g = torch.Generator().manual_seed(seed)
    return dict(input_ids=torch.randint(0, 256, (n,), generator=g), loss_mask=(torch.rand(n, generator=g) > 0.25).long(),
                hidden_state=torch.randn(1, n, H, generator=g).to(torch.bfloat16),
                aux_hidden_state=torch.randn(1, n, 3 * H, generator=g).to(torch.bfloat16))


def _write_run_dir(work, lengths):
    from safetensors.torch import save_file

    dj = os.path.join(work, "draft.json")
    json.dump(DRAFT, open(dj, "w"))
    feat = os.path.join(work, "features")
    os.makedirs(feat)
    for i, n in enumerate(lengths):
        torch.save(_raw(n, 100 + i), os.path.join(feat, f"{i:04d}.ckpt"))
    td = os.path.join(work, "target")
    os.makedirs(td)
    H, V = DRAFT["hidden_size"], DRAFT["vocab_size"]
    json.dump({"architectures": ["LlamaForCausalLM"], "model_type": "llama", "hidden_size": H, "vocab_size": V, "num_hidden_layers": 1,
               "num_attention_heads": 4, "intermediate_size": 256}, open(os.path.join(td, "config.json"), "w"))
    g = torch.Generator().manual_seed(7)
    w = {"lm_head.weight": 0.05 * torch.randn(V, H, generator=g), "model.embed_tokens.weight": 0.05 * torch.randn(V, H, generator=g)}
    save_file(w, os.path.join(td, "model.safetensors"))
    json.dump({"metadata": {}, "weight_map": {k: "model.safetensors" for k in w}}, open(os.path.join(td, "model.safetensors.index.json"), "w"))
    vp = os.path.join(work, "vm.pt")
    t2d = torch.zeros(V, dtype=torch.bool)
    t2d[::2] = True
    Vd = DRAFT["draft_vocab_size"]
    torch.save({"t2d": t2d, "d2t": torch.arange(Vd) * 2 - torch.arange(Vd)}, vp)
    return dj, feat, td, vp


# ------------------------------------------------------------------------------------------------------------------ the topology
def test_topology_accepts_offline_usp_and_keeps_the_refusals():
    RH.setup()
    from types import SimpleNamespace

    from specforge.config.schema import TrainingConfig

    from specforge_amd.reference_plugin import _training_model_factory, check_training_topology

    draft = dict(DRAFT)
    for u, r in ((2, 1), (1, 2), (2, 2)):
        t = TrainingConfig(batch_size=1, attention_backend="usp", sp_ulysses_size=u, sp_ring_size=r)     # the reference's own schema
        check_training_topology(t, draft, mode="offline")                                              # accepted
    refusals = [
        (TrainingConfig(batch_size=1, tp_size=2), draft, "offline", "tp_size"),
        (SimpleNamespace(attention_backend="usp", batch_size=2, sp_ulysses_size=2, sp_ring_size=1, tp_size=1), draft, "offline",
         "batch_size"),
        (TrainingConfig(batch_size=1, attention_backend="usp", sp_ulysses_size=4), dict(draft, num_key_value_heads=2), "offline",
         "num_key_value_heads"),
        (TrainingConfig(batch_size=1, attention_backend="usp", sp_ulysses_size=2),
         dict(draft, rope_scaling={"rope_type": "mrope", "mrope_section": [16, 8, 8]}), "offline", "mrope"),
        (TrainingConfig(batch_size=1, attention_backend="usp", sp_ulysses_size=2), dict(draft, head_dim=32, hidden_size=128),
         "offline", "head_dim"),
        (TrainingConfig(batch_size=1, attention_backend="usp", sp_ring_size=2), draft, "online", "attention_backend 'usp'"),
    ]
    for t, d, mode, key in refusals:
        with pytest.raises(ValueError, match=key):
            check_training_topology(t, d, mode=mode)
    # the model factory runs the same checks with the run's mode (a stand-in config: the refusal comes before any model is built)
    build = _training_model_factory()
    with pytest.raises(ValueError, match="mode 'online'"):
        build(SimpleNamespace(training=TrainingConfig(batch_size=1, attention_backend="usp", sp_ulysses_size=2), mode="online"),
              None, DRAFT, None, None)


# ------------------------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def ref(emu_lib_path):
    RH.setup()
    RH.init_single_rank(29591)
    from specforge_amd import _lib
    from specforge_amd import reference_plugin as RP

    _lib._inject_library_for_tests(emu_lib_path)
    yield RP
    RP.uninstall()
    _lib._inject_library_for_tests(None)


@pytest.mark.parametrize("u,r", [(2, 1), (1, 2), (2, 2), (4, 1)])
def test_plugin_loader_usp_batches_are_the_references(ref, tmp_path, u, r):
    """per SP rank, two epochs (``set_epoch``: a new plan over the draft-dp ranks), uneven lengths, samples shorter than
    sp * (ttt_length + 1), samples longer than max_len, and a ``seek``; the ranged reader served every batch"""
    from specforge.data.preprocessing import OfflineEagle3Dataset
    from specforge.data.utils import DataCollatorWithPadding
    from specforge.launch import _shard_offline_refs
    from specforge.runtime.data_plane import FeatureDataLoader, LocalFeatureStore

    sp, max_len = u * r, 40
    lengths = [33, 5, 2, 17, 40, 47, 9, 3, 28, 1]
    _, feat, _, _ = _write_run_dir(str(tmp_path), lengths)
    alg = ref.registry().resolve(ref.ALGORITHM_NAME)
    source = alg.providers.offline_for("text").build_reader(feat, run_id="t", ttt_length=T, max_len=max_len).read()
    Hip = ref.feature_loader_class()
    for sp_rank in range(sp):
        transform = functools.partial(OfflineEagle3Dataset.process_data_usp, max_len=max_len, ttt_length=T, sp_rank=sp_rank, sp_size=sp,
                                      ring_rank=sp_rank // u, sp_ring_size=r)
        collate = DataCollatorWithPadding()
        collate.sp_degree, collate.ulysses_degree = sp, u       # (what the collator reads from the SP groups of a real run)

        def loader(cls, refs, **kw):
            return cls(LocalFeatureStore("t"), refs=refs, batch_size=1, collate_fn=collate, per_sample_transform=transform,
                       strategy=alg.name, **kw)

        for dp_rank, dp_size in ((0, 1), (1, 2)):
            for epoch in (0, 1):
                refs = _shard_offline_refs(source, use_usp_preprocess=True, seed=3, epoch=epoch, dp_rank=dp_rank, dp_size=dp_size)
                want = list(loader(FeatureDataLoader, refs))
                hip = loader(Hip, refs)
                n = 0
                for b in hip:
                    w = want[n]
                    assert b.sample_ids == w.sample_ids and b.metadata == w.metadata
                    assert set(b.tensors) == set(w.tensors)
                    for k, v in w.tensors.items():
                        assert b.tensors[k].dtype == v.dtype and torch.equal(b.tensors[k], v), (sp_rank, epoch, n, k)
                    n += 1
                assert n == len(want) == len(refs) and hip._ingest is not None and hip._ingest.sp_rank == sp_rank
        hip = loader(Hip, refs)
        hip.seek(3)
        assert [b.sample_ids for b in hip] == [w.sample_ids for w in want[3:]]


# ------------------------------------------------------------------------------------------------------------------ the launches
def _launch(work, paths, name, *, nproc, u, r, acc=1, max_steps=None, total_steps=None, resume_from=None, save_interval=0, timeout=900):
    import yaml

    dj, feat, td, vp = paths
    training = dict(strategy="eagle3", num_epochs=1, batch_size=1, learning_rate=2e-3, max_grad_norm=0.5, ttt_length=T,
                    attention_backend="usp", sp_ulysses_size=u, sp_ring_size=r, save_interval=save_interval, log_interval=1,
                    dist_timeout=60, seed=0, accumulation_steps=acc, warmup_ratio=0.25)
    if max_steps is not None:
        training["max_steps"] = max_steps
    if total_steps is not None:
        training["total_steps"] = total_steps
    if resume_from:
        training["resume_from"] = resume_from
    run = dict(model=dict(target_model_path=td, draft_model_config=dj, embedding_key="model.embed_tokens.weight", vocab_mapping_path=vp,
                          torch_dtype="bfloat16"),
               data=dict(hidden_states_path=feat, max_length=S), training=training, run_id=name, output_dir=os.path.join(work, "out-" + name),
               deployment=dict(mode="local_colocated", trainer=dict(nnodes=1, nproc_per_node=nproc)))
    yp = os.path.join(work, name + ".yaml")
    yaml.safe_dump(run, open(yp, "w"))
    probe = os.path.join(work, "probe-" + name)
    os.makedirs(probe)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE",
                                                            "GROUP_RANK", "TORCHELASTIC_RUN_ID")}
    env.update(SF_TEST_PROBE_DIR=probe, OMP_NUM_THREADS="1", SFEMU_THREADS="2")
    rr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_plugin_usp_worker.py"), "train", "-c", yp], env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert rr.returncode == 0, rr.stdout[-5000:]
    probes = {x: torch.load(os.path.join(probe, f"probe_rank{x}.pt"), weights_only=False) for x in range(nproc)}
    state = torch.load(os.path.join(work, "out-" + name, name + "-latest", "training_state.pt"), weights_only=False)
    return probes, state, rr.stdout


def _api(work, paths, name, probe0, *, world, sp, ring, acc, steps):
    from specforge_amd import build

    out = os.path.join(work, "api-" + name)
    os.makedirs(out)
    feat = paths[1]
    files = [os.path.join(feat, f) for f in sorted(os.listdir(feat)) if f.endswith(".ckpt")]
    import _plugin_usp_worker as W

    args = (world, _free_port(), build.build_emu(), files, paths[0], probe0, out, sp, ring, acc, steps, 0, S, T)
    if world == 1:
        W.run_api(0, *args)
    else:
        mp.spawn(W.run_api, args=args, nprocs=world, join=True)
    return {x: torch.load(os.path.join(out, f"probe_rank{x}.pt"), weights_only=False) for x in range(world)}


# bars of tests/test_usp.py (about twice its measured differences); the difference measured on this comparison beside each
BARS = dict(loss=2.5e-7, acc=0.0, grad=1.3e-2, params=3e-5)
# (the interpreter build is deterministic: these are the values every run measures)
MEASURED = {(2, 1, 1): "loss 2.4e-7, acc 0, grad 3.5e-3, params 3.7e-9, clear 0.38",
            (1, 2, 1): "loss 2.4e-7, acc 0, grad 3.5e-3, params 3.7e-9, clear 0.38",
            (2, 1, 2): "loss 2.4e-7, acc 0, grad 6.4e-3, params 3.8e-6, clear 0.22"}


def _same_bits(a, b, what):
    assert len(a["micro"]) == len(b["micro"]) > 0, what
    for i, (x, y) in enumerate(zip(a["micro"], b["micro"])):
        for k in ("loss", "plosses", "acces"):
            assert torch.equal(x[k], y[k]), (what, i, k, x[k], y[k])
    assert [s["grad_norm"] for s in a["steps"]] == [s["grad_norm"] for s in b["steps"]], what
    assert [s["lr"] for s in a["steps"]] == [s["lr"] for s in b["steps"]], what
    assert torch.equal(a["final"], b["final"]), what


@pytest.mark.parametrize("u,r,dp", [(2, 1, 1), (1, 2, 1), (2, 1, 2)], ids=["world2-ulysses2", "world2-ring2", "world4-dp2-ulysses2"])
def test_specforge_train_usp_equals_the_python_api_run(golden_dir, tmp_path, u, r, dp):
    RH.setup()
    from specforge.training.schedule import resolve_total_steps

    work = str(tmp_path)
    paths = _write_run_dir(work, [S] * N_FILES)
    sp, world = u * r, u * r * dp
    probes, state, log = _launch(work, paths, "usp", nproc=world, u=u, r=r)
    # the groups the backend adopted: the reference's mesh (draft_dp x sp, Ulysses peers consecutive), none built twice
    for x, p in probes.items():
        base = x - x % sp
        assert p["groups"]["sp_group"] == tuple(range(base, base + sp)), (x, p["groups"])
        assert p["groups"]["draft_dp_group"] == tuple(range(x % sp, world, sp))
        if r > 1:
            assert p["groups"]["sp_ring_group"] == tuple(base + t * u + x % u for t in range(r))
    # every rank applies the same world-averaged gradient
    assert all(torch.equal(p["final"], probes[0]["final"]) for p in probes.values())
    # the optimizer's horizon and step count: the reference's own (accumulation_steps * sp micro-steps per optimizer step)
    n_micro = N_FILES // dp
    total = resolve_total_steps(total_steps=None, max_steps=None, num_samples=n_micro, batch_size=1, accumulation_steps=sp, num_epochs=1)
    assert probes[0]["optimizer"]["total_steps"] == total == n_micro // sp
    assert all(len(p["micro"]) == n_micro and len(p["steps"]) == total for p in probes.values())
    assert state["global_step"] == total and state["strategy"] == "eagle3"
    # == the Python-API USP run on the same files, initial weights and topology, bit for bit
    api = _api(work, paths, "usp", os.path.join(work, "probe-usp", "probe_rank0.pt"), world=world, sp=sp, ring=r, acc=sp, steps=total)
    for x in range(world):
        _same_bits(probes[x], api[x], f"rank {x}")
    # == the unsharded single-process run (one sample per micro-step, sp * dp of them per optimizer step) within test_usp's bars
    one = _api(work, paths, "one", os.path.join(work, "probe-usp", "probe_rank0.pt"), world=1, sp=1, ring=1, acc=sp * dp,
               steps=1)[0]
    diffs = dict(loss=0.0, acc=0.0)
    for m in range(sp):                  # the first optimizer window: micro-step m of draft-dp group d is sample perm[d + dp * m]
        for d in range(dp):
            grp = [probes[d * sp + j]["micro"][m] for j in range(sp)]
            want = one["micro"][d + dp * m]
            diffs["loss"] = max(diffs["loss"], float((sum(g["plosses"] for g in grp) / sp - want["plosses"]).abs().max()))
            diffs["acc"] = max(diffs["acc"], float((grp[0]["acces"] - want["acces"]).abs().max()))
    g, gw = probes[0]["grad1"], one["grad1"]
    diffs["grad"] = float((g - gw).abs().max()) / float(gw.abs().max())
    clear = gw.abs() > 4 * (g - gw).abs().max()
    diffs["params"] = float((probes[0]["params1"].float() - one["params1"].float())[clear].abs().max())
    diffs["clear"] = float(clear.float().mean())
    print("specforge train usp vs unsharded:", diffs, "recorded:", MEASURED[(u, r, dp)])
    assert diffs["clear"] > 0.15         # (the rest are small or zero gradients: four samples per window average more of them out)
    for k, bar in BARS.items():
        assert diffs[k] <= bar, (k, diffs[k], bar)


def test_specforge_train_usp_resume_and_sglang_export(golden_dir, tmp_path):
    """SP 2 (world 2): 2 optimizer steps, checkpoint, a NEW launch resumes mid-epoch and takes 2 more == the uninterrupted 4-step run,
    bit for bit; the checkpoint exports to sglang and reloads into the reference's class"""
    work = str(tmp_path)
    paths = _write_run_dir(work, [S] * N_FILES)
    full, state_full, _ = _launch(work, paths, "full", nproc=2, u=2, r=1, total_steps=4)
    assert state_full["global_step"] == 4
    # rank 0 writes the shared checkpoint, every rank its own state (controller.py:839-886)
    assert os.path.exists(os.path.join(work, "out-full", "full-latest", "training_state_rank1.pt"))
    part, state_a, _ = _launch(work, paths, "a", nproc=2, u=2, r=1, max_steps=2, total_steps=4)
    assert state_a["global_step"] == 2
    resumed, state_b, log_b = _launch(work, paths, "b", nproc=2, u=2, r=1, total_steps=4, resume_from=os.path.join(work, "out-a", "a-latest"))
    assert state_b["global_step"] == 4, log_b[-3000:]
    for x in (0, 1):
        assert [s["lr"] for s in part[x]["steps"] + resumed[x]["steps"]] == [s["lr"] for s in full[x]["steps"]]
        assert [s["grad_norm"] for s in part[x]["steps"] + resumed[x]["steps"]] == [s["grad_norm"] for s in full[x]["steps"]]
        assert torch.equal(resumed[x]["final"], full[x]["final"])
    for k, v in state_full["draft_state_dict"].items():
        assert torch.equal(state_b["draft_state_dict"][k], v), k
    # export --to sglang of the SP-trained checkpoint (the reference's exporter, plugin not installed in this process)
    RH.setup()
    from safetensors.torch import load_file
    from specforge.export.to_sglang import export_to_sglang
    from specforge.modeling.auto import AutoDraftModel, AutoDraftModelConfig

    out = export_to_sglang(os.path.join(work, "out-b"), paths[0], os.path.join(work, "sglang"))
    sd = load_file(os.path.join(out, "model.safetensors"))
    for k, v in state_b["draft_state_dict"].items():
        assert torch.equal(sd[k], v), k
    rm = AutoDraftModel.from_config(AutoDraftModelConfig.from_file(paths[0]), torch_dtype=torch.bfloat16)
    missing, unexpected = rm.load_state_dict(sd, strict=False)
    assert not unexpected and all("embed" in k for k in missing)
