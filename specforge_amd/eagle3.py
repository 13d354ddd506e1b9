"""Drop-in ``OnlineEagle3Model`` + ``Eagle3TrainStrategy`` on the HIP engine.

Same constructor arguments, ``forward`` keyword arguments and 7-tuple of per-TTT-step lists as
the reference (specforge/algorithms/eagle3/model.py:100-442) and the same
``forward_loss(batch) -> StepOutput`` contract (specforge/training/strategies/base.py:124-319),
so ``TrainerCore.train_step`` (training/controller.py:328-363) and ``_reduce_eagle3_metrics``
(controller.py:200-304) drive it unchanged.  The whole micro-step is ONE autograd node:
``loss.backward()`` triggers ``Eagle3Engine.backward`` which writes straight into the flat
gradient buffer the parameters' ``.grad`` alias.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .engine import Eagle3Engine
from .model import LlamaForCausalLMEagle3


def loss_mask_suffix_counts(loss_mask: torch.Tensor, n: int = ops.MAX_DIAG + 1):
    """[sum(loss_mask[:, k:]) for k in range(n)] as python ints, from a HOST copy of the [B, S] loss mask: TTT step k scores row
    (b, s) against the mask at position s + k (eagle3/model.py:364-433), so these are the per-step numbers of rows that carry a loss.
    Computed where the mask still is in host memory (the ingest's pinned slot, a CPU batch): never a device read-back."""
    assert not loss_mask.is_cuda
    col = (loss_mask.reshape(loss_mask.shape[0], -1) != 0).sum(dim=0).flip(0).cumsum(0).flip(0).tolist()   # suffix sums over positions
    return [int(col[k]) if k < len(col) else 0 for k in range(n)]


def loss_mask_window_counts(loss_mask: torch.Tensor, ttt_length: int):
    """The USP form of ``loss_mask_suffix_counts``: a rank's [B, S + T] loss mask covers its chunk of S rows plus the T rows of overlap
    from the next shard, and TTT step k scores chunk row s against the mask at s + k -- which may lie in the overlap.  -> [count of
    (b, s), s in [0, S), with loss_mask[b, s + k] != 0 for k in range(T)] as python ints (window sums, not suffix sums), from a HOST
    copy of the mask (the ingest's pinned slot, a CPU batch): never a device read-back."""
    assert not loss_mask.is_cuda
    T = int(ttt_length)
    col = (loss_mask.reshape(loss_mask.shape[0], -1) != 0).sum(dim=0)
    S = col.numel() - T
    if S <= 0:
        return [0] * T
    cs = torch.nn.functional.pad(col.cumsum(0), (1, 0)).tolist()
    return [int(cs[k + S] - cs[k]) for k in range(T)]


def padding_left_shift(t: torch.Tensor) -> torch.Tensor:
    """``padding(tensor, left=False)`` (specforge/utils.py:128-135): shift left by one along dim 1, zero fill."""
    return torch.cat((t[:, 1:], torch.zeros_like(t[:, -1:])), dim=1)


class _TTTStep(torch.autograd.Function):
    """plosses[T] as one node; backward = the engine's hand-written sweep."""

    @staticmethod
    def forward(ctx, anchor, engine, plosses):
        ctx.engine = engine
        return plosses.clone()

    @staticmethod
    def backward(ctx, grad_plosses):
        eng: Eagle3Engine = ctx.engine
        # The upstream gradient lives on the device.  It is only needed as the alpha of the weight-gradient GEMMs at the
        # end of the sweep, so it is copied to pinned memory asynchronously and read back THERE: the host queues the whole
        # data-gradient sweep first and the read-back waits behind ~half a step of queued GPU work instead of stalling
        # the launch of the backward behind the forward.
        gp_dev = grad_plosses.detach().float()
        nt = gp_dev.numel()
        # the engine's device-side input checks (host-supplied row counts, position ids) ride along -- always, so the pinned
        # buffer keeps ONE shape whether or not a batch was checked
        gp_dev = torch.cat([gp_dev.view(-1), eng._flags.to(gp_dev.device)])
        if gp_dev.is_cuda:
            host = eng._upstream_host      # one pinned buffer for the engine's lifetime: allocating
            if host is None or host.shape != gp_dev.shape:   # pinned memory per step costs milliseconds of idle GPU
                host = eng._upstream_host = torch.empty(gp_dev.shape, dtype=torch.float32, pin_memory=True)
            host.copy_(gp_dev, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record()
        else:
            host, ready = gp_dev, None

        def resolve():
            if ready is not None:
                ready.synchronize()
            gp = host.tolist()
            eng.check_flags(gp[nt:])
            gp = gp[:nt]
            g = gp[0]
            # The decay weights are baked into the fused CE gradients; the caller must use the same ones.
            for k, v in enumerate(gp):
                want = g * (eng.decay ** k)
                if abs(v - want) > 1e-6 * max(1.0, abs(want)):
                    raise RuntimeError(
                        f"ploss weights seen in backward ({gp}) are not g*ploss_decay^k with ploss_decay={eng.decay}; "
                        "construct OnlineEagle3Model(ploss_decay=...) with the strategy's value")
            return g

        eng.backward(resolve)
        return None, None, None


class OnlineEagle3Model(nn.Module):
    """EAGLE3 TTT trainer module (reference: eagle3/model.py:100-442) on the HIP engine."""

    def __init__(self, draft_model: LlamaForCausalLMEagle3, length: int = 7, attention_backend: str = "hip",
                 lk_loss_type: Optional[str] = None, kl_scale: float = 1.0, kl_decay: float = 1.0,
                 ploss_decay: float = 0.8, sp_group=None, sp_ulysses_group=None, sp_ring_group=None, mrope_analytic: bool = False, topk=(),
                 chain: bool = False, conf_bins: int = 0, conf_thresholds=()):
        """``attention_backend="usp"``: Ulysses sequence parallelism over ``sp_group`` (set here, or later by
        ``HipDPTrainingBackend.prepare_model`` / the strategy, before the first forward); every other value runs the one-rank
        attention.  ``sp_ring_group`` (with ``sp_ulysses_group``, None for a pure ring): ring x Ulysses over the same SP group
        (training.make_usp_groups); ``sp_group`` alone is pure Ulysses.  ``mrope_analytic``: ``Eagle3Engine.mrope_analytic`` (rope_type
        'mrope': angles computed on the device from the ids -- no table limits; off by default).  ``topk``: ``Eagle3Engine.topk`` -- up to 8
        ascending ints k; after every forward ``last_topk`` holds, per TTT step, the [len(topk)] counts of rows whose target token is in
        the draft's top k (denominators: ``acc_denoms``).  The return tuple of ``forward`` is the reference's seven lists either way.
        ``chain``: ``Eagle3Engine.chain`` -- the joint accepted length of the draft chains; after every forward ``last_chain`` =
        (denoms, corrects): per TTT step the count of rows with a loss mask at every depth so far, and the [1 + len(topk)] counts of
        those that hit at every depth so far (channel 0 top-1, then ``topk``); None when off.
        ``conf_bins`` / ``conf_thresholds``: ``Eagle3Engine.conf_bins`` / ``.conf_thresholds`` -- the draft's top-1 softmax probability
        per row; after every forward ``last_conf`` = (bins, denoms, gate): per TTT step the [3, conf_bins] reliability bins (rows, top-1
        hits, confidence sum), the count of rows with a loss mask at every depth so far, and the [len(conf_thresholds), 2] (drafted,
        accepted) counts of the confidence-gated chains; None when both are unset."""
        super().__init__()
        if lk_loss_type not in (None, "alpha", "lambda"):
            raise ValueError(f"Unknown lk loss type: {lk_loss_type}")  # core/lk_loss.py:99
        if not 1 <= int(length) <= ops.MAX_DIAG + 1:
            raise ValueError(f"ttt_length must be in 1..{ops.MAX_DIAG + 1}")
        self.draft_model = draft_model
        self.length = length
        self.attention_backend = attention_backend
        self.sp_group = sp_group
        self.sp_ulysses_group, self.sp_ring_group = sp_ulysses_group, sp_ring_group
        self.lk_loss_type, self.kl_scale, self.kl_decay = lk_loss_type, kl_scale, kl_decay
        self.ploss_decay = ploss_decay
        self.mrope_analytic = mrope_analytic
        self.topk = Eagle3Engine._check_topk(topk)
        self.last_topk = None
        self.chain = bool(chain)
        self.last_chain = None
        self.conf_bins, self.conf_thresholds = Eagle3Engine._check_conf(conf_bins, conf_thresholds)
        self.last_conf = None
        self._engine: Optional[Eagle3Engine] = None
        dev = next(draft_model.parameters()).device
        self._anchor = nn.Parameter(torch.zeros((), device=dev), requires_grad=True)

    @property
    def engine(self) -> Eagle3Engine:
        """Built on first use: the reference's assembly moves the composite with ``.to(device, dtype)`` AFTER
        constructing it (algorithms/model_providers.py:268-275); adopting the parameters into the flat buffer any
        earlier would be undone by that move."""
        if self._engine is None:
            sp_group = uly_group = ring_group = None
            if self.attention_backend == "usp":
                if self.sp_group is None:
                    raise ValueError("attention_backend 'usp' needs the SP process group (OnlineEagle3Model(sp_group=...), "
                                     "ParallelConfig(sp_size=...) or Eagle3TrainStrategy(sp_group=...))")
                sp_group, uly_group, ring_group = self.sp_group, self.sp_ulysses_group, self.sp_ring_group
            self._engine = Eagle3Engine(self.draft_model, ttt_length=self.length, ploss_decay=self.ploss_decay,
                                        lk_loss_type=self.lk_loss_type, kl_scale=self.kl_scale, kl_decay=self.kl_decay,
                                        sp_group=sp_group, sp_ulysses_group=uly_group, sp_ring_group=ring_group,
                                        mrope_analytic=self.mrope_analytic, topk=self.topk, chain=self.chain,
                                        conf_bins=self.conf_bins, conf_thresholds=self.conf_thresholds)
            object.__setattr__(self.draft_model, "_hip_engine", self._engine)   # found by BF16Optimizer(draft_model)
        return self._engine

    def _apply(self, fn, *a, **kw):
        if self._engine is not None:
            before = self._engine.flat.data.data_ptr()
            super()._apply(fn, *a, **kw)
            if any(p.data_ptr() != self._engine.flat.data[lo:hi].data_ptr()
                   for n, p in self._engine.flat.params.items() for lo, hi in [self._engine.flat.slices[n]]):
                raise RuntimeError("OnlineEagle3Model was moved/cast after its HIP engine adopted the parameters; move the "
                                   "model to its device and dtype before the first forward / optimizer construction")
            assert before == self._engine.flat.data.data_ptr()
            return self
        return super()._apply(fn, *a, **kw)

    def forward(self, input_ids, attention_mask, target=None, loss_mask=None, hidden_states=None, past_key_values=None,
                position_ids=None, target_hidden_for_compact=None, target_head_weight=None,
                compact_teacher_chunk_size: Optional[int] = None, loss_counts=None, position_span=None):
        """``loss_counts`` (optional, not in the reference's signature): loss_counts[k] = number of rows whose loss mask at position
        s + k is set, as HOST integers -- lets the engine run lm_head / CE on those rows only (``loss_mask_suffix_counts``).
        ``position_span`` (optional): (min, max) of ``position_ids`` as host integers (range check / RoPE table growth without a
        device read-back); CPU ``position_ids`` are measured here."""
        if past_key_values is not None:
            raise NotImplementedError("past_key_values is unused by EAGLE3 training (eagle3/model.py:262)")
        train = torch.is_grad_enabled() and self.training
        dev = self.engine.dev
        if self.engine.topk != tuple(self.topk):
            self.engine.topk = self.topk
        if self.engine.chain != bool(self.chain):
            self.engine.chain = self.chain
        if (self.engine.conf_bins, self.engine.conf_thresholds) != Eagle3Engine._check_conf(self.conf_bins, self.conf_thresholds):
            self.engine._set_conf(self.conf_bins, self.conf_thresholds)
        if position_span is None and position_ids is not None and not position_ids.is_cuda and position_ids.numel():
            position_span = (int(position_ids.min()), int(position_ids.max()))
        to = lambda t: None if t is None else t.to(dev)
        out = self.engine.forward(
            input_ids=to(input_ids), attention_mask=attention_mask, loss_mask=to(loss_mask), hidden_states=to(hidden_states),
            target_hidden=to(target_hidden_for_compact), target_head_weight=target_head_weight,
            target_logits=to(target) if target_hidden_for_compact is None else None, position_ids=to(position_ids), train=train,
            loss_counts=loss_counts, position_span=position_span)
        plosses = torch.stack(out["plosses"])
        if train:
            plosses = _TTTStep.apply(self._anchor, self.engine, plosses)
        self.last_artifacts = dict(target_token_ids=out["target_token_ids"], position_mask=out["position_mask"])
        self.last_topk = out.get("topk_corrects")
        self.last_chain = (out["chain_denoms"], out["chain_corrects"]) if "chain_denoms" in out else None
        self.last_conf = (out["conf_bins"], out["conf_denoms"], out["conf_gate"]) if "conf_bins" in out else None
        return (list(plosses.unbind(0)), out["acceptance_rates"], out["acces"], out["acc_corrects"], out["acc_denoms"],
                out["metric_losses"], out["metric_loss_denoms"])


@dataclass(frozen=True)
class StepOutput:
    """training/strategies/base.py:29-42"""

    loss: torch.Tensor
    metrics: Dict[str, Any]
    ratio_metrics: Dict[str, Tuple[Any, Any]] = field(default_factory=dict)
    loss_terms: Optional[Tuple[torch.Tensor, torch.Tensor]] = None


class TargetHead(nn.Module):
    """Frozen teacher projection (specforge/modeling/target/target_head.py:15-108): ``fc`` H -> V_target."""

    def __init__(self, weight: torch.Tensor):
        super().__init__()
        self.fc = nn.Linear(weight.shape[1], weight.shape[0], bias=False, device=weight.device, dtype=weight.dtype)
        with torch.no_grad():
            self.fc.weight.copy_(weight)
        self.fc.weight.requires_grad = False

    @staticmethod
    def preprocess(input_ids, target, loss_mask):
        """target_head.py:103-108: shift target and input_ids left by one, loss_mask -> [B,S,1]"""
        return padding_left_shift(input_ids), padding_left_shift(target), loss_mask[..., None]


def usp_unpad(tensors):
    """A USP shard as the engine takes it: ``chunk + ttt_length`` rows.  The reference's collator (data/utils.py:122-196) pads
    ``input_ids``, ``attention_mask``, ``loss_mask`` and ``target`` of a shard to a multiple of the SP degree but not ``hidden_state``, and
    its model reads the local length from ``hidden_state`` (eagle3/model.py:310, core/eagle3_adapters.py:98-140); the rows past it are
    zeros.  Shards without that padding (``ingest.usp_shard``) come back unchanged."""
    hs = tensors.get("hidden_state")
    if hs is None:
        return tensors
    n = hs.shape[1]
    out = dict(tensors)
    for k in ("input_ids", "attention_mask", "loss_mask", "target"):
        v = out.get(k)
        if v is not None and v.dim() >= 2 and v.shape[1] > n:
            out[k] = v[:, :n]
    return out


class Eagle3TrainStrategy:
    """training/strategies/base.py:124-319.  The teacher always runs the streaming path
    (target hidden state + frozen head weight -> soft targets; [B,S,V_target] is never kept)."""

    name = "eagle3"
    required_features = {"input_ids", "attention_mask", "loss_mask", "hidden_state", "target"}

    def __init__(self, eagle3_model: OnlineEagle3Model, *, target_head: Optional[TargetHead] = None,
                 ploss_decay: float = 0.8, compact_teacher: bool = True, compact_teacher_chunk_size: Optional[int] = None,
                 pinned_staging: bool = True, sp_group=None, sp_ulysses_group=None, sp_ring_group=None):
        """``pinned_staging=False`` (A/B only, ``bench.py --feed cpu_batch_pageable``): CPU batches are shifted on the CPU and
        moved with the blocking pageable ``.to(device)`` the reference's strategy uses (strategies/base.py:256-284)."""
        self.pinned_staging = pinned_staging
        self.eagle3_model = eagle3_model
        if sp_group is not None:        # attention_backend "usp": the SP group the engine exchanges over
            if eagle3_model._engine is not None and eagle3_model._engine.sp_group is not sp_group:
                raise ValueError("sp_group must be set before the HIP engine is built (the first forward)")
            eagle3_model.sp_group = sp_group
            if sp_ring_group is not None:   # ring x Ulysses (training.make_usp_groups)
                eagle3_model.sp_ulysses_group, eagle3_model.sp_ring_group = sp_ulysses_group, sp_ring_group
        self.target_head = target_head
        self.ploss_decay = ploss_decay
        self._stager = None
        if abs(eagle3_model.ploss_decay - ploss_decay) > 1e-12:
            raise ValueError("OnlineEagle3Model.ploss_decay and the strategy's ploss_decay must agree")

    def trainable_module(self) -> nn.Module:
        return self.eagle3_model

    def validate_batch(self, batch) -> None:
        missing = self.required_features - set(batch.tensors)
        if missing:
            raise ValueError(f"eagle3 strategy: batch lacks {sorted(missing)}")

    def _resident(self, tensors):
        """The batch on the engine's device.  Batches from the HIP ingest (``reference_plugin.feature_loader_class``,
        ``ingest.HiddenStateIngest``) already are; a CPU batch (the reference's own loader hands those over and moves them with
        a blocking pageable ``.to(device)``, strategies/base.py:270-289) goes through a pinned double buffer and a HIP copy
        stream -- the TTT shift of ``preprocess`` then runs on the device either way."""
        dev = self.eagle3_model.engine.dev
        if dev.type != "cuda" or not self.pinned_staging or all(v is None or v.is_cuda for v in tensors.values()):
            return tensors
        if self._stager is None:
            from .ingest import PinnedStager

            self._stager = PinnedStager(dev)
        return self._stager.stage(tensors)

    def forward_loss(self, batch, ctx=None) -> StepOutput:
        self.validate_batch(batch)
        tensors = batch.tensors
        if self.eagle3_model.attention_backend == "usp":
            tensors = usp_unpad(tensors)
        # rows per TTT step that carry a loss (host integers): from the loader's metadata, or from the mask while it is still a CPU tensor
        # (USP: per-rank window counts over the chunk + T rows of overlap, loss_mask_window_counts)
        md = getattr(batch, "metadata", None) or {}
        lm0 = tensors.get("loss_mask")
        if self.eagle3_model.attention_backend == "usp":
            counts = md.get("loss_mask_window_counts", getattr(batch, "loss_mask_window_counts", None))
            if counts is None and lm0 is not None and not lm0.is_cuda:
                counts = loss_mask_window_counts(lm0, self.eagle3_model.length)
        else:
            counts = md.get("loss_mask_suffix_counts")
            if counts is None and lm0 is not None and not lm0.is_cuda:
                counts = loss_mask_suffix_counts(lm0)
        pid0 = tensors.get("position_ids")
        span = (int(pid0.min()), int(pid0.max())) if pid0 is not None and not pid0.is_cuda and pid0.numel() else None
        t = self._resident(tensors)
        target_repr = md.get("target_repr")
        kwargs = {}
        if target_repr == "hidden_state":
            if self.target_head is None:
                raise ValueError("target_repr='hidden_state' requires a target_head to re-run the lm_head projection")
            input_ids, target_hidden, loss_mask = TargetHead.preprocess(t["input_ids"], t["target"], t["loss_mask"])
            kwargs = dict(target_hidden_for_compact=target_hidden, target_head_weight=self.target_head.fc.weight.data)
            target = None
        else:
            # logits (or any other / missing target_repr): online capture has already shifted logits and input ids, so
            # they are used exactly as delivered (_prepare_eagle_target, strategies/base.py:95-121)
            input_ids, target, loss_mask = t["input_ids"], t["target"], t["loss_mask"]
        plosses, acceptance_rates, acces, acc_corrects, acc_denoms, metric_losses, metric_loss_denoms = self.eagle3_model(
            input_ids=input_ids, attention_mask=t["attention_mask"], loss_mask=loss_mask, target=target,
            hidden_states=t["hidden_state"], position_ids=t.get("position_ids"), loss_counts=counts, position_span=span, **kwargs)
        weights = [self.ploss_decay ** i for i in range(len(plosses))]
        loss = sum(weights[i] * plosses[i] for i in range(len(plosses)))
        d = lambda xs: [x.detach() for x in xs]
        metrics = dict(plosses=d(plosses), acces=d(acces), acceptance_rates=d(acceptance_rates), acc_corrects=d(acc_corrects),
                       acc_denoms=d(acc_denoms), metric_losses=d(metric_losses), metric_loss_denoms=d(metric_loss_denoms))
        tk = self.eagle3_model.last_topk
        if tk is not None:      # top{k}_corrects: T 0-dim counts each, the shape of acc_corrects (the reference's trainer and evaluator skip them)
            for j, kth in enumerate(self.eagle3_model.topk):
                metrics[f"top{kth}_corrects"] = [step[j].detach() for step in tk]
        ch = self.eagle3_model.last_chain
        if ch is not None:      # chain_denoms / chain_top{k}_corrects: T 0-dim counts each (k = 1, then the model's topk; a 1 in topk is named once)
            metrics["chain_denoms"] = [x.detach() for x in ch[0]]
            for h, kth in enumerate((1,) + tuple(self.eagle3_model.topk)):
                metrics.setdefault(f"chain_top{kth}_corrects", [step[h].detach() for step in ch[1]])
        cf = self.eagle3_model.last_conf
        if cf is not None:      # lists over the T steps of [NB] / 0-dim / [J] counts (the reference's trainer and evaluator skip them)
            metrics["conf_bin_counts"] = [step[0].detach() for step in cf[0]]
            metrics["conf_bin_corrects"] = [step[1].detach() for step in cf[0]]
            metrics["conf_bin_sums"] = [step[2].detach() for step in cf[0]]
            metrics["conf_denoms"] = [x.detach() for x in cf[1]]
            metrics["conf_gate_drafted"] = [step[:, 0].detach() for step in cf[2]]
            metrics["conf_gate_accepted"] = [step[:, 1].detach() for step in cf[2]]
        return StepOutput(loss=loss, metrics=metrics)

    def checkpoint_state_filter(self, state_dict: Dict[str, Any]) -> Dict[str, Any]:
        """strip ``draft_model.``, drop the frozen embedding and engine internals (strategies/base.py:306-319)"""
        return {k.replace("draft_model.", ""): v for k, v in state_dict.items()
                if "draft_model." in k and "embed" not in k.lower()}


class TopKAccumulator:
    """Top-k hit rates of a draft over many batches: float64 sums of ``top{k}_corrects`` and ``acc_denoms`` per TTT step, the ratio taken
    after the sums (the reference's Evaluator forms its per-position accuracy the same way, eval/evaluator.py:47-93, 142-150).

    ``summary()`` -> ``top{k}_acc_{i}`` (the share of step i's scored rows whose target token is among the draft's k best) and
    ``simulated_acc_len_top{k}`` = a0 + a0*a1 + ... over those rates: the Evaluator's ``_simulated_acc_len`` recurrence.  For k = 1 it is
    the reference's expected accepted length of a chain draft.  For k > 1 it is an OPTIMISTIC bound for a top-k tree: it assumes the tree
    keeps every one of the k candidates at every depth (k^depth nodes) and that the per-depth rates, measured along the teacher-forced
    path, carry over to whichever branch was accepted; a served tree prunes to a node budget and accepts less.  The recurrence also
    treats the hits at different depths as independent, which they are not (hard positions miss at every depth): the exact
    teacher-forced figure from the joint hits is ``chain_acc_len_top{k}`` of ``ChainAccumulator`` (``OnlineEagle3Model(chain=True)``)."""

    def __init__(self, topk):
        self.topk = Eagle3Engine._check_topk(topk)
        self.corrects: Optional[torch.Tensor] = None        # [len(topk), T] float64
        self.denoms: Optional[torch.Tensor] = None          # [T] float64

    def update(self, metrics: Dict[str, Any]) -> None:
        """``metrics`` = ``StepOutput.metrics`` of a strategy whose model has ``topk`` set"""
        # (sums stay on the metrics' device: no read-back per batch, ``summary`` pays one)
        c = torch.stack([torch.stack([torch.as_tensor(v).detach().double() for v in metrics[f"top{k}_corrects"]]) for k in self.topk])
        den = torch.stack([torch.as_tensor(v).detach().double() for v in metrics["acc_denoms"]]).to(c.device)
        # (acc_denoms is the count of scored rows clamped to >= 1e-6: a step without any contributes no rows)
        den = torch.where(den >= 1.0, den, torch.zeros_like(den))
        if self.corrects is None:
            self.corrects, self.denoms = torch.zeros_like(c), torch.zeros_like(den)
        self.corrects += c
        self.denoms += den

    @staticmethod
    def simulated_acc_len(rates) -> float:
        cumulative, total = 1.0, 0.0
        for a in rates:
            cumulative *= float(a)
            total += cumulative
        return total

    def summary(self) -> Dict[str, float]:
        if self.corrects is None:
            return {}
        out: Dict[str, float] = {}
        for j, k in enumerate(self.topk):
            rates = (self.corrects[j] / self.denoms.clamp_min(1.0)).cpu().tolist()
            for i, a in enumerate(rates):
                out[f"top{k}_acc_{i}"] = float(a)
            out[f"simulated_acc_len_top{k}"] = self.simulated_acc_len(rates)
        return out


class ChainAccumulator:
    """Accepted length of the draft chains over many batches, from the JOINT hits (``OnlineEagle3Model(chain=True)``): float64 sums of
    ``chain_top{k}_corrects`` and ``chain_denoms`` per TTT depth, the ratio taken after the sums, 0 where the denominator is 0.

    ``summary()`` -> ``chain_top{k}_acc_{i}``: of the rows that could be scored at every depth 0 .. i, the share whose target was among
    the draft's k best at every one of them -- the probability that a chain (k = 1) or a full top-k tree is accepted to depth i + 1 --
    and ``chain_acc_len_top{k}`` = their sum over i, the expected accepted length.  Teacher-forced (the inputs are the dataset's tokens,
    hits are against the teacher's argmax, as ``acces``): exact for a greedy chain and for a full top-k tree along the true path, an
    upper bound for a tree pruned to a node budget.  ``ks``: the channels to report, each 1 or a member of the model's ``topk``."""

    def __init__(self, ks):
        self.ks = tuple(int(k) for k in ks)
        if not self.ks or any(k < 1 for k in self.ks) or len(set(self.ks)) != len(self.ks):
            raise ValueError(f"ChainAccumulator: distinct positive k, got {self.ks}")
        self.corrects: Optional[torch.Tensor] = None        # [len(ks), T] float64
        self.denoms: Optional[torch.Tensor] = None          # [T] float64

    def update(self, metrics: Dict[str, Any]) -> None:
        """``metrics`` = ``StepOutput.metrics`` of a strategy whose model has ``chain`` set"""
        # (sums stay on the metrics' device: no read-back per batch, ``summary`` pays one)
        c = torch.stack([torch.stack([torch.as_tensor(v).detach().double() for v in metrics[f"chain_top{k}_corrects"]]) for k in self.ks])
        den = torch.stack([torch.as_tensor(v).detach().double() for v in metrics["chain_denoms"]]).to(c.device)
        if self.corrects is None:
            self.corrects, self.denoms = torch.zeros_like(c), torch.zeros_like(den)
        self.corrects += c
        self.denoms += den

    def summary(self) -> Dict[str, float]:
        if self.corrects is None:
            return {}
        out: Dict[str, float] = {}
        rates = torch.where(self.denoms > 0, self.corrects / self.denoms.clamp_min(1.0), torch.zeros_like(self.corrects)).cpu().tolist()
        for j, k in enumerate(self.ks):
            for i, a in enumerate(rates[j]):
                out[f"chain_top{k}_acc_{i}"] = float(a)
            out[f"chain_acc_len_top{k}"] = float(sum(rates[j]))
        return out


class ConfidenceAccumulator:
    """Calibration of the draft's confidence and the length of confidence-gated chains over many batches
    (``OnlineEagle3Model(conf_bins=, conf_thresholds=)``): float64 sums of the ``conf_*`` metrics per TTT depth, on the metrics' device,
    every ratio taken after the sums, 0 where a denominator is 0.

    Confidence is the draft's top-1 probability: the softmax at temperature 1 of the logits as stored.  ``summary()`` per depth i, over the
    rows scored at that depth (a loss mask; like ``acces``, not restricted to chains still alive): ``conf_mean_i``, ``conf_acc_i`` (the
    top-1 hit rate), ``conf_ece_i`` = sum_b n_b / n * |hits_b / n_b - sum_b / n_b| (the expected calibration error over the ``bins``
    equal-width bins) and ``conf_reliability_i``, the table: per occupied or empty bin a tuple (count, accuracy, mean confidence).

    Per threshold tau: ``gated_acc_len_tau{tau}`` = sum_k accepted_k / denoms_0 and ``gated_draft_len_tau{tau}`` = sum_k drafted_k /
    denoms_0 -- accepted and drafted tokens per chain, over the rows scored at depth 0 -- and ``gated_acc_per_draft_tau{tau}``, their
    ratio.  Teacher-forced, as ``chain_acc_len_top1``.  ACCEPTED is exact for a greedy chain that stops drafting at the first depth
    whose confidence is under tau.  DRAFTED counts the tokens such a chain proposes up to and including its first rejected one; what a
    drafter proposes AFTER its first wrong token is not observable teacher-forced (its inputs would be its own tokens), so the draft
    cost is a lower bound.  A chain censored by a position without a loss mask stops counting on both sides."""

    def __init__(self, bins, thresholds):
        self.bins, self.thresholds = Eagle3Engine._check_conf(bins, thresholds)
        self.sums: Optional[Dict[str, torch.Tensor]] = None     # key -> float64 [T, ...]

    _KEYS = ("conf_bin_counts", "conf_bin_corrects", "conf_bin_sums", "conf_denoms", "conf_gate_drafted", "conf_gate_accepted")

    def update(self, metrics: Dict[str, Any]) -> None:
        """``metrics`` = ``StepOutput.metrics`` of a strategy whose model has ``conf_bins`` / ``conf_thresholds`` set"""
        new = {k: torch.stack([torch.as_tensor(v).detach().double() for v in metrics[k]]) for k in self._KEYS}
        if self.sums is None:
            self.sums = {k: torch.zeros_like(v) for k, v in new.items()}
        for k, v in new.items():
            self.sums[k] += v.to(self.sums[k].device)

    @staticmethod
    def tau_name(tau: float) -> str:
        return f"{tau:g}"

    def summary(self) -> Dict[str, Any]:
        if self.sums is None:
            return {}
        sm = {k: v.cpu().tolist() for k, v in self.sums.items()}       # (one read-back; math.fsum: correctly rounded, so order-free)
        cnt, hit, cs, den = sm["conf_bin_counts"], sm["conf_bin_corrects"], sm["conf_bin_sums"], sm["conf_denoms"]
        out: Dict[str, Any] = {}
        for i in range(len(cnt) if self.bins else 0):
            n = math.fsum(cnt[i])
            out[f"conf_ece_{i}"] = math.fsum(c * abs(h / c - z / c) for c, h, z in zip(cnt[i], hit[i], cs[i]) if c > 0) / n if n > 0 else 0.0
            out[f"conf_mean_{i}"] = math.fsum(cs[i]) / n if n > 0 else 0.0
            out[f"conf_acc_{i}"] = math.fsum(hit[i]) / n if n > 0 else 0.0
            out[f"conf_reliability_{i}"] = [(c, h / c if c > 0 else 0.0, z / c if c > 0 else 0.0) for c, h, z in zip(cnt[i], hit[i], cs[i])]
        d0 = float(den[0])
        for j, tau in enumerate(self.thresholds):
            acc, dr = math.fsum(row[j] for row in sm["conf_gate_accepted"]), math.fsum(row[j] for row in sm["conf_gate_drafted"])
            name = self.tau_name(tau)
            out[f"gated_acc_len_tau{name}"] = acc / d0 if d0 > 0 else 0.0
            out[f"gated_draft_len_tau{name}"] = dr / d0 if d0 > 0 else 0.0
            out[f"gated_acc_per_draft_tau{name}"] = acc / dr if dr > 0 else 0.0
        return out


@dataclass
class TrainBatch:
    """runtime/contracts.py:80-129 (the fields the strategy reads)"""

    tensors: Dict[str, torch.Tensor]
    metadata: Dict[str, Any] = field(default_factory=dict)
