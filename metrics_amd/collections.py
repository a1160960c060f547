"""L5 — MetricCollection with compute-group state dedup.

Parity: torchmetrics ``collections.py`` (MetricCollection semantics:
dict/list/args inputs, prefix/postfix renaming, nested-collection flattening,
per-metric kwarg routing, compute groups with shared-by-reference state,
copy-on-access).

Compute groups: metrics whose states are equal after the first update (e.g.
Accuracy/Precision/Recall/F1, which all accumulate tp/fp/tn/fn) are merged
into one group; subsequent ``update`` calls only run the group leader's
update and members alias the leader's state tensors. Accessing metrics via
``items()/values()/[key]`` deep-copies states to break aliasing (reference is
re-established on the next update). On an MI355X node this is the difference
between one fused stat-scores kernel launch per batch and N of them.
"""
from __future__ import annotations

from collections import OrderedDict
from copy import deepcopy
from typing import Any, Dict, Hashable, Iterable, Iterator, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor
from torch.nn import ModuleDict

from metrics_amd.metric import Metric
from metrics_amd.utilities import tracing
from metrics_amd.utilities.compute import _reduce_curve_auc
from metrics_amd.utilities.data import _flatten_dict, allclose
from metrics_amd.utilities.prints import rank_zero_warn


def _strip_prefix(s: str, prefix: str) -> str:
    return s[len(prefix):] if s.startswith(prefix) else s


def _strip_suffix(s: str, suffix: str) -> str:
    return s[: -len(suffix)] if s.endswith(suffix) else s


class _StepBuffers(NamedTuple):
    """The per-step buffers of the fused update and what they were made for
    (``_FusedMulticlassUpdatePlan._step_buffers``); None without their leader."""

    device: Any
    rows: int  # capacity of rowstats
    logits: bool
    counts: Tensor
    topk_counts: Optional[Tensor]
    rowstats: Optional[Tensor]
    epoch_buf: Optional[Tensor]


_NO_OWNER: dict = {}  # the __dict__ of a leader that takes no part: holds no buffer


class _FusedMulticlassUpdatePlan:
    """Collection-level cross-metric fusion: the stat-scores, confusion-matrix
    and exact-match group leaders all start with the same argmax pass over the
    (B, C) logits — ONE fused kernel call feeds all of them (MI355X-first:
    the logits are read once from HBM instead of three times).

    ``topk`` is the leader of one stat-scores group with ``top_k > 1``: its
    effective prediction is the target where the target ranks inside the top
    k, else the same argmax, so the same pass counts it into a second scratch.
    It is handled only by a step that really counted it (float logits, a class
    count the slot covers); otherwise it updates on its own, as before."""

    def __init__(self, stat, confmat, exact, curve, topk=None):
        self.stat = stat
        self.confmat = confmat
        self.exact = exact
        self.curve = curve
        self.topk = topk
        self.topk_steps = 0
        self.leaders = tuple(m for m in (stat, confmat, exact, curve) if m is not None)
        # one-pass step (logits read once); METRICS_AMD_ONEPASS=0 keeps the
        # stat + curve-hist + apply kernel sequence, 2 lifts the shape gate
        from metrics_amd.ops import _hip

        mode = _hip.onepass_mode()
        self.onepass = curve is not None and mode != 0
        self.onepass_force = mode == 2
        self.onepass_steps = 0
        self._kept: Optional[_StepBuffers] = None

    def _step_buffers(self, _hip, dev, rows: int, logits: bool) -> "_StepBuffers":
        """The buffers of a step of ``rows`` rows on ``dev``. Each lives in its
        leader's ``__dict__`` (:func:`owner_buffer`). The record of the last
        step is kept and serves again while device, row capacity and kind of
        predictions fit and every buffer still IS the one its owner holds, the
        same identity rule as ``_NativePlan.fits``; that costs a fraction of
        looking each buffer up again. Label predictions take neither the curve
        leader nor the top-k slot along, so they get none of their buffers."""
        stat, curve, topk = self.stat, self.curve, self.topk
        C = stat.num_classes
        if not logits:
            curve = topk = None
        elif topk is not None and not _hip.mc_stat_topk_covers(C):
            topk = None
        kept = self._kept
        curve_own = curve.__dict__ if curve is not None else _NO_OWNER
        if (
            kept is not None and kept.device == dev and rows <= kept.rows and kept.logits == logits
            and kept.counts is stat.__dict__.get("_hip_scratch")
            and kept.topk_counts is (topk.__dict__ if topk is not None else _NO_OWNER).get("_hip_scratch")
            and kept.rowstats is curve_own.get("_hip_rowstats_buf")
            and kept.epoch_buf is curve_own.get("_hip_epoch_buf")
        ):
            return kept
        rowstats = _hip._rowstats_buf(curve, rows, dev) if curve is not None else None
        kept = self._kept = _StepBuffers(
            device=dev, rows=rowstats.shape[1] if rowstats is not None else rows, logits=logits,
            counts=_hip.mc_count_block(stat, C, dev),
            topk_counts=_hip.mc_count_block(topk, C, dev, valid=False) if topk is not None else None,
            rowstats=rowstats,
            epoch_buf=_hip._epoch_buf(dev, curve) if curve is not None else None,
        )
        return kept

    @staticmethod
    def build(collection) -> "Optional[_FusedMulticlassUpdatePlan]":
        from metrics_amd.ops import _hip

        stat = confmat = exact = curve = topk = None
        fuse_topk = _hip.fuse_topk_enabled()
        for members in collection._groups.values():
            leader = getattr(collection, members[0])
            kind = getattr(type(leader), "_hip_fused_kind", None)
            if kind is None or getattr(leader, "validate_args", True):
                continue  # validations are skipped on the fused path
            if kind == "mc_stat":
                if getattr(leader, "multidim_average", "global") != "global":
                    continue
                top_k = getattr(leader, "top_k", 1)
                if top_k == 1 and stat is None:
                    stat = leader
                elif top_k > 1 and topk is None and fuse_topk and leader.num_classes is not None:
                    topk = leader  # the first one; further top-k groups stay on their own
            elif kind == "mc_confmat" and confmat is None:
                confmat = leader
            elif kind == "mc_exact" and exact is None:
                if getattr(leader, "multidim_average", "global") == "global":
                    exact = leader
            elif kind == "mc_curve" and curve is None:
                import os

                if (
                    leader.thresholds is not None
                    and _hip.curve_kernels_cover(leader.thresholds.numel())
                    and getattr(leader, "average", None) != "micro"
                    and os.environ.get("METRICS_AMD_FUSE_CURVE", "1") != "0"
                ):
                    curve = leader
        if stat is None:
            return None
        if topk is not None and (topk.num_classes, topk.ignore_index) != (stat.num_classes, stat.ignore_index):
            topk = None  # counts other rows or classes: it updates on its own
        participants = [m for m in (stat, confmat, exact, curve, topk) if m is not None]
        if len(participants) < 2:
            return None
        ncs = {m.num_classes for m in participants}
        igs = {m.ignore_index for m in participants}
        if len(ncs) != 1 or len(igs) != 1:
            return None
        return _FusedMulticlassUpdatePlan(stat, confmat, exact, curve, topk)

    def try_run(self, *args: Any, **kwargs: Any) -> tuple:
        """Run the fused update if the inputs qualify; returns the handled
        leaders (empty tuple -> caller falls back to per-leader updates)."""
        if kwargs or len(args) != 2:
            return ()
        preds, target = args
        if not (isinstance(preds, Tensor) and isinstance(target, Tensor) and preds.is_cuda):
            return ()
        if target.ndim != 1:
            return ()
        if preds.is_floating_point():
            if preds.ndim != 2 or preds.dtype not in (torch.float32, torch.bfloat16):
                return ()
        elif preds.shape != target.shape:
            return ()
        from metrics_amd.ops import _hip

        if not _hip.hip_available():
            return ()
        stat, confmat, exact, curve, topk = self.stat, self.confmat, self.exact, self.curve, self.topk
        C, dev = stat.num_classes, preds.device
        # the top-k slot rides a step over float logits at a class count the
        # stat kernel's slot covers (the one-pass kernel covers no smaller one);
        # label preds: the curve leader can't ride the fused pass either
        bufs = self._step_buffers(_hip, dev, preds.shape[0], preds.is_floating_point())
        if bufs.epoch_buf is None:
            curve = None
        if bufs.topk_counts is None:
            topk = None
        # the participants of this step, by name: either path below gets them.
        # With a curve leader the pass also emits softmax row-stats + the epoch
        # flag, and the leader's own row-stats kernel is skipped.
        step = _hip.McStepTensors(
            counts=bufs.counts,
            confmat=confmat.confmat if confmat is not None else None,
            tp=stat.tp, fp=stat.fp, tn=stat.tn, fn=stat.fn,
            correct=exact.correct if exact is not None else None,
            total=exact.total if exact is not None else None,
            rowstats=bufs.rowstats, epoch_buf=bufs.epoch_buf,
        )
        if topk is not None:
            step = step._replace(topk_counts=bufs.topk_counts, tp_k=topk.tp, fp_k=topk.fp, tn_k=topk.tn, fn_k=topk.fn)
        k = topk.top_k if topk is not None else 0
        # one native call for the whole step, logits read once; False -> shape
        # not covered, nothing launched, keep the three launches below
        if curve is not None and self.onepass and _hip.mc_onepass_update(
            preds, target, C, stat.ignore_index, step, k, curve, self.onepass_force
        ):
            self.onepass_steps += 1
        else:
            rec = _hip.mc_step(C, stat.ignore_index, step, k)
            B = _hip.mc_step_count(rec, preds, target)
            if curve is not None:
                _hip.curve_hist_into_confmat(
                    preds, target, curve.thresholds, curve.ignore_index, curve.confmat,
                    mode=0, norm="softmax", owner=curve, stats_ready=True, skip_epoch_bump=True,
                )
            # the curve hist reads the epoch flag BEFORE it closes: the apply
            # launch goes behind the hist and its single block closes the epoch
            # for free (saves a dedicated ~4us bump dispatch per step)
            _hip.mc_step_apply(rec, B, close_epoch=curve is not None)
            _hip.mc_step_mark_mutated(step)
        handled = self.leaders if curve is not None else tuple(m for m in self.leaders if m is not self.curve)
        if topk is not None:
            self.topk_steps += 1
            handled = (*handled, topk)
        return handled


def _updates_as_marked(leader) -> bool:
    """True if ``leader`` updates through the ``update`` of the class that
    carries its ``_hip_fused_kind`` (a subclass with an update of its own is
    not what the fused kernels implement)."""
    for klass in type(leader).__mro__:
        if "_hip_fused_kind" in klass.__dict__:
            return type(leader).update is klass.update
    return False


class _FusedSpatialUpdatePlan:
    """Collection-level fusion for multiclass metrics fed (N, C, *spatial)
    predictions with an (N, *spatial) target (dense prediction): ONE native
    call of two launches (``csrc/mc_spatial.hip``) reads the predictions where
    they lie, without the transposed (N*S, C) copy every stand-alone update
    makes, and feeds the leaders of the stat-scores, confusion-matrix,
    exact-match and threshold-curve groups. It takes the leader kinds and the
    qualification rules of :class:`_FusedMulticlassUpdatePlan`, which declines
    such inputs; at least two participants, a stat leader is not required.
    ``METRICS_AMD_FUSE_SPATIAL=0`` builds no plan."""

    def __init__(self, stat, confmat, exact, curve):
        self.stat = stat
        self.confmat = confmat
        self.exact = exact
        self.curve = curve
        self.leaders = tuple(m for m in (stat, confmat, exact, curve) if m is not None)
        self.num_classes = self.leaders[0].num_classes
        self.ignore_index = self.leaders[0].ignore_index
        self.steps = 0
        self.curve_steps = 0

    @staticmethod
    def build(collection) -> "Optional[_FusedSpatialUpdatePlan]":
        from metrics_amd.ops import _hip

        if not _hip.fuse_spatial_enabled():
            return None
        found = {"mc_stat": None, "mc_confmat": None, "mc_exact": None, "mc_curve": None}
        for members in collection._groups.values():
            leader = getattr(collection, members[0])
            kind = getattr(type(leader), "_hip_fused_kind", None)
            if kind not in found or found[kind] is not None:
                continue  # the first leader of each kind; further groups stay on their own
            if getattr(leader, "validate_args", True) or not _updates_as_marked(leader):
                continue  # validations are skipped on the fused path
            if getattr(leader, "multidim_average", "global") != "global":
                continue
            if kind == "mc_stat" and (getattr(leader, "top_k", 1) != 1 or leader.num_classes is None):
                continue
            if kind == "mc_curve" and (
                leader.thresholds is None
                or not _hip.curve_kernels_cover(leader.thresholds.numel())
                or getattr(leader, "average", None) == "micro"
            ):
                continue
            found[kind] = leader
        stat, confmat, exact, curve = found["mc_stat"], found["mc_confmat"], found["mc_exact"], found["mc_curve"]
        participants = [m for m in (stat, confmat, exact, curve) if m is not None]
        if len(participants) < 2:
            return None
        if len({m.num_classes for m in participants}) != 1 or len({m.ignore_index for m in participants}) != 1:
            return None
        return _FusedSpatialUpdatePlan(stat, confmat, exact, curve)

    def try_run(self, *args: Any, **kwargs: Any) -> tuple:
        """Run the fused step if the inputs qualify; returns the handled leaders
        (empty tuple -> every leader updates on its own)."""
        if kwargs or len(args) != 2:
            return ()
        preds, target = args
        if not (isinstance(preds, Tensor) and isinstance(target, Tensor) and preds.is_cuda and target.is_cuda):
            return ()
        if preds.ndim < 3 or preds.dtype not in (torch.float32, torch.bfloat16) or not preds.is_contiguous():
            return ()
        C = self.num_classes
        if preds.shape[1] != C:
            return ()
        if target.dtype != torch.long or not target.is_contiguous() or target.device != preds.device:
            return ()
        if target.shape != (preds.shape[0], *preds.shape[2:]):
            return ()
        from metrics_amd.ops import _hip

        if not _hip.hip_available() or C > _hip.MC_SPATIAL_MAX_C:
            return ()
        stat, confmat, exact, curve = self.stat, self.confmat, self.exact, self.curve
        # above the LDS gate the curve leader updates on its own, the rest still fuses
        if curve is not None and not _hip.mc_spatial_curve_rides(C, curve.thresholds.numel()):
            curve = None
        handled = self.leaders if curve is self.curve else tuple(m for m in self.leaders if m is not self.curve)
        if len(handled) < 2:
            return ()
        if not _hip.mc_spatial_step_update(
            preds, target, C, self.ignore_index, stat=stat, confmat=confmat, exact=exact, curve=curve,
        ):
            return ()
        self.steps += 1
        if curve is not None:
            self.curve_steps += 1
        return handled


class _FusedMultilabelUpdatePlan:
    """Collection-level fusion for multilabel metrics: the leaders of the
    stat-scores, confusion-matrix, exact-match and threshold-curve groups all
    need the same per-element facts (label, ignored, ``x > cut``, bucket of the
    probability), so ONE native call of two launches (``csrc/ml_step.hip``)
    reads the (N, L) predictions and the int64 targets once and feeds all of
    them. At least two participants; a stat leader is not required.

    Inside a plan the confusion-matrix and exact-match leaders threshold with
    the exact rule of the stat kernel (``x > logit(threshold)`` when the batch
    is normalised) instead of comparing a rounded ``sigmoid(x)``: see
    docs/PARITY.md. ``METRICS_AMD_FUSE_MULTILABEL=0`` builds no plan."""

    def __init__(self, stat, confmat, exact, curve):
        self.stat = stat
        self.confmat = confmat
        self.exact = exact
        self.curve = curve
        self.leaders = tuple(m for m in (stat, confmat, exact, curve) if m is not None)
        self.num_labels = self.leaders[0].num_labels
        self.ignore_index = self.leaders[0].ignore_index
        # two participants and one curve leader at most: one of these exists
        self.threshold = next(m.threshold for m in (stat, confmat, exact) if m is not None)
        self.steps = 0
        self.curve_steps = 0

    @staticmethod
    def build(collection) -> "Optional[_FusedMultilabelUpdatePlan]":
        from metrics_amd.ops import _hip

        if not _hip.fuse_multilabel_enabled():
            return None
        found = {"ml_stat": None, "ml_confmat": None, "ml_exact": None, "ml_curve": None}
        for members in collection._groups.values():
            leader = getattr(collection, members[0])
            kind = getattr(type(leader), "_hip_fused_kind", None)
            if kind not in found or found[kind] is not None:
                continue  # the first leader of each kind; further groups stay on their own
            if getattr(leader, "validate_args", True) or not _updates_as_marked(leader):
                continue  # validations are skipped on the fused path
            if getattr(leader, "multidim_average", "global") != "global":
                continue
            if kind == "ml_curve" and leader.thresholds is None:
                continue
            found[kind] = leader
        stat, confmat, exact, curve = found["ml_stat"], found["ml_confmat"], found["ml_exact"], found["ml_curve"]
        participants = [m for m in (stat, confmat, exact, curve) if m is not None]
        if len(participants) < 2:
            return None
        if len({m.num_labels for m in participants}) != 1 or len({m.ignore_index for m in participants}) != 1:
            return None
        if len({float(m.threshold) for m in (stat, confmat, exact) if m is not None}) > 1:
            return None
        return _FusedMultilabelUpdatePlan(stat, confmat, exact, curve)

    def try_run(self, *args: Any, **kwargs: Any) -> tuple:
        """Run the fused step if the inputs qualify; returns the handled leaders
        (empty tuple -> every leader updates on its own)."""
        if kwargs or len(args) != 2:
            return ()
        preds, target = args
        if not (isinstance(preds, Tensor) and isinstance(target, Tensor) and preds.is_cuda and target.is_cuda):
            return ()
        if preds.ndim != 2 or preds.dtype not in (torch.float32, torch.bfloat16) or not preds.is_contiguous():
            return ()
        if target.dtype != torch.long or target.shape != preds.shape or not target.is_contiguous():
            return ()
        if preds.shape[1] != self.num_labels or target.device != preds.device:
            return ()
        from metrics_amd.ops import _hip

        if not _hip.hip_available():
            return ()
        stat, confmat, exact, curve = self.stat, self.confmat, self.exact, self.curve
        # above the LDS gate the curve leader updates on its own, the rest still fuses
        if curve is not None and curve.thresholds.numel() > _hip.ML_STEP_MAX_T:
            curve = None
        handled = self.leaders if curve is self.curve else tuple(m for m in self.leaders if m is not self.curve)
        if len(handled) < 2:
            return ()
        if not _hip.ml_step_update(
            preds, target, self.num_labels, self.ignore_index, self.threshold,
            stat=stat, confmat=confmat, exact=exact, curve=curve,
        ):
            return ()
        self.steps += 1
        if curve is not None:
            self.curve_steps += 1
        return handled


class _FusedBinaryUpdatePlan:
    """Collection-level fusion for binary metrics: the leaders of the
    stat-scores, confusion-matrix and threshold-curve groups all need the same
    per-element facts (label, ignored, ``x > cut``, bucket of the probability),
    so ONE native call of two launches (``csrc/bin_step.hip``) reads the
    predictions and the int64 targets once, as a flat stream, and feeds all of
    them. At least two participants; a stat leader is not required.

    The groups keep their own normalisation decisions (stat: any element
    outside [0, 1]; confusion matrix and curve: any element that is not
    ignored). Inside a plan the confusion-matrix leader thresholds with the
    exact rule of the stat kernel (``x > logit(threshold)`` when the batch is
    normalised) instead of comparing a rounded ``sigmoid(x)``: see
    docs/PARITY.md. ``METRICS_AMD_FUSE_BINARY=0`` builds no plan."""

    def __init__(self, stat, confmat, curve):
        self.stat = stat
        self.confmat = confmat
        self.curve = curve
        self.leaders = tuple(m for m in (stat, confmat, curve) if m is not None)
        self.ignore_index = self.leaders[0].ignore_index
        # two participants and one curve leader at most: one of these exists
        self.threshold = next(m.threshold for m in (stat, confmat) if m is not None)
        self.steps = 0
        self.curve_steps = 0

    @staticmethod
    def build(collection) -> "Optional[_FusedBinaryUpdatePlan]":
        from metrics_amd.ops import _hip

        if not _hip.fuse_binary_enabled():
            return None
        found = {"bin_stat": None, "bin_confmat": None, "bin_curve": None}
        for members in collection._groups.values():
            leader = getattr(collection, members[0])
            kind = getattr(type(leader), "_hip_fused_kind", None)
            if kind not in found or found[kind] is not None:
                continue  # the first leader of each kind; further groups stay on their own
            if getattr(leader, "validate_args", True) or not _updates_as_marked(leader):
                continue  # validations are skipped on the fused path
            if getattr(leader, "multidim_average", "global") != "global":
                continue
            if kind == "bin_curve" and leader.thresholds is None:
                continue
            found[kind] = leader
        stat, confmat, curve = found["bin_stat"], found["bin_confmat"], found["bin_curve"]
        participants = [m for m in (stat, confmat, curve) if m is not None]
        if len(participants) < 2:
            return None
        if len({m.ignore_index for m in participants}) != 1:
            return None
        if len({float(m.threshold) for m in (stat, confmat) if m is not None}) > 1:
            return None
        return _FusedBinaryUpdatePlan(stat, confmat, curve)

    def try_run(self, *args: Any, **kwargs: Any) -> tuple:
        """Run the fused step if the inputs qualify; returns the handled leaders
        (empty tuple -> every leader updates on its own)."""
        if kwargs or len(args) != 2:
            return ()
        preds, target = args
        if not (isinstance(preds, Tensor) and isinstance(target, Tensor) and preds.is_cuda and target.is_cuda):
            return ()
        if preds.dtype not in (torch.float32, torch.bfloat16) or not preds.is_contiguous():
            return ()
        if target.dtype != torch.long or target.shape != preds.shape or not target.is_contiguous():
            return ()
        if target.device != preds.device:
            return ()
        from metrics_amd.ops import _hip

        if not _hip.hip_available():
            return ()
        stat, confmat, curve = self.stat, self.confmat, self.curve
        # above the LDS gate the curve leader updates on its own, the rest still fuses
        if curve is not None and curve.thresholds.numel() > _hip.BIN_STEP_MAX_T:
            curve = None
        handled = self.leaders if curve is self.curve else tuple(m for m in self.leaders if m is not self.curve)
        if len(handled) < 2:
            return ()
        if not _hip.bin_step_update(
            preds, target, self.ignore_index, self.threshold, stat=stat, confmat=confmat, curve=curve,
        ):
            return ()
        self.steps += 1
        if curve is not None:
            self.curve_steps += 1
        return handled


class _FusedRankingUpdatePlan:
    """Collection-level fusion for the multilabel ranking metrics: coverage
    error, ranking average precision and ranking loss all come from the same
    per-row counts, so ONE native call of two launches (``csrc/ml_rank.hip``)
    with the combined ``want`` mask reads the scores and the int64 targets once
    and adds into the states of every leader. At least two leaders.

    The plan is additive: its leaders are of a kind no other plan takes, so it
    runs whether or not another plan handled the step, and a multilabel
    collection with stat, curve and ranking members takes one ``ml_step`` call
    and one ranking call. ``METRICS_AMD_RANKING_KERNEL=0`` builds no plan."""

    def __init__(self, leaders):
        self.leaders = tuple(leaders)
        self.num_labels = self.leaders[0].num_labels
        self.ignore_index = self.leaders[0].ignore_index
        self.steps = 0

    @staticmethod
    def build(collection) -> "Optional[_FusedRankingUpdatePlan]":
        from metrics_amd.ops import _hip

        if not _hip.ranking_kernel_enabled():
            return None
        found: Dict[str, Any] = {}
        for members in collection._groups.values():
            leader = getattr(collection, members[0])
            if getattr(type(leader), "_hip_fused_kind", None) != "ml_rank":
                continue
            measure = getattr(type(leader), "_rank_measure", None)
            if measure is None or measure in found:
                continue  # the first leader of each measure; further groups stay on their own
            if getattr(leader, "validate_args", True) or not _updates_as_marked(leader):
                continue  # validations are skipped on the fused path
            found[measure] = leader
        leaders = list(found.values())
        if len(leaders) < 2:
            return None
        if len({m.num_labels for m in leaders}) != 1 or len({m.ignore_index for m in leaders}) != 1:
            return None
        return _FusedRankingUpdatePlan(leaders)

    def try_run(self, *args: Any, **kwargs: Any) -> tuple:
        """Run the fused call if the inputs qualify; returns the handled leaders
        (empty tuple -> every leader updates on its own)."""
        if kwargs or len(args) != 2:
            return ()
        preds, target = args
        if not (isinstance(preds, Tensor) and isinstance(target, Tensor) and preds.is_cuda and target.is_cuda):
            return ()
        if preds.ndim != 2 or preds.dtype not in (torch.float32, torch.bfloat16) or not preds.is_contiguous():
            return ()
        if target.dtype != torch.long or target.shape != preds.shape or not target.is_contiguous():
            return ()
        if preds.shape[1] != self.num_labels or target.device != preds.device:
            return ()
        from metrics_amd.functional.classification.ranking import _ranking_kernel_inputs
        from metrics_amd.ops import _hip

        if not _hip.hip_available():
            return ()
        inputs = _ranking_kernel_inputs(preds, target, self.num_labels)
        if inputs is None:
            return ()
        pairs = {type(m)._rank_measure: (m.measure, m.total) for m in self.leaders}
        if not _hip.ml_ranking_into(inputs[0], inputs[1], self.ignore_index, owner=self.leaders[0], **pairs):
            return ()
        self.steps += 1
        return self.leaders


class _FusedMulticlassComputePlan:
    """Collection-level compute: every member that declares what it computes
    (``Metric._compute_plan_spec``) over the stat-scores, confusion-matrix,
    exact-match or threshold-curve group gets its result from ONE native call
    of at most three launches (``csrc/mc_compute.hip``) instead of one Python
    wrapper, cache lookup, allocation and launch per metric. The step also
    performs the curve leader's lazy flush. Members it does not cover compute
    on their own, as before."""

    _STATES = {
        "linear": ("tp", "fp", "tn", "fn"),
        "confmat_scalar": ("confmat",),
        "exact": ("correct", "total"),
        "curve_auc": ("confmat",),
    }

    def __init__(self, leaders, members):
        # kind -> leader metric; (metric, kind, spec, slot) per covered member:
        # slot = index into the step's `out` buffer (curve: unused)
        self.leaders = leaders
        self.members = members
        self.formulas = [p for m, kind, spec, _ in members if kind == "linear"
                         for p in spec[1].params(spec[2])]
        self.native = None
        self.steps = 0

    @classmethod
    def build(cls, collection) -> "Optional[_FusedMulticlassComputePlan]":
        leaders: dict = {}
        covered: list = []
        for names in collection._groups.values():
            group = [getattr(collection, n) for n in names]
            specs = [m._compute_plan_spec() for m in group]
            kinds = {s[0] for s in specs if s is not None}
            # one kind per group (its members share states) and one group per
            # kind; whatever is left computes on its own
            if len(kinds) != 1 or next(iter(kinds)) in leaders:
                continue
            leaders[kinds.pop()] = group[0]
            covered += [(m, s) for m, s in zip(group, specs) if s is not None]
        if not covered:
            return None
        # out = [linear 0..n-1 | mcc, kappa, jaccard | exact]
        n_linear = sum(1 for _, s in covered if s[0] == "linear")
        members, nxt = [], 0
        for m, spec in covered:
            kind = spec[0]
            if kind == "linear":
                slot, nxt = nxt, nxt + 1
            elif kind == "confmat_scalar":
                slot = n_linear + spec[1]
            else:
                slot = n_linear + 3
            members.append((m, kind, spec, slot))
        return cls(leaders, members)

    def _state_tensors(self, _hip):
        """The leaders' state tensors as the native plan's ``ComputeStates``, or
        None if a state is not a tensor (list states)."""
        out = {}
        for kind, leader in self.leaders.items():
            for name in self._STATES[kind]:
                t = getattr(leader, name)
                if not isinstance(t, Tensor):
                    return None
                # both the confusion-matrix and the curve group call their state "confmat"
                out["curve_state" if kind == "curve_auc" else name] = t
        curve = self.leaders.get("curve_auc")
        if curve is not None:
            out["hist"] = curve.__dict__.get("_hip_hist_buf")
        return _hip.ComputeStates(**out)

    def _build_native(self, states):
        """A native plan over ``states``, or None if they do not fit one plan."""
        from metrics_amd.ops import _hip

        tp, confmat, curve_state, hist = states.tp, states.confmat, states.curve_state, states.hist
        present = [t for t in states if t is not None]
        dev = present[0].device
        if not all(t.is_cuda and t.device == dev and t.is_contiguous() and t.dtype == torch.long for t in present):
            return None
        sizes = set()
        if tp is not None:
            if tp.ndim != 1 or not (tp.shape == states.fp.shape == states.tn.shape == states.fn.shape):
                return None
            sizes.add(tp.numel())
        if confmat is not None:
            if confmat.ndim != 2 or confmat.shape[0] != confmat.shape[1]:
                return None
            sizes.add(confmat.shape[0])
        if states.correct is not None and (states.correct.numel() != 1 or states.total.numel() != 1):
            return None
        T = 1
        if curve_state is not None:
            if curve_state.ndim != 4 or curve_state.shape[2:] != (2, 2):
                return None
            T, c = curve_state.shape[0], curve_state.shape[1]
            if not _hip.curve_kernels_cover(T) or (hist is not None and hist.shape != (c, T + 1, 2)):
                return None
            sizes.add(c)
        if len(sizes) > 1:
            return None
        C = sizes.pop() if sizes else 1
        return _hip._ComputePlan(dev, C, T, states, self.formulas, 0.0)

    def try_run(self) -> bool:
        """Fill ``_computed`` of every covered member that has no cached result.
        False: nothing was launched and nothing changed, the caller computes
        every member as before."""
        from metrics_amd.ops import _hip

        if not (_hip.compute_plan_enabled() and _hip.hip_available()) or tracing.is_enabled():
            return False
        tensors = self._state_tensors(_hip)
        if tensors is None:
            return False
        todo = []
        dist: dict = {}  # distributed_available_fn -> its answer, asked once
        for m, kind, spec, slot in self.members:
            # every fast-path condition of Metric._wrap_compute; a member that
            # wants a sync sends the whole collection down the old path
            if m._is_synced or m.__dict__.get("_pending_sync_event") is not None:
                return False
            if m._to_sync:
                fn = m.distributed_available_fn
                if fn not in dist:
                    dist[fn] = fn()
                if dist[fn]:
                    return False
            if m._computed is not None or not m.compute_with_cache:
                continue
            leader = self.leaders[kind]
            if m is not leader and not all(
                getattr(m, name) is getattr(leader, name) for name in self._STATES[kind]
            ):
                continue  # not an alias of the leader's states: computes on its own
            todo.append((m, kind, spec, slot))
        if not todo:
            return True
        native = self.native
        if native is None or not native.fits(tensors):
            native = self.native = self._build_native(tensors)
            if native is None:
                return False
        curve = self.leaders.get("curve_auc")
        flush = False
        if curve is not None and curve.__dict__.get("_lazy_dirty"):
            T, C = tensors.curve_state.shape[:2]
            if curve.__dict__.get("_hip_lazy_meta") != (C, T, 1) or tensors.hist is None:
                return False
            curve.__dict__["_lazy_dirty"] = False  # the step is the flush
            flush = True
        # a histogram the one-pass step left in pending format is completed by the same call
        out, auc = native.step(flush, _hip.take_b0_pending(curve) if flush else None)
        self.steps += 1
        vals = out.unbind(0)
        for m, kind, spec, slot in todo:
            if kind == "curve_auc":
                mode = spec[1]
                m._computed = _reduce_curve_auc(auc[2 * mode], auc[2 * mode + 1], spec[2])  # fresh tensor
            else:
                m._computed = vals[slot]
        return True


class MetricCollection(ModuleDict):
    """A dict-like container of metrics sharing one ``update``/``compute`` call pattern.

    Args:
        metrics: a single Metric, a sequence of Metrics (keyed by class name),
            or a dict name->Metric (keys sorted alphabetically). Nested
            ``MetricCollection`` inputs are flattened.
        additional_metrics: further metrics when ``metrics`` is not a dict.
        prefix / postfix: strings pre/appended to every output key.
        compute_groups: True (auto-detect groups after the first update),
            False (disable), or an explicit list of lists of metric names.
    """

    _modules: Dict[str, Metric]  # type: ignore[assignment]

    def __init__(
        self,
        metrics: Union[Metric, Sequence[Metric], Dict[str, Metric]],
        *additional_metrics: Metric,
        prefix: Optional[str] = None,
        postfix: Optional[str] = None,
        compute_groups: Union[bool, List[List[str]]] = True,
    ) -> None:
        super().__init__()
        self._fused_plan: Any = False
        self._fused_ml_plan: Any = False
        self._fused_bin_plan: Any = False
        self._fused_rank_plan: Any = False
        self._fused_sp_plan: Any = False
        self._compute_plan: Any = False
        self.prefix = self._check_arg(prefix, "prefix")
        self.postfix = self._check_arg(postfix, "postfix")
        self._enable_compute_groups = compute_groups
        self._groups_checked: bool = False
        self._state_is_copy: bool = False

        self.add_metrics(metrics, *additional_metrics)

    # ------------------------------------------------------------------ calls
    @property
    def metric_state(self) -> Dict[str, Dict[str, Any]]:
        """States of every metric in the collection."""
        return {k: m.metric_state for k, m in self.items(keep_base=False, copy_state=False)}

    @torch.jit.unused
    def forward(self, *args: Any, **kwargs: Any) -> Dict[str, Any]:
        """Call forward on every metric; kwargs are routed per-metric by update signature."""
        return self._compute_and_reduce("forward", *args, **kwargs)

    def update(self, *args: Any, **kwargs: Any) -> None:
        """Call update on every metric (or only group leaders once groups are formed)."""
        if self._groups_checked:
            # invalidate cached compute results on ALL members; straight from
            # the module dict: a Module attribute lookup per member and step
            # costs more than everything else in this loop
            modules = self._modules
            for m in modules.values():
                m._computed = None
            if self._fused_plan is False:
                self._fused_plan = _FusedMulticlassUpdatePlan.build(self)
            fused_done: tuple = ()
            if self._fused_plan is not None:
                with tracing.range("MetricCollection.fused_update"):
                    fused_done = self._fused_plan.try_run(*args, **kwargs)
            # the spatial plan takes the (N, C, *spatial) inputs the plan above
            # declines, for the same leader kinds; built by the first step that
            # plan did not handle
            if not fused_done:
                if self._fused_sp_plan is False:
                    self._fused_sp_plan = _FusedSpatialUpdatePlan.build(self)
                if self._fused_sp_plan is not None:
                    with tracing.range("MetricCollection.fused_spatial_update"):
                        fused_done = self._fused_sp_plan.try_run(*args, **kwargs)
            # the multilabel plan: its leaders are of other kinds, so a
            # collection runs at most one of the two
            if self._fused_ml_plan is False:
                self._fused_ml_plan = _FusedMultilabelUpdatePlan.build(self)
            if self._fused_ml_plan is not None and not fused_done:
                with tracing.range("MetricCollection.fused_ml_update"):
                    fused_done = self._fused_ml_plan.try_run(*args, **kwargs)
            # the binary plan, likewise of kinds of its own; built by the first
            # step neither other plan handled
            if not fused_done:
                if self._fused_bin_plan is False:
                    self._fused_bin_plan = _FusedBinaryUpdatePlan.build(self)
                if self._fused_bin_plan is not None:
                    with tracing.range("MetricCollection.fused_bin_update"):
                        fused_done = self._fused_bin_plan.try_run(*args, **kwargs)
            # the ranking plan is additive: its leaders are of a kind none of
            # the plans above takes, so it runs next to whichever of them ran
            if self._fused_rank_plan is False:
                self._fused_rank_plan = _FusedRankingUpdatePlan.build(self)
            if self._fused_rank_plan is not None:
                with tracing.range("MetricCollection.fused_rank_update"):
                    fused_done = (*fused_done, *self._fused_rank_plan.try_run(*args, **kwargs))
            # run only each group's leader
            # identity check: Metric.__eq__ is the compositional operator
            # (returns a CompositionalMetric, which is always truthy)
            done_ids = set(map(id, fused_done)) if fused_done else ()
            for members in self._groups.values():
                leader = modules[members[0]]
                if id(leader) in done_ids:
                    leader._update_count += 1
                    continue
                leader.update(*args, **leader._filter_kwargs(**kwargs))
            if self._state_is_copy:
                # re-establish the alias links broken by a copy-on-access
                self._compute_groups_create_state_ref()
                self._state_is_copy = False
            return

        # first update: run every metric, then detect groups from equal states
        for m in self.values(copy_state=False):
            m.update(*args, **m._filter_kwargs(**kwargs))
        if self._enable_compute_groups:
            # group detection compares state VALUES: lazily-accumulated curve
            # histograms would leave every curve confmat at zero and merge
            # unrelated metrics — materialize first
            for m in self.values(copy_state=False):
                m._maybe_flush_lazy()
            self._merge_compute_groups()
            self._compute_groups_create_state_ref()
            self._groups_checked = True

    def compute(self) -> Dict[str, Any]:
        """Compute the result of every metric; one state sync per compute group."""
        return self._compute_and_reduce("compute")

    def _compute_and_reduce(self, method_name: str, *args: Any, **kwargs: Any) -> Dict[str, Any]:
        if method_name == "compute" and self._groups_checked and not self._state_is_copy:
            # one native call for every member that declared what it computes;
            # their results land in `_computed`, which the loop below returns
            if self._compute_plan is False:
                self._compute_plan = _FusedMulticlassComputePlan.build(self)
            if self._compute_plan is not None:
                self._compute_plan.try_run()
        # lazy curve histograms live on group LEADERS; members alias the
        # leader's states and may compute first — materialize before iterating
        if self._groups_checked:
            for members in self._groups.values():
                getattr(self, members[0])._maybe_flush_lazy()
        result = {}
        for k, m in self.items(keep_base=True, copy_state=False):
            if method_name == "compute":
                result[k] = m.compute()
            elif method_name == "forward":
                result[k] = m(*args, **m._filter_kwargs(**kwargs))
            else:
                raise ValueError(f"method_name should be either 'compute' or 'forward', but got {method_name}")

        _, duplicates = _flatten_dict(result)

        flat: Dict[str, Any] = {}
        for k, m in self._modules.items():  # states were linked for the loop above
            res = result[k]
            if isinstance(res, dict):
                for key, v in res.items():
                    if duplicates:
                        base_k = _strip_prefix(k, getattr(m, "prefix", None) or "")
                        base_k = _strip_suffix(base_k, getattr(m, "postfix", None) or "")
                        key = f"{base_k}_{key}"
                    if getattr(m, "_from_collection", None) and m.prefix is not None:
                        key = f"{m.prefix}{key}"
                    if getattr(m, "_from_collection", None) and m.postfix is not None:
                        key = f"{key}{m.postfix}"
                    flat[key] = v
            else:
                flat[k] = res
        return {self._set_name(k): v for k, v in flat.items()}

    def reset(self) -> None:
        """Reset every metric."""
        for m in self.values(copy_state=False):
            m.reset()
        if self._enable_compute_groups and self._groups_checked:
            # resets allocate fresh default tensors: re-link group members
            self._compute_groups_create_state_ref()

    # ---------------------------------------------------------- compute groups
    def _merge_compute_groups(self) -> None:
        """Merge groups whose (leader) states compare equal, until a fixed point."""
        merged = True
        while merged:
            merged = False
            ids = list(self._groups.keys())
            for i in ids:
                if i not in self._groups:
                    continue
                for j in ids:
                    if j == i or j not in self._groups:
                        continue
                    m_i = getattr(self, self._groups[i][0])
                    m_j = getattr(self, self._groups[j][0])
                    if self._equal_metric_states(m_i, m_j):
                        self._groups[i].extend(self._groups.pop(j))
                        merged = True
        # re-index 0..n-1
        self._groups = {idx: members for idx, members in enumerate(self._groups.values())}

    @staticmethod
    def _equal_metric_states(metric1: Metric, metric2: Metric) -> bool:
        """True if two metrics hold state that is equal in keys, shapes and values."""
        if len(metric1._defaults) == 0 or len(metric2._defaults) == 0:
            return False
        if metric1._defaults.keys() != metric2._defaults.keys():
            return False
        for key in metric1._defaults:
            s1, s2 = getattr(metric1, key), getattr(metric2, key)
            if type(s1) is not type(s2):
                return False
            if isinstance(s1, Tensor):
                if s1.shape != s2.shape or not allclose(s1, s2):
                    return False
            elif isinstance(s1, list):
                if len(s1) != len(s2):
                    return False
                if not all(a.shape == b.shape and allclose(a, b) for a, b in zip(s1, s2)):
                    return False
        return True

    def _compute_groups_create_state_ref(self, copy: bool = False) -> None:
        """Alias (or deep-copy) the leader's states onto every group member."""
        if copy:
            for members in self._groups.values():
                getattr(self, members[0])._maybe_flush_lazy()
        if not self._state_is_copy:
            modules = self._modules  # getattr(self, name) without Module.__getattr__
            for members in self._groups.values():
                leader = modules[members[0]]
                for name in members[1:]:
                    member = modules[name]
                    for state in leader._defaults:
                        leader_state = getattr(leader, state)
                        if copy:
                            setattr(member, state, deepcopy(leader_state))
                        elif getattr(member, state) is not leader_state:
                            # already linked is the steady state of every compute();
                            # a Module setattr costs ten times the check
                            setattr(member, state, leader_state)
                    if copy or member._update_count != leader._update_count:
                        member._update_count = deepcopy(leader._update_count) if copy else leader._update_count
        self._state_is_copy = copy

    @property
    def compute_groups(self) -> Dict[int, List[str]]:
        """The current compute groups (group index -> member names)."""
        return self._groups

    # ------------------------------------------------------------- management
    def add_metrics(
        self, metrics: Union[Metric, Sequence[Metric], Dict[str, Metric]], *additional_metrics: Metric
    ) -> None:
        """Add metrics to the collection."""
        if isinstance(metrics, Metric):
            metrics = [metrics]
        if isinstance(metrics, Sequence):
            metrics = list(metrics)
            remain: list = []
            for m in additional_metrics:
                (metrics if isinstance(m, (Metric, MetricCollection)) else remain).append(m)
            if remain:
                rank_zero_warn(
                    f"You have passed extra arguments {remain} which are not `Metric` so they will be ignored."
                )
        elif additional_metrics:
            raise ValueError(
                f"You have passed extra arguments {additional_metrics} which are not compatible"
                f" with first passed dictionary {metrics} so they will be ignored."
            )

        if isinstance(metrics, dict):
            for name in sorted(metrics.keys()):
                metric = metrics[name]
                if not isinstance(metric, (Metric, MetricCollection)):
                    raise ValueError(
                        f"Value {metric} belonging to key {name} is not an instance of"
                        " `metrics_amd.Metric` or `metrics_amd.MetricCollection`"
                    )
                if isinstance(metric, Metric):
                    self[name] = metric
                else:  # flatten a nested collection, carrying its renaming
                    for k, v in metric.items(keep_base=False):
                        v.postfix = metric.postfix
                        v.prefix = metric.prefix
                        v._from_collection = True
                        self[f"{name}_{k}"] = v
        elif isinstance(metrics, Sequence):
            for metric in metrics:
                if not isinstance(metric, (Metric, MetricCollection)):
                    raise ValueError(
                        f"Input {metric} to `MetricCollection` is not a instance of"
                        " `metrics_amd.Metric` or `metrics_amd.MetricCollection`"
                    )
                if isinstance(metric, Metric):
                    name = metric.__class__.__name__
                    if name in self:
                        raise ValueError(f"Encountered two metrics both named {name}")
                    self[name] = metric
                else:
                    for k, v in metric.items(keep_base=False):
                        v.postfix = metric.postfix
                        v.prefix = metric.prefix
                        v._from_collection = True
                        self[k] = v
        else:
            raise ValueError(
                "Unknown input to MetricCollection. Expected `Metric`, `MetricCollection` or `dict`/`sequence` of the"
                f" previous, but got {metrics}"
            )

        self._groups_checked = False
        self._compute_plan = False
        if self._enable_compute_groups:
            self._init_compute_groups()
        else:
            self._groups = {}

    def _init_compute_groups(self) -> None:
        if isinstance(self._enable_compute_groups, list):
            self._groups = dict(enumerate(self._enable_compute_groups))
            for members in self._groups.values():
                for metric in members:
                    if metric not in self:
                        raise ValueError(
                            f"Input {metric} in `compute_groups` argument does not match a metric in the collection."
                            f" Please make sure that {self._enable_compute_groups} matches {self.keys(keep_base=True)}"
                        )
            self._groups_checked = True
        else:
            self._groups = {i: [str(k)] for i, k in enumerate(self.keys(keep_base=True))}

    def clone(self, prefix: Optional[str] = None, postfix: Optional[str] = None) -> "MetricCollection":
        """Deep copy of the collection, optionally re-keyed."""
        mc = deepcopy(self)
        if prefix:
            mc.prefix = self._check_arg(prefix, "prefix")
        if postfix:
            mc.postfix = self._check_arg(postfix, "postfix")
        return mc

    def persistent(self, mode: bool = True) -> None:
        """Toggle state persistence on every metric."""
        for m in self.values(copy_state=False):
            m.persistent(mode)

    def set_dtype(self, dst_type: Union[str, torch.dtype]) -> "MetricCollection":
        """Cast the states of every metric."""
        for m in self.values(copy_state=False):
            m.set_dtype(dst_type)
        return self

    # ------------------------------------------------------------- dict-style
    def _set_name(self, base: str) -> str:
        name = base if self.prefix is None else self.prefix + base
        return name if self.postfix is None else name + self.postfix

    def _to_renamed_dict(self) -> Mapping[str, Metric]:
        out = OrderedDict()
        for k, v in self._modules.items():
            out[self._set_name(k)] = v
        return out

    def __iter__(self) -> Iterator[Hashable]:
        return iter(self.keys())

    def keys(self, keep_base: bool = False) -> Iterable[Hashable]:
        """Keys, with prefix/postfix applied unless ``keep_base``."""
        if keep_base:
            return self._modules.keys()
        return self._to_renamed_dict().keys()

    def items(self, keep_base: bool = False, copy_state: bool = True) -> Iterable[Tuple[str, Metric]]:
        """(key, metric) pairs; by default breaks group-state aliasing via copies."""
        self._compute_groups_create_state_ref(copy_state)
        if keep_base:
            return self._modules.items()
        return self._to_renamed_dict().items()

    def values(self, copy_state: bool = True) -> Iterable[Metric]:
        """Metrics; by default breaks group-state aliasing via copies."""
        self._compute_groups_create_state_ref(copy_state)
        return self._modules.values()

    def __getitem__(self, key: str, copy_state: bool = True) -> Metric:
        """Look up a single metric (prefix/postfix-stripped key)."""
        self._compute_groups_create_state_ref(copy_state)
        if self.prefix:
            key = _strip_prefix(key, self.prefix)
        if self.postfix:
            key = _strip_suffix(key, self.postfix)
        return self._modules[key]

    @staticmethod
    def _check_arg(arg: Optional[str], name: str) -> Optional[str]:
        if arg is None or isinstance(arg, str):
            return arg
        raise ValueError(f"Expected input `{name}` to be a string, but got {type(arg)}")

    def __repr__(self) -> str:
        repr_str = super().__repr__()[:-2]
        if self.prefix:
            repr_str += f",\n  prefix={self.prefix}{',' if self.postfix else ''}"
        if self.postfix:
            repr_str += f"{',' if not self.prefix else ''}\n  postfix={self.postfix}"
        return repr_str + "\n)"

    def plot(
        self,
        val: Optional[Union[dict, Sequence[dict]]] = None,
        ax: Optional[Any] = None,
        together: bool = False,
    ) -> Sequence[Any]:
        """Plot all metric values — one axis per metric, or all in one if ``together``."""
        from metrics_amd.utilities.plot import plot_single_or_multi_val

        if not isinstance(together, bool):
            raise ValueError(f"Expected argument `together` to be a boolean, but got {type(together)}")
        val = val or self.compute()
        if together:
            return plot_single_or_multi_val(val, ax=ax)
        fig_axs = []
        for i, (k, m) in enumerate(self.items(keep_base=False, copy_state=False)):
            if isinstance(val, dict):
                f, a = m.plot(val[k], ax=ax[i] if ax is not None else ax)
            elif isinstance(val, Sequence):
                f, a = m.plot([v[k] for v in val], ax=ax[i] if ax is not None else ax)
            else:
                raise ValueError(f"Unsupported value type for plotting: {type(val)}")
            fig_axs.append((f, a))
        return fig_axs
