"""Multilabel ranking metrics. Parity: torchmetrics ``functional/classification/ranking.py``."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from metrics_amd.functional.classification.confusion_matrix import (
    _multilabel_confusion_matrix_arg_validation,
    _multilabel_confusion_matrix_format,
)
from metrics_amd.functional.classification.stat_scores import _multilabel_stat_scores_tensor_validation
from metrics_amd.utilities.compute import normalize_logits_if_needed

# `want` bits of the ranking kernel (csrc/ml_rank.hip, ops/_hip.py RANK_WANT_*)
_WANT_COVERAGE, _WANT_LRAP, _WANT_LOSS = 1, 2, 4


def _rank_data(x: Tensor) -> Tensor:
    """Rank of each element (1 = smallest); ties get the same (min-style) rank via unique inverse."""
    _, inverse, counts = torch.unique(x, sorted=True, return_inverse=True, return_counts=True)
    ranks = counts.cumsum(dim=0)
    return ranks[inverse]


def _multilabel_ranking_format(
    preds: Tensor,
    target: Tensor,
    num_labels: int,
    ignore_index: Optional[int] = None,
) -> Tuple[Tensor, Tensor]:
    preds, target = _multilabel_confusion_matrix_format(
        preds, target, num_labels, threshold=0.0, ignore_index=ignore_index, should_threshold=False
    )
    return preds, target


def _ranking_kernel_inputs(preds: Tensor, target: Tensor, num_labels: int) -> Optional[Tuple[Tensor, Tensor]]:
    """The normalised (N, L) scores and the int64 targets as the gfx950 kernel
    (csrc/ml_rank.hip) reads them, or None where the torch path below runs: CPU
    tensors, fp64 or integer predictions, more labels than the kernel stages,
    ``METRICS_AMD_RANKING_KERNEL=0``. No host sync, no clone for ``ignore_index``
    (the kernel applies it). The sigmoid runs here, in the input dtype and over
    the whole tensor, exactly as ``_multilabel_ranking_format`` decides it, so
    the kernel sees the ties the torch path sees; fp16 is widened afterwards,
    which is exact."""
    if not (preds.is_cuda and target.is_cuda and target.device == preds.device):
        return None
    if preds.dtype not in (torch.float32, torch.bfloat16, torch.float16) or target.is_floating_point():
        return None
    if preds.ndim < 2 or preds.shape != target.shape or preds.shape[1] != num_labels or preds.numel() == 0:
        return None
    from metrics_amd.ops import _hip

    if not _hip.ranking_kernel_enabled() or num_labels > _hip.ML_RANK_MAX_L:
        return None
    scores = normalize_logits_if_needed(preds, "sigmoid")
    if scores.dtype == torch.float16:
        scores = scores.float()
    if scores.ndim > 2:
        scores = scores.movedim(1, -1).reshape(-1, num_labels)
        target = target.movedim(1, -1).reshape(-1, num_labels)
    return scores.contiguous(), target.long().contiguous()


def _ranking_kernel_sums(
    preds: Tensor, target: Tensor, num_labels: int, ignore_index: Optional[int], want: int
) -> Optional[Tensor]:
    """(measure, total) of the one measure ``want`` names, from the kernel, or
    None where the torch path runs."""
    inputs = _ranking_kernel_inputs(preds, target, num_labels)
    if inputs is None:
        return None
    from metrics_amd.ops import multilabel_ranking_sums

    sums = multilabel_ranking_sums(inputs[0], inputs[1], ignore_index, want)
    return None if sums is None else sums[want.bit_length() - 1]


def _multilabel_coverage_error_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, int]:
    """How far along the score-sorted label list one must go to cover all true labels."""
    offset = torch.zeros_like(preds)
    offset[target == 0] = preds.min().abs() + 10  # Any number >1 works
    preds_mod = preds + offset
    preds_min = preds_mod.min(dim=1)[0]
    coverage = (preds >= preds_min[:, None]).sum(dim=1).to(torch.float32)
    return coverage.sum(), coverage.numel()


def multilabel_coverage_error(
    preds: Tensor,
    target: Tensor,
    num_labels: int,
    ignore_index: Optional[int] = None,
    validate_args: bool = True,
) -> Tensor:
    """Multilabel coverage error."""
    if validate_args:
        _multilabel_confusion_matrix_arg_validation(num_labels, threshold=0.0, ignore_index=ignore_index)
        _multilabel_stat_scores_tensor_validation(preds, target, num_labels, "global", ignore_index)
    sums = _ranking_kernel_sums(preds, target, num_labels, ignore_index, _WANT_COVERAGE)
    if sums is not None:
        return sums[0] / sums[1]
    preds, target = _multilabel_ranking_format(preds, target, num_labels, ignore_index)
    coverage, total = _multilabel_coverage_error_update(preds, target)
    return coverage / total


def _multilabel_ranking_average_precision_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, int]:
    """Label ranking average precision (samplewise mean of per-label precision at each true label)."""
    neg_preds = -preds
    score = torch.tensor(0.0, device=neg_preds.device)
    n_preds, n_labels = neg_preds.shape
    for i in range(n_preds):
        relevant = target[i] == 1
        ranking = _rank_data(neg_preds[i][relevant]).float()
        if len(ranking) > 0 and len(ranking) < n_labels:
            rank = _rank_data(neg_preds[i])[relevant].float()
            score_idx = (ranking / rank).mean()
        else:
            score_idx = torch.ones_like(score)
        score += score_idx
    return score, n_preds


def multilabel_ranking_average_precision(
    preds: Tensor,
    target: Tensor,
    num_labels: int,
    ignore_index: Optional[int] = None,
    validate_args: bool = True,
) -> Tensor:
    """Multilabel ranking average precision."""
    if validate_args:
        _multilabel_confusion_matrix_arg_validation(num_labels, threshold=0.0, ignore_index=ignore_index)
        _multilabel_stat_scores_tensor_validation(preds, target, num_labels, "global", ignore_index)
    sums = _ranking_kernel_sums(preds, target, num_labels, ignore_index, _WANT_LRAP)
    if sums is not None:
        return sums[0] / sums[1]
    preds, target = _multilabel_ranking_format(preds, target, num_labels, ignore_index)
    score, total = _multilabel_ranking_average_precision_update(preds, target)
    return score / total


def _multilabel_ranking_loss_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, int]:
    """Average number of wrongly-ordered (true, false) label pairs, weighted."""
    n_preds, n_labels = preds.shape
    relevant = target == 1
    n_relevant = relevant.sum(dim=1)

    # rows that are all-negative or all-positive carry no ranking signal; drop them
    mask = (n_relevant > 0) & (n_relevant < n_labels)
    preds = preds[mask]
    relevant = relevant[mask]
    n_relevant = n_relevant[mask]

    # Nothing is relevant
    if len(preds) == 0:
        return torch.tensor(0.0, device=preds.device), 1

    inverse = preds.argsort(dim=1).argsort(dim=1)
    per_label_loss = ((n_labels - inverse) * relevant).to(torch.float32)
    correction = 0.5 * n_relevant * (n_relevant + 1)
    denom = n_relevant * (n_labels - n_relevant)
    loss = (per_label_loss.sum(dim=1) - correction) / denom
    return loss.sum(), n_preds


def multilabel_ranking_loss(
    preds: Tensor,
    target: Tensor,
    num_labels: int,
    ignore_index: Optional[int] = None,
    validate_args: bool = True,
) -> Tensor:
    """Multilabel ranking loss."""
    if validate_args:
        _multilabel_confusion_matrix_arg_validation(num_labels, threshold=0.0, ignore_index=ignore_index)
        _multilabel_stat_scores_tensor_validation(preds, target, num_labels, "global", ignore_index)
    sums = _ranking_kernel_sums(preds, target, num_labels, ignore_index, _WANT_LOSS)
    if sums is not None:
        return sums[0] / sums[1]
    preds, target = _multilabel_ranking_format(preds, target, num_labels, ignore_index)
    loss, total = _multilabel_ranking_loss_update(preds, target)
    return loss / total
