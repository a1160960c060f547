"""Modular multilabel ranking metrics. Parity: torchmetrics ``classification/ranking.py``."""
from __future__ import annotations

from typing import Any, Optional

import torch
from torch import Tensor

from metrics_amd.metric import Metric
from metrics_amd.functional.classification.ranking import (
    _multilabel_coverage_error_update,
    _multilabel_ranking_average_precision_update,
    _multilabel_ranking_format,
    _multilabel_ranking_loss_update,
    _ranking_kernel_inputs,
)
from metrics_amd.functional.classification.confusion_matrix import _multilabel_confusion_matrix_arg_validation
from metrics_amd.functional.classification.stat_scores import _multilabel_stat_scores_tensor_validation


class _MultilabelRankingBase(Metric):
    higher_is_better: Optional[bool] = None
    is_differentiable: bool = False
    full_state_update: bool = False
    measure: Tensor
    total: Tensor

    _update_fn = None  # set in subclasses
    _hip_fused_kind = "ml_rank"  # the update below is what csrc/ml_rank.hip implements
    _rank_measure: str  # "coverage", "lrap" or "loss": the argument of ml_ranking_into

    def __init__(
        self,
        num_labels: int,
        ignore_index: Optional[int] = None,
        validate_args: bool = True,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if validate_args:
            _multilabel_confusion_matrix_arg_validation(num_labels, threshold=0.0, ignore_index=ignore_index)
        self.validate_args = validate_args
        self.num_labels = num_labels
        self.ignore_index = ignore_index
        self.add_state("measure", torch.tensor(0.0), dist_reduce_fx="sum")
        self.add_state("total", torch.tensor(0.0), dist_reduce_fx="sum")

    def update(self, preds: Tensor, target: Tensor) -> None:
        """Accumulate the ranking measure."""
        if self.validate_args:
            _multilabel_stat_scores_tensor_validation(preds, target, self.num_labels, "global", self.ignore_index)
        # GPU: the kernel adds into the two states in place, no host sync
        inputs = _ranking_kernel_inputs(preds, target, self.num_labels)
        if inputs is not None:
            from metrics_amd.ops import _hip

            pairs = {self._rank_measure: (self.measure, self.total)}
            if _hip.ml_ranking_into(inputs[0], inputs[1], self.ignore_index, owner=self, **pairs):
                return
        preds, target = _multilabel_ranking_format(preds, target, self.num_labels, self.ignore_index)
        measure, total = type(self)._compute_update(preds, target)
        self.measure += measure
        self.total += total

    def compute(self) -> Tensor:
        """Average measure."""
        return self.measure / self.total

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class MultilabelCoverageError(_MultilabelRankingBase):
    """Multilabel coverage error (stateful)."""

    higher_is_better = False
    plot_lower_bound: float = 0.0
    _rank_measure = "coverage"

    @staticmethod
    def _compute_update(preds: Tensor, target: Tensor):
        return _multilabel_coverage_error_update(preds, target)


class MultilabelRankingAveragePrecision(_MultilabelRankingBase):
    """Multilabel ranking average precision (stateful)."""

    higher_is_better = True
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 1.0
    _rank_measure = "lrap"

    @staticmethod
    def _compute_update(preds: Tensor, target: Tensor):
        return _multilabel_ranking_average_precision_update(preds, target)


class MultilabelRankingLoss(_MultilabelRankingBase):
    """Multilabel ranking loss (stateful)."""

    higher_is_better = False
    plot_lower_bound: float = 0.0
    _rank_measure = "loss"

    @staticmethod
    def _compute_update(preds: Tensor, target: Tensor):
        return _multilabel_ranking_loss_update(preds, target)
