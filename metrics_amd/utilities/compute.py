"""L0 numeric helpers.

Parity: torchmetrics ``utilities/compute.py`` (_safe_divide, _safe_xlogy,
_safe_matmul, _auc_compute, _adjust_weights_safe_divide,
normalize_logits_if_needed).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from metrics_amd.utilities.data import interp  # noqa: F401  (re-export)


def _safe_matmul(x: Tensor, y: Tensor) -> Tensor:
    """Matmul that upcasts half dtypes to fp32 for the accumulate.

    On MI355X the bf16 MFMA path accumulates in fp32 natively (hipBLASLt), so
    this only changes the *output* dtype to fp32 for numerically-sensitive
    consumers.
    """
    if x.is_floating_point() and x.dtype in (torch.float16, torch.bfloat16):
        return (x.float() @ y.float())
    return x @ y


def _safe_xlogy(x: Tensor, y: Tensor) -> Tensor:
    """x * log(y), defined as 0 where x == 0."""
    res = x * torch.log(y)
    res[x == 0] = 0.0
    return res


def _safe_divide(num: Tensor, denom: Tensor, zero_division: float = 0.0) -> Tensor:
    """num / denom with 0-denominator entries replaced by ``zero_division``."""
    num = num if num.is_floating_point() else num.float()
    denom = denom if denom.is_floating_point() else denom.float()
    zero_division_t = torch.tensor(zero_division, dtype=num.dtype, device=num.device)
    return torch.where(denom != 0, num / denom, zero_division_t)


def _adjust_weights_safe_divide(
    score: Tensor, average: Optional[str], multilabel: bool, tp: Tensor, fp: Tensor, fn: Tensor,
    top_k: int = 1,
) -> Tensor:
    """Apply macro / weighted averaging over per-class scores, skipping empty classes."""
    if average is None or average == "none":
        return score
    if average == "weighted":
        weights = tp + fn
    else:  # macro
        weights = torch.ones_like(score)
        if not multilabel:
            weights[tp + fp + fn == 0 if top_k == 1 else tp + fn == 0] = 0.0
    return _safe_divide(weights * score, weights.sum(-1, keepdim=True)).sum(-1)


_AVG_MODE = {"macro": 0, "weighted": 1, "micro": 2}


class LinearFormula(NamedTuple):
    """A stat-score reduction as the HIP kernels evaluate it:
    ``post_a * safe_div(num . s, den . s, zero_division) + post_b`` with
    ``s = (tp, fp, tn, fn)``, then micro / macro / weighted averaging as
    ``_adjust_weights_safe_divide`` does (``zero_w_topk``: macro drops classes
    with ``tp + fn == 0`` instead of ``tp + fp + fn == 0``).

    The one statement of each metric's coefficients: the functional reducers
    hand it to ``_hip.linear_stat_compute`` and the metric classes declare it to
    the collection compute plan.
    """

    num: Tuple[float, float, float, float]
    den: Tuple[float, float, float, float]
    zero_w_topk: bool = False
    zero_division: float = 0.0
    post_a: float = 1.0
    post_b: float = 0.0

    def params(self, average: str) -> Tuple[float, ...]:
        """The 13 floats per formula of ``k_linear_stat_multi``."""
        return (
            *(float(c) for c in self.num), *(float(c) for c in self.den),
            float(_AVG_MODE[average]), float(1 if self.zero_w_topk else 0),
            float(self.zero_division), float(self.post_a), float(self.post_b),
        )

    def evaluate(self, tp: Tensor, fp: Tensor, tn: Tensor, fn: Tensor, average: str) -> Tensor:
        """The same reduction in plain torch."""
        stats = [x.float() for x in (tp, fp, tn, fn)]
        num = sum(c * x for c, x in zip(self.num, stats))
        den = sum(c * x for c, x in zip(self.den, stats))
        if average == "micro":
            num, den = num.sum(-1), den.sum(-1)
        score = self.post_a * _safe_divide(num, den, self.zero_division) + self.post_b
        if average == "micro":
            return score
        return _adjust_weights_safe_divide(score, average, False, tp, fp, fn, 2 if self.zero_w_topk else 1)


def _reduce_curve_auc(res: Tensor, weights: Tensor, average: Optional[str]) -> Optional[Tensor]:
    """Average the per-class AUROC / AP vector of ``_hip.curve_auc_from_confmat``
    (no NaNs: its safe divides return 0). None for an unknown ``average``."""
    if average in (None, "none"):
        return res
    if average == "macro":
        return res.mean()
    if average == "weighted":
        w = _safe_divide(weights, weights.sum())
        return (res * w).sum()
    return None


def _auc_compute_without_check(x: Tensor, y: Tensor, direction: float, axis: int = -1) -> Tensor:
    """Trapezoidal area under (x, y); ``direction`` flips sign for decreasing x."""
    with torch.no_grad():
        auc_score = torch.trapz(y, x, dim=axis) * direction
    return auc_score


def _auc_compute(x: Tensor, y: Tensor, reorder: bool = False) -> Tensor:
    with torch.no_grad():
        if reorder:
            x, x_idx = torch.sort(x, stable=True)
            y = y[x_idx]
        dx = x[1:] - x[:-1]
        if (dx < 0).any():
            if (dx <= 0).all():
                direction = -1.0
            else:
                raise ValueError(
                    "The `x` tensor is neither increasing or decreasing. Try setting reorder=True."
                )
        else:
            direction = 1.0
        return _auc_compute_without_check(x, y, direction)


def auc(x: Tensor, y: Tensor, reorder: bool = False) -> Tensor:
    """Area under the curve y = f(x) using the trapezoidal rule."""
    if x.ndim > 1 or y.ndim > 1:
        raise ValueError(f"Expected both x and y to be 1d, got {x.ndim}d and {y.ndim}d")
    if x.numel() != y.numel():
        raise ValueError("Expected the same number of elements in x and y")
    return _auc_compute(x, y, reorder=reorder)


def normalize_logits_if_needed(tensor: Tensor, normalization: str, keep: Optional[Tensor] = None) -> Tensor:
    """Apply sigmoid/softmax iff values fall outside [0, 1].

    ``keep`` (bool, one entry per sample along dim 0) restricts the range test
    to the kept samples: the binary and multiclass curve formats drop ignored
    samples BEFORE the test, and GPU callers that leave the mask to the kernel
    pass it here so the decision is the same.

    Single-pass check; we control the device and accept the device sync the
    ``.any()`` implies only on CPU — on GPU the branchless torch.where form is
    used to avoid a host sync (the hot update kernels bypass this entirely and
    normalize in-kernel).
    """
    assert normalization in ("sigmoid", "softmax")
    if keep is not None:
        outside = (tensor < 0) | (tensor > 1)
        condition = (outside & keep.reshape(-1, *([1] * (tensor.ndim - 1)))).any()
        return torch.where(
            condition,
            torch.sigmoid(tensor) if normalization == "sigmoid" else torch.softmax(tensor, dim=-1),
            tensor,
        )
    if tensor.device.type == "cpu":
        if not torch.all((tensor >= 0) * (tensor <= 1)):
            tensor = tensor.sigmoid() if normalization == "sigmoid" else tensor.softmax(dim=-1)
        return tensor
    # branchless on device: no host<->device sync
    condition = ((tensor < 0) | (tensor > 1)).any()
    return torch.where(
        condition,
        torch.sigmoid(tensor) if normalization == "sigmoid" else torch.softmax(tensor, dim=-1),
        tensor,
    )
