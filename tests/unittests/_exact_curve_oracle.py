"""Oracles of the exact (``thresholds=None``) classification curves, numpy only.

``curve_by_definition`` is the definition itself, with no sort and no running
sum. The thresholds of a column are its distinct scores under float equality
(so ``+0.0`` and ``-0.0`` are one threshold), descending, and for each
threshold ``t``::

    tps = sum(w[(score >= t) & (target == pos_label)])
    fps = sum(w[(score >= t) & (target != pos_label)])

Counts are int64, weighted sums fp64. It costs O(n * k): use it up to about
n = 8192, or wherever the number of distinct scores k is small.
``curve_by_sort`` is the second oracle for larger inputs: a stable argsort of
fp64 copies and an int64 (fp64 when weighted) cumulative sum.
``tests/unittests/classification/test_exact_curve_oracle.py`` shows that the
two are identical on every small case.

NaN is outside the definition (``score >= t`` is false for it and it equals
nothing): both oracles refuse it. Cases with NaN carry their expected outcome
written out by hand (``tests/unittests/_exact_curve_cases.py``).

The curve and area functions below are the fp64 chain of the public metrics on
top of these counts.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

Curve = Tuple[np.ndarray, np.ndarray, np.ndarray]  # fps, tps, thresholds


def _trapz(y, x) -> float:
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0))


def _prepare(scores, target, pos_label, weights):
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    pos = np.asarray(target).reshape(-1) == pos_label
    if np.isnan(s).any():
        raise ValueError("NaN scores are outside the definition; write the expected outcome out by hand")
    w = None if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    return s, pos, w


def curve_by_definition(scores, target, pos_label: int = 1, weights=None) -> Curve:
    s, pos, w = _prepare(scores, target, pos_label, weights)
    thr = np.unique(s)[::-1]  # np.unique compares with ==: the two zeros are one value
    dtype = np.int64 if w is None else np.float64
    tps, fps = np.zeros(len(thr), dtype), np.zeros(len(thr), dtype)
    for k, t in enumerate(thr):
        above = s >= t
        if w is None:
            tps[k] = np.count_nonzero(above & pos)
            fps[k] = np.count_nonzero(above & ~pos)
        else:
            tps[k] = w[above & pos].sum()
            fps[k] = w[above & ~pos].sum()
    return fps, tps, thr


def curve_by_sort(scores, target, pos_label: int = 1, weights=None) -> Curve:
    s, pos, w = _prepare(scores, target, pos_label, weights)
    order = np.argsort(-s, kind="stable")  # -(-0.0) == -(+0.0): the zeros stay tied
    s, pos = s[order], pos[order]
    last = np.flatnonzero(np.append(s[1:] != s[:-1], True))  # last element of each tie group
    if w is None:
        tps = np.cumsum(pos.astype(np.int64))[last]
        fps = last + 1 - tps
    else:
        w = w[order]
        tps = np.cumsum(np.where(pos, w, 0.0))[last]
        fps = np.cumsum(np.where(pos, 0.0, w))[last]
    return fps, tps, s[last]


def curve(scores, target, pos_label: int = 1, weights=None, limit: int = 8192) -> Curve:
    """The definition up to ``limit`` elements, the sort oracle above."""
    fn = curve_by_definition if np.asarray(scores).size <= limit else curve_by_sort
    return fn(scores, target, pos_label, weights)


# ------------------------------------------------------------ public curves
def _ratio(num, den):
    """``_safe_divide``: 0 where the denominator is 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros_like(num), where=den != 0)


def roc(fps, tps, thr):
    """(fpr, tpr, thresholds) with the leading (0, 0) point at threshold 1. A
    column without negatives (positives) has fpr (tpr) zero throughout."""
    fps, tps = np.append(0, fps).astype(np.float64), np.append(0, tps).astype(np.float64)
    return _ratio(fps, fps[-1]), _ratio(tps, tps[-1]), np.append(1.0, thr)


def precision_recall(fps, tps, thr):
    """(precision, recall, thresholds): ascending thresholds, the closing (1, 0)
    point appended. Recall of a column without positives is 0 / 0 = NaN there."""
    fps, tps = np.asarray(fps, np.float64), np.asarray(tps, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = tps / (tps + fps)
        recall = tps / tps[-1]
    return np.append(precision[::-1], 1.0), np.append(recall[::-1], 0.0), np.asarray(thr)[::-1]


def auroc(fps, tps, thr, max_fpr: Optional[float] = None) -> float:
    fpr, tpr, _ = roc(fps, tps, thr)
    if max_fpr is None or max_fpr == 1:
        return _trapz(tpr, fpr)
    stop = np.searchsorted(fpr, max_fpr, side="right")
    weight = (max_fpr - fpr[stop - 1]) / (fpr[stop] - fpr[stop - 1])
    tpr = np.append(tpr[:stop], tpr[stop - 1] + weight * (tpr[stop] - tpr[stop - 1]))
    fpr = np.append(fpr[:stop], max_fpr)
    partial = _trapz(tpr, fpr)
    min_area = 0.5 * max_fpr ** 2  # McClish correction
    return float(0.5 * (1 + (partial - min_area) / (max_fpr - min_area)))


def average_precision(fps, tps, thr) -> float:
    precision, recall, _ = precision_recall(fps, tps, thr)
    return float(-np.sum((recall[1:] - recall[:-1]) * precision[:-1]))


def ulps32(value, exact) -> np.ndarray:
    """|value - exact| in fp32 ulps of ``exact`` (fp64 arithmetic)."""
    value, exact = np.asarray(value, np.float64), np.asarray(exact, np.float64)
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return np.abs(value - exact) / ulp
