"""Ignore/normalise ordering cases shared by the CPU tape test and the GPU tests.

The reference normalises its inputs (sigmoid / softmax) iff a value lies
outside [0, 1], and it orders that test differently per metric family:

* stat scores (binary, multilabel): the test sees EVERY element, ignored ones
  included;
* binary and multiclass threshold curves: ignored samples are removed first;
* multilabel threshold curve: the test sees every element.

Each case has exactly one out-of-range value. In the ``ignored`` flavour it
sits on an ignored sample, in the ``kept`` flavour (the mirror) on a kept one.
``tests/unittests/test_curve_oracle.py`` proves :func:`reference_normalises`
against the reference's own recorded answers; the GPU tests then use it.

All values are chosen so that the normalised scores are either exact
(sigmoid(0) = 0.5, softmax of an all-equal row = float32(1)/C) or far from
every threshold, so every expected count is exact.
"""
from __future__ import annotations

import torch

IGNORE = -1
STAT_THRESHOLD = 0.5
BINARY_THR = torch.linspace(0, 1, 5)  # 0.5 is hit exactly by sigmoid(0)
KINDS = ("binary_stat", "multilabel_stat", "binary_curve", "multiclass_curve", "multilabel_curve")


def _third_thresholds(C: int) -> torch.Tensor:
    inv = torch.tensor(1.0) / C  # float32(1)/C, what softmax gives an all-equal row
    lo = torch.nextafter(inv, torch.tensor(0.0))
    hi = torch.nextafter(inv, torch.tensor(1.0))
    return torch.stack([lo, inv, hi, torch.tensor(0.5), torch.tensor(0.9)]).sort().values


def multiclass_case(C: int, where: str, rows: int = 6):
    """(preds (rows+1, C), target, thresholds). Every row but the last is in range:
    all-equal rows of 0.25 (softmax gives float32(1)/C exactly, a threshold) and one
    valid probability row. The last row carries the only out-of-range value, 5.0 in
    column 0; it is the ignored sample in the ``ignored`` flavour."""
    g = torch.Generator().manual_seed(17 + C)
    p = torch.zeros(rows + 1, C)
    for r in range(rows):
        p[r] = 0.25  # all-equal and in range: softmax gives float32(1)/C exactly
    p[1, : min(C, 3)] = torch.tensor([0.2, 0.3, 0.5])[: min(C, 3)]
    p[1, 3:] = 0.0  # a valid probability row, 0.5 hits its threshold exactly when raw
    t = torch.randint(0, C, (rows + 1,), generator=g)
    t[0], t[1], t[2] = 0, 2 % C, C - 1
    hot = rows  # the last row is the one that differs between the flavours
    p[hot] = 0.0
    p[hot, 0] = 5.0
    t[hot] = IGNORE if where == "ignored" else 0
    if where == "kept":  # the ignored sample still exists, with in-range values
        p[3] = 0.125
        t[3] = IGNORE
    return p, t, _third_thresholds(C)


def case(kind: str, where: str):
    """(preds, target, thresholds-or-None) on CPU, float32."""
    assert kind in KINDS and where in ("ignored", "kept")
    if kind in ("binary_stat", "binary_curve"):
        p = torch.tensor([0.25, 0.5, 0.75, 1.0, 0.0, 0.3, 0.5, 0.0])
        t = torch.tensor([0, 1, 1, 0, 1, 0, IGNORE, 1])
        p[6 if where == "ignored" else 7] = 7.0
        return p, t, (BINARY_THR if kind == "binary_curve" else None)
    if kind in ("multilabel_stat", "multilabel_curve"):
        p = torch.tensor([[0.25, 0.5, 0.75], [1.0, 0.0, 0.3], [0.5, 0.0, 0.25], [0.0, 0.75, 0.5]])
        t = torch.tensor([[0, 1, 1], [0, 1, 0], [1, IGNORE, 0], [1, 0, 1]])
        if where == "ignored":
            p[2, 1] = 7.0
        else:
            p[3, 2] = 7.0
        return p, t, (BINARY_THR if kind == "multilabel_curve" else None)
    return multiclass_case(3, where)


def make_curve_metric(kind: str, preds: torch.Tensor, thr: torch.Tensor, **kw):
    """This project's stand-alone curve metric for ``kind`` (validate_args on, on CPU)."""
    import metrics_amd as ma

    if kind == "binary_curve":
        return ma.BinaryPrecisionRecallCurve(thresholds=thr, ignore_index=IGNORE, **kw)
    if kind == "multiclass_curve":
        return ma.MulticlassPrecisionRecallCurve(
            num_classes=preds.shape[1], thresholds=thr, ignore_index=IGNORE, **kw)
    assert kind == "multilabel_curve"
    return ma.MultilabelPrecisionRecallCurve(num_labels=preds.shape[1], thresholds=thr, ignore_index=IGNORE, **kw)


def reference_normalises(kind: str, preds: torch.Tensor, target: torch.Tensor) -> bool:
    """The reference's decision, as read from its code and proved by the tape test."""
    outside = (preds < 0) | (preds > 1)
    if kind in ("binary_curve", "multiclass_curve"):
        keep = target != IGNORE
        outside = outside & keep.reshape(-1, *([1] * (preds.ndim - 1)))
    return bool(outside.any())


def normalised(kind: str, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """float32 scores after the reference's decision (plain torch, CPU)."""
    preds = preds.float().cpu()
    if not reference_normalises(kind, preds, target.cpu()):
        return preds
    return preds.softmax(-1) if kind == "multiclass_curve" else preds.sigmoid()


def stat_oracle(scores: torch.Tensor, target: torch.Tensor, multilabel: bool) -> torch.Tensor:
    """[tp, fp, tn, fn, support] (per label for multilabel), score > 0.5, ignored elements left out."""
    pred = scores.double() > STAT_THRESHOLD
    keep = target != IGNORE
    lab = target == 1
    dim = 0 if multilabel else None

    def cnt(m):
        return (m & keep).sum(dim) if multilabel else (m & keep).sum()

    tp, fp, tn, fn = cnt(pred & lab), cnt(pred & ~lab), cnt(~pred & ~lab), cnt(~pred & lab)
    return torch.stack([tp, fp, tn, fn, tp + fn], -1)
