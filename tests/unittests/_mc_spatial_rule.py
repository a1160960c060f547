"""The rule of the fused spatial multiclass step (``csrc/mc_spatial.hip``) in
CPU torch, no ``metrics_amd.ops`` call anywhere.

``preds`` is (N, C, *spatial) float, ``target`` (N, *spatial) int64. A pixel is
one (n, s); its column the C values ``preds[n, :, s]``.

- argmax: the largest non-NaN value of the column, the lowest index on a tie
  (+0.0 and -0.0 tie), index 0 when every element is NaN;
- a pixel is counted iff its target is not ``ignore_index`` and ``0 <= t < C``:
  tp[t] if argmax == t, else fp[argmax] and fn[t]; tn[c] = counted - tp - fp - fn;
  confmat[t, argmax] += 1;
- exact match: a sample is correct iff no pixel whose target is not ignored has
  argmax != t; an out-of-range target that is not ignored is a mismatch, an
  ignored pixel never is. total = N.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor


def mc_spatial_argmax(preds: Tensor) -> Tensor:
    """(N, C, *spatial) -> (N, *spatial) int64."""
    x = preds.detach().cpu().to(torch.float64)  # exact for fp32 and bf16
    x = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x)
    best = x.max(dim=1, keepdim=True).values
    C = x.shape[1]
    idx = torch.arange(C).reshape(1, C, *([1] * (x.ndim - 2))).expand_as(x)
    # lowest index holding the maximum (-0.0 == +0.0 under ==)
    return torch.where(x == best, idx, torch.full_like(idx, C)).min(dim=1).values


def mc_spatial_rule(preds: Tensor, target: Tensor, num_classes: int,
                    ignore_index: Optional[int]) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(tp, fp, tn, fn) of shape (C,), confmat (C, C), correct (1,), total (1,), int64."""
    C = num_classes
    N = preds.shape[0]
    S = math.prod(preds.shape[2:])
    p = mc_spatial_argmax(preds).reshape(N, S)
    t = target.detach().cpu().long().reshape(N, S)
    kept = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != ignore_index
    counted = kept & (t >= 0) & (t < C)
    pc, tc = p[counted], t[counted]
    confmat = torch.bincount(tc * C + pc, minlength=C * C).reshape(C, C)
    tp = confmat.diagonal().clone()
    fp = confmat.sum(0) - tp
    fn = confmat.sum(1) - tp
    tn = int(counted.sum()) - tp - fp - fn
    mismatch = kept & ~(counted & (p == t))
    correct = (~mismatch.any(dim=1)).sum().reshape(1)
    return tp, fp, tn, fn, confmat, correct, torch.tensor([N])


def mc_spatial_rule_sum(batches: Sequence[Tuple[Tensor, Tensor]], num_classes: int, ignore_index: Optional[int]):
    """The rule summed over ``batches`` of (preds, target)."""
    acc = None
    for preds, target in batches:
        out = mc_spatial_rule(preds, target, num_classes, ignore_index)
        acc = out if acc is None else tuple(a + b for a, b in zip(acc, out))
    return acc
