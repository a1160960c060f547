"""The per-row rule of the fused step's stat slots, in plain torch int64.

For a row ``x[0..C)`` converted to fp32, target ``t`` and argmax ``a`` (largest
non-NaN value, lowest index on a tie; none for an all-NaN row):

* the row is valid iff it is not ignored, ``0 <= t < C`` and it has an argmax;
  a row that is not valid is counted in neither slot;
* ``rank = #{ j : x[j] > x[t] or (x[j] == x[t] and j < t) }`` with IEEE compares
  (NaN compares false on both sides, ``+0.0 == -0.0``);
* the top-k slot predicts ``p = t if rank < k else a``, the top-1 slot ``p = a``;
* ``p == t`` counts ``tp[t]``, otherwise ``fp[p]`` and ``fn[t]``;
  ``tn = valid - tp - fp - fn`` per class.
"""
import torch


def stat_rule_deltas(preds, target, k=None, ignore_index=None):
    """Per-class ``(tp, fp, tn, fn)`` int64 deltas of one (B, C) batch on the
    CPU; ``k=None`` gives the top-1 slot, an int the top-k slot."""
    x = preds.detach().float().cpu()
    t = target.detach().long().cpu()
    B, C = x.shape
    idx = torch.arange(C)[None, :]
    nan = x.isnan()
    has = (~nan).any(dim=1)
    rowbest = torch.where(nan, torch.full_like(x, float("-inf")), x).max(dim=1).values
    hit = (x == rowbest[:, None]) & ~nan
    a = torch.where(hit, idx, torch.full_like(idx, C)).min(dim=1).values  # C: no argmax
    valid = (t >= 0) & (t < C) & has
    if ignore_index is not None:
        valid &= t != ignore_index
    tc = t.clamp(0, C - 1)
    if k is None:
        p = a
    else:
        xt = x.gather(1, tc[:, None])
        rank = ((x > xt) | ((x == xt) & (idx < tc[:, None]))).sum(dim=1)
        p = torch.where(rank < k, tc, a)
    right = valid & (p == tc)
    wrong = valid & (p != tc)
    tp = torch.bincount(tc[right], minlength=C)
    fp = torch.bincount(p[wrong], minlength=C)
    fn = torch.bincount(tc[wrong], minlength=C)
    tn = int(valid.sum()) - tp - fp - fn
    return tp, fp, tn, fn
