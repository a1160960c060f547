"""The rule of the fused binary step (``csrc/bin_step.hip``), in CPU torch.

The input is read as a flat stream. The label is ``target == 1``; an element
whose target is ``ignore_index`` counts in nothing. The prediction is
``x > thr`` without and ``x > log(thr / (1 - thr))`` (float32) with
normalisation. The groups decide on normalisation separately, as the
stand-alone updates (and the reference library) do:

- stat scores: sigmoid iff ANY element of ``preds``, ignored positions
  included, lies outside [0, 1];
- confusion matrix (and the curve): sigmoid iff any element whose target is
  NOT ignored lies outside [0, 1].

NaN is not outside, +-inf is.
"""
import torch


def bin_rule_decisions(preds, target, ignore_index):
    """(outside_all, outside_kept) of one batch."""
    x = preds.detach().cpu().float().flatten()
    target = target.detach().cpu().flatten()
    out = (x < 0) | (x > 1)
    live = torch.ones_like(out) if ignore_index is None else target != ignore_index
    return bool(out.any()), bool((out & live).any())


def _counts(x, target, live, cut):
    pred = x > cut
    lab = target == 1
    tp = (live & pred & lab).sum().reshape(1)
    fp = (live & pred & ~lab).sum().reshape(1)
    tn = (live & ~pred & ~lab).sum().reshape(1)
    fn = (live & ~pred & lab).sum().reshape(1)
    return tp, fp, tn, fn


def bin_rule_deltas(preds, target, threshold, ignore_index):
    """((tp, fp, tn, fn) each (1,), confmat (2, 2)) of one batch."""
    x = preds.detach().cpu().float().flatten()
    target = target.detach().cpu().flatten()
    thr = torch.tensor(threshold, dtype=torch.float32)
    lthr = torch.log(thr / (1.0 - thr))
    live = torch.ones_like(x, dtype=torch.bool) if ignore_index is None else target != ignore_index
    outside_all, outside_kept = bin_rule_decisions(preds, target, ignore_index)
    stat = _counts(x, target, live, lthr if outside_all else thr)
    tp, fp, tn, fn = _counts(x, target, live, lthr if outside_kept else thr)
    confmat = torch.stack([torch.cat([tn, fp]), torch.cat([fn, tp])])
    return stat, confmat


def bin_rule_sum(batches, threshold, ignore_index):
    """The accumulated states after ``batches``, in the order of :func:`bin_rule_deltas`."""
    stat = confmat = None
    for p, t in batches:
        s, c = bin_rule_deltas(p, t, threshold, ignore_index)
        if stat is None:
            stat, confmat = s, c
        else:
            stat = tuple(a + b for a, b in zip(stat, s))
            confmat = confmat + c
    return stat, confmat


def bin_rule_curve(batches, thresholds, ignore_index):
    """The (T, 2, 2) curve state after ``batches``: p = x or sigmoid(x) by the
    kept-elements decision, prediction ``p >= threshold``, layout
    [t][target][pred]."""
    thr = torch.as_tensor(thresholds, dtype=torch.float32)
    state = torch.zeros(thr.numel(), 2, 2, dtype=torch.long)
    for p, t in batches:
        x = p.detach().cpu().float().flatten()
        t = t.detach().cpu().flatten()
        live = torch.ones_like(x, dtype=torch.bool) if ignore_index is None else t != ignore_index
        _, outside_kept = bin_rule_decisions(p, t, ignore_index)
        x, lab = x[live], t[live] == 1
        if outside_kept:
            x = torch.sigmoid(x)
        pred = x.unsqueeze(0) >= thr.unsqueeze(1)  # (T, n); NaN is negative everywhere
        lab = lab.unsqueeze(0)
        state[:, 1, 1] += (pred & lab).sum(1)
        state[:, 0, 1] += (pred & ~lab).sum(1)
        state[:, 1, 0] += (~pred & lab).sum(1)
        state[:, 0, 0] += (~pred & ~lab).sum(1)
    return state
