"""The rule of the fused multilabel step (``csrc/ml_step.hip``), in CPU torch.

The batch is normalised with sigmoid iff any element of ``preds``, ignored
positions included, lies outside [0, 1] (NaN is not outside). The prediction is
``x > thr`` without and ``x > log(thr / (1 - thr))`` (float32) with
normalisation, the label is ``target == 1``, an element whose target is
``ignore_index`` counts in no stat count and no confusion matrix.

Exact match is the rule of ``MultilabelExactMatch.update`` as it stands, which
is the reference library's: a row is correct iff every one of its ``L``
elements has ``pred == target``, and an ignored element (target -1 after
formatting) equals no prediction. So a row with an ignored element, an
all-ignored row included, is never correct. The fused step has to agree with
the stand-alone update bit for bit, hence with this.
"""
import torch


def ml_rule_deltas(preds, target, threshold, ignore_index):
    """((tp, fp, tn, fn) each (L,), confmat (L, 2, 2), correct, total) of one batch."""
    x = preds.detach().cpu().float()
    target = target.detach().cpu()
    thr = torch.tensor(threshold, dtype=torch.float32)
    outside = bool(((x < 0) | (x > 1)).any())
    cut = torch.log(thr / (1.0 - thr)) if outside else thr
    pred = x > cut
    live = torch.ones_like(pred) if ignore_index is None else target != ignore_index
    lab = target == 1
    tp = (live & pred & lab).sum(0)
    fp = (live & pred & ~lab).sum(0)
    tn = (live & ~pred & ~lab).sum(0)
    fn = (live & ~pred & lab).sum(0)
    confmat = torch.stack([torch.stack([tn, fp], -1), torch.stack([fn, tp], -1)], -2)
    correct = (live & (pred == lab)).all(1).sum().reshape(1)
    return (tp, fp, tn, fn), confmat, correct, torch.tensor([x.shape[0]])


def ml_rule_sum(batches, threshold, ignore_index):
    """The accumulated states after ``batches``, in the order of :func:`ml_rule_deltas`."""
    stat = confmat = correct = total = None
    for p, t in batches:
        s, c, k, n = ml_rule_deltas(p, t, threshold, ignore_index)
        if stat is None:
            stat, confmat, correct, total = s, c, k, n
        else:
            stat = tuple(a + b for a, b in zip(stat, s))
            confmat, correct, total = confmat + c, correct + k, total + n
    return stat, confmat, correct, total
