"""The top-k slot of the fused multiclass step, without a GPU.

1. The per-row rule the kernels implement (``_topk_rule.stat_rule_deltas``)
   against the reference's ``multiclass_stat_scores(top_k=k, average=None)``,
   replayed from a golden tape. Tie-free rows only: on ties the reference's
   ``topk`` order is not specified, the rule's is.
2. Which collections get a fused update plan with a top-k leader.
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.collections import _FusedMulticlassUpdatePlan
from tests.unittests._golden import ref_value
from tests.unittests._topk_rule import stat_rule_deltas


def _tie_free(B, C, gen):
    return torch.stack([torch.randperm(C, generator=gen) * 0.01 - 1.0 for _ in range(B)])


def test_rule_matches_reference():
    gen = torch.Generator().manual_seed(5)
    for C in (8, 136):
        for B in (2, 5, 257):
            for k in (2, 5, C):
                for ig in (None, 3, -1):
                    preds = _tie_free(B, C, gen)
                    target = torch.randint(0, C, (B,), generator=gen)
                    target[::3] = 3  # rows the ignore_index=3 cases drop
                    if ig == -1:
                        target[1::4] = -1

                    def _ref(preds=preds, target=target, C=C, k=k, ig=ig):
                        from torchmetrics.functional.classification import multiclass_stat_scores

                        return multiclass_stat_scores(
                            preds, target, num_classes=C, top_k=k, average=None, ignore_index=ig
                        )

                    want = ref_value(f"stat_scores C={C} B={B} k={k} ignore={ig}", _ref)  # (C, 5)
                    tp, fp, tn, fn = stat_rule_deltas(preds, target, k, ig)
                    got = torch.stack([tp, fp, tn, fn, tp + fn], dim=1)
                    assert torch.equal(got, want.long()), (C, B, k, ig)


# ---------------------------------------------------------------- plan selection
C = 16


def _batch(gen, B=6):
    """Random rows, the first with the target at rank 1: top-1 and top-5 states
    differ after one update, so they form two compute groups."""
    preds = torch.randn(B, C, generator=gen)
    target = torch.randint(0, C, (B,), generator=gen)
    preds[0, 2], preds[0, 7], target[0] = 8.0, 7.0, 7
    return preds, target


def _bench16(kw):
    return {
        "acc_micro": ma.MulticlassAccuracy(average="micro", **kw),
        "acc_macro": ma.MulticlassAccuracy(average="macro", **kw),
        "precision": ma.MulticlassPrecision(average="macro", **kw),
        "recall": ma.MulticlassRecall(average="macro", **kw),
        "f1": ma.MulticlassF1Score(average="macro", **kw),
        "fbeta2": ma.MulticlassFBetaScore(beta=2.0, average="macro", **kw),
        "specificity": ma.MulticlassSpecificity(average="macro", **kw),
        "npv": ma.MulticlassNegativePredictiveValue(average="macro", **kw),
        "hamming": ma.MulticlassHammingDistance(average="macro", **kw),
        "jaccard": ma.MulticlassJaccardIndex(average="macro", **kw),
        "exact_match": ma.MulticlassExactMatch(**kw),
        "cohen_kappa": ma.MulticlassCohenKappa(**kw),
        "mcc": ma.MulticlassMatthewsCorrCoef(**kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=20, **kw),
        "avg_precision": ma.MulticlassAveragePrecision(average="macro", thresholds=20, **kw),
    }


def _plan_topk(metrics, update=True):
    coll = ma.MetricCollection(metrics)
    if update:
        coll.update(*_batch(torch.Generator().manual_seed(3)))
    plan = _FusedMulticlassUpdatePlan.build(coll)
    return coll, (plan.topk if plan is not None else None)


KW = dict(num_classes=C, validate_args=False)


@pytest.mark.parametrize("which", ["top1_top5", "top1_top5_confmat", "bench16_top5"])
def test_plan_takes_the_topk_leader(which):
    top5 = ma.MulticlassAccuracy(top_k=5, average="micro", **KW)
    metrics = {"top1": ma.MulticlassAccuracy(average="micro", **KW), "top5": top5}
    if which == "top1_top5_confmat":
        metrics["confmat"] = ma.MulticlassConfusionMatrix(**KW)
    elif which == "bench16_top5":
        metrics = {**_bench16(KW), "top5": top5}
    coll, topk = _plan_topk(metrics)
    assert topk is coll._modules["top5"]
    # it leads a group of its own: the states differ from the top-1 group's
    assert ["top5"] in list(coll.compute_groups.values())


@pytest.mark.parametrize(
    "why", ["num_classes", "ignore_index", "samplewise", "validate_args", "env"]
)
def test_plan_leaves_the_topk_leader_out(monkeypatch, why):
    kw5 = dict(KW)
    update = True
    if why == "num_classes":
        kw5["num_classes"] = C + 1
        update = False  # no batch fits both class counts; groups are one per metric then
    elif why == "ignore_index":
        kw5["ignore_index"] = 3
    elif why == "samplewise":
        kw5["multidim_average"] = "samplewise"
    elif why == "validate_args":
        kw5["validate_args"] = True
    else:
        monkeypatch.setenv("METRICS_AMD_FUSE_TOPK", "0")
    metrics = {
        "top1": ma.MulticlassAccuracy(average="micro", **KW),
        "top5": ma.MulticlassAccuracy(top_k=5, average="micro", **kw5),
        "confmat": ma.MulticlassConfusionMatrix(**KW),
    }
    if why == "samplewise":
        # samplewise wants (B, C, extra) inputs, which the top_k > 1 update does
        # not take: the plan is built from the one-metric groups
        update = False
    _, topk = _plan_topk(metrics, update)
    assert topk is None


def test_second_topk_group_stays_on_its_own():
    metrics = {
        "top1": ma.MulticlassAccuracy(average="micro", **KW),
        "top3": ma.MulticlassAccuracy(top_k=3, average="micro", **KW),
        "top5": ma.MulticlassAccuracy(top_k=5, average="micro", **KW),
    }
    coll = ma.MetricCollection(metrics)
    gen = torch.Generator().manual_seed(3)
    preds, target = _batch(gen)
    preds[1, 0], preds[1, 1], preds[1, 2], preds[1, 3], target[1] = 9.0, 8.5, 8.0, 7.5, 3  # rank 3
    coll.update(preds, target)
    plan = _FusedMulticlassUpdatePlan.build(coll)
    assert plan is not None and plan.topk is coll._modules["top3"]
