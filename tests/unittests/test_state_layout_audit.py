"""Automated state-layout audit vs the reference.

For every same-named Metric class in both top-level namespaces that can be
instantiated with a small common-argument guess, the registered state names
and default shapes/dtypes must match — this is what makes checkpoints
(state_dict with persistent=True) interchangeable across the two
implementations for the whole surface, not just the hand-picked five in
test_state_dict_compat.py.

Known deliberate deviations are listed with reasons.

The reference's layouts are replayed from the golden tape under
tests/golden/reference/ (see tests/unittests/_golden.py).
"""
from __future__ import annotations

import torch

import metrics_amd as ma
from tests.unittests._golden import ref_value

# argument guesses tried in order until one constructs BOTH classes
_ARG_GUESSES = (
    {},
    {"num_classes": 5},
    {"num_labels": 4},
    {"num_classes": 5, "thresholds": 20},
    {"num_labels": 4, "thresholds": 20},
    {"thresholds": 20},
    {"num_outputs": 1},
    {"task": "binary"},
)

# our state layout deliberately differs (documented MI355X design choices)
_KNOWN_DEVIATIONS = {
    # fused per-class counter layout: micro-average metrics keep (C,) counts
    # so they can share a compute group with macro metrics (see
    # test_ref_differential_modular.test_collection_compute_groups_match)
    "MulticlassAccuracy", "MulticlassPrecision", "MulticlassRecall", "MulticlassF1Score",
    "MulticlassFBetaScore", "MulticlassSpecificity", "MulticlassNegativePredictiveValue",
    "MulticlassHammingDistance", "MulticlassStatScores", "MulticlassJaccardIndex",
    "MulticlassExactMatch",
    # detection: own RLE pack instead of pycocotools tuples
    "MeanAveragePrecision",
    # O(1) accumulated statistics instead of the reference's raw preds/target
    # cat-lists (SURVEY 5.7 state-size handling: no unbounded image buffers)
    "ErrorRelativeGlobalDimensionlessSynthesis", "RelativeAverageSpectralError",
    # simple RCCL-reducible denominator stats (sum/min/max) instead of the
    # reference's running mean/var with dist_reduce_fx=None merge
    "NormalizedRootMeanSquaredError",
    # nominal association metrics: O(1) (C,C) contingency counts instead of
    # the reference's unbounded preds/target cat lists (num_classes is a
    # required argument in both; value parity in test_ref_differential_modular)
    "CramersV", "PearsonsContingencyCoefficient", "TheilsU", "TschuprowsT",
}


def _instantiate(cls):
    for kw in _ARG_GUESSES:
        try:
            return cls(**kw), kw
        except Exception:
            continue
    return None, None


def _reference_layouts():
    """{top-level name: None | [constructor kwargs, {state: ["tensor", shape, dtype] | ["list"]}]}
    for everything the reference exports (runs only while the tape is recorded)."""
    import warnings

    import torchmetrics as tm

    out = {}
    for name in dir(tm):
        ref_cls = getattr(tm, name)
        out[name] = None
        if not isinstance(ref_cls, type):
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref, kw = _instantiate(ref_cls)
        if ref is None or not hasattr(ref, "_defaults"):
            continue
        out[name] = [kw, {
            k: ["tensor", tuple(d.shape), str(d.dtype)] if isinstance(d, torch.Tensor) else ["list"]
            for k, d in ref._defaults.items()
        }]
    return out


def test_state_layout_matches_reference():
    ref_layouts = ref_value("state layouts", _reference_layouts)

    common = sorted(set(dir(ma)) & set(ref_layouts))
    checked, mismatches, skipped = [], [], []
    for name in common:
        ours_cls = getattr(ma, name)
        if not (isinstance(ours_cls, type) and issubclass(ours_cls, ma.Metric)):
            continue
        if name in _KNOWN_DEVIATIONS:
            continue
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ours, kw1 = _instantiate(ours_cls)
        kw2, ref_defaults = ref_layouts[name] or (None, None)
        if ours is None or ref_defaults is None or kw1 != kw2:
            skipped.append(name)
            continue
        k1, k2 = set(ours._defaults), set(ref_defaults)
        if k1 != k2:
            mismatches.append((name, sorted(k1), sorted(k2)))
            continue
        for k in k1:
            d1, d2 = ours._defaults[k], ref_defaults[k]
            if isinstance(d1, torch.Tensor) != (d2[0] == "tensor"):
                mismatches.append((name, k, type(d1), d2[0]))
            elif isinstance(d1, torch.Tensor) and (tuple(d1.shape) != tuple(d2[1]) or str(d1.dtype) != d2[2]):
                mismatches.append((name, k, (d1.shape, d1.dtype), (d2[1], d2[2])))
        checked.append(name)
    assert len(checked) >= 60, f"audit only covered {len(checked)} classes (skipped: {skipped[:20]})"
    assert not mismatches, mismatches
