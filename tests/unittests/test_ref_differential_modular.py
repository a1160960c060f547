"""Modular-layer differential vs the reference: wrappers, aggregators,
composition and collections driven with identical batch sequences.

The functional harness (test_ref_differential.py) pins the math; this one
pins the STATEFUL layer — forward()-vs-forward() per batch and final
compute()-vs-compute() — where the wrapper/aggregation logic lives.

The reference side is replayed from the golden tapes under
tests/golden/reference/ (see tests/unittests/_golden.py).
"""
from __future__ import annotations

import pytest
import torch

import metrics_amd as ma
from tests.unittests._golden import ref_module, ref_value


def _tm():
    return ref_module("torchmetrics")


def _cmp(a, b, atol=1e-5):
    if isinstance(a, dict):
        assert set(a) == set(b), (set(a), set(b))
        for k in a:
            _cmp(a[k], b[k], atol)
        return
    if isinstance(a, (list, tuple)):
        for x, y in zip(a, b):
            _cmp(x, y, atol)
        return
    a = torch.as_tensor(a).float()
    b = torch.as_tensor(b).float()
    both_nan = torch.isnan(a) & torch.isnan(b)
    assert torch.allclose(a[~both_nan], b[~both_nan], atol=atol, rtol=1e-4), (a, b)


def _drive(ours, ref, batches, atol=1e-5, check_forward=True):
    for args in batches:
        got = ours(*[x.clone() if isinstance(x, torch.Tensor) else x for x in args])
        exp = ref(*[x.clone() if isinstance(x, torch.Tensor) else x for x in args])
        if check_forward:
            _cmp(got, exp, atol)
    _cmp(ours.compute(), ref.compute(), atol)


def _vals(seed, n_batches=4, shape=(32,)):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(*shape, generator=g),) for _ in range(n_batches)]


# ------------------------------------------------------------- aggregation
@pytest.mark.parametrize("name", ["MeanMetric", "SumMetric", "MaxMetric", "MinMetric", "CatMetric"])
def test_aggregators(name):
    tm = _tm()
    _drive(getattr(ma, name)(), getattr(tm, name)(), _vals(3))


def test_mean_metric_weighted():
    tm = _tm()
    g = torch.Generator().manual_seed(4)
    batches = [(torch.randn(16, generator=g), torch.rand(16, generator=g)) for _ in range(3)]
    _drive(ma.MeanMetric(), tm.MeanMetric(), batches)


@pytest.mark.parametrize("strategy", ["ignore", 0.5])
def test_aggregator_nan_strategy(strategy):
    tm = _tm()
    g = torch.Generator().manual_seed(5)
    batches = []
    for _ in range(3):
        v = torch.randn(16, generator=g)
        v[::5] = float("nan")
        batches.append((v,))
    _drive(ma.MeanMetric(nan_strategy=strategy), tm.MeanMetric(nan_strategy=strategy), batches)


@pytest.mark.parametrize("name", ["RunningMean", "RunningSum"])
def test_running_aggregators(name):
    tm = _tm()
    _drive(getattr(ma, name)(window=3), getattr(tm, name)(window=3), _vals(6, n_batches=7))


# ----------------------------------------------------------------- wrappers
def _cls_batches(seed, n=4, b=32, c=5):
    g = torch.Generator().manual_seed(seed)
    return [
        (torch.randn(b, c, generator=g).softmax(-1), torch.randint(0, c, (b,), generator=g))
        for _ in range(n)
    ]


def test_classwise_wrapper():
    tm = _tm()
    ours = ma.ClasswiseWrapper(ma.MulticlassAccuracy(num_classes=5, average=None), labels=["a", "b", "c", "d", "e"])
    ref = tm.ClasswiseWrapper(
        tm.classification.MulticlassAccuracy(num_classes=5, average=None), labels=["a", "b", "c", "d", "e"]
    )
    _drive(ours, ref, _cls_batches(6))


def test_minmax_wrapper():
    tm = _tm()
    ours = ma.MinMaxMetric(ma.MulticlassAccuracy(num_classes=5))
    ref = tm.MinMaxMetric(tm.classification.MulticlassAccuracy(num_classes=5))
    _drive(ours, ref, _cls_batches(7))


def test_multioutput_wrapper():
    tm = _tm()
    g = torch.Generator().manual_seed(8)
    batches = [(torch.randn(32, 3, generator=g), torch.randn(32, 3, generator=g)) for _ in range(4)]
    ours = ma.MultioutputWrapper(ma.MeanSquaredError(), num_outputs=3)
    ref = tm.MultioutputWrapper(tm.MeanSquaredError(), num_outputs=3)
    _drive(ours, ref, batches)


def test_multitask_wrapper():
    tm = _tm()
    g = torch.Generator().manual_seed(9)
    ours = ma.MultitaskWrapper({"cls": ma.BinaryAccuracy(), "reg": ma.MeanSquaredError()})
    ref = tm.wrappers.MultitaskWrapper({"cls": tm.classification.BinaryAccuracy(), "reg": tm.MeanSquaredError()})
    for _ in range(3):
        preds = {"cls": torch.rand(32, generator=g), "reg": torch.randn(32, generator=g)}
        target = {"cls": torch.randint(0, 2, (32,), generator=g), "reg": torch.randn(32, generator=g)}
        got = ours(preds, target)
        exp = ref({k: v.clone() for k, v in preds.items()}, {k: v.clone() for k, v in target.items()})
        _cmp(got, exp)
    _cmp(ours.compute(), ref.compute())


def test_running_wrapper():
    tm = _tm()
    ours = ma.Running(ma.MeanMetric(), window=3)
    ref = tm.wrappers.Running(tm.MeanMetric(), window=3)
    _drive(ours, ref, _vals(10, n_batches=7))


def test_metric_tracker():
    tm = _tm()
    ours = ma.MetricTracker(ma.MulticlassAccuracy(num_classes=5))
    ref = tm.MetricTracker(tm.classification.MulticlassAccuracy(num_classes=5))
    for step in range(3):
        ours.increment()
        ref.increment()
        for args in _cls_batches(20 + step, n=2):
            ours.update(*args)
            ref.update(*args)
    _cmp(ours.compute_all(), ref.compute_all())
    b1, i1 = ours.best_metric(return_step=True)
    b2, i2 = ref.best_metric(return_step=True)
    assert i1 == i2
    _cmp(b1, b2)


def test_bootstrapper_same_rng():
    """BootStrapper resampling consumes the global torch RNG — with the same
    seed both implementations must draw identical resamplings."""
    tm = _tm()
    g = torch.Generator().manual_seed(11)
    batches = [
        (torch.rand(64, generator=g), torch.randint(0, 2, (64,), generator=g)) for _ in range(3)
    ]
    ours = ma.BootStrapper(ma.BinaryAccuracy(), num_bootstraps=8, mean=True, std=True)
    ref = tm.BootStrapper(tm.classification.BinaryAccuracy(), num_bootstraps=8, mean=True, std=True)
    torch.manual_seed(123)
    for args in batches:
        ours.update(*args)
    torch.manual_seed(123)
    for args in batches:
        ref.update(*args)
    _cmp(ours.compute(), ref.compute())


# ------------------------------------------------------------- composition
def test_compositional_metric():
    tm = _tm()
    oa, ob = ma.MulticlassAccuracy(num_classes=5), ma.MulticlassPrecision(num_classes=5)
    ra, rb = tm.classification.MulticlassAccuracy(num_classes=5), tm.classification.MulticlassPrecision(num_classes=5)
    ours = (oa + ob) * 2 - 0.5
    ref = (ra + rb) * 2 - 0.5
    for args in _cls_batches(12):
        ours.update(*args)
        ref.update(*args)
    _cmp(ours.compute(), ref.compute())


# -------------------------------------------------------------- collections
def test_collection_compute_groups_match():
    tm = _tm()

    def build(pkg, cls_mod):
        return pkg.MetricCollection([
            cls_mod.MulticlassAccuracy(num_classes=5, average="micro"),
            cls_mod.MulticlassPrecision(num_classes=5),
            cls_mod.MulticlassRecall(num_classes=5),
            cls_mod.MulticlassConfusionMatrix(num_classes=5),
        ])

    ours = build(ma, ma)
    ref = build(tm, tm.classification)
    for args in _cls_batches(13):
        ours.update(*args)
        ref.update(*args)
    _cmp(ours.compute(), ref.compute())
    # our per-class fused state layout lets micro-average metrics share the
    # macro metrics' group (the reference keeps scalar states for micro and
    # cannot merge them) — dedup must be AT LEAST as aggressive, never less
    assert len(ours.compute_groups) <= len(ref.compute_groups), (
        ours.compute_groups,
        ref.compute_groups,
    )


# ------------------------------------------------------------------ text
def test_text_error_rate_modules():
    tm = _tm()
    import random

    rnd = random.Random(41)
    words = ["the", "cat", "sat", "mat", "dog", "ran"]

    def sent():
        return " ".join(rnd.choice(words) for _ in range(rnd.randint(3, 9)))

    batches = [([sent() for _ in range(8)], [sent() for _ in range(8)]) for _ in range(3)]
    for our_cls, ref_cls in [
        (ma.text.CharErrorRate, tm.text.CharErrorRate),
        (ma.text.WordErrorRate, tm.text.WordErrorRate),
        (ma.text.MatchErrorRate, tm.text.MatchErrorRate),
        (ma.text.WordInfoLost, tm.text.WordInfoLost),
        (ma.text.WordInfoPreserved, tm.text.WordInfoPreserved),
        (ma.text.TranslationEditRate, tm.text.TranslationEditRate),
    ]:
        ours, ref = our_cls(), ref_cls()
        for p, t in batches:
            got, exp = ours(p, t), ref(p, t)
            _cmp(got, exp)
        _cmp(ours.compute(), ref.compute())


# ------------------------------------------------------------- retrieval
@pytest.mark.parametrize(
    ("name", "kwargs"),
    [
        ("RetrievalMAP", {}),
        ("RetrievalMRR", {}),
        ("RetrievalPrecision", {"top_k": 3}),
        ("RetrievalRecall", {"top_k": 3}),
        ("RetrievalHitRate", {"top_k": 3}),
        ("RetrievalFallOut", {"top_k": 3}),
        ("RetrievalNormalizedDCG", {}),
        ("RetrievalRPrecision", {}),
        ("RetrievalMAP", {"empty_target_action": "skip"}),
        ("RetrievalPrecision", {"empty_target_action": "pos", "top_k": 2}),
    ],
)
def test_retrieval_modules(name, kwargs):
    tm = _tm()
    g = torch.Generator().manual_seed(51)
    batches = [
        (
            torch.rand(120, generator=g),
            torch.randint(0, 2, (120,), generator=g),
            torch.randint(0, 12, (120,), generator=g),
        )
        for _ in range(3)
    ]
    ours = getattr(ma.retrieval, name)(**kwargs)
    ref = getattr(tm.retrieval, name)(**kwargs)
    for p, t, idx in batches:
        ours.update(p, t, indexes=idx)
        ref.update(p, t, indexes=idx)
    _cmp(ours.compute(), ref.compute())


def test_detection_iou_module():
    tm = _tm()
    from tests.unittests.detection._ref_oracle import load_legacy_map

    load_legacy_map()  # installs the torchvision stub so the ref module runs
    import importlib

    try:
        ref = ref_module("torchmetrics.detection.iou").IntersectionOverUnion()
    except Exception as err:
        pytest.skip(f"reference IoU module unavailable offline: {err}")
    g = torch.Generator().manual_seed(52)

    def boxes(n):
        xy = torch.rand(n, 2, generator=g) * 60
        wh = torch.rand(n, 2, generator=g) * 25 + 4
        return torch.cat([xy, xy + wh], 1)

    ours = ma.detection.IntersectionOverUnion()
    for _ in range(2):
        p = [{"boxes": boxes(6), "scores": torch.rand(6, generator=g), "labels": torch.randint(0, 2, (6,), generator=g)}]
        t = [{"boxes": boxes(4), "labels": torch.randint(0, 2, (4,), generator=g)}]
        ours.update(p, t)
        ref.update(p, t)
    _cmp(ours.compute(), ref.compute())


def test_classification_curve_modules():
    tm = _tm()
    g = torch.Generator().manual_seed(53)
    batches = [(torch.rand(96, generator=g), torch.randint(0, 2, (96,), generator=g)) for _ in range(3)]
    for our_cls, ref_cls, kw in [
        (ma.BinaryROC, tm.classification.BinaryROC, {"thresholds": None}),
        (ma.BinaryROC, tm.classification.BinaryROC, {"thresholds": 15}),
        (ma.BinaryPrecisionRecallCurve, tm.classification.BinaryPrecisionRecallCurve, {"thresholds": None}),
        (ma.BinaryAUROC, tm.classification.BinaryAUROC, {"thresholds": None}),
        (ma.BinaryAveragePrecision, tm.classification.BinaryAveragePrecision, {"thresholds": None}),
        (ma.BinaryCalibrationError, tm.classification.BinaryCalibrationError, {"n_bins": 10}),
    ]:
        ours, ref = our_cls(**kw), ref_cls(**kw)
        for p, t in batches:
            ours.update(p, t)
            ref.update(p, t)
        _cmp(ours.compute(), ref.compute())


def test_transform_wrappers():
    tm = _tm()
    g = torch.Generator().manual_seed(61)
    batches = [(torch.rand(32, generator=g), torch.randint(0, 5, (32,), generator=g)) for _ in range(3)]
    ours = ma.wrappers.BinaryTargetTransformer(ma.BinaryAccuracy(), threshold=2)
    ref = tm.wrappers.BinaryTargetTransformer(tm.classification.BinaryAccuracy(), threshold=2)
    for p, t in batches:
        _cmp(ours(p, t), ref(p, t))
    _cmp(ours.compute(), ref.compute())

    ours2 = ma.wrappers.LambdaInputTransformer(ma.MeanSquaredError(), transform_pred=lambda x: x * 2)
    ref2 = tm.wrappers.LambdaInputTransformer(tm.MeanSquaredError(), transform_pred=lambda x: x * 2)
    for p, t in batches:
        _cmp(ours2(p, t.float()), ref2(p, t.float()))
    _cmp(ours2.compute(), ref2.compute())


def test_feature_share_wrapper():
    tm = _tm()

    class Backbone(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.calls = 0

        def forward(self, x):
            self.calls += 1
            return x.flatten(1)

    # FeatureShare needs metrics with a `feature_network` attribute; use toy
    # FID-style metrics if available on both sides — otherwise skip
    pytest.skip("FeatureShare needs model-backed metrics (offline-gated); covered by wrapper unit tests")


@pytest.mark.parametrize("name", ["IntersectionOverUnion", "GeneralizedIntersectionOverUnion", "DistanceIntersectionOverUnion", "CompleteIntersectionOverUnion"])
@pytest.mark.parametrize("kwargs", [{}, {"respect_labels": False}, {"class_metrics": True}, {"iou_threshold": 0.3}])
def test_detection_iou_family(name, kwargs):
    tm = _tm()
    from tests.unittests.detection._ref_oracle import load_legacy_map

    load_legacy_map()
    # torchmetrics.detection.__init__ gates exports on torchvision at its
    # first import (before our stub existed) — import the submodule directly
    import importlib

    mod_name = {"IntersectionOverUnion": "iou", "GeneralizedIntersectionOverUnion": "giou",
                "DistanceIntersectionOverUnion": "diou", "CompleteIntersectionOverUnion": "ciou"}[name]
    try:
        ref_mod = ref_module(f"torchmetrics.detection.{mod_name}")
        ref = getattr(ref_mod, name)(**kwargs)
    except Exception as err:
        pytest.skip(f"reference module unavailable offline: {err}")
    g = torch.Generator().manual_seed(63)

    def boxes(n):
        xy = torch.rand(n, 2, generator=g) * 60
        wh = torch.rand(n, 2, generator=g) * 25 + 4
        return torch.cat([xy, xy + wh], 1)

    ours = getattr(ma.detection, name)(**kwargs)
    for i in range(3):
        nd, ng = (6, 4) if i != 1 else (0, 3)  # include an empty-preds image
        p = [{"boxes": boxes(nd), "scores": torch.rand(nd, generator=g), "labels": torch.randint(0, 2, (nd,), generator=g)}]
        t = [{"boxes": boxes(ng), "labels": torch.randint(0, 2, (ng,), generator=g)}]
        ours.update(p, t)
        ref.update(p, t)
    _cmp(ours.compute(), ref.compute())


# ------------------------------------------- broad accumulation differential
def _img(seed, s=32):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, 3, s, s, generator=g), torch.rand(2, 3, s, s, generator=g)


def _aud(seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(2, 4000, generator=g)
    return t + 0.4 * torch.randn(2, 4000, generator=g), t


def _reg2(seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(64, generator=g)
    return p, 0.6 * p + 0.5 * torch.randn(64, generator=g)


def _lab(seed, k=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, k, (80,), generator=g), torch.randint(0, k, (80,), generator=g)


def _seg1h(seed, c=3, s=12):
    g = torch.Generator().manual_seed(seed)
    p = torch.nn.functional.one_hot(torch.randint(0, c, (2, s, s), generator=g), c).movedim(-1, 1)
    t = torch.nn.functional.one_hot(torch.randint(0, c, (2, s, s), generator=g), c).movedim(-1, 1)
    return p, t


_ACC_CASES = [
    # (path, kwargs, input_gen, atol)
    ("PeakSignalNoiseRatio", {}, _img, 1e-4),
    ("PeakSignalNoiseRatio", {"data_range": 1.0}, _img, 1e-4),
    ("StructuralSimilarityIndexMeasure", {"data_range": 1.0}, _img, 1e-5),
    ("MultiScaleStructuralSimilarityIndexMeasure", {"data_range": 1.0}, lambda s: _img(s, 192), 1e-4),
    ("UniversalImageQualityIndex", {}, _img, 1e-5),
    ("SpectralAngleMapper", {}, _img, 1e-5),
    ("ErrorRelativeGlobalDimensionlessSynthesis", {}, _img, 1e-3),
    ("RelativeAverageSpectralError", {}, _img, 1e-3),
    ("RootMeanSquaredErrorUsingSlidingWindow", {}, _img, 1e-4),
    ("TotalVariation", {}, lambda s: (_img(s)[0],), 1e-3),
    ("TotalVariation", {"reduction": "mean"}, lambda s: (_img(s)[0],), 1e-4),
    ("SignalNoiseRatio", {}, _aud, 1e-4),
    ("ScaleInvariantSignalNoiseRatio", {}, _aud, 1e-4),
    ("SignalDistortionRatio", {}, _aud, 1e-2),
    ("ScaleInvariantSignalDistortionRatio", {}, _aud, 1e-4),
    ("MeanSquaredError", {}, _reg2, 1e-5),
    ("MeanAbsoluteError", {}, _reg2, 1e-5),
    ("MeanSquaredLogError", {}, lambda s: tuple(x.abs() for x in _reg2(s)), 1e-5),
    ("LogCoshError", {}, _reg2, 1e-5),
    ("MinkowskiDistance", {"p": 3}, _reg2, 1e-4),
    ("TweedieDevianceScore", {"power": 1.5}, lambda s: tuple(x.abs() + 0.1 for x in _reg2(s)), 1e-4),
    ("KLDivergence", {}, lambda s: (torch.rand(8, 5, generator=torch.Generator().manual_seed(s)).softmax(-1), torch.rand(8, 5, generator=torch.Generator().manual_seed(s + 1)).softmax(-1)), 1e-5),
    ("CosineSimilarity", {}, lambda s: (torch.randn(16, 8, generator=torch.Generator().manual_seed(s)), torch.randn(16, 8, generator=torch.Generator().manual_seed(s + 1))), 1e-5),
    ("ExplainedVariance", {}, _reg2, 1e-5),
    ("R2Score", {}, _reg2, 1e-5),
    ("PearsonCorrCoef", {}, _reg2, 1e-5),
    ("SpearmanCorrCoef", {}, _reg2, 1e-5),
    ("KendallRankCorrCoef", {}, _reg2, 1e-5),
    ("ConcordanceCorrCoef", {}, _reg2, 1e-5),
    ("CriticalSuccessIndex", {"threshold": 0.5}, lambda s: (torch.rand(100, generator=torch.Generator().manual_seed(s)), torch.rand(100, generator=torch.Generator().manual_seed(s + 1))), 1e-5),
    ("CohenKappa", {"task": "binary"}, lambda s: (torch.rand(80, generator=torch.Generator().manual_seed(s)), torch.randint(0, 2, (80,), generator=torch.Generator().manual_seed(s + 1))), 1e-5),
]

_ACC_NS = [
    ("image", "SpatialCorrelationCoefficient", {}, _img, 1e-4),
    ("image", "VisualInformationFidelity", {}, lambda s: _img(s, 64), 1e-4),
    ("image", "PeakSignalNoiseRatioWithBlockedEffect", {}, lambda s: tuple(x[:, :1] for x in _img(s)), 1e-4),
    ("clustering", "MutualInfoScore", {}, _lab, 1e-5),
    ("clustering", "AdjustedRandScore", {}, _lab, 1e-5),
    ("clustering", "NormalizedMutualInfoScore", {}, _lab, 1e-5),
    ("clustering", "FowlkesMallowsIndex", {}, _lab, 1e-5),
    ("clustering", "HomogeneityScore", {}, _lab, 1e-5),
    ("clustering", "CompletenessScore", {}, _lab, 1e-5),
    ("clustering", "VMeasureScore", {}, _lab, 1e-5),
    ("nominal", "CramersV", {"num_classes": 5}, _lab, 1e-4),
    ("nominal", "PearsonsContingencyCoefficient", {"num_classes": 5}, _lab, 1e-4),
    ("nominal", "TschuprowsT", {"num_classes": 5}, _lab, 1e-4),
    ("nominal", "TheilsU", {"num_classes": 5}, _lab, 1e-4),
    ("segmentation", "MeanIoU", {"num_classes": 3}, _seg1h, 1e-5),
    ("segmentation", "DiceScore", {"num_classes": 3}, _seg1h, 1e-5),
    ("segmentation", "GeneralizedDiceScore", {"num_classes": 3}, _seg1h, 1e-5),
    ("segmentation", "HausdorffDistance", {"num_classes": 3}, _seg1h, 1e-4),
]


def _acc_check(our_cls, ref_cls, kwargs, gen, atol):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = our_cls(**kwargs), ref_cls(**kwargs)
        for b in range(3):
            args = gen(90 + b)
            ours.update(*args)
            ref.update(*args)
        _cmp(ours.compute(), ref.compute(), atol)


@pytest.mark.parametrize(
    ("name", "kwargs", "gen", "atol"), _ACC_CASES, ids=[f"{c[0]}_{i}" for i, c in enumerate(_ACC_CASES)]
)
def test_modular_accumulation(name, kwargs, gen, atol):
    tm = _tm()
    _acc_check(getattr(ma, name), getattr(tm, name), kwargs, gen, atol)


@pytest.mark.parametrize(
    ("ns", "name", "kwargs", "gen", "atol"), _ACC_NS, ids=[f"{c[1]}_{i}" for i, c in enumerate(_ACC_NS)]
)
def test_modular_accumulation_ns(ns, name, kwargs, gen, atol):
    import importlib

    _tm()
    our_ns = importlib.import_module(f"metrics_amd.{ns}")
    ref_ns = ref_module(f"torchmetrics.{ns}")
    our_cls = getattr(our_ns, name, None)
    ref_cls = getattr(ref_ns, name, None)
    if our_cls is None or ref_cls is None:
        pytest.fail(f"{ns}.{name} missing: ours={our_cls is not None} ref={ref_cls is not None}")
    _acc_check(our_cls, ref_cls, kwargs, gen, atol)


def _panoptic(seed):
    # preds = target with 15% label noise so IoU>0.5 matches actually occur
    # (fully random maps give PQ == 0 on both sides, a trivial comparison)
    g = torch.Generator().manual_seed(seed)
    cat = torch.tensor([0, 1, 2, 7])[torch.randint(0, 4, (2, 16, 16), generator=g)]
    inst = torch.randint(0, 3, (2, 16, 16), generator=g)
    pt = torch.stack([cat, inst], dim=-1)
    pp = pt.clone()
    noise = torch.rand(pt.shape[:-1], generator=g) < 0.15
    pp[..., 0][noise] = torch.tensor([0, 1, 2, 7])[torch.randint(0, 4, (int(noise.sum()),), generator=g)]
    return pp, pt


def _multisrc(seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(2, 3, 1500, generator=g)
    return t + 0.3 * torch.randn(2, 3, 1500, generator=g), t


def _texts(seed):
    corpus = [
        "the cat sat on the mat",
        "a quick brown fox jumps over the lazy dog",
        "hello world this is a test",
        "metrics are computed on device",
        "the rain in spain stays mainly on the plain",
        "pack my box with five dozen liquor jugs",
    ]
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, len(corpus), (4,), generator=g).tolist()
    jdx = torch.randint(0, len(corpus), (4,), generator=g).tolist()
    preds = [corpus[i] for i in idx]
    target = [[corpus[j], corpus[(j + 1) % len(corpus)]] for j in jdx]
    return preds, target


def _texts_flat(seed):
    p, t = _texts(seed)
    return p, [x[0] for x in t]


_ACC_NS2 = [
    ("detection", "PanopticQuality", {"things": {1, 2}, "stuffs": {7}, "allow_unknown_preds_category": True}, _panoptic, 1e-5),
    ("detection", "ModifiedPanopticQuality", {"things": {1, 2}, "stuffs": {7}, "allow_unknown_preds_category": True}, _panoptic, 1e-5),
    ("audio", "ComplexScaleInvariantSignalNoiseRatio", {}, lambda s: (torch.randn(2, 40, 10, 2, generator=torch.Generator().manual_seed(s)), torch.randn(2, 40, 10, 2, generator=torch.Generator().manual_seed(s + 1))), 1e-4),
    ("audio", "SourceAggregatedSignalDistortionRatio", {}, _multisrc, 1e-4),
    ("audio", "PermutationInvariantTraining", {"metric_func": None}, _multisrc, 1e-4),
    ("text", "BLEUScore", {}, _texts, 1e-5),
    ("text", "BLEUScore", {"n_gram": 2, "smooth": True}, _texts, 1e-5),
    ("text", "SacreBLEUScore", {}, _texts, 1e-5),
    ("text", "CHRFScore", {}, _texts, 1e-5),
    ("text", "CHRFScore", {"return_sentence_level_score": True}, _texts, 1e-5),
    ("text", "TranslationEditRate", {}, _texts, 1e-5),
    ("text", "CharErrorRate", {}, _texts_flat, 1e-5),
    ("text", "WordErrorRate", {}, _texts_flat, 1e-5),
    ("text", "MatchErrorRate", {}, _texts_flat, 1e-5),
    ("text", "WordInfoLost", {}, _texts_flat, 1e-5),
    ("text", "WordInfoPreserved", {}, _texts_flat, 1e-5),
    ("text", "ExtendedEditDistance", {}, _texts_flat, 1e-5),
    ("text", "EditDistance", {}, _texts_flat, 1e-5),
    ("text", "EditDistance", {"reduction": "sum"}, _texts_flat, 1e-5),
]


@pytest.mark.parametrize(
    ("ns", "name", "kwargs", "gen", "atol"), _ACC_NS2, ids=[f"{c[1]}_{i}" for i, c in enumerate(_ACC_NS2)]
)
def test_modular_accumulation_ns2(ns, name, kwargs, gen, atol):
    import importlib

    _tm()
    if name == "PermutationInvariantTraining":
        import metrics_amd.functional.audio as our_fa

        ref_fa = ref_module("torchmetrics.functional.audio")

        our_kw = {"metric_func": our_fa.scale_invariant_signal_noise_ratio}
        ref_kw = {"metric_func": ref_fa.scale_invariant_signal_noise_ratio}
    else:
        our_kw = ref_kw = kwargs
    our_ns = importlib.import_module(f"metrics_amd.{ns}")
    ref_ns = ref_module(f"torchmetrics.{ns}")
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = getattr(our_ns, name)(**our_kw), getattr(ref_ns, name)(**ref_kw)
        for b in range(3):
            args = gen(90 + b)
            ours.update(*args)
            ref.update(*args)
        _cmp(ours.compute(), ref.compute(), atol)


def _dlambda(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, 4, 16, 16, generator=g), torch.rand(2, 4, 16, 16, generator=g)


_ACC_NS3 = [
    ("regression", "MeanAbsolutePercentageError", {}, lambda s: tuple(x.abs() + 0.1 for x in _reg2(s)), 1e-5),
    ("regression", "SymmetricMeanAbsolutePercentageError", {}, lambda s: tuple(x.abs() + 0.1 for x in _reg2(s)), 1e-5),
    ("regression", "WeightedMeanAbsolutePercentageError", {}, lambda s: tuple(x.abs() + 0.1 for x in _reg2(s)), 1e-5),
    ("regression", "RelativeSquaredError", {}, _reg2, 1e-5),
    ("regression", "RelativeSquaredError", {"squared": False}, _reg2, 1e-5),
    ("regression", "NormalizedRootMeanSquaredError", {"normalization": "mean"}, lambda s: tuple(x.abs() + 0.1 for x in _reg2(s)), 1e-5),
    ("regression", "NormalizedRootMeanSquaredError", {"normalization": "range"}, _reg2, 1e-5),
    ("regression", "NormalizedRootMeanSquaredError", {"normalization": "std"}, _reg2, 1e-5),
    ("image", "SpectralDistortionIndex", {}, _dlambda, 1e-5),
    ("image", "QualityWithNoReference", {}, lambda s: (
        torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(s)),
        {
            "ms": torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(s + 1)),
            "pan": torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(s + 2)),
            "pan_lr": torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(s + 3)),
        },
    ), 1e-4),
]


@pytest.mark.parametrize(
    ("ns", "name", "kwargs", "gen", "atol"), _ACC_NS3, ids=[f"{c[1]}_{i}" for i, c in enumerate(_ACC_NS3)]
)
def test_modular_accumulation_ns3(ns, name, kwargs, gen, atol):
    import importlib
    import warnings

    _tm()
    our_ns = importlib.import_module(f"metrics_amd.{ns}")
    ref_ns = ref_module(f"torchmetrics.{ns}")
    our_cls = getattr(our_ns, name, None)
    ref_cls = getattr(ref_ns, name, None)
    if ref_cls is None:
        pytest.skip(f"{ns}.{name} absent in reference")
    assert our_cls is not None, f"{ns}.{name} missing in metrics_amd"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = our_cls(**kwargs), ref_cls(**kwargs)
        for b in range(3):
            args = gen(90 + b)
            ours.update(*args)
            ref.update(*args)
        _cmp(ours.compute(), ref.compute(), atol)


_FWD_CASES = [c for c in _ACC_CASES if c[0] not in {"SpearmanCorrCoef", "KendallRankCorrCoef"}]


@pytest.mark.parametrize(
    ("name", "kwargs", "gen", "atol"), _FWD_CASES, ids=[f"{c[0]}_{i}" for i, c in enumerate(_FWD_CASES)]
)
def test_modular_forward(name, kwargs, gen, atol):
    """forward() parity: per-batch return values AND the accumulated compute.

    Exercises the full-state/reduced-state forward machinery, which the
    update()-based accumulation differential does not touch.
    """
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = getattr(ma, name)(**kwargs), getattr(tm, name)(**kwargs)
        for b in range(3):
            args = gen(70 + b)
            _cmp(ours(*args), ref(*args), atol)
        _cmp(ours.compute(), ref.compute(), atol)


_FWD_NS = [c for c in _ACC_NS + _ACC_NS2 + _ACC_NS3 if c[1] not in {"PermutationInvariantTraining"}]


@pytest.mark.parametrize(
    ("ns", "name", "kwargs", "gen", "atol"), _FWD_NS, ids=[f"{c[1]}_{i}" for i, c in enumerate(_FWD_NS)]
)
def test_modular_forward_ns(ns, name, kwargs, gen, atol):
    import importlib
    import warnings

    _tm()
    our_ns = importlib.import_module(f"metrics_amd.{ns}")
    ref_ns = ref_module(f"torchmetrics.{ns}")
    our_cls = getattr(our_ns, name, None)
    ref_cls = getattr(ref_ns, name, None)
    if ref_cls is None:
        pytest.skip(f"{ns}.{name} absent in reference")
    assert our_cls is not None, f"{ns}.{name} missing in metrics_amd"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = our_cls(**kwargs), ref_cls(**kwargs)
        for b in range(3):
            args = gen(70 + b)
            _cmp(ours(*args), ref(*args), atol)
        _cmp(ours.compute(), ref.compute(), atol)


def _bin_pt(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(120, generator=g), torch.randint(0, 2, (120,), generator=g)


def _mc_pt(seed, c=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(120, c, generator=g).softmax(-1), torch.randint(0, c, (120,), generator=g)


def _ml_pt(seed, l=4):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(120, l, generator=g), torch.randint(0, 2, (120, l), generator=g)


_CLS_FWD = [
    ("BinaryAccuracy", {}, _bin_pt),
    ("BinaryAccuracy", {"ignore_index": 0}, _bin_pt),
    ("BinaryPrecision", {}, _bin_pt),
    ("BinaryRecall", {"threshold": 0.3}, _bin_pt),
    ("BinaryF1Score", {}, _bin_pt),
    ("BinaryFBetaScore", {"beta": 0.5}, _bin_pt),
    ("BinarySpecificity", {}, _bin_pt),
    ("BinaryCohenKappa", {}, _bin_pt),
    ("BinaryMatthewsCorrCoef", {}, _bin_pt),
    ("BinaryHammingDistance", {}, _bin_pt),
    ("BinaryJaccardIndex", {}, _bin_pt),
    ("BinaryAUROC", {}, _bin_pt),
    ("BinaryAUROC", {"thresholds": 25}, _bin_pt),
    ("BinaryAveragePrecision", {}, _bin_pt),
    ("BinaryCalibrationError", {}, _bin_pt),
    ("BinaryStatScores", {}, _bin_pt),
    ("BinaryConfusionMatrix", {}, _bin_pt),
    ("BinaryNegativePredictiveValue", {}, _bin_pt),
    ("BinaryHingeLoss", {}, _bin_pt),
    ("MulticlassAccuracy", {"num_classes": 5}, _mc_pt),
    ("MulticlassAccuracy", {"num_classes": 5, "average": "micro"}, _mc_pt),
    ("MulticlassAccuracy", {"num_classes": 5, "average": "weighted"}, _mc_pt),
    ("MulticlassAccuracy", {"num_classes": 5, "average": None}, _mc_pt),
    ("MulticlassAccuracy", {"num_classes": 5, "top_k": 2}, _mc_pt),
    ("MulticlassAccuracy", {"num_classes": 5, "ignore_index": 2}, _mc_pt),
    ("MulticlassPrecision", {"num_classes": 5}, _mc_pt),
    ("MulticlassRecall", {"num_classes": 5, "average": "weighted"}, _mc_pt),
    ("MulticlassF1Score", {"num_classes": 5}, _mc_pt),
    ("MulticlassFBetaScore", {"num_classes": 5, "beta": 2.0}, _mc_pt),
    ("MulticlassSpecificity", {"num_classes": 5}, _mc_pt),
    ("MulticlassCohenKappa", {"num_classes": 5}, _mc_pt),
    ("MulticlassCohenKappa", {"num_classes": 5, "weights": "linear"}, _mc_pt),
    ("MulticlassMatthewsCorrCoef", {"num_classes": 5}, _mc_pt),
    ("MulticlassJaccardIndex", {"num_classes": 5}, _mc_pt),
    ("MulticlassAUROC", {"num_classes": 5}, _mc_pt),
    ("MulticlassAUROC", {"num_classes": 5, "thresholds": 25}, _mc_pt),
    ("MulticlassAveragePrecision", {"num_classes": 5}, _mc_pt),
    ("MulticlassCalibrationError", {"num_classes": 5}, _mc_pt),
    ("MulticlassExactMatch", {"num_classes": 5}, lambda s: (_mc_pt(s)[0].reshape(24, 5, 5).argmax(1), _mc_pt(s)[1].reshape(24, 5))),
    ("MulticlassConfusionMatrix", {"num_classes": 5}, _mc_pt),
    ("MulticlassHingeLoss", {"num_classes": 5}, _mc_pt),
    ("MultilabelAccuracy", {"num_labels": 4}, _ml_pt),
    ("MultilabelAccuracy", {"num_labels": 4, "average": "micro"}, _ml_pt),
    ("MultilabelPrecision", {"num_labels": 4}, _ml_pt),
    ("MultilabelRecall", {"num_labels": 4}, _ml_pt),
    ("MultilabelF1Score", {"num_labels": 4}, _ml_pt),
    ("MultilabelSpecificity", {"num_labels": 4}, _ml_pt),
    ("MultilabelHammingDistance", {"num_labels": 4}, _ml_pt),
    ("MultilabelJaccardIndex", {"num_labels": 4}, _ml_pt),
    ("MultilabelAUROC", {"num_labels": 4}, _ml_pt),
    ("MultilabelAveragePrecision", {"num_labels": 4}, _ml_pt),
    ("MultilabelExactMatch", {"num_labels": 4}, _ml_pt),
    ("MultilabelRankingAveragePrecision", {"num_labels": 4}, _ml_pt),
    ("MultilabelRankingLoss", {"num_labels": 4}, _ml_pt),
    ("MultilabelCoverageError", {"num_labels": 4}, _ml_pt),
    ("MultilabelConfusionMatrix", {"num_labels": 4}, _ml_pt),
]


@pytest.mark.parametrize(
    ("name", "kwargs", "gen"), _CLS_FWD, ids=[f"{c[0]}_{i}" for i, c in enumerate(_CLS_FWD)]
)
def test_classification_forward(name, kwargs, gen):
    import warnings

    tm = _tm()
    our_cls = getattr(ma.classification, name)
    ref_cls = getattr(tm.classification, name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = our_cls(**kwargs), ref_cls(**kwargs)
        for b in range(3):
            args = gen(60 + b)
            _cmp(ours(*args), ref(*args), 1e-5)
        _cmp(ours.compute(), ref.compute(), 1e-5)


def _ret_pt(seed):
    g = torch.Generator().manual_seed(seed)
    n = 150
    return (
        torch.rand(n, generator=g),
        torch.randint(0, 2, (n,), generator=g),
        torch.randint(0, 12, (n,), generator=g),
    )


_RET_FWD = [
    ("RetrievalMAP", {}),
    ("RetrievalMRR", {}),
    ("RetrievalNormalizedDCG", {}),
    ("RetrievalNormalizedDCG", {"top_k": 5}),
    ("RetrievalPrecision", {"top_k": 3}),
    ("RetrievalRecall", {"top_k": 3}),
    ("RetrievalFallOut", {"top_k": 3}),
    ("RetrievalHitRate", {"top_k": 3}),
    ("RetrievalRPrecision", {}),
    ("RetrievalAUROC", {}),
]


@pytest.mark.parametrize(("name", "kwargs"), _RET_FWD, ids=[f"{c[0]}_{i}" for i, c in enumerate(_RET_FWD)])
def test_retrieval_forward(name, kwargs):
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = getattr(ma.retrieval, name)(**kwargs)
        ref = getattr(tm.retrieval, name)(**kwargs)
        for b in range(3):
            p, t, idx = _ret_pt(60 + b)
            _cmp(ours(p, t, indexes=idx), ref(p, t, indexes=idx), 1e-5)
        _cmp(ours.compute(), ref.compute(), 1e-5)


def test_wrappers_forward_differential():
    """forward() parity for the wrapper classes around a live base metric."""
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = [
            (
                ma.MultioutputWrapper(ma.MeanSquaredError(), num_outputs=3),
                tm.MultioutputWrapper(tm.MeanSquaredError(), num_outputs=3),
                lambda s: (
                    torch.randn(32, 3, generator=torch.Generator().manual_seed(s)),
                    torch.randn(32, 3, generator=torch.Generator().manual_seed(s + 1)),
                ),
            ),
            (
                ma.wrappers.Running(ma.MeanSquaredError(), window=2),
                tm.wrappers.Running(tm.MeanSquaredError(), window=2),
                lambda s: (
                    torch.randn(32, generator=torch.Generator().manual_seed(s)),
                    torch.randn(32, generator=torch.Generator().manual_seed(s + 1)),
                ),
            ),
            (
                ma.ClasswiseWrapper(ma.MulticlassF1Score(num_classes=4, average=None)),
                tm.ClasswiseWrapper(tm.classification.MulticlassF1Score(num_classes=4, average=None)),
                lambda s: (
                    torch.randn(64, 4, generator=torch.Generator().manual_seed(s)).softmax(-1),
                    torch.randint(0, 4, (64,), generator=torch.Generator().manual_seed(s + 1)),
                ),
            ),
        ]
        for ours, ref, gen in pairs:
            for b in range(4):
                args = gen(50 + b)
                _cmp(ours(*args), ref(*args), 1e-5)
            _cmp(ours.compute(), ref.compute(), 1e-5)


def test_collection_forward_differential():
    """MetricCollection forward parity (compute groups on) across mixed tasks."""
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = ma.MetricCollection(
            {
                "acc": ma.MulticlassAccuracy(num_classes=5),
                "prec": ma.MulticlassPrecision(num_classes=5),
                "auroc": ma.MulticlassAUROC(num_classes=5),
                "cal": ma.MulticlassCalibrationError(num_classes=5),
            }
        )
        ref = tm.MetricCollection(
            {
                "acc": tm.classification.MulticlassAccuracy(num_classes=5),
                "prec": tm.classification.MulticlassPrecision(num_classes=5),
                "auroc": tm.classification.MulticlassAUROC(num_classes=5),
                "cal": tm.classification.MulticlassCalibrationError(num_classes=5),
            }
        )
        for b in range(3):
            g = torch.Generator().manual_seed(40 + b)
            p = torch.randn(96, 5, generator=g).softmax(-1)
            t = torch.randint(0, 5, (96,), generator=g)
            vo, vr = ours(p, t), ref(p, t)
            assert set(vo) == set(vr)
            for k in vr:
                _cmp(vo[k], vr[k], 1e-5)
        vo, vr = ours.compute(), ref.compute()
        for k in vr:
            _cmp(vo[k], vr[k], 1e-5)


def test_rouge_perplexity_accumulation():
    """ROUGE (dict-valued) and Perplexity accumulation parity."""
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # rougeLsum needs nltk in the reference (not installable offline)
        keys = ("rouge1", "rouge2", "rougeL")
        ours = ma.text.ROUGEScore(rouge_keys=keys)
        ref = tm.text.ROUGEScore(rouge_keys=keys)
        for b in range(3):
            p, t = _texts_flat(80 + b)
            ours.update(p, t)
            ref.update(p, t)
        vo, vr = ours.compute(), ref.compute()
        assert set(vo) == set(vr)
        for k in vr:
            _cmp(vo[k], vr[k], 1e-5)

        op = ma.text.Perplexity(ignore_index=-100)
        rp = tm.text.Perplexity(ignore_index=-100)
        for b in range(3):
            g = torch.Generator().manual_seed(80 + b)
            logits = torch.randn(2, 8, 20, generator=g)
            target = torch.randint(0, 20, (2, 8), generator=g)
            target[0, :2] = -100
            op.update(logits, target)
            rp.update(logits, target)
        _cmp(op.compute(), rp.compute(), 1e-4)


def test_rouge_forward_differential():
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = ma.text.ROUGEScore(use_stemmer=False, rouge_keys=("rouge1", "rouge2", "rougeL"))
        ref = tm.text.ROUGEScore(use_stemmer=False, rouge_keys=("rouge1", "rouge2", "rougeL"))
        for b in range(3):
            p, t = _texts_flat(85 + b)
            vo, vr = ours(p, t), ref(p, t)
            for k in vr:
                _cmp(vo[k], vr[k], 1e-5)
        vo, vr = ours.compute(), ref.compute()
        for k in vr:
            _cmp(vo[k], vr[k], 1e-5)


def test_aggregation_differential():
    """SumMetric/MeanMetric/MaxMetric/MinMetric/CatMetric + Running wrappers
    under each nan strategy, with scalar / tensor / weighted updates."""
    import warnings

    tm = _tm()
    g = torch.Generator().manual_seed(5)
    batches = [torch.randn(6, generator=g) for _ in range(3)]
    batches[1][2] = float("nan")
    weights = [torch.rand(6, generator=g) + 0.1 for _ in range(3)]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("SumMetric", "MaxMetric", "MinMetric", "CatMetric"):
            for nan_strategy in ("warn", "ignore", 0.5):
                if name in ("MaxMetric", "MinMetric") and nan_strategy == "ignore":
                    pass
                ours = getattr(ma, name)(nan_strategy=nan_strategy)
                ref = getattr(tm, name)(nan_strategy=nan_strategy)
                for b in batches:
                    ours.update(b)
                    ref.update(b)
                _cmp(ours.compute(), ref.compute(), 1e-6)

        for nan_strategy in ("warn", "ignore", 0.25):
            ours = ma.MeanMetric(nan_strategy=nan_strategy)
            ref = tm.MeanMetric(nan_strategy=nan_strategy)
            for b, w in zip(batches, weights):
                ours.update(b, w)
                ref.update(b, w)
            _cmp(ours.compute(), ref.compute(), 1e-6)

        # scalar updates + default weight path
        ours = ma.MeanMetric()
        ref = tm.MeanMetric()
        for v in (1.5, 2.0, -0.5):
            ours.update(v)
            ref.update(v)
        _cmp(ours.compute(), ref.compute(), 1e-6)

        for cls_name in ("RunningMean", "RunningSum"):
            ours = getattr(ma, cls_name)(window=2)
            ref = getattr(tm, cls_name)(window=2)
            for b in batches:
                vo, vr = ours(b.nan_to_num()), ref(b.nan_to_num())
                _cmp(vo, vr, 1e-6)
            _cmp(ours.compute(), ref.compute(), 1e-6)


_DTYPE_CASES = [
    ("MeanSquaredError", {}, _reg2),
    ("PearsonCorrCoef", {}, _reg2),
    ("PeakSignalNoiseRatio", {}, _img),
    ("StructuralSimilarityIndexMeasure", {"data_range": 1.0}, _img),
    ("UniversalImageQualityIndex", {}, _img),
    ("ScaleInvariantSignalNoiseRatio", {}, _aud),
    ("R2Score", {}, _reg2),
]


@pytest.mark.parametrize(("name", "kwargs", "gen"), _DTYPE_CASES, ids=[c[0] for c in _DTYPE_CASES])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float16])
def test_modular_dtype_parity(name, kwargs, gen, dtype):
    """fp64/fp16 inputs accumulate to the same value as the reference."""
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = getattr(ma, name)(**kwargs), getattr(tm, name)(**kwargs)
        for b in range(2):
            args = tuple(x.to(dtype) for x in gen(95 + b))
            ours.update(*args)
            ref.update(*args)
        atol = 1e-6 if dtype == torch.float64 else 1e-2
        _cmp(ours.compute().float(), ref.compute().float(), atol)


def _emb(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(60, 4, generator=g), torch.randint(0, 3, (60,), generator=g)


_ACC_NS4 = [
    ("classification", "BinaryPrecisionAtFixedRecall", {"min_recall": 0.5}, _bin_pt, 1e-5),
    ("classification", "BinaryRecallAtFixedPrecision", {"min_precision": 0.5}, _bin_pt, 1e-5),
    ("classification", "BinarySpecificityAtSensitivity", {"min_sensitivity": 0.5}, _bin_pt, 1e-5),
    ("classification", "BinarySensitivityAtSpecificity", {"min_specificity": 0.5}, _bin_pt, 1e-5),
    ("classification", "BinaryLogAUC", {}, _bin_pt, 1e-4),
    ("classification", "MulticlassPrecisionAtFixedRecall", {"num_classes": 5, "min_recall": 0.5}, _mc_pt, 1e-5),
    ("classification", "MulticlassRecallAtFixedPrecision", {"num_classes": 5, "min_precision": 0.5}, _mc_pt, 1e-5),
    ("clustering", "CalinskiHarabaszScore", {}, _emb, 1e-4),
    ("clustering", "DaviesBouldinScore", {}, _emb, 1e-4),
    ("clustering", "DunnIndex", {}, _emb, 1e-4),
    ("clustering", "RandScore", {}, _lab, 1e-5),
    ("clustering", "AdjustedMutualInfoScore", {}, _lab, 1e-5),
]


@pytest.mark.parametrize(
    ("ns", "name", "kwargs", "gen", "atol"), _ACC_NS4, ids=[f"{c[1]}_{i}" for i, c in enumerate(_ACC_NS4)]
)
def test_modular_accumulation_ns4(ns, name, kwargs, gen, atol):
    import importlib
    import warnings

    _tm()
    our_ns = importlib.import_module(f"metrics_amd.{ns}")
    ref_ns = ref_module(f"torchmetrics.{ns}")
    our_cls = getattr(our_ns, name, None)
    ref_cls = getattr(ref_ns, name, None)
    if ref_cls is None:
        pytest.skip(f"{ns}.{name} absent in reference")
    assert our_cls is not None, f"{ns}.{name} missing in metrics_amd"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = our_cls(**kwargs), ref_cls(**kwargs)
        for b in range(3):
            args = gen(90 + b)
            ours.update(*args)
            ref.update(*args)
        _cmp(ours.compute(), ref.compute(), atol)


_ACC_NS5 = [
    ("segmentation", "MeanIoU", {"num_classes": 3, "per_class": True}, _seg1h, 1e-5),
    ("segmentation", "DiceScore", {"num_classes": 3, "average": "micro"}, _seg1h, 1e-5),
    ("segmentation", "DiceScore", {"num_classes": 3, "average": "none"}, _seg1h, 1e-5),
    ("segmentation", "GeneralizedDiceScore", {"num_classes": 3, "per_class": True}, _seg1h, 1e-5),
    ("segmentation", "MeanIoU", {"num_classes": 3, "input_format": "index"},
     lambda s: tuple(x.argmax(1) for x in _seg1h(s)), 1e-5),
    ("regression", "CosineSimilarity", {"reduction": "sum"},
     lambda s: (torch.randn(16, 8, generator=torch.Generator().manual_seed(s)),
                torch.randn(16, 8, generator=torch.Generator().manual_seed(s + 1))), 1e-4),
    ("regression", "ExplainedVariance", {"multioutput": "raw_values"},
     lambda s: (torch.randn(64, 3, generator=torch.Generator().manual_seed(s)),
                torch.randn(64, 3, generator=torch.Generator().manual_seed(s + 1))), 1e-5),
    ("regression", "R2Score", {"multioutput": "variance_weighted"},
     lambda s: (torch.randn(64, 3, generator=torch.Generator().manual_seed(s)),
                torch.randn(64, 3, generator=torch.Generator().manual_seed(s + 1))), 1e-5),
    ("regression", "R2Score", {"adjusted": 2},
     lambda s: (torch.randn(64, 3, generator=torch.Generator().manual_seed(s)),
                torch.randn(64, 3, generator=torch.Generator().manual_seed(s + 1))), 1e-5),
]


@pytest.mark.parametrize(
    ("ns", "name", "kwargs", "gen", "atol"), _ACC_NS5, ids=[f"{c[1]}_{i}" for i, c in enumerate(_ACC_NS5)]
)
def test_modular_accumulation_ns5(ns, name, kwargs, gen, atol):
    import importlib
    import warnings

    _tm()
    our_ns = importlib.import_module(f"metrics_amd.{ns}")
    ref_ns = ref_module(f"torchmetrics.{ns}")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours, ref = getattr(our_ns, name)(**kwargs), getattr(ref_ns, name)(**kwargs)
        for b in range(3):
            args = gen(90 + b)
            ours.update(*args)
            ref.update(*args)
        _cmp(ours.compute(), ref.compute(), atol)


def test_compositional_differential():
    """Metric arithmetic (CompositionalMetric) parity with the reference."""
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")

        def make(mod):
            a = mod.classification.BinaryPrecision()
            b = mod.classification.BinaryRecall()
            return a, b

        for expr in (
            lambda a, b: a + b,
            lambda a, b: 2 * a * b / (a + b + 1e-8),  # F1 from parts
            lambda a, b: a - b,
            lambda a, b: a**2,
            lambda a, b: abs(a - b),
            lambda a, b: a == b,
        ):
            oa, ob = make(ma)
            ra, rb = make(tm)
            oc, rc = expr(oa, ob), expr(ra, rb)
            for s in range(3):
                g = torch.Generator().manual_seed(30 + s)
                p = torch.rand(80, generator=g)
                t = torch.randint(0, 2, (80,), generator=g)
                oc.update(p, t)
                rc.update(p, t)
            _cmp(oc.compute().float(), rc.compute().float(), 1e-6)


def test_tracker_multi_epoch_differential():
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = ma.MetricTracker(ma.MulticlassAccuracy(num_classes=4), maximize=True)
        ref = tm.MetricTracker(tm.classification.MulticlassAccuracy(num_classes=4), maximize=True)
        for epoch in range(3):
            ours.increment()
            ref.increment()
            for b in range(2):
                g = torch.Generator().manual_seed(epoch * 10 + b)
                p = torch.randn(50, 4, generator=g).softmax(-1)
                t = torch.randint(0, 4, (50,), generator=g)
                ours.update(p, t)
                ref.update(p, t)
        _cmp(torch.stack(ours.compute_all() if isinstance(ours.compute_all(), list) else [ours.compute_all()]).flatten(),
             torch.stack(ref.compute_all() if isinstance(ref.compute_all(), list) else [ref.compute_all()]).flatten(), 1e-6)
        ob, oi = ours.best_metric(return_step=True)
        rb, ri = ref.best_metric(return_step=True)
        assert abs(float(ob) - float(rb)) < 1e-6 and int(oi) == int(ri)


@pytest.mark.parametrize("aggregation", ["mean", "median", "min", "max"])
def test_retrieval_aggregation_differential(aggregation):
    import warnings

    tm = _tm()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("RetrievalMAP", "RetrievalMRR", "RetrievalPrecision"):
            kw = {"aggregation": aggregation}
            if name == "RetrievalPrecision":
                kw["top_k"] = 3
            ours = getattr(ma.retrieval, name)(**kw)
            ref = getattr(tm.retrieval, name)(**kw)
            for b in range(2):
                p, t, idx = _ret_pt(60 + b)
                ours.update(p, t, indexes=idx)
                ref.update(p, t, indexes=idx)
            _cmp(ours.compute(), ref.compute(), 1e-6)


@pytest.mark.parametrize("opt", ["sum", "none", "full_image", "contrast"])
def test_ssim_option_differential(opt):
    import warnings

    tm = _tm()
    kw = {"data_range": 1.0}
    if opt in ("sum", "none"):
        kw["reduction"] = opt
    elif opt == "full_image":
        kw["return_full_image"] = True
    else:
        kw["return_contrast_sensitivity"] = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = ma.StructuralSimilarityIndexMeasure(**kw)
        ref = tm.StructuralSimilarityIndexMeasure(**kw)
        for b in range(2):
            p, t = _img(88 + b)
            ours.update(p, t)
            ref.update(p, t)
        vo, vr = ours.compute(), ref.compute()
        if isinstance(vr, tuple):
            for a, b_ in zip(vo, vr):
                _cmp(a, b_, 1e-5)
        else:
            _cmp(vo, vr, 1e-5)


_SIG_NAMESPACES = ["", "classification", "regression", "retrieval", "text", "audio", "image",
                   "detection", "segmentation", "clustering", "nominal", "aggregation",
                   "wrappers", "shape", "pairwise", "functional",
                   "functional.classification", "functional.regression", "functional.retrieval",
                   "functional.text", "functional.audio", "functional.image",
                   "functional.detection", "functional.segmentation", "functional.clustering",
                   "functional.nominal", "functional.pairwise", "functional.shape",
                   "functional.multimodal"]


def _reference_signatures():
    """{namespace: {callable: [[param, "required" | "value" | "opaque", default], ...]}}
    of the reference's public callables (runs only while the tape is recorded)."""
    import importlib
    import inspect

    from tests.unittests._golden import _to_data

    out = {}
    for ns in _SIG_NAMESPACES:
        try:
            ref_ns = importlib.import_module(f"torchmetrics.{ns}" if ns else "torchmetrics")
        except Exception:
            continue
        sigs = {}
        for n in getattr(ref_ns, "__all__", []):
            rc = getattr(ref_ns, n, None)
            if rc is None or not (inspect.isclass(rc) or callable(rc)):
                continue
            try:
                rsig = inspect.signature(rc.__init__ if inspect.isclass(rc) else rc)
            except (ValueError, TypeError):
                continue
            params = []
            for pname, rp in rsig.parameters.items():
                if rp.default is inspect.Parameter.empty:
                    params.append([pname, "required", None])
                    continue
                ok, data = _to_data(rp.default)
                params.append([pname, "value", data] if ok else [pname, "opaque", repr(rp.default)])
            sigs[n] = params
        out[ns] = sigs
    return out


def test_constructor_signature_parity():
    """Every shared public callable accepts at least the reference's named
    parameters (introspection parity: help()/IDE/keyword-call compatible)."""
    import importlib
    import inspect
    import warnings

    ref_sigs = ref_value("public signatures", _reference_signatures)
    # every recorded default is plain data, so each one is compared by value
    assert not [(ns, n, p) for ns, sigs in ref_sigs.items() for n, ps in sigs.items() for p in ps if p[1] == "opaque"]
    mismatches = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ns in _SIG_NAMESPACES:
            if ns not in ref_sigs:
                continue
            try:
                our_ns = importlib.import_module(f"metrics_amd.{ns}") if ns else ma
            except Exception:
                continue
            for n, rparams in ref_sigs[ns].items():
                oc = getattr(our_ns, n, None)
                if oc is None:
                    continue
                try:
                    osig = inspect.signature(oc.__init__ if inspect.isclass(oc) else oc)
                except (ValueError, TypeError):
                    continue
                miss = [p for p, _, _ in rparams
                        if p not in ("self", "kwargs", "args") and p not in osig.parameters]
                if miss:
                    mismatches.append((ns or "top", n, miss))
                for pname, kind, rd in rparams:
                    if pname in ("self", "kwargs", "args") or pname not in osig.parameters:
                        continue
                    od = osig.parameters[pname].default
                    if kind == "required" or od is inspect.Parameter.empty:
                        if (kind == "required") != (od is inspect.Parameter.empty):
                            mismatches.append((ns or "top", n, pname, "required-ness", repr(rd), repr(od)))
                        continue
                    eq = rd == od
                    if isinstance(eq, bool) and not eq and not (rd != rd and od != od):
                        mismatches.append((ns or "top", n, pname, "default", repr(rd), repr(od)))
    assert not mismatches, mismatches


@pytest.mark.parametrize("zero_division", [0.0, 1.0])
def test_zero_division_differential(zero_division):
    """zero_division flows to the same values as the reference (degenerate
    all-one-class inputs make divisions by zero actually happen)."""
    import warnings

    tm = _tm()
    p = torch.zeros(40)  # all predicted negative -> tp + fp = 0
    t = torch.ones(40, dtype=torch.long)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("BinaryF1Score", "BinaryFBetaScore", "BinaryJaccardIndex"):
            kw = {"zero_division": zero_division}
            if "FBeta" in name:
                kw["beta"] = 0.5
            ours = getattr(ma, name)(**kw)
            ref = getattr(tm.classification, name)(**kw)
            ours.update(p, t)
            ref.update(p, t)
            _cmp(ours.compute(), ref.compute(), 1e-6)
