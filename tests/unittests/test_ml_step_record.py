"""The fused multilabel step without a GPU.

1. The step record: the ``ctypes`` mirror in ``ops/_hip.py`` against ``MlStep``
   in ``csrc/ml_step.h`` (names, order, size), and the builder that fills it by
   name. A field out of place on the Python side would hand a kernel the wrong
   state tensor without failing. Needs only the built library.
2. Which collections get a fused multilabel update plan.
3. The rule the kernels implement (``_ml_rule``) against the stand-alone CPU
   updates, on inputs clear of the rounding band around the cut-off.
"""
import ctypes

import pytest
import torch

import metrics_amd as ma
from metrics_amd.collections import _FusedMultilabelUpdatePlan
from metrics_amd.ops import _hip
from tests.unittests._ml_rule import ml_rule_sum

needs_lib = pytest.mark.skipif(not _hip.hip_available(), reason="kernel library not built")


# ------------------------------------------------------------------ the record
@needs_lib
def test_sizes_are_equal():
    assert _hip._lib().ma_ml_step_sizeof() == ctypes.sizeof(_hip.MlStep)


@needs_lib
def test_field_names_equal_the_header():
    names = _hip.ml_step_native_fields(_hip._lib())
    assert [name for name, _ in _hip.MlStep._fields_] == names
    assert len(set(names)) == len(names)
    # every field is 8 bytes wide: no padding, offsets follow from the order
    assert ctypes.sizeof(_hip.MlStep) == 8 * len(names)
    for i, (name, _) in enumerate(_hip.MlStep._fields_):
        assert getattr(_hip.MlStep, name).offset == 8 * i, name


@needs_lib
def test_a_swapped_mirror_is_caught():
    """A mirror with two pointers swapped has the right size and field count;
    the name check is what rejects it."""
    fields = dict(_hip.MlStep._fields_)
    order = [name for name, _ in _hip.MlStep._fields_]
    i, j = order.index("fp"), order.index("fn")
    order[i], order[j] = order[j], order[i]

    class Swapped(ctypes.Structure):
        _fields_ = [(name, fields[name]) for name in order]

    assert ctypes.sizeof(Swapped) == _hip._lib().ma_ml_step_sizeof()
    assert [name for name, _ in Swapped._fields_] != _hip.ml_step_native_fields(_hip._lib())


class _Fake:
    def __init__(self, ptr, shape=()):
        self._ptr, self.shape = ptr, shape

    def data_ptr(self):
        return self._ptr


def test_builder_fills_fields_by_name():
    """``ml_step`` on stand-ins that only have ``data_ptr`` and ``shape``: every
    named tensor lands in the field of its name, absent groups stay 0."""
    names = [n for n in _hip.MlStepTensors._fields if n not in ("thresholds", "region_flags")]
    t = _hip.MlStepTensors(
        thresholds=_Fake(5000, (200,)), region_flags=_Fake(6000, (77,)),
        **{n: _Fake(1000 + 8 * i) for i, n in enumerate(names)},
    )
    rec = _hip.ml_step(130, -1, 0.25, t, (1, 0.0, 199.0))
    assert (rec.L, rec.ignore_index, rec.has_ignore, rec.thr) == (130, -1, 1, 0.25)
    for i, n in enumerate(names):
        assert getattr(rec, n) == 1000 + 8 * i, n
    assert (rec.thresholds, rec.T, rec.region_flags, rec.region_cap) == (5000, 200, 6000, 77)
    assert (rec.uniform, rec.t0, rec.inv_step) == (1, 0.0, 199.0)

    rec = _hip.ml_step(7, None, 0.5, _hip.MlStepTensors(counts=_Fake(64), records=_Fake(72)))
    assert (rec.L, rec.ignore_index, rec.has_ignore, rec.thr, rec.counts, rec.records) == (7, 0, 0, 0.5, 64, 72)
    for n in [n for n, _ in _hip.MlStep._fields_ if n not in ("L", "thr", "counts", "records")]:
        assert getattr(rec, n) == 0, n


@needs_lib
def test_layout_gate_is_the_lds_budget():
    """ML_STEP_MAX_T is the last T the native layout accepts (narrowest chunk)."""
    assert _hip.ml_step_layout(8, 5, _hip.ML_STEP_MAX_T) is not None
    assert _hip.ml_step_layout(8, 5, _hip.ML_STEP_MAX_T + 1) is None
    # chunk width: the widest that pads L by at most an eighth
    assert [_hip.ml_step_layout(L, 64, 0)[2] for L in (1, 14, 64, 65, 80, 96, 130, 1000)] == [
        16, 16, 64, 16, 16, 32, 16, 64]


# -------------------------------------------------------------- plan selection
L = 6
KW = dict(num_labels=L, validate_args=False)


def _batch(gen, n=5):
    return torch.randn(n, L, generator=gen), torch.randint(0, 2, (n, L), generator=gen)


def _plan(metrics, update=True):
    coll = ma.MetricCollection(metrics)
    if update:
        coll.update(*_batch(torch.Generator().manual_seed(3)))
    return coll, _FusedMultilabelUpdatePlan.build(coll)


def _full(kw_stat=KW, kw_confmat=KW, kw_exact=KW, kw_curve=KW):
    return {
        "f1": ma.MultilabelF1Score(average="macro", **kw_stat),
        "acc": ma.MultilabelAccuracy(average="micro", **kw_stat),
        "confmat": ma.MultilabelConfusionMatrix(**kw_confmat),
        "exact": ma.MultilabelExactMatch(**kw_exact),
        "auroc": ma.MultilabelAUROC(thresholds=5, **kw_curve),
        "ap": ma.MultilabelAveragePrecision(thresholds=5, **kw_curve),
    }


def test_plan_takes_one_leader_of_each_kind():
    coll, plan = _plan(_full())
    assert plan is not None
    groups = list(coll.compute_groups.values())
    assert sorted(map(sorted, groups)) == [["acc", "f1"], ["ap", "auroc"], ["confmat"], ["exact"]]
    m = coll._modules
    assert plan.stat in (m["acc"], m["f1"]) and plan.confmat is m["confmat"] and plan.exact is m["exact"]
    assert plan.curve in (m["ap"], m["auroc"])
    assert (plan.num_labels, plan.ignore_index, plan.threshold, plan.steps) == (L, None, 0.5, 0)


def test_plan_without_a_stat_leader():
    coll, plan = _plan({"confmat": ma.MultilabelConfusionMatrix(**KW), "mcc_exact": ma.MultilabelExactMatch(**KW)})
    assert plan is not None and plan.stat is None and plan.curve is None


def test_mcc_and_jaccard_share_the_confmat_kind():
    coll, plan = _plan({
        "mcc": ma.MultilabelMatthewsCorrCoef(**KW), "jac": ma.MultilabelJaccardIndex(**KW),
        "f1": ma.MultilabelF1Score(**KW),
    })
    assert plan is not None and plan.confmat in (coll._modules["mcc"], coll._modules["jac"])


@pytest.mark.parametrize(
    "why", ["threshold", "ignore_index", "validate_args", "samplewise", "single", "env"]
)
def test_no_plan(monkeypatch, why):
    update = True
    other = dict(KW)
    if why == "threshold":
        other["threshold"] = 0.25
    elif why == "ignore_index":
        other["ignore_index"] = -1
    elif why == "validate_args":
        other["validate_args"] = True
    elif why == "samplewise":
        other["multidim_average"] = "samplewise"
        update = False  # samplewise wants (N, L, extra) inputs; groups are one per metric then
    elif why == "env":
        monkeypatch.setenv("METRICS_AMD_FUSE_MULTILABEL", "0")
    if why == "single":
        metrics = {"f1": ma.MultilabelF1Score(**KW), "acc": ma.MultilabelAccuracy(average="micro", **KW)}
    elif why == "samplewise":
        metrics = {"f1": ma.MultilabelF1Score(**KW), "exact": ma.MultilabelExactMatch(**other)}
    else:
        metrics = {"f1": ma.MultilabelF1Score(**KW), "confmat": ma.MultilabelConfusionMatrix(**other)}
    _, plan = _plan(metrics, update)
    assert plan is None


def test_curve_without_thresholds_stays_out():
    kw_curve = dict(KW, thresholds=None)
    metrics = {
        "f1": ma.MultilabelF1Score(**KW), "confmat": ma.MultilabelConfusionMatrix(**KW),
        "prc": ma.MultilabelPrecisionRecallCurve(**kw_curve),
    }
    _, plan = _plan(metrics)
    assert plan is not None and plan.curve is None


def test_cpu_inputs_are_declined():
    coll, _ = _plan(_full())
    gen = torch.Generator().manual_seed(4)
    coll.update(*_batch(gen))
    assert coll._fused_ml_plan is not None and coll._fused_ml_plan.steps == 0


# -------------------------------------------------------------------- the rule
@pytest.mark.parametrize("ig", [None, -1])
@pytest.mark.parametrize("thr", [0.5, 0.25])
@pytest.mark.parametrize("kind", ["logits", "probs"])
def test_rule_matches_the_standalone_updates(kind, thr, ig):
    gen = torch.Generator().manual_seed(11)
    batches = []
    for n in (9, 1, 33):
        k = torch.randint(-12, 12, (n, L), generator=gen) if kind == "logits" else torch.randint(0, 16, (n, L), generator=gen)
        p = (k + 0.5) * 0.5 if kind == "logits" else k / 16.0 + 1.0 / 32.0
        t = torch.randint(0, 2, (n, L), generator=gen)
        if ig is not None:
            t[torch.rand(n, L, generator=gen) < 0.2] = ig
        batches.append((p, t))
    kw = dict(KW, threshold=thr, ignore_index=ig)
    stat, confmat, exact = ma.MultilabelStatScores(average=None, **kw), ma.MultilabelConfusionMatrix(**kw), ma.MultilabelExactMatch(**kw)
    for p, t in batches:
        for m in (stat, confmat, exact):
            m.update(p, t)
    want_stat, want_confmat, want_correct, want_total = ml_rule_sum(batches, thr, ig)
    for name, w in zip(("tp", "fp", "tn", "fn"), want_stat):
        assert torch.equal(getattr(stat, name), w), name
    assert torch.equal(confmat.confmat, want_confmat)
    assert torch.equal(exact.correct.reshape(1), want_correct) and torch.equal(exact.total.reshape(1), want_total)
