"""The fused binary step without a GPU.

1. The step record: the ``ctypes`` mirror in ``ops/_hip.py`` against ``BinStep``
   in ``csrc/bin_step.h`` (names, order, size), and the builder that fills it by
   name. A field out of place on the Python side would hand a kernel the wrong
   state tensor without failing. Needs only the built library.
2. Which collections get a fused binary update plan.
3. The rule the kernels implement (``_bin_rule``), with its two normalisation
   decisions, against the stand-alone CPU updates, on inputs clear of the
   rounding band around the cut-off.
"""
import ctypes

import pytest
import torch

import metrics_amd as ma
from metrics_amd.collections import _FusedBinaryUpdatePlan
from metrics_amd.ops import _hip
from tests.unittests._bin_rule import bin_rule_curve, bin_rule_decisions, bin_rule_sum

needs_lib = pytest.mark.skipif(not _hip.hip_available(), reason="kernel library not built")


# ------------------------------------------------------------------ the record
@needs_lib
def test_sizes_are_equal():
    assert _hip._lib().ma_bin_step_sizeof() == ctypes.sizeof(_hip.BinStep)


@needs_lib
def test_field_names_equal_the_header():
    names = _hip.bin_step_native_fields(_hip._lib())
    assert [name for name, _ in _hip.BinStep._fields_] == names
    assert len(set(names)) == len(names)
    # every field is 8 bytes wide: no padding, offsets follow from the order
    assert ctypes.sizeof(_hip.BinStep) == 8 * len(names)
    for i, (name, _) in enumerate(_hip.BinStep._fields_):
        assert getattr(_hip.BinStep, name).offset == 8 * i, name


@needs_lib
def test_a_swapped_mirror_is_caught():
    """A mirror with two pointers swapped has the right size and field count;
    the name check is what rejects it."""
    fields = dict(_hip.BinStep._fields_)
    order = [name for name, _ in _hip.BinStep._fields_]
    i, j = order.index("fp"), order.index("fn")
    order[i], order[j] = order[j], order[i]

    class Swapped(ctypes.Structure):
        _fields_ = [(name, fields[name]) for name in order]

    assert ctypes.sizeof(Swapped) == _hip._lib().ma_bin_step_sizeof()
    assert [name for name, _ in Swapped._fields_] != _hip.bin_step_native_fields(_hip._lib())


class _Fake:
    def __init__(self, ptr, shape=()):
        self._ptr, self.shape = ptr, shape

    def data_ptr(self):
        return self._ptr


def test_builder_fills_fields_by_name():
    """``bin_step`` on stand-ins that only have ``data_ptr`` and ``shape``:
    every named tensor lands in the field of its name, absent groups stay 0."""
    names = [n for n in _hip.BinStepTensors._fields if n != "thresholds"]
    t = _hip.BinStepTensors(
        thresholds=_Fake(5000, (200,)), **{n: _Fake(1000 + 8 * i) for i, n in enumerate(names)},
    )
    rec = _hip.bin_step(-1, 0.25, t, (1, 0.0, 199.0))
    assert (rec.ignore_index, rec.has_ignore, rec.thr) == (-1, 1, 0.25)
    for i, n in enumerate(names):
        assert getattr(rec, n) == 1000 + 8 * i, n
    assert (rec.thresholds, rec.T) == (5000, 200)
    assert (rec.uniform, rec.t0, rec.inv_step) == (1, 0.0, 199.0)

    rec = _hip.bin_step(None, 0.5, _hip.BinStepTensors(counts=_Fake(64), records=_Fake(72)))
    assert (rec.ignore_index, rec.has_ignore, rec.thr, rec.counts, rec.records) == (0, 0, 0.5, 64, 72)
    for n in [n for n, _ in _hip.BinStep._fields_ if n not in ("thr", "counts", "records")]:
        assert getattr(rec, n) == 0, n


@needs_lib
def test_layout_gate_is_the_lds_budget():
    """BIN_STEP_MAX_T is the last T the native layout accepts."""
    for dt in (0, 1):
        assert _hip.bin_step_layout(5, dt, _hip.BIN_STEP_MAX_T) is not None
        assert _hip.bin_step_layout(5, dt, _hip.BIN_STEP_MAX_T + 1) is None
    # beyond it the stand-alone curve kernels still serve
    assert _hip.BIN_STEP_MAX_T < _hip.CURVE_MAX_T


@needs_lib
def test_layout_units_and_grid():
    records, unit, epv, grid, tgrid, lds, ncopy = _hip.bin_step_layout(1, 1, 200)
    assert (epv, grid, tgrid) == (8, 1, 2) and unit % epv == 0 and records >= 1024
    assert _hip.bin_step_layout(1, 0, 0)[2:6] == (4, 1, 1, 0)
    # the dynamic LDS: `ncopy` pairs of (T+1, 2) u32 histograms and T floats
    assert lds == ncopy * 2 * 201 * 2 * 4 + 200 * 4
    # one block per unit until the cap (a remainder below one vector is scalar
    # work of block 0); nothing but the tail kernel for an empty batch
    sizes = (0, unit - 1, unit, unit + 1, unit + epv, 3 * unit)
    assert [_hip.bin_step_layout(n, 1, 5)[3] for n in sizes] == [0, 1, 1, 1, 2, 3]
    # the block grows with the batch, 256, 512, 1024 threads of 16 elements,
    # as long as 128 blocks still get a unit each
    for n, want in ((128 * 8192 - 1, 4096), (128 * 8192, 8192), (128 * 16384 - 1, 8192), (128 * 16384, 16384)):
        assert _hip.bin_step_layout(n, 1, 5)[1] == want, n
    big_unit, _, cap = _hip.bin_step_layout(1 << 30, 0, 5)[1:4]
    assert 1 <= cap <= records and big_unit == 16384
    assert _hip.bin_step_layout(cap * big_unit + 4, 0, 5)[3] == cap  # one vector more than a whole grid pass
    assert _hip.bin_step_layout(1 << 31, 0, 5) is None and _hip.bin_step_layout(4, 2, 5) is None


# -------------------------------------------------------------- plan selection
KW = dict(validate_args=False)


def _batch(gen, n=9):
    return torch.randn(n, generator=gen), torch.randint(0, 2, (n,), generator=gen)


def _plan(metrics, update=True):
    coll = ma.MetricCollection(metrics)
    if update:
        coll.update(*_batch(torch.Generator().manual_seed(3)))
    return coll, _FusedBinaryUpdatePlan.build(coll)


def _full(kw_stat=KW, kw_confmat=KW, kw_curve=KW):
    return {
        "f1": ma.BinaryF1Score(**kw_stat),
        "acc": ma.BinaryAccuracy(**kw_stat),
        "confmat": ma.BinaryConfusionMatrix(**kw_confmat),
        "auroc": ma.BinaryAUROC(thresholds=5, **kw_curve),
        "ap": ma.BinaryAveragePrecision(thresholds=5, **kw_curve),
    }


def test_plan_takes_one_leader_of_each_kind():
    coll, plan = _plan(_full())
    assert plan is not None
    groups = list(coll.compute_groups.values())
    assert sorted(map(sorted, groups)) == [["acc", "f1"], ["ap", "auroc"], ["confmat"]]
    m = coll._modules
    assert plan.stat in (m["acc"], m["f1"]) and plan.confmat is m["confmat"]
    assert plan.curve in (m["ap"], m["auroc"])
    assert (plan.ignore_index, plan.threshold, plan.steps, plan.curve_steps) == (None, 0.5, 0, 0)


def test_plan_without_a_stat_leader():
    coll, plan = _plan({"confmat": ma.BinaryConfusionMatrix(**KW), "auroc": ma.BinaryAUROC(thresholds=5, **KW)})
    assert plan is not None and plan.stat is None and plan.curve is coll._modules["auroc"]
    assert plan.threshold == 0.5


@pytest.mark.parametrize("name", ["BinaryMatthewsCorrCoef", "BinaryJaccardIndex", "BinaryCohenKappa"])
def test_confmat_kinds_share_state_and_update(name):
    """The classes marked "bin_confmat" hold the (2, 2) state of
    BinaryConfusionMatrix and update it in the same way."""
    gen = torch.Generator().manual_seed(5)
    m, ref = getattr(ma, name)(ignore_index=-1, **KW), ma.BinaryConfusionMatrix(ignore_index=-1, **KW)
    assert type(m)._hip_fused_kind == "bin_confmat" and list(m._defaults) == ["confmat"]
    for _ in range(2):
        p, t = _batch(gen, 33)
        t[::5] = -1
        m.update(p, t)
        ref.update(p, t)
    assert torch.equal(m.confmat, ref.confmat)
    coll, plan = _plan({"m": getattr(ma, name)(**KW), "f1": ma.BinaryF1Score(**KW)})
    assert plan is not None and plan.confmat is coll._modules["m"]


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
        update = False  # samplewise wants (N, extra) inputs; groups are one per metric then
    elif why == "env":
        monkeypatch.setenv("METRICS_AMD_FUSE_BINARY", "0")
    if why == "single":
        metrics = {"f1": ma.BinaryF1Score(**KW), "acc": ma.BinaryAccuracy(**KW)}
    elif why == "samplewise":
        metrics = {"f1": ma.BinaryF1Score(**other), "auroc": ma.BinaryAUROC(thresholds=5, **KW)}
    else:
        metrics = {"f1": ma.BinaryF1Score(**KW), "confmat": ma.BinaryConfusionMatrix(**other)}
    _, plan = _plan(metrics, update)
    assert plan is None


def test_curve_without_thresholds_stays_out():
    metrics = {
        "f1": ma.BinaryF1Score(**KW), "confmat": ma.BinaryConfusionMatrix(**KW),
        "prc": ma.BinaryPrecisionRecallCurve(thresholds=None, **KW),
    }
    _, plan = _plan(metrics)
    assert plan is not None and plan.curve is None


def test_cpu_inputs_are_declined():
    coll, _ = _plan(_full())
    gen = torch.Generator().manual_seed(4)
    coll.update(*_batch(gen))
    assert coll._fused_bin_plan is not None and coll._fused_bin_plan.steps == 0


# -------------------------------------------------------------------- the rule
def _rule_batches(kind, ig, gen):
    batches = []
    for shape in ((9,), (1,), (3, 11)):
        n = torch.Size(shape)
        k = torch.randint(-12, 12, n, generator=gen) if kind == "logits" else torch.randint(0, 16, n, generator=gen)
        p = (k + 0.5) * 0.5 if kind == "logits" else k / 16.0 + 1.0 / 32.0
        t = torch.randint(0, 2, n, generator=gen)
        if ig is not None:
            t[torch.rand(n, generator=gen) < 0.2] = ig
        batches.append((p, t))
    return batches


def _standalone(batches, thr, ig):
    kw = dict(KW, ignore_index=ig)
    stat, confmat = ma.BinaryStatScores(threshold=thr, **kw), ma.BinaryConfusionMatrix(threshold=thr, **kw)
    curve = ma.BinaryPrecisionRecallCurve(thresholds=5, **kw)
    for p, t in batches:
        for m in (stat, confmat, curve):
            m.update(p, t)
    return stat, confmat, curve


def _assert_rule(batches, thr, ig):
    stat, confmat, curve = _standalone(batches, thr, ig)
    want_stat, want_confmat = bin_rule_sum(batches, thr, ig)
    for name, w in zip(("tp", "fp", "tn", "fn"), want_stat):
        assert torch.equal(getattr(stat, name).reshape(1), w), name
    assert torch.equal(confmat.confmat, want_confmat)
    assert torch.equal(curve.confmat, bin_rule_curve(batches, curve.thresholds, ig))


@pytest.mark.parametrize("ig", [None, -1])
@pytest.mark.parametrize("thr", [0.5, 0.25])
@pytest.mark.parametrize("kind", ["logits", "probs"])
def test_rule_matches_the_standalone_updates(kind, thr, ig):
    _assert_rule(_rule_batches(kind, ig, torch.Generator().manual_seed(11)), thr, ig)


@pytest.mark.parametrize("thr", [0.5, 0.25])
def test_rule_has_two_decisions(thr):
    """The only value outside [0, 1] sits at an ignored position: the stat
    group takes the sigmoid cut, confusion matrix and curve take the raw one.
    0.53125 lies between the two cuts (0.5 and logit(0.5) = 0 are both below
    it, so 0.28125 and thr = 0.25 make the difference there)."""
    ig = -1
    p = torch.tensor([0.03125, 0.28125, 0.53125, 0.78125, 0.46875, 7.5, 0.09375, 0.96875])
    t = torch.tensor([0, 1, 1, 0, 0, ig, 1, 1])
    assert bin_rule_decisions(p, t, ig) == (True, False)
    assert bin_rule_decisions(p, t, None) == (True, True)
    (tp, fp, tn, fn), confmat = bin_rule_sum([(p, t)], thr, ig)
    # sigmoid cut: every kept value is positive; raw cut: x > thr
    assert (int(tp), int(fp), int(tn), int(fn)) == (4, 3, 0, 0)
    raw_pos = [x > thr for x in p.tolist()]
    want_tp = sum(1 for x, y in zip(raw_pos, t.tolist()) if x and y == 1)
    assert int(confmat[1, 1]) == want_tp and want_tp < 4
    _assert_rule([(p, t)], thr, ig)
    # the converse: the outside value is kept, every group normalises
    t2 = t.clone()
    t2[5] = 1
    assert bin_rule_decisions(p, t2, ig) == (True, True)
    _assert_rule([(p, t2)], thr, ig)
