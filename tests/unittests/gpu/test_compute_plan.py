"""The collection compute plan (``csrc/mc_compute.hip``,
``collections._FusedMulticlassComputePlan``) against the path it replaces.

Two instances of the bench collection get the same seeded updates; one computes
with the plan, the other with ``METRICS_AMD_COMPUTE_PLAN=0``, where every member
computes through its own kernels as before. The old path is the oracle: every
output and every state must be equal bit for bit (``torch.equal``; NaNs, which
kappa can return, are compared by their bits), above all the curve
``(T, C, 2, 2)`` state after the flush.

Shapes are the smallest at which each part can go wrong:

    C    T    B
    5    3   32   last class tile partial (C % CTILE = 1)
    9    1   32   AUROC has zero terms, AP the appended endpoint only
    8    2   32   smallest T with an AUROC term
  257    7   64   second stride of the 256-thread loops, two column tiles in
                  the moments kernel
  136  300   32   T > 256: two terms per reduction slot

Label predictions cannot be fed to a threshold-curve metric at all (its format
step needs (B, C) scores), so they run on a collection without the curve
metrics; the curve leader updating outside the fused step is covered with fp16
logits, which every leader takes through its own update.
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3, 32), (9, 1, 32), (8, 2, 32), (257, 7, 64), (136, 300, 32)]
SHAPE_IDS = [f"C{c}-T{t}-B{b}" for c, t, b in SHAPES]
CURVE = ("auroc", "avg_precision")
CONFMAT = ("jaccard", "cohen_kappa", "mcc", "confmat")


def _collection(C, T, ignore_index=None, drop=(), nocache=()):
    """bench.py's build_collection, member for member."""
    kw = dict(num_classes=C, validate_args=False, ignore_index=ignore_index)
    metrics = {
        "acc_micro": lambda **k: ma.MulticlassAccuracy(average="micro", **k),
        "acc_macro": lambda **k: ma.MulticlassAccuracy(average="macro", **k),
        "precision": lambda **k: ma.MulticlassPrecision(average="macro", **k),
        "recall": lambda **k: ma.MulticlassRecall(average="macro", **k),
        "f1": lambda **k: ma.MulticlassF1Score(average="macro", **k),
        "fbeta2": lambda **k: ma.MulticlassFBetaScore(beta=2.0, average="macro", **k),
        "specificity": lambda **k: ma.MulticlassSpecificity(average="macro", **k),
        "npv": lambda **k: ma.MulticlassNegativePredictiveValue(average="macro", **k),
        "hamming": lambda **k: ma.MulticlassHammingDistance(average="macro", **k),
        "jaccard": lambda **k: ma.MulticlassJaccardIndex(average="macro", **k),
        "exact_match": lambda **k: ma.MulticlassExactMatch(**k),
        "cohen_kappa": lambda **k: ma.MulticlassCohenKappa(**k),
        "mcc": lambda **k: ma.MulticlassMatthewsCorrCoef(**k),
        "confmat": lambda **k: ma.MulticlassConfusionMatrix(**k),
        "auroc": lambda **k: ma.MulticlassAUROC(average="macro", thresholds=T, **k),
        "avg_precision": lambda **k: ma.MulticlassAveragePrecision(average="macro", thresholds=T, **k),
    }
    built = {
        name: make(**kw, **({"compute_with_cache": False} if name in nocache else {}))
        for name, make in metrics.items() if name not in drop
    }
    return ma.MetricCollection(built).to("cuda")


def _batches(C, B, n, dtype=torch.bfloat16, seed=0, absent=False, ignore_index=None, labels=False):
    """n seeded (preds, target) batches. absent: the upper half of the classes
    occurs neither as target nor as prediction."""
    g = torch.Generator().manual_seed(1000 * C + seed)
    hi = max(1, C // 2) if absent else C
    out = []
    for _ in range(n):
        logits = torch.randn(B, C, generator=g)
        if absent:
            logits[:, hi:] -= 50.0
        target = torch.randint(0, hi, (B,), generator=g)
        if ignore_index is not None:
            target[torch.rand(B, generator=g) < 0.25] = ignore_index
        preds = logits.argmax(1) if labels else logits.to(dtype)
        out.append((preds.cuda(), target.cuda()))
    return out


def _states(coll):
    out = {}
    for name, m in coll.items(keep_base=True, copy_state=False):
        m._maybe_flush_lazy()
        for key in m._defaults:
            out[f"{name}.{key}"] = getattr(m, key).clone()
    return out


def _same(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _play(monkeypatch, plan_on, coll, script):
    """Run ("update", batch) / ("compute",) / ("reset",) / ("uncache",) steps;
    returns the result of every compute and the final states."""
    monkeypatch.setenv(_hip.COMPUTE_PLAN_ENV, "1" if plan_on else "0")
    results = []
    for step in script:
        if step[0] == "update":
            coll.update(*step[1])
        elif step[0] == "compute":
            results.append(coll.compute())
        elif step[0] == "reset":
            coll.reset()
        elif step[0] == "uncache":  # drop cached results without touching a state
            for m in coll.values(copy_state=False):
                m._computed = None
    states = _states(coll)
    torch.cuda.synchronize()
    return results, states


def _compare(monkeypatch, make, script, want_steps=None):
    new = make()
    got, got_states = _play(monkeypatch, True, new, script)
    old = make()
    exp, exp_states = _play(monkeypatch, False, old, script)
    assert not getattr(old._compute_plan, "steps", 0), "the oracle ran the plan"
    if want_steps is not None:
        assert new._compute_plan.steps == want_steps
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g.keys() == e.keys()
        for k in e:
            assert _same(g[k], e[k]), (f"compute {i}", k, g[k], e[k])
    assert got_states.keys() == exp_states.keys()
    for k in exp_states:
        assert torch.equal(got_states[k], exp_states[k]), ("state", k)
    return new, got


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_matches_the_per_metric_path(monkeypatch, shape, dtype):
    """Several updates then compute; compute, update, compute."""
    C, T, B = shape
    b = _batches(C, B, 4, dtype)
    script = [("update", b[0]), ("update", b[1]), ("update", b[2]), ("compute",),
              ("update", b[3]), ("compute",)]
    new, got = _compare(monkeypatch, lambda: _collection(C, T), script, want_steps=2)
    covered = {id(m) for m, *_ in new._compute_plan.members}
    assert len(covered) == 15  # all but the raw confusion matrix
    # the second compute saw the update: cached results were invalidated
    assert not _same(got[0]["confmat"], got[1]["confmat"])


@pytest.mark.parametrize("ignore_index", [None, 0, 3], ids=["noignore", "ignore0", "ignore3"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[4]], ids=[SHAPE_IDS[0], SHAPE_IDS[3], SHAPE_IDS[4]])
def test_absent_classes_and_ignore_index(monkeypatch, shape, ignore_index):
    """Classes that never occur as target or prediction take every
    zero-denominator branch; an ignore_index that names a class also sends
    jaccard down its own path while the rest of its group stays covered."""
    C, T, B = shape
    b = _batches(C, B, 3, absent=True, ignore_index=ignore_index)
    script = [("update", x) for x in b] + [("compute",)]
    _compare(monkeypatch, lambda: _collection(C, T, ignore_index=ignore_index), script, want_steps=1)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[SHAPE_IDS[1], SHAPE_IDS[3]])
def test_compute_twice_without_update(monkeypatch, shape):
    """The second compute returns the cached results on both paths. With the
    cache dropped and still no update, the plan takes the nothing-to-flush
    path: equal values, every state unchanged (checked against the oracle,
    whose states no compute touches)."""
    C, T, B = shape
    b = _batches(C, B, 2)
    script = [("update", b[0]), ("update", b[1]), ("compute",), ("compute",), ("uncache",), ("compute",)]
    new, got = _compare(monkeypatch, lambda: _collection(C, T), script, want_steps=2)
    for k in got[0]:
        assert got[1][k] is got[0][k]
        assert _same(got[2][k], got[0][k]), k
        if k != "confmat":
            assert got[2][k].data_ptr() != got[0][k].data_ptr()
    assert not new.auroc.__dict__.get("_lazy_dirty")


def test_curve_leader_updated_outside_the_fused_step(monkeypatch):
    """fp16 logits: every leader updates on its own and the curve state is
    accumulated eagerly, so the step has nothing to flush on a fresh result."""
    C, T, B = 257, 7, 64
    b = _batches(C, B, 3, torch.float16)
    script = [("update", x) for x in b] + [("compute",)]
    new, _ = _compare(monkeypatch, lambda: _collection(C, T), script, want_steps=1)
    assert not new.auroc.__dict__.get("_lazy_dirty")


@pytest.mark.parametrize("drop", [CURVE, CONFMAT], ids=["no-curve", "no-confmat"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[3]])
def test_collection_without_a_leader(monkeypatch, shape, drop):
    C, T, B = shape
    b = _batches(C, B, 3)
    script = [("update", x) for x in b] + [("compute",)]
    _compare(monkeypatch, lambda: _collection(C, T, drop=drop), script, want_steps=1)


def test_label_predictions(monkeypatch):
    C, T, B = 257, 7, 64
    b = _batches(C, B, 3, labels=True)
    script = [("update", x) for x in b] + [("compute",)]
    _compare(monkeypatch, lambda: _collection(C, T, drop=CURVE), script, want_steps=1)


def test_reset_rebuilds_the_plan(monkeypatch):
    C, T, B = 136, 300, 32
    b = _batches(C, B, 5)
    script = [("update", b[0]), ("update", b[1]), ("compute",), ("update", b[2]), ("compute",),
              ("reset",), ("update", b[3]), ("update", b[4]), ("compute",), ("uncache",), ("compute",)]
    seen = []
    real = _hip._ComputePlan

    class Counting(real):
        __slots__ = ()

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self)

    monkeypatch.setattr(_hip, "_ComputePlan", Counting)
    _compare(monkeypatch, lambda: _collection(C, T), script, want_steps=4)
    # four steps, two native plans: the second compute reuses the first plan,
    # reset() replaces the state tensors and with them the plan
    assert len(seen) == 2


def test_member_without_cache_falls_back(monkeypatch):
    C, T, B = 257, 7, 64
    b = _batches(C, B, 3)
    script = [("update", x) for x in b] + [("compute",), ("compute",)]
    new, got = _compare(
        monkeypatch, lambda: _collection(C, T, nocache=("f1", "mcc", "auroc")), script, want_steps=1
    )
    for name in ("f1", "mcc", "auroc"):
        assert getattr(new, name)._computed is None
        assert got[1][name] is not got[0][name]


def test_compute_before_update_still_warns(monkeypatch):
    monkeypatch.setenv(_hip.COMPUTE_PLAN_ENV, "1")
    coll = _collection(8, 2)
    with pytest.warns(UserWarning, match="was called before the ``update`` method") as rec:
        coll.compute()
    names = {type(m).__name__ for m in coll.values(copy_state=False)}
    warned = {n for n in names if any(f"metric {n} " in str(w.message) for w in rec)}
    assert warned == names


def test_successive_computes_do_not_share_storage(monkeypatch):
    monkeypatch.setenv(_hip.COMPUTE_PLAN_ENV, "1")
    C, T, B = 257, 7, 64
    b = _batches(C, B, 3)
    coll = _collection(C, T)
    coll.update(*b[0])
    coll.update(*b[1])
    first = coll.compute()
    kept = {k: v.clone() for k, v in first.items()}
    coll.update(*b[2])
    second = coll.compute()
    torch.cuda.synchronize()
    assert coll._compute_plan.steps == 2
    for k in first:
        assert first[k].untyped_storage().data_ptr() != second[k].untyped_storage().data_ptr(), k
        assert _same(first[k], kept[k]), k  # the second compute wrote nowhere into the first
