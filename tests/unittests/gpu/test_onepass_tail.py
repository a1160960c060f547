"""Two-launch one-pass step (k_mc_onepass + k_onepass_tail, csrc/mc_onepass.hip)
against the kernel sequence it replaces (METRICS_AMD_ONEPASS=0).

Every quantity the per-block records, the tail's record sum, the class-sliced
epilogue and the deferred tiles carry is an integer count, so the whole
``compute()`` output and the raw states must be ``torch.equal``.

Shapes: bf16 C=136 (smallest covered C, NV=1 with a ragged last vector), bf16
C=1000, fp32 C=132; T=5 non-uniform and T=200 linspace; B=1 and 5 (fewer rows
than one block's waves / a second block), 257 (a partial 256-row tile behind a
full one), 1031 (several row tiles), 4100 (more rows than 4 x 1024 waves: waves
loop over two rows). Input kinds, one update each on the same collection:
logits (nothing deferred), probabilities (everything deferred, no softmax),
probabilities with one logit row (that row binned in launch 1, all others
deferred and softmaxed in the tail), out-of-range targets (binned != sum P),
every row ignored (valid = binned = deferred = 0), some rows ignored.
"""
import warnings

import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

_IGNORE = 3
_SHAPES = [(torch.bfloat16, 136), (torch.bfloat16, 1000), (torch.float32, 132)]
_SHAPE_IDS = ["bf16-C136", "bf16-C1000", "fp32-C132"]
_THRESHOLDS = {"T5": [0.05, 0.2, 0.35, 0.6, 0.95], "T200": 200}
_BATCHES = (1, 5, 257, 1031, 4100)
# (preds kind, target kind); the first list runs without ignore_index, the second with
_KINDS_PLAIN = [("logits", "plain"), ("probs", "plain"), ("onelogit", "plain"), ("logits", "bad")]
_KINDS_IGNORE = [("onelogit", "allignore"), ("onelogit", "someignore"), ("probs", "someignore")]


def _make(C, thresholds, ignore_index):
    kw = dict(num_classes=C, validate_args=False, ignore_index=ignore_index)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),  # stat scores
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=thresholds, **kw),
    })


def _preds(kind, B, C, dtype, gen):
    logits = torch.randn(B, C, generator=gen, device="cuda") * 3.0
    if kind == "logits":
        return logits.to(dtype)
    probs = torch.softmax(logits, dim=1).to(dtype)  # every element stays in [0,1]
    if kind == "onelogit":
        probs[B // 2] = logits[B // 2].to(dtype)
    return probs


def _target(kind, B, C, gen):
    t = torch.randint(0, C, (B,), generator=gen, device="cuda")
    if kind == "allignore":
        t[:] = _IGNORE
    elif kind == "someignore":
        t[torch.rand(B, generator=gen, device="cuda") < 1 / 3] = _IGNORE
        t[0] = _IGNORE
    elif kind == "bad":
        t[0] = -1
        t[B - 1] = C
    return t


def _batches(kinds, B, C, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [(_preds(p, B, C, dtype, gen), _target(t, B, C, gen)) for p, t in kinds]


def _states(coll):
    for m in coll.values(copy_state=False):
        m._maybe_flush_lazy()
    acc, cm, ex, au = coll.acc, coll.confmat, coll.exact, coll.auroc
    return {
        "tp": acc.tp.clone(), "fp": acc.fp.clone(), "tn": acc.tn.clone(), "fn": acc.fn.clone(),
        "confmat": cm.confmat.clone(), "correct": ex.correct.clone(), "total": ex.total.clone(),
        "curve": au.confmat.clone(),
    }


def _compute(coll):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return {k: v.clone() for k, v in coll.compute().items()}


def _run(monkeypatch, mode, C, thresholds, ignore_index, batches, script):
    """``script(coll, batches, snap)`` drives the collection; ``snap()`` records
    the raw states; what it returns is handed back as ``extra``. Returns the
    snapshots + the final compute(), the number of one-pass steps and extra."""
    with monkeypatch.context() as m:
        m.setenv(_hip.ONEPASS_ENV, mode)
        coll = _make(C, thresholds, ignore_index).to("cuda")
        out = []
        extra = script(coll, batches, lambda: out.append(_states(coll)))
        out.append(_compute(coll))
        return out, coll._fused_plan.onepass_steps, extra


def _assert_same(new, old):
    assert len(new) == len(old)
    for n, (got, want) in enumerate(zip(new, old)):
        assert got.keys() == want.keys()
        for k in want:
            assert torch.equal(got[k], want[k]), (n, k)


def _each_update(coll, batches, snap):
    # the first update runs every metric on its own (compute groups form after
    # it); the fused plan serves every later one
    for p, t in batches:
        coll.update(p, t)
        snap()


def _check(monkeypatch, C, thresholds, ignore_index, batches, script, fused_updates):
    new, steps_new, extra_new = _run(monkeypatch, "2", C, thresholds, ignore_index, batches, script)
    old, steps_old, extra_old = _run(monkeypatch, "0", C, thresholds, ignore_index, batches, script)
    assert steps_old == 0 and steps_new == fused_updates
    _assert_same(new, old)
    return extra_new, extra_old


@pytest.mark.parametrize("thr_name", list(_THRESHOLDS))
@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_tail_matches_two_kernel(monkeypatch, shape, thr_name):
    dtype, C = shape
    thresholds = _THRESHOLDS[thr_name]
    for B in _BATCHES:
        for kinds, ignore_index in ((_KINDS_PLAIN, None), (_KINDS_IGNORE, _IGNORE)):
            batches = _batches([("logits", "plain")] + kinds, B, C, dtype, seed=C + B)
            _check(monkeypatch, C, thresholds, ignore_index, batches, _each_update, len(kinds))


@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_smaller_grid_after_larger(monkeypatch, shape):
    """B=1031 (258 blocks, every record non-trivial: one logit row sets
    `outside`, all other rows are deferred) and then B=5 all-in-range
    probabilities (2 blocks): a stale record of the larger grid would turn the
    softmax decision or the counts."""
    dtype, C = shape
    warm = _batches([("logits", "plain")], 5, C, dtype, seed=11)
    big = _batches([("onelogit", "plain")], 1031, C, dtype, seed=12)
    small = _batches([("probs", "plain"), ("logits", "plain")], 5, C, dtype, seed=13)
    _check(monkeypatch, C, 200, None, warm + big + small, _each_update, 3)


@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_compute_reset_update(monkeypatch, shape):
    """Two updates, compute(), reset(), one more update: both scratches are
    zero again and the epoch closed after every step."""
    dtype, C = shape
    batches = _batches([("logits", "plain"), ("onelogit", "bad"), ("probs", "plain"),
                        ("onelogit", "plain")], 257, C, dtype, seed=21)

    def script(coll, batches, snap):
        coll.update(*batches[0])  # forms the compute groups
        coll.update(*batches[1])
        coll.update(*batches[2])
        snap()
        mid = _compute(coll)
        coll.reset()
        coll.update(*batches[3])
        snap()
        return mid

    mid_new, mid_old = _check(monkeypatch, C, _THRESHOLDS["T5"], None, batches, script, 3)
    _assert_same([mid_new], [mid_old])


def test_two_updates_graphed(monkeypatch):
    """The two-update sequence captured once and replayed through GraphedUpdate."""
    dtype, C, B = torch.bfloat16, 1000, 257
    batches = _batches([("logits", "plain"), ("onelogit", "someignore"), ("probs", "someignore")],
                       B, C, dtype, seed=31)

    def script(coll, batches, snap):
        coll.update(*batches[0])  # forms the compute groups
        # parallel=False: the capture goes through MetricCollection.update,
        # i.e. through the fused plan
        graphed = ma.graphs.GraphedUpdate(coll, *batches[0], parallel=False)
        steps_at_capture = coll._fused_plan.onepass_steps
        for p, t in batches[1:]:
            graphed.update(p, t)
        snap()
        return steps_at_capture

    new, _, captured_new = _run(monkeypatch, "2", C, 200, _IGNORE, batches, script)
    old, _, captured_old = _run(monkeypatch, "0", C, 200, _IGNORE, batches, script)
    assert captured_new > 0 and captured_old == 0
    _assert_same(new, old)
