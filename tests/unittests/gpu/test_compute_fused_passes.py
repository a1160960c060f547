"""The passes that ``MetricCollection.compute()`` shares (csrc/mc_compute.hip,
csrc/compute_common.h), each against the kernels it replaces. Everything here
is integer counting or the same fp32 expression, so every comparison is
``torch.equal``.

A. The flush completes a histogram in pending-b0 format in its staged tile
   (``curve_suffix_tile`` with ``pending``). Oracle: ``ma_curve_resolve_pending``
   followed by the flush without ``pending``, the sequence before.
B. One pass over the (C, C) confusion matrix gives the moments scratch and a
   copy. Oracle: ``ma_confmat_moments`` and ``clone()``.
C. Both in one grid, behind the collection: the whole ``compute()`` against
   ``METRICS_AMD_COMPUTE_PLAN=0``.

Shapes of A: C = 3, 4, 5, 9 leave a partial last tile at 2, 4 and 8 classes
per block, C = 136 gives 34 blocks; T = 1 (a class row of four words), 2 and
200 (a row longer than one pass of a wave); thresholds whose bucket of 0.0 is
1 (a grid starting at 0), 0 (all above 0) and T (all at or below 0).
"""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------- A
def _thresholds(T, b0):
    if b0 == 1:  # a grid that starts at 0
        return torch.linspace(0, 1, T) if T > 1 else torch.tensor([0.0])
    if b0 == 0:  # every threshold above 0
        return torch.linspace(0.05, 0.95, T) if T > 1 else torch.tensor([0.5])
    return torch.linspace(-1.0, 0.0, T) if T > 1 else torch.tensor([0.0 - 0.25])  # b0 == T


def _b0_of(thr):
    return int(torch.searchsorted(thr, torch.tensor([0.0]), right=True))


def _by_hand(C, T, b0, seed, owe=True):
    """A histogram short of some elements of bucket b0 and the P and R for
    which the two identities restore them (owe=False: nothing is owed,
    P = R = 0 would then break the identities, so P and R are the row sums)."""
    gen = torch.Generator().manual_seed(seed)
    full = torch.randint(0, 50, (C, T + 1, 2), generator=gen)
    full[:, b0, :] += 1000
    per_class = full.sum(dim=(1, 2))
    R = int(per_class.max()) + 7
    full[:, b0, 0] += R - per_class
    P = full[:, :, 1].sum(dim=1)
    hist = full.clone()
    if owe:
        hist[:, b0, 0] -= torch.randint(0, 900, (C,), generator=gen)
        hist[:, b0, 1] -= torch.minimum(torch.randint(0, 900, (C,), generator=gen), full[:, b0, 1])
    return hist, torch.cat([P, torch.full((C,), R, dtype=torch.long)])


def _flush_both_ways(hist, pr, thr, C, T, seed):
    """(state, hist, P|R, tail) after the parent's sequence and after the flush
    with pending, from equal starting points."""
    gen = torch.Generator().manual_seed(seed)
    state0 = torch.randint(0, 1 << 40, (T, C, 2, 2), generator=gen)
    tail = torch.arange(1, 38)  # stands for the records behind P and R
    out = []
    for fused in (False, True):
        h = hist.clone().cuda()
        pend = torch.cat([pr, tail]).cuda()
        state = state0.clone().cuda()
        thr_d = thr.float().contiguous().cuda()
        if fused:
            _hip.curve_suffix_flush(h, state, thr_d, pend)
        else:
            _hip.curve_resolve_pending(h, thr_d, pend)
            _hip.curve_suffix_flush(h, state)
        torch.cuda.synchronize()
        out.append((state.cpu(), h.cpu(), pend[: 2 * C].cpu(), pend[2 * C:].cpu()))
    return out, tail


def _assert_flush_equal(out, tail, C):
    (s_old, h_old, p_old, t_old), (s_new, h_new, p_new, t_new) = out
    assert torch.equal(s_new, s_old)
    assert torch.equal(h_new, h_old) and int(h_new.abs().sum()) == 0  # the flush zeroes it
    assert torch.equal(p_new, p_old) and torch.equal(p_new, torch.zeros(2 * C, dtype=torch.long))
    assert torch.equal(t_new, tail) and torch.equal(t_old, tail)


_A_SHAPES = [(C, T) for C in (3, 4, 5, 9, 136) for T in (1, 2, 200)]


@pytest.mark.parametrize("b0_kind", [1, 0, "T"], ids=["b0=1", "b0=0", "b0=T"])
@pytest.mark.parametrize("C,T", _A_SHAPES, ids=[f"C{c}-T{t}" for c, t in _A_SHAPES])
def test_flush_pays_pending_like_the_resolve_kernel(C, T, b0_kind):
    b0 = T if b0_kind == "T" else b0_kind
    thr = _thresholds(T, b0)
    assert _b0_of(thr) == b0
    hist, pr = _by_hand(C, T, b0, seed=31 * C + T)
    out, tail = _flush_both_ways(hist, pr, thr, C, T, seed=C + 7 * T)
    _assert_flush_equal(out, tail, C)


@pytest.mark.parametrize("ctile", ["2", "4", "8"])
def test_tile_remainders_at_every_ctile(ctile):
    """MA_SUFFIX_CTILE is read once per process: each tile width in a process
    of its own, over the C of the shape list with a partial last tile."""
    code = textwrap.dedent("""
        import torch
        from tests.unittests.gpu import test_compute_fused_passes as t
        for C in (3, 4, 5, 9):
            for T in (1, 2, 200):
                thr = t._thresholds(T, 1)
                hist, pr = t._by_hand(C, T, 1, seed=C * T)
                out, tail = t._flush_both_ways(hist, pr, thr, C, T, seed=C + T)
                t._assert_flush_equal(out, tail, C)
        print("ok")
    """)
    env = dict(os.environ, MA_SUFFIX_CTILE=ctile)
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stderr[-2000:]


def test_nothing_owed_with_the_pointer_given():
    """P = R = 0 on a histogram that is empty: both deficits are zero."""
    C, T = 9, 2
    thr = _thresholds(T, 1)
    hist = torch.zeros(C, T + 1, 2, dtype=torch.long)
    out, tail = _flush_both_ways(hist, torch.zeros(2 * C, dtype=torch.long), thr, C, T, seed=3)
    _assert_flush_equal(out, tail, C)
    # and a complete histogram with its own row sums as P and R
    hist, pr = _by_hand(C, T, 1, seed=4, owe=False)
    out, tail = _flush_both_ways(hist, pr, thr, C, T, seed=5)
    _assert_flush_equal(out, tail, C)


def _collection(C, thresholds, names):
    kw = dict(num_classes=C, validate_args=False)
    make = {
        "acc_macro": lambda: ma.MulticlassAccuracy(average="macro", **kw),
        "f1": lambda: ma.MulticlassF1Score(average="macro", **kw),
        "exact_match": lambda: ma.MulticlassExactMatch(**kw),
        "jaccard": lambda: ma.MulticlassJaccardIndex(average="macro", **kw),
        "cohen_kappa": lambda: ma.MulticlassCohenKappa(**kw),
        "mcc": lambda: ma.MulticlassMatthewsCorrCoef(**kw),
        "confmat": lambda: ma.MulticlassConfusionMatrix(**kw),
        "auroc": lambda: ma.MulticlassAUROC(average="macro", thresholds=thresholds, **kw),
        "avg_precision": lambda: ma.MulticlassAveragePrecision(average="macro", thresholds=thresholds, **kw),
    }
    return ma.MetricCollection({n: make[n]() for n in names}).to("cuda")


_CURVE = ("auroc", "avg_precision")
_CM = ("jaccard", "cohen_kappa", "mcc", "confmat")
_STAT = ("acc_macro", "f1", "exact_match")
_ALL = _STAT + _CM + _CURVE


def _logit_batches(C, B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, C, generator=g).to(torch.bfloat16).cuda(), torch.randint(0, C, (B,), generator=g).cuda())
            for _ in range(n)]


@pytest.mark.parametrize("T", [1, 2])
def test_pending_histogram_of_real_one_pass_steps(monkeypatch, T):
    """C = 136 passes the one-pass gate at T = 1 and 2 (C >= 5 T, C % 8 == 0):
    the histogram, P and R of a few real steps."""
    C = 136
    monkeypatch.setenv(_hip.ONEPASS_ENV, "2")
    coll = _collection(C, _thresholds(T, 1).cuda(), _ALL)
    for b in _logit_batches(C, 64, 4, seed=T):
        coll.update(*b)
    own = coll.auroc.__dict__
    assert own.get("_hip_b0_pending"), "no one-pass step ran"
    hist = own["_hip_hist_buf"].cpu().clone()
    pr = own["_hip_onepass_scratch"][: 2 * C].cpu().clone()
    assert int(pr[C:].sum()) > 0
    out, tail = _flush_both_ways(hist, pr, _thresholds(T, 1), C, T, seed=11)
    _assert_flush_equal(out, tail, C)


# ------------------------------------------------------------------------- B
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 130])
def test_one_pass_moments_and_copy(C):
    gen = torch.Generator().manual_seed(C)
    cm = torch.randint(0, 1000, (C, C), generator=gen)
    big = torch.rand(C, C, generator=gen) < 0.2
    cm[big] += torch.randint(1 << 32, 1 << 45, (C, C), generator=gen)[big]
    cm.view(-1)[0] = (1 << 33) + 5  # at least one entry above 2^32 at every C
    cm = cm.cuda()
    want = torch.zeros(3 * C, dtype=torch.long, device="cuda")
    _hip.confmat_moments(cm, want)
    got = torch.zeros(3 * C, dtype=torch.long, device="cuda")
    copy = torch.full((C, C), -1, dtype=torch.long, device="cuda")
    _hip.confmat_moments_copy(cm, got, copy)
    only = torch.zeros(3 * C, dtype=torch.long, device="cuda")
    _hip.confmat_moments_copy(cm, only, None)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(only, want)
    assert torch.equal(want[:C], cm.sum(1)) and torch.equal(want[C:2 * C], cm.sum(0))
    assert torch.equal(copy, cm.clone())


def test_returned_confusion_matrix_owns_its_storage(monkeypatch):
    monkeypatch.setenv(_hip.COMPUTE_PLAN_ENV, "1")
    C = 65
    coll = _collection(C, 8, _ALL)
    b = _logit_batches(C, 64, 3, seed=2)
    coll.update(*b[0])
    coll.update(*b[1])
    first = coll.compute()
    assert coll._compute_plan.steps == 1
    ptrs = {k: v.untyped_storage().data_ptr() for k, v in first.items()}
    assert ptrs["confmat"] != coll.confmat.confmat.untyped_storage().data_ptr()
    assert all(ptrs["confmat"] != p for k, p in ptrs.items() if k != "confmat")
    assert torch.equal(first["confmat"], coll.confmat.confmat)
    kept = first["confmat"].clone()
    coll.update(*b[2])
    second = coll.compute()
    torch.cuda.synchronize()
    assert second["confmat"].untyped_storage().data_ptr() != ptrs["confmat"]
    assert torch.equal(first["confmat"], kept) and not torch.equal(second["confmat"], kept)


# ------------------------------------------------------------------------- C
def _same(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _play(monkeypatch, plan_on, onepass, names, script, batches):
    monkeypatch.setenv(_hip.COMPUTE_PLAN_ENV, "1" if plan_on else "0")
    monkeypatch.setenv(_hip.ONEPASS_ENV, onepass)
    coll = _collection(136, 8, names)
    results, was_pending = [], []
    for step in script:
        if step == "uncache":  # drop the cached results: the next compute has nothing to flush
            for m in coll.values(copy_state=False):
                m._computed = None
        elif step == "compute":
            curve = getattr(coll, "auroc", None)
            was_pending.append(bool(curve is not None and curve.__dict__.get("_hip_b0_pending")))
            results.append(coll.compute())
        else:
            coll.update(*batches[step])
    states = {}
    for name, m in coll.items(keep_base=True, copy_state=False):
        m._maybe_flush_lazy()
        for key in m._defaults:
            states[f"{name}.{key}"] = getattr(m, key).clone()
    torch.cuda.synchronize()
    return coll, results, states, was_pending


_SCRIPT = [0, 1, 2, "compute", "compute", "uncache", "compute", 3, "compute", 4, "compute"]


@pytest.mark.parametrize("onepass", ["2", "0"], ids=["pending", "not-pending"])
@pytest.mark.parametrize("names", [_STAT[:1] + _CURVE, _CM, _CM + _CURVE, _ALL],
                         ids=["curve-only", "confmat-only", "both", "both-stat-exact"])
def test_collection_compute_equals_the_per_metric_path(monkeypatch, names, onepass):
    """Updates, compute, compute again (cached), compute with the cache dropped
    (flush == 0: the state is only read), update, compute, update, compute;
    C = 136, T = 8, B = 64."""
    batches = _logit_batches(136, 64, 5, seed=17)
    new, got, got_states, pend = _play(monkeypatch, True, onepass, names, _SCRIPT, batches)
    old, exp, exp_states, _ = _play(monkeypatch, False, onepass, names, _SCRIPT, batches)
    assert new._compute_plan.steps == 4 and not getattr(old._compute_plan, "steps", 0)
    if names == _ALL:
        assert pend[0] == (onepass == "2"), "the flush did not meet the histogram format it is here for"
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g.keys() == e.keys()
        for k in e:
            assert _same(g[k], e[k]), (f"compute {i}", k)
    for k in got[0]:
        assert got[1][k] is got[0][k]  # the cached path
        assert _same(got[2][k], got[0][k]), k  # nothing to flush: equal values
    assert got_states.keys() == exp_states.keys()
    for k in exp_states:
        assert torch.equal(got_states[k], exp_states[k]), ("state", k)
    if {"auroc", "confmat"} <= set(names):
        native = new._compute_plan.native
        assert native.launches(True, True) == 2 and native.launches(False, False) == 2
