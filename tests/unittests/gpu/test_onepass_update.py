"""One-pass fused collection update (csrc/mc_onepass.hip) against the
two-kernel sequence it replaces (METRICS_AMD_ONEPASS=0).

Every state involved is an integer count, rowmax/rowinv come from the same
fold order and the bucket from the same functions, and the b0 bucket is filled
by an exact integer identity — so the two paths must agree BIT FOR BIT
(``torch.equal``), not within a tolerance.

Shapes are the smallest at which the wave-per-row register mapping can break:
C=136 (one partial vector per lane, most lanes idle), 520 (65 bf16 vectors: one
lane holds two), 1000 (ragged second vector), 1024 (exact fit), 1001 (not
covered: must fall back and still match); B=1 (single row), 3 (fewer rows than
the four waves of a block), 5 (a second block with one row), 257 (block tail).
"""
import warnings

import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

_T_INNER = [0.05, 0.2, 0.35, 0.6, 0.95]  # first threshold > 0, last < 1
_THRESHOLDS = {
    "T200": 200,
    "T5": 5,
    "list3": [0.1, 0.5, 0.9],  # b0 is bucket 0
    "inner": _T_INNER,
}
# (targets, thresholds) pairs: every target mode and every threshold spec twice
_PAIRS = [
    ("plain", "T200"), ("plain", "list3"), ("ignore", "T5"),
    ("ignore", "T200"), ("bad", "inner"), ("bad", "T5"),
    ("plain", "inner"), ("ignore", "list3"),
]
_IGNORE = 3


def _make(C, thresholds, ignore_index):
    kw = dict(num_classes=C, validate_args=False, ignore_index=ignore_index)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=thresholds, **kw),
        "ap": ma.MulticlassAveragePrecision(average="macro", thresholds=thresholds, **kw),
    })


def _preds(regime, B, C, dtype, gen):
    logits = torch.randn(B, C, generator=gen, device="cuda") * 3.0
    if regime == "logits":
        return logits.to(dtype)
    probs = torch.softmax(logits, dim=1).to(dtype)  # every element stays in [0,1]
    if regime == "probs":
        return probs
    if regime == "probs15":  # one element out of range: every OTHER row is deferred, flag set
        probs[B // 2, 3] = 1.5
        return probs
    assert regime == "mixed"  # exactly one all-in-range row among logits
    out = logits.to(dtype)
    out[B // 2] = probs[B // 2]
    return out


def _target(mode, B, C, gen, allow_bad=True):
    t = torch.randint(0, C, (B,), generator=gen, device="cuda")
    if mode == "ignore":
        t[torch.rand(B, generator=gen, device="cuda") < 1 / 3] = _IGNORE
        if B > 1:
            t[0] = _IGNORE
    elif mode == "bad" and allow_bad:
        t[0] = -1
        if B > 1:
            t[B - 1] = C
    return t


def _batches(C, B, dtype, tmode, regimes, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [(_preds(r, B, C, dtype, gen), _target(tmode, B, C, gen, allow_bad=i > 0))
            for i, r in enumerate(regimes)]


def _states(coll):
    acc, cm, ex, au = coll.acc, coll.confmat, coll.exact, coll.auroc
    # the lazily accumulated histogram lives on the curve GROUP LEADER (AP and
    # AUROC share one group; members alias the leader's confmat)
    for m in coll.values(copy_state=False):
        m._maybe_flush_lazy()
    torch.cuda.synchronize()
    return {
        "tp": acc.tp.clone(), "fp": acc.fp.clone(), "tn": acc.tn.clone(), "fn": acc.fn.clone(),
        "confmat": cm.confmat.clone(), "correct": ex.correct.clone(), "total": ex.total.clone(),
        "curve": au.confmat.clone(),
    }


def _compute(coll):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return {k: v.clone() for k, v in coll.compute().items()}


# first update runs every metric on its own (compute groups form after it);
# the fused plan serves every later one: three alternating regimes, compute,
# then the two mixed-decision regimes, compute
_SEQ_A = ["logits", "logits", "probs", "logits"]
_SEQ_B = ["probs15", "mixed"]


def _run(monkeypatch, onepass, C, thresholds, tmode, batches_a, batches_b):
    with monkeypatch.context() as m:
        m.setenv(_hip.ONEPASS_ENV, "2" if onepass else "0")  # 2: no shape gate
        coll = _make(C, thresholds, _IGNORE if tmode == "ignore" else None).to("cuda")
        for p, t in batches_a:
            coll.update(p, t)
        out = [_states(coll), _compute(coll)]
        for p, t in batches_b:
            coll.update(p, t)
        out += [_states(coll), _compute(coll)]
        rows = coll._fused_plan.curve.__dict__["_hip_rowstats_buf"][:, : batches_b[-1][0].shape[0]].clone()
        return out, coll._fused_plan.onepass_steps, rows


def _assert_same(new, old):
    for got, want in zip(new, old):
        assert got.keys() == want.keys()
        for k in want:
            assert torch.equal(got[k], want[k]), k


def _check_pair(monkeypatch, C, B, dtype, tmode, thr_name, expect_onepass=True):
    thresholds = _THRESHOLDS[thr_name]
    batches_a = _batches(C, B, dtype, tmode, _SEQ_A, seed=1000 + C + B)
    batches_b = _batches(C, B, dtype, tmode, _SEQ_B, seed=2000 + C + B)
    new, steps_new, rows_new = _run(monkeypatch, True, C, thresholds, tmode, batches_a, batches_b)
    old, steps_old, rows_old = _run(monkeypatch, False, C, thresholds, tmode, batches_a, batches_b)
    fused_updates = len(_SEQ_A) - 1 + len(_SEQ_B)
    assert steps_old == 0
    assert steps_new == (fused_updates if expect_onepass else 0)
    _assert_same(new, old)
    # same fold => bit-identical row statistics (a done row carries -rinv)
    assert torch.equal(rows_new[0], rows_old[0])
    assert torch.equal(rows_new[1].abs(), rows_old[1])


@pytest.mark.parametrize("pair", _PAIRS, ids=[f"{a}-{b}" for a, b in _PAIRS])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [136, 520, 1000, 1024])
def test_onepass_matches_two_kernel(monkeypatch, C, dtype, pair):
    tmode, thr_name = pair
    for B in (1, 3, 5, 257):
        _check_pair(monkeypatch, C, B, dtype, tmode, thr_name)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_unsupported_c_falls_back(monkeypatch, dtype):
    # C=1001 is no multiple of the vector width: the two-kernel path must serve it
    _check_pair(monkeypatch, 1001, 1, dtype, "plain", "T200", expect_onepass=False)


def _cpu_collection(C, thresholds, ignore_index, batches):
    coll = _make(C, thresholds, ignore_index)
    for p, t in batches:
        coll.update(p.float().cpu(), t.cpu())  # same values, upcast: the kernels compute in fp32
    return coll


@pytest.mark.parametrize("tmode", ["plain", "ignore"])
@pytest.mark.parametrize("thr_name", ["T200", "list3"])
@pytest.mark.parametrize("C", [136, 520, 1000, 1024])
def test_fp32_probabilities_exact_vs_cpu(monkeypatch, C, thr_name, tmode):
    """Probability inputs: no softmax anywhere, every row deferred — all
    states must equal the CPU collection exactly."""
    thresholds = _THRESHOLDS[thr_name]
    ignore_index = _IGNORE if tmode == "ignore" else None
    batches = _batches(C, 129, torch.float32, tmode, ["probs", "probs", "probs"], seed=31 + C)
    with monkeypatch.context() as m:
        m.setenv(_hip.ONEPASS_ENV, "2")
        gpu = _make(C, thresholds, ignore_index).to("cuda")
        for p, t in batches:
            gpu.update(p, t)
        got = _states(gpu)
        assert gpu._fused_plan.onepass_steps == 2
    cpu = _cpu_collection(C, thresholds, ignore_index, batches)
    want = {
        "tp": cpu.acc.tp, "fp": cpu.acc.fp, "tn": cpu.acc.tn, "fn": cpu.acc.fn,
        "confmat": cpu.confmat.confmat, "correct": cpu.exact.correct, "total": cpu.exact.total,
        "curve": cpu.auroc.confmat,
    }
    for k, v in want.items():
        assert torch.equal(got[k].cpu(), v), k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [136, 520, 1000, 1024])
def test_logits_auroc_ap_vs_cpu(monkeypatch, C, dtype):
    """Logits: AUROC/AP against the CPU collection at the tolerance
    test_device_parity_sweep.py uses (atol 1e-4, rtol 1e-3)."""
    batches = _batches(C, 129, dtype, "plain", ["logits", "logits", "logits"], seed=57 + C)
    with monkeypatch.context() as m:
        m.setenv(_hip.ONEPASS_ENV, "2")
        gpu = _make(C, 200, None).to("cuda")
        for p, t in batches:
            gpu.update(p, t)
        got = _compute(gpu)
        assert gpu._fused_plan.onepass_steps == 2
    cpu = _cpu_collection(C, 200, None, batches)
    want = _compute(cpu)
    for k in ("auroc", "ap"):
        assert torch.allclose(got[k].float().cpu(), want[k].float(), atol=1e-4, rtol=1e-3,
                              equal_nan=True), (k, got[k], want[k])


def test_onepass_under_graphed_update(monkeypatch):
    """Capture the one-pass step into a hipGraph, replay three times
    (logits, probabilities, logits): same equalities."""
    C, B, dtype = 1000, 257, torch.bfloat16
    warm = _batches(C, B, dtype, "plain", ["logits"], seed=7)[0]
    batches = _batches(C, B, dtype, "ignore", ["logits", "probs", "logits"], seed=8)

    def run(onepass):
        with monkeypatch.context() as m:
            m.setenv(_hip.ONEPASS_ENV, "2" if onepass else "0")  # 2: no shape gate
            coll = _make(C, 200, _IGNORE).to("cuda")
            coll.update(*warm)  # form the compute groups
            # parallel=False: the capture goes through MetricCollection.update,
            # i.e. through the fused plan
            graphed = ma.graphs.GraphedUpdate(coll, *warm, parallel=False)
            steps_at_capture = coll._fused_plan.onepass_steps
            for p, t in batches:
                graphed.update(p, t)
            return [_states(coll), _compute(coll)], steps_at_capture

    new, steps_new = run(True)
    old, steps_old = run(False)
    assert steps_new > 0 and steps_old == 0
    _assert_same(new, old)


def test_default_gate_follows_guard_table(monkeypatch):
    """Default mode: the one-pass step serves C >= 5*T only (C=1000 at T=200
    yes, C=520 no); both still match the two-kernel path (checked above)."""
    monkeypatch.delenv(_hip.ONEPASS_ENV, raising=False)
    for C, expect in ((1000, 2), (520, 0)):
        coll = _make(C, 200, None).to("cuda")
        for p, t in _batches(C, 5, torch.bfloat16, "plain", ["logits"] * 3, seed=3):
            coll.update(p, t)
        torch.cuda.synchronize()
        assert coll._fused_plan.onepass_steps == expect
