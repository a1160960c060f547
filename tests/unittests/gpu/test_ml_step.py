"""The fused multilabel step (``csrc/ml_step.hip``) on the GPU.

A collection of F1, Accuracy, HammingDistance, ConfusionMatrix, ExactMatch,
AUROC and AveragePrecision runs its updates from the second one on through the
fused plan (``coll._fused_ml_plan``, ``plan.steps``).

Oracle A: the same run with ``METRICS_AMD_FUSE_MULTILABEL=0``, where every
leader updates on its own: every state and every ``compute()`` value must be
equal bit for bit. Oracle B: the rule in CPU torch (``_ml_rule``) for the
stat, confusion-matrix and exact-match states. The curve is checked against
oracle A only; its own oracle tests are ``test_curve_edges.py``.

Inputs stay clear of the rounding band around the cut-off (inside a plan the
confusion-matrix and exact-match leaders threshold exactly, docs/PARITY.md)
and are exact in bf16: logits ``(randint(-12, 12) + 0.5) * 0.5``,
probabilities ``k/16 + 1/32``, plus planted edge values.
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip
from tests.unittests._curve_oracle import NONUNIFORM
from tests.unittests._ml_rule import ml_rule_sum

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
INF, NAN = float("inf"), float("nan")

# (N, L). The layout (ml_step.hip): chunk width CW in {16, 32, 64} labels, a
# region = 8 loads of one wave = 8 * 64/CW rows, 16 waves per block.
SHAPES = [
    (1, 1), (3, 7), (5, 8), (4, 64), (4, 65), (257, 33), (300, 130), (70, 1000),
    # chunk width: L = 64 -> CW 64 (above), 65 -> CW 16 (above), 96 -> CW 32,
    # 72 -> CW 16 again (96 would pad by more than an eighth)
    (4, 96), (4, 72),
    # one chunk exactly full and one label more, at CW = 16: L = 16 and 17
    (5, 16), (5, 17),
    # region rows at CW = 16: 32 rows fill one region, 33 open a second
    (32, 7), (33, 7),
    # region rows at CW = 64 (8 rows) and CW = 32 (16 rows)
    (8, 64), (9, 64), (16, 96), (17, 96),
    # more regions than the 16 waves of one block: a second block per chunk
    (16 * 32 + 1, 7),
]
CONFIGS = [(ig, thr, spec) for ig in (None, -1) for thr in (0.5, 0.25) for spec in (1, 5, 200, "list")]


def _id(v):
    return {BF16: "bf16", FP32: "fp32"}.get(v, str(v))


def _thresholds(spec):
    return list(NONUNIFORM) if spec == "list" else spec


def _make(L, ig, thr, spec):
    kw = dict(num_labels=L, validate_args=False, ignore_index=ig)
    cut = dict(kw, threshold=thr)
    return ma.MetricCollection({
        "f1": ma.MultilabelF1Score(average="macro", **cut),
        "acc": ma.MultilabelAccuracy(average="micro", **cut),
        "hamming": ma.MultilabelHammingDistance(**cut),
        "confmat": ma.MultilabelConfusionMatrix(**cut),
        "exact": ma.MultilabelExactMatch(**cut),
        "auroc": ma.MultilabelAUROC(thresholds=_thresholds(spec), **kw),
        "ap": ma.MultilabelAveragePrecision(thresholds=_thresholds(spec), **kw),
    }).to("cuda")


def _next_above_one(dtype):
    return 1.0 + (2.0 ** -7 if dtype == BF16 else 2.0 ** -23)


def _plant(p, values):
    """``values`` at evenly spread positions of ``p`` (as many as fit)."""
    flat = p.view(-1)
    n = min(len(values), flat.numel())
    for i in range(n):
        flat[(i * flat.numel()) // n] = values[i]
    return p


def _target(N, L, ig, gen):
    t = torch.randint(0, 2, (N, L), generator=gen)
    if ig is not None:
        t[torch.rand(N, L, generator=gen) < 0.1] = ig
    return t


def _logits(N, L, dtype, thr, ig, gen, plant=True):
    p = ((torch.randint(-12, 12, (N, L), generator=gen) + 0.5) * 0.5).to(dtype)
    if plant:
        # 0.0 and -0.0 sit exactly on the logit cut-off of thr = 0.5 (strict >)
        _plant(p, [0.0, -0.0, thr, 1.0, _next_above_one(dtype), INF, -INF, NAN])
    return p, _target(N, L, ig, gen)


def _probs(N, L, dtype, thr, ig, gen, plant=True):
    p = (torch.randint(0, 16, (N, L), generator=gen) / 16.0 + 1.0 / 32.0).to(dtype)
    if plant:
        _plant(p, [0.0, -0.0, thr, 1.0, NAN])  # all inside [0, 1]: NaN is not outside
    return p, _target(N, L, ig, gen)


def _states(coll):
    for m in coll.values(copy_state=False):
        m._maybe_flush_lazy()
    torch.cuda.synchronize()
    out = {}
    for name, m in coll.items(keep_base=True, copy_state=False):
        for s in m._defaults:
            out[f"{name}.{s}"] = getattr(m, s).clone()
    return out


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _run(monkeypatch, fuse, L, ig, thr, spec, batches):
    monkeypatch.setenv(_hip.FUSE_MULTILABEL_ENV, fuse)
    coll = _make(L, ig, thr, spec)
    for p, t in batches:
        coll.update(p.cuda(), t.cuda())
    values = {n: v.clone() for n, v in coll.compute().items()}
    return coll, _states(coll), values


def _assert_rule(states, batches, thr, ig, what=""):
    stat, confmat, correct, total = ml_rule_sum(batches, thr, ig)
    for s, w in zip(("tp", "fp", "tn", "fn"), stat):
        for name in ("f1", "acc", "hamming"):
            assert torch.equal(states[f"{name}.{s}"].cpu(), w), (what, name, s)
    assert torch.equal(states["confmat.confmat"].cpu(), confmat), what
    assert torch.equal(states["exact.correct"].cpu().reshape(1), correct), what
    assert torch.equal(states["exact.total"].cpu().reshape(1), total), what


def _check_both(monkeypatch, L, ig, thr, spec, batches, curve_rides=True):
    coll, got, values = _run(monkeypatch, "1", L, ig, thr, spec, batches)
    plan = coll._fused_ml_plan
    assert plan is not None and plan.steps == len(batches) - 1
    assert plan.curve_steps == (plan.steps if curve_rides else 0)
    old_coll, old, old_values = _run(monkeypatch, "0", L, ig, thr, spec, batches)
    assert old_coll._fused_ml_plan is None
    assert got.keys() == old.keys() and values.keys() == old_values.keys()
    for name, v in old.items():
        assert torch.equal(got[name], v), name
    for name, v in old_values.items():
        assert _same(values[name], v), name
    _assert_rule(got, batches, thr, ig)
    return coll


def _three(make, N, L, dtype, thr, ig, gen):
    """Three updates with N large, small, large: stale records, flags and
    mismatch words of a larger step would show in the next one."""
    return [make(n, L, dtype, thr, ig, gen) for n in (N, max(1, N // 3), N)]


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("N,L", SHAPES, ids=_id)
def test_shapes_match_unfused_run_and_rule(monkeypatch, N, L, dtype):
    # every (ignore_index, threshold, thresholds) combination is met across the shapes
    i = SHAPES.index((N, L)) * 2 + (dtype == BF16)
    gen = torch.Generator().manual_seed(1000 * L + N)
    for kind, cfg in ((_logits, CONFIGS[i % 16]), (_probs, CONFIGS[(i + 5) % 16])):
        ig, thr, spec = cfg
        _check_both(monkeypatch, L, ig, thr, spec, _three(kind, N, L, dtype, thr, ig, gen))


@pytest.mark.parametrize("ig,thr,spec", CONFIGS, ids=_id)
def test_every_configuration(monkeypatch, ig, thr, spec):
    gen = torch.Generator().manual_seed(17)
    _check_both(monkeypatch, 130, ig, thr, spec, _three(_logits, 300, 130, BF16, thr, ig, gen))
    _check_both(monkeypatch, 8, ig, thr, spec, _three(_probs, 5, 8, FP32, thr, ig, gen))


def test_waves_walk_several_regions(monkeypatch):
    """N = 33000 at L = 64, T = 200: 4125 regions of 8 rows against 256 blocks
    of 16 waves, so the first waves take a second region with their counters,
    certainty and histogram carried over."""
    gen = torch.Generator().manual_seed(5)
    assert _hip.ml_step_layout(64, 33000, 200)[2:5] == (64, 8, 256)
    batches = [_logits(40, 64, BF16, 0.5, -1, gen), _logits(33000, 64, BF16, 0.5, -1, gen),
               _probs(33000, 64, BF16, 0.5, -1, gen)]
    _check_both(monkeypatch, 64, -1, 0.5, 200, batches)


def test_curve_above_the_lds_gate_updates_on_its_own(monkeypatch):
    gen = torch.Generator().manual_seed(6)
    T = _hip.ML_STEP_MAX_T + 1
    batches = _three(_logits, 37, 8, BF16, 0.5, -1, gen)
    coll = _check_both(monkeypatch, 8, -1, 0.5, T, batches, curve_rides=False)
    assert coll._fused_ml_plan.curve is not None  # in the plan, declined per step


@pytest.mark.parametrize("N,L,dtype", [(257, 33, BF16), (70, 1000, FP32)], ids=_id)
@pytest.mark.parametrize("case", ["probs", "logits", "last_outside", "last_outside_ignored", "probs_then_logits"])
def test_sigmoid_decision(monkeypatch, case, N, L, dtype):
    gen = torch.Generator().manual_seed(23 + L)
    ig, thr = -1, 0.5
    first = _logits(N, L, dtype, thr, ig, gen)
    if case == "probs":  # everything deferred
        rest = [_probs(N, L, dtype, thr, ig, gen) for _ in range(2)]
    elif case == "logits":
        rest = [_logits(N, L, dtype, thr, ig, gen) for _ in range(2)]
    elif case.startswith("last_outside"):
        # the single outside element is the last one of the last row: all
        # regions but its own are deferred, and the whole batch is sigmoid,
        # also when that element sits at an ignored position
        p, t = _probs(N, L, dtype, thr, ig, gen)
        p[-1, -1] = 1.5
        t[-1, -1] = ig if case.endswith("ignored") else 1
        rest = [(p, t), _probs(N, L, dtype, thr, ig, gen)]
    else:
        rest = [_probs(N, L, dtype, thr, ig, gen), _logits(N, L, dtype, thr, ig, gen)]
    _check_both(monkeypatch, L, ig, thr, 5, [first] + rest)


@pytest.mark.parametrize("ig", [None, -1], ids=_id)
def test_exact_match_rows(monkeypatch, ig):
    """Rows that are right everywhere, but for: a row of ignored targets, a
    mismatch only in the first label, a mismatch only in the last label (with
    L = 1000 another chunk, so another block, than the first)."""
    N, L, thr = 12, 1000, 0.5
    gen = torch.Generator().manual_seed(3)
    batches = [_logits(N, L, BF16, thr, ig, gen)]
    for _ in range(2):
        t = torch.randint(0, 2, (N, L), generator=gen)
        p = (t * 2.0 - 1.0).to(BF16) * 1.75  # every prediction right
        p[1, 0], p[2, L - 1] = -p[1, 0], -p[2, L - 1]
        if ig is not None:
            t[0, :] = ig
            t[5, 500] = ig
        batches.append((p, t))
    coll = _check_both(monkeypatch, L, ig, thr, 5, batches)
    # an ignored element never matches (MultilabelExactMatch.update, the reference)
    wrong = 2 if ig is None else 4
    first = int(ml_rule_sum(batches[:1], thr, ig)[2])
    assert int(coll._modules["exact"].correct) == first + 2 * (N - wrong)


def test_protocol(monkeypatch):
    monkeypatch.setenv(_hip.FUSE_MULTILABEL_ENV, "1")
    N, L, ig, thr, spec, dtype = 70, 130, -1, 0.5, 200, BF16
    gen = torch.Generator().manual_seed(9)
    b = [_logits(N, L, dtype, thr, ig, gen) for _ in range(3)] + [_probs(N, L, dtype, thr, ig, gen)]
    b += [_logits(N // 2, L, dtype, thr, ig, gen) for _ in range(2)]
    dev = [(p.cuda(), t.cuda()) for p, t in b]

    coll = _make(L, ig, thr, spec)
    coll.update(*dev[0])
    coll.update(*dev[1])  # builds the plan, allocates the buffers
    plan = coll._fused_ml_plan
    assert plan is not None and plan.steps == 1
    v1 = {n: v.clone() for n, v in coll.compute().items()}

    # steady state: nothing may wait for the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        coll.update(*dev[2])
        coll.update(*dev[3])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert plan.steps == 3 and plan.curve_steps == 3
    # compute() between updates returns the value of the fresh states
    v2 = coll.compute()
    assert not _same(v1["confmat"], v2["confmat"]) and not _same(v1["auroc"], v2["auroc"])
    _assert_rule(_states(coll), b[:4], thr, ig, "before reset")

    # state_dict() after a step flushes the lazy histogram
    for m in coll.values(copy_state=False):
        m.persistent(True)
    coll.update(*dev[3])
    sd = {k: v.clone() for k, v in coll.state_dict().items()}
    old = _make(L, ig, thr, spec)
    monkeypatch.setenv(_hip.FUSE_MULTILABEL_ENV, "0")
    for p, t in dev[:4] + [dev[3]]:
        old.update(p, t)
    assert old._fused_ml_plan is None
    for name, v in _states(old).items():
        assert torch.equal(sd[name], v), name
    monkeypatch.setenv(_hip.FUSE_MULTILABEL_ENV, "1")

    # reset() replaces the states: the record follows, the scratch is zero again
    coll.reset()
    coll.update(*dev[4])
    coll.update(*dev[5])
    _assert_rule(_states(coll), b[4:], thr, ig, "after reset")
    assert plan.steps == 6

    # a stand-alone update of the curve leader between two fused steps: the
    # epoch protocol is intact and the histogram holds the sum of the three
    coll.reset()
    coll.update(*dev[0])
    plan.curve.update(*dev[3])
    coll.update(*dev[1])
    assert plan.steps == 8
    ref = ma.MultilabelAUROC(num_labels=L, thresholds=spec, ignore_index=ig, validate_args=False).to("cuda")
    for i in (0, 3, 1):
        ref.update(*dev[i])
    ref._maybe_flush_lazy()
    plan.curve._maybe_flush_lazy()
    assert torch.equal(plan.curve.confmat, ref.confmat)


def test_uncovered_inputs_are_declined(monkeypatch):
    """fp16 predictions and 3-D inputs: every leader updates on its own and the
    results equal the unfused run."""
    N, L, ig, thr, spec = 37, 33, -1, 0.5, 5
    gen = torch.Generator().manual_seed(13)
    p0, t0 = _logits(N, L, FP32, thr, ig, gen)
    p1, t1 = _logits(N, L, FP32, thr, ig, gen, plant=False)  # exact in fp16 too
    p2 = ((torch.randint(-12, 12, (N, L, 3), generator=gen) + 0.5) * 0.5)
    t2 = torch.randint(0, 2, (N, L, 3), generator=gen)
    batches = [(p0, t0), (p1.half(), t1), (p2, t2), (p1, t1)]
    coll, got, values = _run(monkeypatch, "1", L, ig, thr, spec, batches)
    assert coll._fused_ml_plan is not None and coll._fused_ml_plan.steps == 1
    _, old, old_values = _run(monkeypatch, "0", L, ig, thr, spec, batches)
    for name, v in old.items():
        assert torch.equal(got[name], v), name
    for name, v in old_values.items():
        assert _same(values[name], v), name
