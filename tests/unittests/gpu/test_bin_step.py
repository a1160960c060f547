"""The fused binary step (``csrc/bin_step.hip``) on the GPU.

A collection of F1, Accuracy, HammingDistance, ConfusionMatrix,
MatthewsCorrCoef, AUROC and AveragePrecision runs its updates from the second
one on through the fused plan (``coll._fused_bin_plan``, ``plan.steps``).

Oracle A: the same run with ``METRICS_AMD_FUSE_BINARY=0``, where every leader
updates on its own: every state and every ``compute()`` value must be equal bit
for bit. Oracle B: the rule in CPU torch (``_bin_rule``) for the stat and
confusion-matrix states. The curve is checked against oracle A only; its own
oracle tests are ``test_curve_edges.py``.

Inputs stay clear of the rounding band around the cut-off (inside a plan the
confusion-matrix leader thresholds exactly, docs/PARITY.md) and are exact in
bf16: logits ``(randint(-12, 12) + 0.5) * 0.5``, probabilities ``k/16 + 1/32``,
plus planted edge values.
"""
import copy

import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip
from tests.unittests._bin_rule import bin_rule_decisions, bin_rule_sum
from tests.unittests._curve_oracle import NONUNIFORM

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
INF, NAN = float("inf"), float("nan")

# The layout (bin_step.hip): 16-byte vectors of 8 bf16 / 4 fp32, one unit = 16
# elements per thread of a block, blocks grid-stride over the units. Below
# 128 * 8192 elements a block has 256 threads: UNIT elements per block and pass.
UNIT = 4096
# element counts around one vector of either dtype, around one unit, ndim > 2
SHAPES = [(1,), (3,), (4,), (5,), (7,), (8,), (9,), (UNIT - 1,), (UNIT,), (UNIT + 1,), (2, 3, 5, 7), (3, UNIT)]
CONFIGS = [(ig, thr, spec) for ig in (None, -1) for thr in (0.5, 0.25) for spec in (1, 5, 200, "list")]


def _id(v):
    return {BF16: "bf16", FP32: "fp32"}.get(v, str(v))


def _dt(dtype):
    return 0 if dtype == FP32 else 1


def _thresholds(spec):
    return list(NONUNIFORM) if spec == "list" else spec


def _make(ig, thr, spec):
    kw = dict(validate_args=False, ignore_index=ig)
    cut = dict(kw, threshold=thr)
    return ma.MetricCollection({
        "f1": ma.BinaryF1Score(**cut),
        "acc": ma.BinaryAccuracy(**cut),
        "hamming": ma.BinaryHammingDistance(**cut),
        "confmat": ma.BinaryConfusionMatrix(**cut),
        "mcc": ma.BinaryMatthewsCorrCoef(**cut),
        "auroc": ma.BinaryAUROC(thresholds=_thresholds(spec), **kw),
        "ap": ma.BinaryAveragePrecision(thresholds=_thresholds(spec), **kw),
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


def _target(shape, ig, gen):
    t = torch.randint(0, 2, shape, generator=gen)
    if ig is not None:
        t[torch.rand(shape, generator=gen) < 0.1] = ig
    return t


def _logits(shape, dtype, thr, ig, gen, plant=True):
    p = ((torch.randint(-12, 12, shape, generator=gen) + 0.5) * 0.5).to(dtype)
    if plant:
        # 0.0 and -0.0 sit exactly on the logit cut-off of thr = 0.5 (strict >)
        _plant(p, [0.0, -0.0, thr, 1.0, _next_above_one(dtype), INF, -INF, NAN])
    return p, _target(shape, ig, gen)


def _probs(shape, dtype, thr, ig, gen, plant=True):
    p = (torch.randint(0, 16, shape, generator=gen) / 16.0 + 1.0 / 32.0).to(dtype)
    if plant:
        _plant(p, [0.0, -0.0, thr, 1.0, NAN])  # all inside [0, 1]: NaN is not outside
    return p, _target(shape, ig, gen)


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


def _cuda(batches):
    return [(p if p.is_cuda else p.cuda(), t if t.is_cuda else t.cuda()) for p, t in batches]


def _run(monkeypatch, fuse, ig, thr, spec, batches):
    monkeypatch.setenv(_hip.FUSE_BINARY_ENV, fuse)
    coll = _make(ig, thr, spec)
    for p, t in _cuda(batches):
        coll.update(p, t)
    values = {n: v.clone() for n, v in coll.compute().items()}
    return coll, _states(coll), values


def _assert_rule(states, batches, thr, ig, what=""):
    stat, confmat = bin_rule_sum(batches, thr, ig)
    for s, w in zip(("tp", "fp", "tn", "fn"), stat):
        for name in ("f1", "acc", "hamming"):
            assert torch.equal(states[f"{name}.{s}"].cpu().reshape(1), w), (what, name, s)
    for name in ("confmat", "mcc"):
        assert torch.equal(states[f"{name}.confmat"].cpu(), confmat), (what, name)


def _check_both(monkeypatch, ig, thr, spec, batches, curve_rides=True):
    coll, got, values = _run(monkeypatch, "1", ig, thr, spec, batches)
    plan = coll._fused_bin_plan
    assert plan is not None and plan.steps == len(batches) - 1
    assert plan.curve_steps == (plan.steps if curve_rides else 0)
    old_coll, old, old_values = _run(monkeypatch, "0", ig, thr, spec, batches)
    assert old_coll._fused_bin_plan is None
    assert got.keys() == old.keys() and values.keys() == old_values.keys()
    for name, v in old.items():
        assert torch.equal(got[name], v), name
    for name, v in old_values.items():
        assert _same(values[name], v), name
    _assert_rule(got, batches, thr, ig)
    return coll


def _scaled(shape, k):
    """``shape`` with about a k-th of its elements (at least one)."""
    return (*shape[:-1], max(1, shape[-1] // k))


def _three(make, shape, dtype, thr, ig, gen):
    """Three updates, large, small, large: stale records or scratch of a larger
    step would show in the next one."""
    return [make(s, dtype, thr, ig, gen) for s in (shape, _scaled(shape, 3), shape)]


def test_the_layout_the_shapes_are_placed_on():
    for dtype, epv in ((FP32, 4), (BF16, 8)):
        lay = _hip.bin_step_layout(UNIT, _dt(dtype), 200)
        assert lay[1:4] == (UNIT, epv, 1)
        assert _hip.bin_step_layout(UNIT + epv, _dt(dtype), 200)[3] == 2


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_shapes_match_unfused_run_and_rule(monkeypatch, shape, dtype):
    # every (ignore_index, threshold, thresholds) combination is met across the shapes
    i = SHAPES.index(shape) * 2 + (dtype == BF16)
    gen = torch.Generator().manual_seed(1000 + i)
    for kind, cfg in ((_logits, CONFIGS[i % 16]), (_probs, CONFIGS[(i + 5) % 16])):
        ig, thr, spec = cfg
        _check_both(monkeypatch, ig, thr, spec, _three(kind, shape, dtype, thr, ig, gen))


@pytest.mark.parametrize("ig,thr,spec", CONFIGS, ids=_id)
def test_every_configuration(monkeypatch, ig, thr, spec):
    gen = torch.Generator().manual_seed(17)
    _check_both(monkeypatch, ig, thr, spec, _three(_logits, (2 * UNIT + 77,), BF16, thr, ig, gen))
    _check_both(monkeypatch, ig, thr, spec, _three(_probs, (45,), FP32, thr, ig, gen))


def test_empty_batch(monkeypatch):
    """N = 0 launches the tail alone: nothing changes but the epoch."""
    gen = torch.Generator().manual_seed(2)
    b = [_logits((40,), BF16, 0.5, -1, gen), _logits((0,), BF16, 0.5, -1, gen), _probs((40,), BF16, 0.5, -1, gen)]
    _check_both(monkeypatch, -1, 0.5, 200, b)


def test_blocks_walk_several_units(monkeypatch):
    """One vector more than a whole grid pass: block 0 takes a second unit with
    its counters, certainty and histograms carried over."""
    gen = torch.Generator().manual_seed(5)
    _, unit, epv, cap = _hip.bin_step_layout(1 << 30, 1, 200)[:4]
    n = cap * unit + epv + 1
    assert _hip.bin_step_layout(n, 1, 200)[3] == cap and n > cap * unit
    batches = [_logits((40,), BF16, 0.5, -1, gen), _logits((n,), BF16, 0.5, -1, gen), _probs((n,), BF16, 0.5, -1, gen)]
    _check_both(monkeypatch, -1, 0.5, 200, batches)


@pytest.mark.parametrize("n", [128 * 8192 - 1, 128 * 8192 + 9, 128 * 16384 - 1], ids=_id)
def test_block_size_thresholds(monkeypatch, n):
    """The block has 256, 512 or 1024 threads by the size of the batch (the
    last 256-thread size, the first and the last 512-thread size; the first
    1024-thread size is ``test_blocks_walk_several_units``)."""
    gen = torch.Generator().manual_seed(n)
    assert _hip.bin_step_layout(n, 1, 200)[1] == (4096 if n < 128 * 8192 else 8192)
    batches = [_probs((40,), BF16, 0.25, -1, gen), _logits((n,), BF16, 0.25, -1, gen), _probs((n,), BF16, 0.25, -1, gen)]
    _check_both(monkeypatch, -1, 0.25, 200, batches)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("sliced", ["preds", "target", "both"])
def test_misaligned_contiguous_slices(monkeypatch, sliced, dtype):
    """``buf[1:]`` is contiguous but starts 2, 4 or 8 bytes past a 16-byte
    boundary: the scalar head takes the elements in front of the first aligned
    vector, the target vectors are read 8-byte aligned."""
    gen = torch.Generator().manual_seed(31)
    ig, thr = -1, 0.25
    n = 2 * UNIT + 13
    batches = []
    for kind in (_logits, _probs, _logits):
        p, t = kind((n + 1,), dtype, thr, ig, gen)
        p, t = p.cuda(), t.cuda()
        p = p[1:] if sliced in ("preds", "both") else p[:-1].clone()
        t = t[1:] if sliced in ("target", "both") else t[:-1].clone()
        assert p.is_contiguous() and t.is_contiguous()
        assert (p.data_ptr() % 16 != 0) == (sliced != "target") and (t.data_ptr() % 16 != 0) == (sliced != "preds")
        batches.append((p, t))
    _check_both(monkeypatch, ig, thr, 200, batches)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
def test_decision_is_per_batch(monkeypatch, dtype):
    """Probabilities, logits, probabilities: each batch decides for itself, and
    scratch and records are clean between the steps."""
    gen = torch.Generator().manual_seed(41)
    ig, thr, shape = -1, 0.5, (3 * UNIT + 5,)
    b = [_logits(shape, dtype, thr, ig, gen), _probs(shape, dtype, thr, ig, gen), _logits(shape, dtype, thr, ig, gen),
         _probs(shape, dtype, thr, ig, gen)]
    _check_both(monkeypatch, ig, thr, 200, b)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("thr", [0.5, 0.25], ids=_id)
@pytest.mark.parametrize("case", ["ignored_outside", "kept_outside_last", "kept_outside_first", "kept_outside_body_end"])
def test_two_decisions(monkeypatch, case, thr, dtype):
    """The stat group normalises iff any element lies outside [0, 1], the
    confusion matrix and the curve iff any kept one does."""
    gen = torch.Generator().manual_seed(23)
    ig, n = -1, 3 * UNIT + 5
    first = _logits((n,), dtype, thr, ig, gen)
    p, t = _probs((n,), dtype, thr, ig, gen)
    if case == "ignored_outside":
        # every kept value in [0, 1], one ignored 7.5: stat takes the sigmoid
        # cut, confusion matrix and curve the raw one
        p[n // 2], t[n // 2] = 7.5, ig
        want = (True, False)
    else:
        # one kept outside value; as the LAST element every other wave has
        # binned raw before it and none of that may reach the result
        at = {"kept_outside_last": n - 1, "kept_outside_first": 0, "kept_outside_body_end": n - 6}[case]
        p[at], t[at] = 1.5, 1
        want = (True, True)
    assert bin_rule_decisions(p, t, ig) == want
    _check_both(monkeypatch, ig, thr, 5, [first, (p, t), _probs((n,), dtype, thr, ig, gen)])


def test_curve_above_the_lds_gate_updates_on_its_own(monkeypatch):
    gen = torch.Generator().manual_seed(6)
    T = _hip.BIN_STEP_MAX_T + 1
    batches = _three(_logits, (37,), BF16, 0.5, -1, gen)
    coll = _check_both(monkeypatch, -1, 0.5, T, batches, curve_rides=False)
    assert coll._fused_bin_plan.curve is not None  # in the plan, declined per step


def test_curve_at_the_lds_gate_rides(monkeypatch):
    """The largest T of the fused step: both histograms and the thresholds fill
    the LDS of a workgroup, one pair of histograms per block."""
    gen = torch.Generator().manual_seed(7)
    T = _hip.BIN_STEP_MAX_T
    assert _hip.bin_step_layout(UNIT + 9, 1, T)[5:] == (20 * T + 16, 1)
    batches = [_logits((UNIT + 9,), BF16, 0.5, -1, gen), _probs((UNIT + 9,), BF16, 0.5, -1, gen),
               _logits((37,), BF16, 0.5, -1, gen)]
    _check_both(monkeypatch, -1, 0.5, T, batches)


def test_two_runs_are_identical(monkeypatch):
    gen = torch.Generator().manual_seed(8)
    b = _three(_logits, (2 * UNIT + 3,), BF16, 0.5, -1, gen) + _three(_probs, (2 * UNIT + 3,), BF16, 0.5, -1, gen)
    _, s1, v1 = _run(monkeypatch, "1", -1, 0.5, 200, b)
    _, s2, v2 = _run(monkeypatch, "1", -1, 0.5, 200, b)
    for name, v in s1.items():
        assert torch.equal(s2[name], v), name
    for name, v in v1.items():
        assert _same(v2[name], v), name


def test_protocol(monkeypatch):
    monkeypatch.setenv(_hip.FUSE_BINARY_ENV, "1")
    ig, thr, spec, dtype, shape = -1, 0.5, 200, BF16, (2 * UNIT + 70,)
    gen = torch.Generator().manual_seed(9)
    b = [_logits(shape, dtype, thr, ig, gen) for _ in range(3)] + [_probs(shape, dtype, thr, ig, gen)]
    b += [_logits((UNIT // 2,), dtype, thr, ig, gen) for _ in range(2)]
    dev = _cuda(b)

    coll = _make(ig, thr, spec)
    coll.update(*dev[0])
    coll.update(*dev[1])  # builds the plan, allocates the buffers
    plan = coll._fused_bin_plan
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
    old = _make(ig, thr, spec)
    monkeypatch.setenv(_hip.FUSE_BINARY_ENV, "0")
    for p, t in dev[:4] + [dev[3]]:
        old.update(p, t)
    assert old._fused_bin_plan is None
    for name, v in _states(old).items():
        assert torch.equal(sd[name], v), name
    # ... and loads back into a fresh collection
    fresh = _make(ig, thr, spec)
    for m in fresh.values(copy_state=False):
        m.persistent(True)
    fresh.load_state_dict(sd)
    for name, v in _states(fresh).items():
        assert torch.equal(sd[name], v), name
    monkeypatch.setenv(_hip.FUSE_BINARY_ENV, "1")

    # reset() replaces the states: the record follows, the scratch is zero again
    coll.reset()
    coll.update(*dev[4])
    coll.update(*dev[5])
    _assert_rule(_states(coll), b[4:], thr, ig, "after reset")
    assert plan.steps == 6

    # a deep copy drops the kept record, builds its own and steps correctly
    twin = copy.deepcopy(coll)
    tplan = twin._fused_bin_plan
    assert tplan is not plan and tplan.stat is not plan.stat
    assert plan.stat.__dict__.get("_hip_bin_rec") is not None and tplan.stat.__dict__.get("_hip_bin_rec") is None
    twin.update(*dev[3])
    coll.update(*dev[3])
    assert tplan.steps == plan.steps == 7
    want = _states(coll)
    for name, v in _states(twin).items():
        assert torch.equal(want[name], v), name
    _assert_rule(want, b[4:] + [b[3]], thr, ig, "after deepcopy")

    # stand-alone updates of the curve leader and of the stat leader between
    # two fused steps: the epoch protocol is intact, the histogram holds the
    # sum of the three and the stat states all four
    coll.reset()
    coll.update(*dev[0])
    plan.curve.update(*dev[3])
    plan.stat.update(*dev[2])
    coll.update(*dev[1])
    assert plan.steps == 9
    kw = dict(ignore_index=ig, validate_args=False)
    ref = ma.BinaryAUROC(thresholds=spec, **kw).to("cuda")
    for i in (0, 3, 1):
        ref.update(*dev[i])
    ref._maybe_flush_lazy()
    plan.curve._maybe_flush_lazy()
    assert torch.equal(plan.curve.confmat, ref.confmat)
    ref = ma.BinaryStatScores(threshold=thr, **kw).to("cuda")
    for i in (0, 2, 1):
        ref.update(*dev[i])
    for s in ("tp", "fp", "tn", "fn"):
        assert torch.equal(getattr(plan.stat, s), getattr(ref, s)), s


def test_the_unfused_update_waits_for_the_device(monkeypatch):
    """The negative control of the no-sync check in ``test_protocol``: with an
    ``ignore_index`` the stand-alone confusion-matrix update indexes with a
    boolean mask, which is a host sync in every step."""
    monkeypatch.setenv(_hip.FUSE_BINARY_ENV, "0")
    gen = torch.Generator().manual_seed(9)
    dev = _cuda([_logits((UNIT + 70,), BF16, 0.5, -1, gen) for _ in range(3)])
    coll = _make(-1, 0.5, 200)
    coll.update(*dev[0])
    coll.update(*dev[1])
    assert coll._fused_bin_plan is None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            coll.update(*dev[2])
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_uncovered_inputs_are_declined(monkeypatch):
    """fp16 predictions and a non-contiguous view: every leader updates on its
    own and the results equal the unfused run."""
    ig, thr, spec, n = -1, 0.5, 5, 300
    gen = torch.Generator().manual_seed(13)
    p0, t0 = _logits((n,), FP32, thr, ig, gen)
    p1, t1 = _logits((n,), FP32, thr, ig, gen, plant=False)  # exact in fp16 too
    p2, t2 = _logits((n, 2), FP32, thr, ig, gen, plant=False)
    batches = [(p0, t0), (p1.half(), t1), (p2.cuda()[:, 0], t2.cuda()[:, 0]), (p1, t1)]
    coll, got, values = _run(monkeypatch, "1", ig, thr, spec, batches)
    assert coll._fused_bin_plan is not None and coll._fused_bin_plan.steps == 1
    _, old, old_values = _run(monkeypatch, "0", ig, thr, spec, batches)
    for name, v in old.items():
        assert torch.equal(got[name], v), name
    for name, v in old_values.items():
        assert _same(values[name], v), name
