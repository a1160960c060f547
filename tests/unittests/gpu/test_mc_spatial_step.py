"""The fused spatial multiclass step (``csrc/mc_spatial.hip``) on the GPU.

A collection of F1, Accuracy, JaccardIndex, ConfusionMatrix, ExactMatch, AUROC
and AveragePrecision fed (N, C, *spatial) predictions runs its updates from the
second one on through the fused plan (``coll._fused_sp_plan``, ``plan.steps``).

Oracle A: the same run with ``METRICS_AMD_FUSE_SPATIAL=0``, where every leader
updates on its own: every state and every ``compute()`` value of the stat,
confusion-matrix and exact-match families must be equal bit for bit, and the
curve states as well for probability inputs (every tile is deferred there and a
bucket is a pure function of the value). Oracle B: the rule in CPU torch
(``_mc_spatial_rule``) for every integer state, planted NaN / inf / zero columns
and an out-of-range target included. The curve on logits goes through the
interval oracle of ``_curve_oracle``.

Inputs are exact in bf16: logits ``(randint(-12, 12) + 0.5) * 0.5``,
probabilities ``k/16 + 1/32``. Shapes are placed with ``ma_mc_spatial_layout``.
"""
import math

import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip
from tests.unittests import _curve_oracle as oracle
from tests.unittests._curve_oracle import NONUNIFORM
from tests.unittests._mc_spatial_rule import mc_spatial_rule_sum

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = [FP32, BF16]
INF, NAN = float("inf"), float("nan")
_MACHINE_EPS = 8 * 2.0 ** -24
STAT, CONFMAT, EXACT, CURVE = ("f1", "acc"), ("jaccard", "confmat"), ("exact",), ("auroc", "ap")


def _id(v):
    return {BF16: "bf16", FP32: "fp32"}.get(v, str(v))


def _dt(dtype):
    return 0 if dtype == FP32 else 1


def _layout(N, C, S, dtype, T=0):
    keys = ("V", "vec", "tile_px", "threads", "grid", "tgrid", "lds", "cm_lds", "thr_lds", "n_tiles", "flag_cap", "rec_words")
    lay = _hip.mc_spatial_layout(N, C, S, _dt(dtype), T)
    assert lay is not None, (N, C, S, dtype, T)
    return dict(zip(keys, lay))


def _thresholds(spec):
    return list(NONUNIFORM) if spec == "list" else spec


def _num_thresholds(spec):
    return len(NONUNIFORM) if spec == "list" else spec


def _make(C, ig, spec, validate_args=False):
    kw = dict(num_classes=C, ignore_index=ig, validate_args=validate_args)
    return ma.MetricCollection({
        "f1": ma.MulticlassF1Score(**kw),
        "acc": ma.MulticlassAccuracy(**kw),
        "jaccard": ma.MulticlassJaccardIndex(**kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(thresholds=_thresholds(spec), **kw),
        "ap": ma.MulticlassAveragePrecision(thresholds=_thresholds(spec), **kw),
    }).to("cuda")


def _target(N, C, spatial, ig, gen):
    t = torch.randint(0, C, (N, *spatial), generator=gen)
    if ig is not None:
        t[torch.rand(t.shape, generator=gen) < 0.1] = ig
    return t


def _logits(N, C, spatial, dtype, ig, gen):
    p = ((torch.randint(-12, 12, (N, C, *spatial), generator=gen) + 0.5) * 0.5).to(dtype)
    return p, _target(N, C, spatial, ig, gen)


def _probs(N, C, spatial, dtype, ig, gen):
    p = (torch.randint(0, 16, (N, C, *spatial), generator=gen) / 16.0 + 1.0 / 32.0).to(dtype)
    return p, _target(N, C, spatial, ig, gen)


KINDS = {"logits": _logits, "probs": _probs}


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


def _run(monkeypatch, fuse, C, ig, spec, batches, **kw):
    monkeypatch.setenv(_hip.FUSE_SPATIAL_ENV, fuse)
    coll = _make(C, ig, spec, **kw)
    for p, t in _cuda(batches):
        coll.update(p, t)
    values = {n: v.clone() for n, v in coll.compute().items()}
    return coll, _states(coll), values


def _assert_rule(states, batches, C, ig, what=""):
    tp, fp, tn, fn, confmat, correct, total = mc_spatial_rule_sum([(p.cpu(), t.cpu()) for p, t in batches], C, ig)
    for s, w in zip(("tp", "fp", "tn", "fn"), (tp, fp, tn, fn)):
        for name in STAT:
            assert torch.equal(states[f"{name}.{s}"].cpu(), w), (what, name, s)
    for name in CONFMAT:
        assert torch.equal(states[f"{name}.confmat"].cpu(), confmat), (what, name)
    assert torch.equal(states["exact.correct"].cpu().reshape(1), correct), what
    assert torch.equal(states["exact.total"].cpu().reshape(1), total), what


def _assert_equal_runs(got, values, ref, ref_values, curve, what=""):
    families = STAT + CONFMAT + EXACT + (CURVE if curve else ())
    for name, v in ref.items():
        if name.split(".")[0] in families:
            assert torch.equal(got[name], v), (what, name)
    for name, v in ref_values.items():
        if name in families:
            assert _same(values[name], v), (what, name)


def _check_both(monkeypatch, C, ig, spec, batches, curve_equal, steps=None, curve_rides=True, rule=True, what=""):
    """The fused run against oracle A (and B); returns the fused collection."""
    coll, got, values = _run(monkeypatch, "1", C, ig, spec, batches)
    plan = coll._fused_sp_plan
    assert plan is not None, what
    assert plan.steps == (len(batches) - 1 if steps is None else steps), (what, plan.steps)
    assert plan.curve_steps == (plan.steps if curve_rides else 0), (what, plan.curve_steps)
    ref_coll, ref, ref_values = _run(monkeypatch, "0", C, ig, spec, batches)
    assert ref_coll._fused_sp_plan is None
    _assert_equal_runs(got, values, ref, ref_values, curve_equal, what)
    if rule:
        _assert_rule(got, batches, C, ig, what)
    return coll


# --------------------------------------------------------------- shapes
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_sizes_around_one_vector(monkeypatch, dtype, kind):
    gen = torch.Generator().manual_seed(1)
    for S in (1, 3, 4, 5, 7, 8, 9):
        b = [KINDS[kind](2, 3, (S,), dtype, -1, gen) for _ in range(3)]
        _check_both(monkeypatch, 3, -1, 5, b, curve_equal=kind == "probs", what=f"S={S}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_sizes_around_one_wave_tile(monkeypatch, dtype):
    """One below, at and one above a wave tile of the vector path (which is
    also a multiple of the 64-pixel tile of the element-per-lane path)."""
    gen = torch.Generator().manual_seed(2)
    tile = _layout(1, 5, 64 * 8, dtype)["tile_px"]
    assert tile == 64 * _layout(1, 5, 64 * 8, dtype)["V"]
    for S in (tile - 1, tile, tile + 1, 63, 64, 65):
        lay = _layout(2, 5, S, dtype)
        assert lay["n_tiles"] == 2 * math.ceil(S / lay["tile_px"])
        b = [_logits(2, 5, (S,), dtype, 255, gen) for _ in range(2)] + [_probs(2, 5, (S,), dtype, 255, gen)]
        _check_both(monkeypatch, 5, 255, 5, b, curve_equal=False, what=f"S={S}")


def test_a_wave_wraps_its_grid_stride(monkeypatch):
    """More tiles than the full grid has waves: the first waves take two."""
    probe = _layout(1, 2, 1 << 24, FP32, 5)
    waves = probe["grid"] * (probe["threads"] // 64)
    assert probe["grid"] == probe["rec_words"] // 3  # the grid cap
    S = 64 * (waves + 1) + 1  # element-per-lane path: 64 pixels per tile
    lay = _layout(1, 2, S, FP32, 5)
    assert lay["vec"] == 0 and lay["n_tiles"] == waves + 2 and lay["grid"] == probe["grid"]
    gen = torch.Generator().manual_seed(3)
    b = [_logits(1, 2, (S,), FP32, -1, gen), _probs(1, 2, (S,), FP32, -1, gen), _logits(1, 2, (S,), FP32, -1, gen)]
    _check_both(monkeypatch, 2, -1, 5, b, curve_equal=False)


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_images_after_the_first_start_misaligned(monkeypatch, dtype, N):
    gen = torch.Generator().manual_seed(4 + N)
    V = _layout(1, 4, 8, dtype)["V"]
    S = 64 * V + 3
    assert S % V != 0 and _layout(N, 4, S, dtype)["vec"] == 0
    b = [_probs(N, 4, (S,), dtype, -1, gen) for _ in range(3)]
    _check_both(monkeypatch, 4, -1, 5, b, curve_equal=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_contiguous_slices_with_a_storage_offset(monkeypatch, dtype):
    """``buf[1:]`` of a batch keeps the 16-byte alignment (vector path at an
    offset); a view one element into a flat buffer loses it (element path)."""
    gen = torch.Generator().manual_seed(6)
    C, H, W = 3, 4, 8
    batches = []
    for i in range(3):
        p, t = _probs(3, C, (H, W), dtype, -1, gen)
        p, t = p.cuda(), t.cuda()
        sl = (p[1:], t[1:])
        flat = torch.zeros(p.numel() + 1, dtype=dtype, device="cuda")
        flat[1:] = p.reshape(-1)
        off = (flat[1:].view(3, C, H, W), t)
        assert sl[0].is_contiguous() and sl[0].storage_offset() > 0 and sl[0].data_ptr() % 16 == 0
        assert off[0].is_contiguous() and off[0].data_ptr() % 16 != 0
        batches += [sl, off]
    _check_both(monkeypatch, C, -1, 5, batches, curve_equal=True)


@pytest.mark.parametrize("spatial", [(6,), (3, 8), (2, 3, 4)], ids=["ndim3", "ndim4", "ndim5"])
def test_ndim_3_4_5(monkeypatch, spatial):
    gen = torch.Generator().manual_seed(7)
    b = [_logits(2, 6, spatial, BF16, -1, gen) for _ in range(2)] + [_probs(2, 6, spatial, BF16, -1, gen)]
    _check_both(monkeypatch, 6, -1, 5, b, curve_equal=False)
    b = [_probs(2, 6, spatial, FP32, None, gen) for _ in range(3)]
    _check_both(monkeypatch, 6, None, "list", b, curve_equal=True)


@pytest.mark.parametrize("C", [2, 3, 19, 64, 65, 128, 129])
def test_class_counts(monkeypatch, C):
    """Both sides of the tiny kernel's LDS-matrix switch (64) and of the
    stand-alone stat kernels' switch (128)."""
    gen = torch.Generator().manual_seed(C)
    dtype = BF16 if C % 2 else FP32
    b = [_logits(2, C, (72,), dtype, -1, gen), _probs(2, C, (72,), dtype, -1, gen), _logits(2, C, (72,), dtype, -1, gen)]
    _check_both(monkeypatch, C, -1, 5, b, curve_equal=False, what="T=5")
    if _hip.mc_spatial_curve_rides(C, 200):
        b = [_probs(2, C, (72,), dtype, 255, gen) for _ in range(3)]
        _check_both(monkeypatch, C, 255, 200, b, curve_equal=True, what="T=200")


def test_both_sides_of_this_steps_lds_matrix_switch(monkeypatch):
    """The (C, C) matrix is counted in LDS while it fits behind the histogram
    and with global atomics beyond; where that happens at T = 200 is taken
    from the layout."""
    gen = torch.Generator().manual_seed(20)
    cmax = _hip.mc_spatial_max_curve_classes(200)
    first = next(c for c in range(2, cmax + 1) if _layout(2, c, 72, BF16, 200)["cm_lds"] == 0)
    assert 2 < first <= cmax and _layout(2, first - 1, 72, BF16, 200)["cm_lds"] == 1
    for C in (first - 1, first):
        b = [_logits(2, C, (72,), BF16, -1, gen), _probs(2, C, (72,), BF16, -1, gen), _logits(2, C, (72,), BF16, -1, gen)]
        _check_both(monkeypatch, C, -1, 200, b, curve_equal=False, what=f"C={C}")


def test_class_cap(monkeypatch):
    cap = _hip.MC_SPATIAL_MAX_C
    assert cap >= 256
    gen = torch.Generator().manual_seed(8)
    b = [_probs(1, cap, (9,), FP32, -1, gen) for _ in range(3)]
    _check_both(monkeypatch, cap, -1, 5, b, curve_equal=True)
    b = [_probs(1, cap + 1, (9,), FP32, -1, gen) for _ in range(3)]
    _check_both(monkeypatch, cap + 1, -1, 5, b, curve_equal=True, steps=0, what="one above the cap")


# ------------------------------------------------------- configurations
@pytest.mark.parametrize("spec", [1, 5, 200, "list"])
@pytest.mark.parametrize("ig", [None, -1, 255])
def test_configurations(monkeypatch, ig, spec):
    gen = torch.Generator().manual_seed(9)
    C, spatial = 19, (5, 24)
    b = [_probs(2, C, spatial, BF16, ig, gen) for _ in range(3)]
    _check_both(monkeypatch, C, ig, spec, b, curve_equal=True, what="probs")
    b = [_logits(2, C, spatial, FP32, ig, gen) for _ in range(3)]
    _check_both(monkeypatch, C, ig, spec, b, curve_equal=False, what="logits")


def test_all_ignored_and_empty_batches(monkeypatch):
    """The stand-alone stat update cannot reshape an empty (0, C, *spatial)
    batch, so oracle A runs without it: an empty batch adds nothing."""
    gen = torch.Generator().manual_seed(10)
    C, spatial, ig = 5, (3, 11), -1
    first = _probs(3, C, spatial, FP32, ig, gen)
    all_ignored = (_probs(3, C, spatial, FP32, ig, gen)[0], torch.full((3, *spatial), ig))
    one_sample = _probs(3, C, spatial, FP32, ig, gen)
    one_sample[1][1] = ig  # exact match counts that sample correct
    empty = (torch.zeros(0, C, *spatial), torch.zeros(0, *spatial, dtype=torch.long))
    b = [first, all_ignored, one_sample, empty, _probs(3, C, spatial, FP32, ig, gen)]
    coll, got, values = _run(monkeypatch, "1", C, ig, 5, b)
    assert coll._fused_sp_plan.steps == 4 and coll._fused_sp_plan.curve_steps == 4
    _assert_rule(got, b, C, ig)
    ref_coll, ref, ref_values = _run(monkeypatch, "0", C, ig, 5, b[:3] + b[4:])
    assert ref_coll._fused_sp_plan is None
    _assert_equal_runs(got, values, ref, ref_values, curve=True)


# ------------------------------------------------------- planted values
def _planted(C, dtype, gen):
    p, t = _logits(2, C, (40,), dtype, -1, gen)
    t[0, :8] = torch.arange(8) % C  # none of the planted pixels is ignored
    p[0, 1, 0] = NAN  # partial NaN
    p[0, :, 1] = NAN  # all NaN
    p[0, 2, 2] = INF
    p[0, 1:3, 3] = INF  # tie of infinities: the lower index
    p[0, :, 4] = -INF
    p[0, :, 5] = -1.0
    p[0, 1, 5], p[0, 2, 5] = 0.0, -0.0  # +0.0 / -0.0 tie
    p[0, :, 6] = -1.0
    p[0, 1, 6], p[0, 2, 6] = -0.0, 0.0
    p[0, 0, 7] = NAN
    p[0, 1, 7] = -INF  # nothing exceeds -inf: index 0
    t[1, 3] = C + 5  # out of range, not ignored
    return p, t


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C", [3, 19, 129])
def test_planted_values_follow_the_rule(monkeypatch, C, dtype):
    gen = torch.Generator().manual_seed(11 + C)
    b = [_planted(C, dtype, gen) for _ in range(3)]
    coll, got, _ = _run(monkeypatch, "1", C, -1, 5, b)
    assert coll._fused_sp_plan.steps == 2 and coll._fused_sp_plan.curve_steps == 2
    # the first update is a stand-alone one; the rule is held against the fused steps
    first = _run(monkeypatch, "1", C, -1, 5, b[:1])[1]
    delta = {k: v - first[k] for k, v in got.items() if v.dtype == torch.long}
    _assert_rule(delta, b[1:], C, -1)


@pytest.mark.parametrize("C", [3, 64, 128])
def test_all_nan_columns_equal_the_unfused_run(monkeypatch, C):
    """An all-NaN column has argmax 0 in the tiny kernel, in torch.argmax and
    here; above C = 128 the stand-alone wave kernel drops such a row
    (docs/PARITY.md), so the comparison stops at 128."""
    gen = torch.Generator().manual_seed(12)
    b = []
    for _ in range(3):
        p, t = _logits(2, C, (33,), FP32, -1, gen)
        p[0, :, 5] = NAN
        p[1, :, 32] = NAN
        t[0, 5], t[1, 32] = 0, 1
        b.append((p, t))
    _check_both(monkeypatch, C, -1, 5, b, curve_equal=False, rule=False)


# ------------------------------------------------------- curve decision
def _rows(p):
    return p.movedim(1, -1).reshape(-1, p.shape[1])


def _rowinv_error(metric, logits, what=""):
    """Largest relative difference between the stored rowinv and fp64 1/sum(exp(x - max))."""
    x = _rows(logits).float().cpu().double()
    buf = metric.__dict__["_hip_rowstats_buf"][:, : x.shape[0]].cpu().double()
    mx = x.max(1).values
    assert torch.equal(buf[0], mx), what  # the online max is exact
    ref = 1.0 / torch.exp(x - mx[:, None]).sum(1)
    return float(((buf[1].abs() - ref).abs() / ref).max())


def _interval_sum(batches, thr, eps, ig):
    certain = amb = None
    for p, t in batches:
        probs = torch.softmax(_rows(p).float().cpu().double(), -1)
        c, a = oracle.multiclass_confmat_interval(probs, t.cpu().reshape(-1), thr, eps, ig)
        certain, amb = (c, a) if certain is None else (certain + c, amb + a)
    return certain, amb


def test_decision_is_per_batch(monkeypatch):
    """A probability batch, a batch with one kept pixel at 1 + ulp (softmax)
    and a batch whose only value outside [0,1] sits at an ignored pixel (no
    softmax), after the stand-alone first update."""
    gen = torch.Generator().manual_seed(13)
    C, spatial, ig, T = 7, (6, 20), -1, 100
    first = _probs(2, C, spatial, FP32, ig, gen)
    plain = _probs(2, C, spatial, FP32, ig, gen)
    above = _probs(2, C, spatial, FP32, ig, gen)
    above[1][1, 2, 7] = 3
    above[0][1, 4, 2, 7] = 1.0 + 2.0 ** -23
    hidden = _probs(2, C, spatial, FP32, ig, gen)
    hidden[1][0, 5, 19] = ig
    hidden[0][0, 1, 5, 19] = 9.5
    # oracle A on the two batches that are not softmaxed
    _check_both(monkeypatch, C, ig, T, [first, plain, hidden], curve_equal=True)
    coll = _check_both(monkeypatch, C, ig, T, [first, plain, above, hidden], curve_equal=False)
    # the softmaxed batch through the interval oracle, the others exactly
    curve = coll._fused_sp_plan.curve
    thr = torch.linspace(0, 1, T)
    exact = sum(oracle.multiclass_confmat(_rows(p).float(), t.reshape(-1), thr, ig) for p, t in (first, plain, hidden))
    monkeypatch.setenv(_hip.FUSE_SPATIAL_ENV, "1")
    probe = _make(C, ig, T)
    probe.update(*_cuda([first])[0])
    probe.update(*_cuda([above])[0])
    measured = _rowinv_error(probe._fused_sp_plan.curve, above[0])
    eps = 4 * measured + _MACHINE_EPS
    assert eps <= 1e-5, (measured, eps)
    certain, amb = _interval_sum([above], thr, eps, ig)
    curve._maybe_flush_lazy()
    oracle.assert_within(curve.confmat, certain + exact, amb)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize(
    "shape", [(3, 19, 5, 24, 100, 4.0), (2, 21, 7, 9, 200, 4.0), (2, 96, 4, 40, 200, 3.0), (3, 101, 3, 8, 200, 3.0)],
    ids=["C19-T100", "C21-T200", "C96-T200", "C101-T200"],
)
def test_random_logits_softmax_within_interval(monkeypatch, shape, dtype):
    """Every count lies in [certain, certain + ambiguous] of the fp64 oracle, where a
    score is ambiguous within a relative band eps around a threshold:
    eps = 4 * (largest relative error of the stored rowinv against fp64, measured here
    after every update) + 8 * 2^-24, as in ``test_curve_edges.py``. The test fails,
    instead of widening the band, if eps exceeds 1e-5 or if more than 0.5 % of the
    counted elements are ambiguous (fp64 alone at eps = 1e-5 leaves at most 0.00015 %
    for these shapes).

    Measured on an MI355X, rowinv relative error (the larger of the stand-alone first
    update and the two fused steps; the serial fold over C classes rounds C times, so
    it grows with C), fp32 / bf16: 3.10e-7 / 3.23e-7 (C=19), 3.90e-7 / 2.56e-7 (C=21),
    7.61e-7 / 5.36e-7 (C=96), 4.34e-7 / 4.85e-7 (C=101); eps is 1.5e-6 .. 3.6e-6 and the
    ambiguous share came out at most 0.00005 % of the counted elements.
    """
    monkeypatch.setenv(_hip.FUSE_SPATIAL_ENV, "1")
    N, C, H, W, T, scale = shape
    g = torch.Generator().manual_seed(sum(shape[:5]))
    batches = []
    for _ in range(3):
        logits = (torch.randn(N, C, H, W, generator=g) * scale).to(dtype)
        batches.append((logits, torch.randint(0, C, (N, H, W), generator=g)))
    thr = torch.linspace(0, 1, T)
    coll = _make(C, None, T)
    measured = 0.0
    for i, (p, t) in enumerate(_cuda(batches)):
        coll.update(p, t)
        # the first update is a stand-alone one of every member, the others are the leader's
        owner = coll._fused_sp_plan.curve if i else getattr(coll, "auroc")
        measured = max(measured, _rowinv_error(owner, batches[i][0], f"update {i}"))
    plan = coll._fused_sp_plan
    assert plan.steps == 2 and plan.curve_steps == 2
    eps = 4 * measured + _MACHINE_EPS
    print(f"rowinv relative error {measured:.3e}, eps {eps:.3e} ({shape}, {dtype})")
    assert eps <= 1e-5, (measured, eps)
    certain, amb = _interval_sum(batches, thr, eps, None)
    share = float(amb[:, :, :, 0].sum()) / (3 * N * H * W * C * T)
    print(f"ambiguous share {share:.5%}")
    assert share <= 0.005, share
    plan.curve._maybe_flush_lazy()
    oracle.assert_within(plan.curve.confmat, certain, amb)


def test_curve_gate(monkeypatch):
    """The largest C that rides at T = 200 rides; one above it the curve
    leader updates on its own and the other leaders still fuse."""
    gen = torch.Generator().manual_seed(14)
    cmax = _hip.mc_spatial_max_curve_classes(200)
    assert _hip.mc_spatial_curve_rides(cmax, 200) and not _hip.mc_spatial_curve_rides(cmax + 1, 200)
    b = [_probs(2, cmax, (3, 8), BF16, -1, gen) for _ in range(3)]
    _check_both(monkeypatch, cmax, -1, 200, b, curve_equal=True)
    b = [_probs(2, cmax + 1, (3, 8), BF16, -1, gen) for _ in range(3)]
    _check_both(monkeypatch, cmax + 1, -1, 200, b, curve_equal=True, curve_rides=False)


# ------------------------------------------------------------- protocol
def test_two_runs_give_identical_bits(monkeypatch):
    gen = torch.Generator().manual_seed(15)
    b = [_logits(2, 19, (5, 24), BF16, -1, gen) for _ in range(4)]
    _, s1, v1 = _run(monkeypatch, "1", 19, -1, 200, b)
    _, s2, v2 = _run(monkeypatch, "1", 19, -1, 200, b)
    for name, v in s1.items():
        assert torch.equal(s2[name], v), name
    for name, v in v1.items():
        assert _same(v2[name], v), name


def test_protocol(monkeypatch):
    monkeypatch.setenv(_hip.FUSE_SPATIAL_ENV, "1")
    C, ig, T, spatial = 19, -1, 200, (5, 24)
    gen = torch.Generator().manual_seed(16)
    b = [_logits(3, C, spatial, BF16, ig, gen) for _ in range(3)] + [_probs(3, C, spatial, BF16, ig, gen) for _ in range(3)]
    dev = _cuda(b)
    coll = _make(C, ig, T)
    coll.update(*dev[0])
    coll.update(*dev[1])  # builds the plan, allocates the buffers
    plan = coll._fused_sp_plan
    assert plan is not None and plan.steps == 1 and coll._fused_plan.try_run(*dev[1]) == ()
    E = plan.curve.__dict__["_hip_epoch_buf"]
    e1 = E.cpu().tolist()

    # steady state: nothing may wait for the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        coll.update(*dev[2])
        coll.update(*dev[3])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert plan.steps == 3 and plan.curve_steps == 3
    e3 = E.cpu().tolist()
    assert e3[1] == e1[1] + 2 and e3[0] <= e3[1]  # one epoch per step, E[0] never ahead
    base = plan.stat
    for owner, key in ((base, "_hip_sp_counts"), (plan.exact, "_hip_sp_rowbad"), (plan.curve, "_hip_sp_tile_flags")):
        assert int(owner.__dict__[key].count_nonzero()) == 0, key
    _assert_rule(_states(coll), b[:4], C, ig, "four updates")

    # a stand-alone update of the curve leader between two fused steps
    plan.curve.update(*dev[4])
    coll.update(*dev[5])
    assert plan.steps == 4
    e5 = E.cpu().tolist()
    assert e5[1] == e3[1] + 2 and e5[0] <= e5[1]
    ref = ma.MulticlassAUROC(num_classes=C, thresholds=T, ignore_index=ig, validate_args=False).to("cuda")
    for i in (3, 4, 5):  # the probability batches: exact whatever path binned them
        ref.update(*dev[i])
    ref._maybe_flush_lazy()
    thr = torch.linspace(0, 1, T)
    want = sum(oracle.multiclass_confmat(_rows(p).float(), t.reshape(-1), thr, ig) for p, t in b[3:])
    assert torch.equal(ref.confmat.cpu(), want)
    eps = 1e-5  # the bound the interval tests hold the measured eps under
    certain, amb = _interval_sum(b[:3], thr, eps, ig)
    plan.curve._maybe_flush_lazy()
    oracle.assert_within(plan.curve.confmat, certain + want, amb)


def test_the_unfused_update_waits_for_the_device(monkeypatch):
    """The negative control of the no-sync check in ``test_protocol``: with an
    ``ignore_index`` the stand-alone exact-match update writes through a
    boolean mask, which is a host sync in every step."""
    monkeypatch.setenv(_hip.FUSE_SPATIAL_ENV, "0")
    gen = torch.Generator().manual_seed(16)
    dev = _cuda([_logits(3, 19, (5, 24), BF16, -1, gen) for _ in range(3)])
    coll = _make(19, -1, 200)
    coll.update(*dev[0])
    coll.update(*dev[1])
    assert coll._fused_sp_plan is None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            coll.update(*dev[2])
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_2d_batches_with_a_pending_histogram_then_a_4d_batch(monkeypatch):
    """The one-pass step over (B, C) logits leaves the curve leader's histogram
    in pending-b0 format; the spatial step flushes it before it adds to it."""
    monkeypatch.setenv(_hip.ONEPASS_ENV, "2")
    C, T, ig = 136, 100, -1
    assert _hip.mc_spatial_curve_rides(C, T)
    gen = torch.Generator().manual_seed(17)
    flat = []
    for _ in range(2):
        p = ((torch.randint(-12, 12, (70, C), generator=gen) + 0.5) * 0.5).to(BF16)
        flat.append((p, torch.randint(0, C, (70,), generator=gen)))
    b = flat + [_probs(2, C, (3, 8), BF16, ig, gen), _probs(2, C, (3, 8), BF16, ig, gen)]
    coll, got, values = _run(monkeypatch, "1", C, ig, T, b)
    assert coll._fused_plan.onepass_steps == 1 and coll._fused_sp_plan.steps == 2
    assert coll._fused_sp_plan.curve_steps == 2
    ref_coll, ref, ref_values = _run(monkeypatch, "0", C, ig, T, b)
    assert ref_coll._fused_plan.onepass_steps == 1 and ref_coll._fused_sp_plan is None
    _assert_equal_runs(got, values, ref, ref_values, curve=True)
    # the flag itself: pending after the 2-D step, cleared by the spatial step
    probe = _make(C, ig, T)
    for p, t in _cuda(flat):
        probe.update(p, t)
    curve = probe._fused_plan.curve
    assert curve.__dict__.get("_hip_b0_pending")
    probe.update(*_cuda(b[2:3])[0])
    assert not curve.__dict__.get("_hip_b0_pending") and curve.__dict__.get("_lazy_dirty")


# ------------------------------------------------------ declined inputs
def test_uncovered_inputs_are_declined(monkeypatch):
    """fp16, channels-last and a keyword call: every leader updates on its own
    and the results equal the unfused run."""
    C, ig, gen = 5, -1, torch.Generator().manual_seed(18)
    p0, t0 = _probs(2, C, (4, 8), FP32, ig, gen)
    p1, t1 = _probs(2, C, (4, 8), FP32, ig, gen)  # exact in fp16 too
    p2, t2 = _probs(2, C, (4, 8), FP32, ig, gen)
    batches = [(p0, t0), (p1.half(), t1), (p2.cuda().to(memory_format=torch.channels_last), t2), (p1, t1)]
    assert not batches[2][0].is_contiguous()
    coll, got, values = _run(monkeypatch, "1", C, ig, 5, batches)
    assert coll._fused_sp_plan.steps == 1  # the last batch alone
    coll.update(preds=p2.cuda(), target=t2.cuda())
    assert coll._fused_sp_plan.steps == 1
    got, values = _states(coll), {n: v.clone() for n, v in coll.compute().items()}
    monkeypatch.setenv(_hip.FUSE_SPATIAL_ENV, "0")
    ref_coll = _make(C, ig, 5)
    for p, t in _cuda(batches):
        ref_coll.update(p, t)
    ref_coll.update(preds=p2.cuda(), target=t2.cuda())
    assert ref_coll._fused_sp_plan is None
    ref, ref_values = _states(ref_coll), {n: v.clone() for n, v in ref_coll.compute().items()}
    _assert_equal_runs(got, values, ref, ref_values, curve=True)


def test_integer_predictions_are_declined(monkeypatch):
    """(N, *spatial) label predictions, in a collection without curve members
    (those take scores only)."""
    C, ig, gen = 5, -1, torch.Generator().manual_seed(21)

    def make():
        kw = dict(num_classes=C, ignore_index=ig, validate_args=False)
        return ma.MetricCollection({
            "f1": ma.MulticlassF1Score(**kw), "confmat": ma.MulticlassConfusionMatrix(**kw),
            "exact": ma.MulticlassExactMatch(**kw),
        }).to("cuda")

    p0, t0 = _probs(2, C, (4, 8), FP32, ig, gen)
    p1, t1 = _probs(2, C, (4, 8), FP32, ig, gen)
    labels = torch.randint(0, C, (2, 4, 8), generator=gen)
    batches = _cuda([(p0, t0), (labels, t1), (p1, t1)])
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv(_hip.FUSE_SPATIAL_ENV, fuse)
        coll = make()
        for p, t in batches:
            coll.update(p, t)
        out[fuse] = (_states(coll), {n: v.clone() for n, v in coll.compute().items()})
        plan = coll._fused_sp_plan
        assert (plan.steps, plan.curve_steps) == (1, 0) if fuse == "1" else plan is None
    for name, v in out["0"][0].items():
        assert torch.equal(out["1"][0][name], v), name
    for name, v in out["0"][1].items():
        assert _same(out["1"][1][name], v), name


def test_validate_args_builds_no_plan(monkeypatch):
    gen = torch.Generator().manual_seed(19)
    b = [_probs(2, 5, (4, 8), FP32, None, gen) for _ in range(3)]
    coll, got, values = _run(monkeypatch, "1", 5, None, 5, b, validate_args=True)
    assert coll._fused_sp_plan is None
    _, ref, ref_values = _run(monkeypatch, "0", 5, None, 5, b, validate_args=True)
    _assert_equal_runs(got, values, ref, ref_values, curve=True)
    _assert_rule(got, b, 5, None)
