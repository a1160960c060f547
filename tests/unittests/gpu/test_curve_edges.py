"""Threshold-curve and fused stat kernels at the values where they can go wrong.

Random floats almost never land ON a threshold, never are NaN and never put an
out-of-range value on an ignored sample. Here the scores come from adversarial
pools (every threshold, its float neighbours, signed zeros, denormals, 1 and
the float below it — tests/unittests/_curve_oracle.py), and the expected value
is an independent fp64 oracle that is proved against the CPU ops and against
the reference's own record in tests/unittests/test_curve_oracle.py.

The kernels are integer-exact by design, so every assertion is ``torch.equal``
except the random-logit interval check at the end.
"""
import warnings

import pytest
import torch

import metrics_amd as ma
from metrics_amd import ops
from metrics_amd.ops import _hip
from tests.unittests import _curve_cases as cases
from tests.unittests import _curve_oracle as oracle

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]
SPECS = oracle.threshold_specs()
IGN = -1


def _dev(*xs):
    return tuple(x.cuda() for x in xs)


def _mc_target(scores, thr, C):
    """Row targets that put label 1 on an exact threshold hit wherever a row has one."""
    hit = torch.isin(scores.float(), thr)
    first = hit.float().argmax(1)
    rows = torch.arange(scores.shape[0])
    return torch.where(hit.any(1), first, rows % C).long()


# =====================================================================
# a. raw ops, no normalisation
# =====================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("spec", list(SPECS))
def test_binary_hist_pools(spec, dtype):
    """N = 1, 257 and 2048*256+257 (the grid is capped at 2048 blocks of 256: the
    last size wraps the grid-stride loop), with and without ignore_index, and a
    batch in which every sample is ignored."""
    thr = SPECS[spec]
    pool = oracle.value_pool(thr, dtype)
    thr_d = thr.cuda()
    for N in (1, 257, 2048 * 256 + 257):
        scores, labels = oracle.binary_layout(pool, N)
        if N >= 2 * pool.numel():
            assert oracle.coverage(scores, labels, pool) == [True, True]
        got = ops.binary_curve_confmat(scores.cuda(), labels.cuda(), thr_d).cpu()
        assert torch.equal(got, oracle.binary_confmat(scores, labels, thr)), (spec, N)
        tgt = labels.clone()
        tgt[::3] = IGN
        got = ops.binary_curve_confmat(scores.cuda(), tgt.cuda(), thr_d, ignore_index=IGN).cpu()
        assert torch.equal(got, oracle.binary_confmat(scores, tgt, thr, ignore_index=IGN)), (spec, N, "ignore")
    scores, labels = oracle.binary_layout(pool, 257)
    none = torch.full_like(labels, IGN)
    got = ops.binary_curve_confmat(scores.cuda(), none.cuda(), thr_d, ignore_index=IGN).cpu()
    assert torch.equal(got, torch.zeros(thr.numel(), 2, 2, dtype=torch.long))


def test_matrix_layout_covers_lanes_chunks_and_rows():
    """The (B, C) layout the kernel tests below use: at B=257, C=19 every pool value of
    every spec meets both labels, and exact threshold hits land on the first and the
    last lane of a wave, the first and the last class (of the row and of a 4-wide
    chunk), and on the last row — with label 0 and with label 1."""
    B, C = 257, 19
    for spec, thr in SPECS.items():
        for dtype in DTYPES:
            pool = oracle.value_pool(thr, dtype)
            scores, labels = oracle.matrix_layout(pool, B, C)
            assert oracle.coverage(scores, labels, pool) == [True, True], (spec, dtype)
            if dtype == torch.bfloat16 and spec not in ("lin1", "lin2", "lin5"):
                continue  # larger grids have too few bf16-exact values; lin5 gives 0.25/0.5/0.75
            hit = torch.isin(scores.float(), thr)
            rows, cols = hit.nonzero(as_tuple=True)
            for lab in (0, 1):
                sel = labels[rows, cols] == lab
                r, c = rows[sel], cols[sel]
                assert (r % 64 == 0).any() and (r % 64 == 63).any(), (spec, dtype, lab)
                assert (c == 0).any() and (c == C - 1).any(), (spec, dtype, lab)
                assert (c % 4 == 0).any() and (c % 4 == 3).any(), (spec, dtype, lab)
                assert (r == B - 1).any(), (spec, dtype, lab)


def _matrix_case(thr, dtype, B, C):
    pool = oracle.value_pool(thr, dtype)
    scores, ml = oracle.matrix_layout(pool, B, C)
    mc = _mc_target(scores, thr, C)
    mc_ign = mc.clone()
    mc_ign[::3] = IGN
    ml_ign = ml.clone()
    ml_ign.view(-1)[::5] = IGN
    want = {
        "mc": oracle.multiclass_confmat(scores, mc, thr),
        "mc_ign": oracle.multiclass_confmat(scores, mc_ign, thr, ignore_index=IGN),
        "ml": oracle.multilabel_confmat(scores, ml, thr),
        "ml_ign": oracle.multilabel_confmat(scores, ml_ign, thr, ignore_index=IGN),
    }
    return scores.cuda(), {"mc": mc.cuda(), "mc_ign": mc_ign.cuda(), "ml": ml.cuda(), "ml_ign": ml_ign.cuda()}, want


def _check_matrix(scores_d, tgts, want, thr_d, tag):
    for name, t in tgts.items():
        fn = ops.multiclass_curve_confmat if name.startswith("mc") else ops.multilabel_curve_confmat
        got = fn(scores_d, t, thr_d, ignore_index=IGN if name.endswith("_ign") else None).cpu()
        assert torch.equal(got, want[name]), (tag, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("spec", list(SPECS))
def test_ballot_hist_pools(monkeypatch, spec, dtype):
    """Ballot-merge kernel. Chunk override 4 with C % 4 == 0 takes the float4/ushort4
    tile load, chunk 1 with C in {16, 17, 19} the XCD band remap (gridDim.x >= 16) with
    and without a tail, chunk 3 a ragged last chunk; 0 is the default heuristic."""
    thr = SPECS[spec]
    thr_d = thr.cuda()
    monkeypatch.setattr(_hip, "_CURVE_VARIANT", 0)
    for B in (1, 63, 257):
        for C in (1, 3, 4, 5, 8, 16, 17, 19):
            scores_d, tgts, want = _matrix_case(thr, dtype, B, C)
            for chunk in (0, 1, 3, 4):
                monkeypatch.setattr(_hip, "_CURVE_CCHUNK", chunk)
                _check_matrix(scores_d, tgts, want, thr_d, (spec, B, C, chunk))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("spec", list(SPECS))
def test_lds_hist_pools(monkeypatch, spec, dtype):
    """LDS-privatised variant (probe knob). A chunk override above 32 must not drop
    classes 32.. of a chunk: the launcher clamps it to the 32 classes a block maps."""
    thr = SPECS[spec]
    thr_d = thr.cuda()
    monkeypatch.setattr(_hip, "_CURVE_VARIANT", 1)
    for C in (1, 31, 32, 33, 65):
        for B in (1, 7, 9, 257, 600):
            scores_d, tgts, want = _matrix_case(thr, dtype, B, C)
            for chunk in (0, 8, 64):
                monkeypatch.setattr(_hip, "_CURVE_CCHUNK", chunk)
                _check_matrix(scores_d, tgts, want, thr_d, (spec, B, C, chunk))


@pytest.mark.parametrize("T", [1, 63, 64, 127, 128, 1280])
def test_suffix_accumulates_onto_state_and_rezeroes_hist(T):
    """T+1 in {2, 64, 65, 128, 129}: the wave-parallel scan of the tiled suffix kernel
    with an empty, exact and ragged last lane chunk; C=5 leaves a class tail in its
    4-class tile; T=1280 is the first size served by the one-class-per-block kernel.
    Two updates through curve_hist_into_confmat(owner=None) onto a non-zero state; the
    pooled histogram must be all zero afterwards."""
    B, C = 257, 5
    thr = torch.linspace(0, 1, T) if T > 1 else torch.tensor([0.5])
    pool = oracle.value_pool(thr, torch.float32)
    scores, ml = oracle.matrix_layout(pool, B, C)
    mc = _mc_target(scores, thr, C)
    g = torch.Generator().manual_seed(T)
    thr_d = thr.cuda()
    # multiclass / multilabel: transposed (T, C, 2, 2) state
    for mode, tgt, fn in ((0, mc, oracle.multiclass_confmat), (1, ml, oracle.multilabel_confmat)):
        prior = torch.randint(1, 1000, (T, C, 2, 2), generator=g)
        state = prior.cuda()
        for _ in range(2):
            _hip.curve_hist_into_confmat(scores.cuda(), tgt.cuda(), thr_d, None, state, mode=mode, owner=None)
        assert torch.equal(state.cpu(), prior + 2 * fn(scores, tgt, thr)), (T, mode)
        assert not bool(_hip._pooled_hist(C, T, state.device).any())
    # binary: (T, 2, 2) state, one-block suffix kernel
    bs, bl = oracle.binary_layout(pool, 2 * pool.numel() + 7)
    prior = torch.randint(1, 1000, (T, 2, 2), generator=g)
    state = prior.cuda()
    for _ in range(2):
        _hip.curve_hist_into_confmat(bs.cuda(), bl.cuda(), thr_d, None, state, mode=0, owner=None)
    assert torch.equal(state.cpu(), prior + 2 * oracle.binary_confmat(bs, bl, thr))
    assert not bool(_hip._pooled_hist(1, T, state.device).any())


@pytest.mark.parametrize("variant", [0, 1], ids=["ballot", "lds"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("spec", ["lin2", "lin5", "lin65", "lin200", "list"])
def test_nan_scores_are_negative_at_every_threshold(monkeypatch, spec, dtype, variant):
    """NaN compares false against every threshold: bucket 0 on the uniform grid (O(1)
    guess) exactly as on the non-uniform one (binary search) and in the reference."""
    thr = SPECS[spec]
    thr_d = thr.cuda()
    monkeypatch.setattr(_hip, "_CURVE_VARIANT", variant)
    pool = torch.cat([oracle.value_pool(thr, dtype), torch.full((3,), float("nan"), dtype=dtype)])
    scores, labels = oracle.binary_layout(pool, 2 * pool.numel() + 5)
    assert torch.isnan(scores[labels == 0].float()).any() and torch.isnan(scores[labels == 1].float()).any()
    want = oracle.binary_confmat(scores, labels, thr)
    n_nan = [int(torch.isnan(scores[labels == lab].float()).sum()) for lab in (0, 1)]
    assert int(want[0, 0, 0]) >= n_nan[0] and int(want[0, 1, 0]) >= n_nan[1]  # tn / fn even at the lowest threshold
    got = ops.binary_curve_confmat(scores.cuda(), labels.cuda(), thr_d).cpu()
    assert torch.equal(got, want), spec
    B, C = 63, 5
    ms, ml = oracle.matrix_layout(pool, B, C)
    # large pools do not fit 63 x 5 twice over: place NaN by hand, both labels, first and last
    # lane, first and last class
    for (r, c), lab in (((0, 0), 0), ((0, C - 1), 1), ((B - 1, 0), 1), ((B - 1, C - 1), 0), ((31, 2), 1)):
        ms[r, c] = float("nan")
        ml[r, c] = lab
    assert torch.isnan(ms[ml == 0].float()).any() and torch.isnan(ms[ml == 1].float()).any()
    nan_col = torch.isnan(ms.float()).float().argmax(1)
    mc = torch.where(torch.isnan(ms.float()).any(1), nan_col, torch.arange(B) % C)  # label 1 on a NaN
    assert torch.equal(ops.multiclass_curve_confmat(ms.cuda(), mc.cuda(), thr_d).cpu(),
                       oracle.multiclass_confmat(ms, mc, thr))
    assert torch.equal(ops.multilabel_curve_confmat(ms.cuda(), ml.cuda(), thr_d).cpu(),
                       oracle.multilabel_confmat(ms, ml, thr))


@pytest.mark.parametrize("guess", [(1, 0.37, 3.0), (1, -5.0, 1e6), (1, 2.0, -40.0)],
                         ids=["coarse", "far-above", "negative-step"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_uniform_guess_may_be_arbitrarily_wrong(monkeypatch, dtype, guess):
    """_uniform_params promises that the +-1 fixup keeps results exact even if the
    guess is off; its cache is keyed by data pointer, so a stale entry for another
    grid is reachable. Force wrong parameters for the non-uniform grid."""
    thr = SPECS["list"]
    thr_d = thr.cuda()
    monkeypatch.setattr(_hip, "_uniform_params", lambda t: guess)
    pool = torch.cat([oracle.value_pool(thr, dtype), torch.full((2,), float("nan"), dtype=dtype)])
    scores, labels = oracle.binary_layout(pool, 2 * pool.numel() + 1)
    assert torch.equal(ops.binary_curve_confmat(scores.cuda(), labels.cuda(), thr_d).cpu(),
                       oracle.binary_confmat(scores, labels, thr))
    ms, ml = oracle.matrix_layout(pool, 63, 5)
    mc = _mc_target(ms, thr, 5)
    for variant in (0, 1):
        monkeypatch.setattr(_hip, "_CURVE_VARIANT", variant)
        assert torch.equal(ops.multiclass_curve_confmat(ms.cuda(), mc.cuda(), thr_d).cpu(),
                           oracle.multiclass_confmat(ms, mc, thr))
        assert torch.equal(ops.multilabel_curve_confmat(ms.cuda(), ml.cuda(), thr_d).cpu(),
                           oracle.multilabel_confmat(ms, ml, thr))


# =====================================================================
# b. metric level, in-kernel normalisation, exact cases
# =====================================================================
def _state(metric):
    metric._maybe_flush_lazy()
    torch.cuda.synchronize()
    return metric.confmat.cpu()


def _make_collection(C, thresholds, ignore_index):
    kw = dict(num_classes=C, validate_args=False, ignore_index=ignore_index)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=thresholds, **kw),
        "ap": ma.MulticlassAveragePrecision(average="macro", thresholds=thresholds, **kw),
    })


def _fused_curve_state(monkeypatch, onepass, C, thresholds, ignore_index, preds, target, updates=3):
    """The curve state of the fused collection after ``updates`` identical updates (the
    first runs every metric on its own, the fused plan serves the rest)."""
    with monkeypatch.context() as m:
        m.setenv(_hip.ONEPASS_ENV, "2" if onepass else "0")
        coll = _make_collection(C, thresholds, ignore_index).to("cuda")
        for _ in range(updates):
            coll.update(preds, target)
        for metric in coll.values(copy_state=False):
            metric._maybe_flush_lazy()
        torch.cuda.synchronize()
        assert coll._fused_plan is not None
        assert coll._fused_plan.onepass_steps == ((updates - 1) if onepass else 0)
        return coll.auroc.confmat.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("thresholds", [torch.linspace(0, 1, 5), torch.tensor([0.0, 0.5, 0.5, 1.0])],
                         ids=["lin5", "list"])
def test_sigmoid_exact_values(thresholds, dtype):
    """sigmoid(+-0) = 0.5 and sigmoid(30) = sigmoid(inf) = 1.0 hit thresholds exactly and
    must count as >=; sigmoid(-inf) = 0 meets threshold 0. The ordinary logits land far
    from every threshold, so the fp64 sigmoid decides them the same way."""
    inf = float("inf")
    logits = torch.tensor([0.0, -0.0, 30.0, -30.0, inf, -inf, 2.0, -1.5, 0.75, 0.0, 30.0, -inf], dtype=dtype)
    target = torch.tensor([1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0])
    probs = (1.0 / (1.0 + torch.exp(-logits.double()))).float()
    assert probs[0] == 0.5 and probs[1] == 0.5 and probs[2] == 1.0 and probs[4] == 1.0 and probs[5] == 0.0
    want = oracle.binary_confmat(probs, target, thresholds)
    m = ma.BinaryPrecisionRecallCurve(thresholds=thresholds).cuda()
    m.update(*_dev(logits, target))
    assert torch.equal(_state(m), want)
    # multilabel rides the same sigmoid in the (B, C) kernel
    ml_logits, ml_target = logits.reshape(4, 3), target.reshape(4, 3)
    mm = ma.MultilabelPrecisionRecallCurve(num_labels=3, thresholds=thresholds).cuda()
    mm.update(*_dev(ml_logits, ml_target))
    assert torch.equal(_state(mm), oracle.multilabel_confmat(probs.reshape(4, 3), ml_target, thresholds))


def _softmax_exact_batch(C, dtype):
    """Rows of all 2.0 (out of range: they decide "softmax") and rows of all 0.0 (in
    range) both give exactly float32(1)/C; one-hot rows are valid probabilities whose
    softmax lies far from every threshold. The decision is batch-global: the in-range
    rows must be normalised too."""
    B = 9
    x = torch.zeros(B, C)
    x[0] = 2.0
    x[4] = 2.0
    x[8] = 2.0
    for r, c in ((1, 0), (3, C - 1), (6, C // 2)):
        x[r, c] = 1.0  # a valid probability row
    target = torch.tensor([0, 0, C - 1, C - 1, 1 % C, 2 % C, C // 2, 0, C - 1])
    inv = torch.tensor(1.0) / C
    thr = torch.stack([torch.nextafter(inv, torch.tensor(0.0)), inv, torch.nextafter(inv, torch.tensor(1.0)),
                       torch.tensor(0.5), torch.tensor(0.9)]).sort().values
    probs = torch.softmax(x.double(), -1).float()
    assert bool((probs[0] == inv).all()) and bool((probs[2] == inv).all())  # exact hits of thr
    return x.to(dtype), target, thr, probs


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("C", [3, 4, 19, 136])
def test_softmax_exact_values(monkeypatch, C, dtype):
    x, target, thr, probs = _softmax_exact_batch(C, dtype)
    want = oracle.multiclass_confmat(probs, target, thr)
    # exactly-1/C counts as >= at thr == 1/C and as < at its upper neighbour
    i = int((thr == torch.tensor(1.0) / C).nonzero()[0])
    assert int(want[i, :, :, 1].sum()) - int(want[i + 1, :, :, 1].sum()) >= 5 * C
    m = ma.MulticlassPrecisionRecallCurve(num_classes=C, thresholds=thr).cuda()
    m.update(*_dev(x, target))
    assert torch.equal(_state(m), want)
    if C == 136:
        for onepass in (True, False):
            got = _fused_curve_state(monkeypatch, onepass, C, thr, None, *_dev(x, target))
            assert torch.equal(got, 3 * want), onepass


@pytest.mark.parametrize("onepass", [True, False], ids=["onepass", "two-kernel"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_fused_collection_pools_all_rows_deferred(monkeypatch, dtype, onepass):
    """The pools of section a. through the fused collection at C=136: every score is in
    [0, 1], so nothing is normalised and the one-pass kernel defers every row to its
    tail kernel. B = 1, 5, 257."""
    C = 136
    for spec, thr in SPECS.items():
        pool = oracle.value_pool(thr, dtype)
        for B in (1, 5, 257):
            scores, _ = oracle.matrix_layout(pool, B, C)
            target = _mc_target(scores, thr, C)
            want = oracle.multiclass_confmat(scores, target, thr)
            got = _fused_curve_state(monkeypatch, onepass, C, thr, None, *_dev(scores, target))
            assert torch.equal(got, 3 * want), (spec, B)


# =====================================================================
# c. ignore / normalise ordering
# =====================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("where", ["ignored", "kept"])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_ignore_normalise_order_on_gpu(kind, where, dtype):
    """The cases of the CPU tape test through the GPU metrics. Expected: the oracle after
    the reference's decision (which elements its range test sees is proved on the tape)."""
    p, t, thr = cases.case(kind, where)
    p = p.to(dtype)
    scores = cases.normalised(kind, p, t)
    if kind == "binary_stat":
        m = ma.BinaryStatScores(threshold=cases.STAT_THRESHOLD, ignore_index=cases.IGNORE).cuda()
        m.update(*_dev(p, t))
        assert torch.equal(m.compute().cpu().long(), cases.stat_oracle(scores, t, multilabel=False))
        return
    if kind == "multilabel_stat":
        m = ma.MultilabelStatScores(num_labels=p.shape[1], threshold=cases.STAT_THRESHOLD, average=None,
                                    ignore_index=cases.IGNORE).cuda()
        m.update(*_dev(p, t))
        assert torch.equal(m.compute().cpu().long(), cases.stat_oracle(scores, t, multilabel=True))
        return
    fn = {"binary_curve": oracle.binary_confmat, "multiclass_curve": oracle.multiclass_confmat,
          "multilabel_curve": oracle.multilabel_confmat}[kind]
    want = fn(scores, t, thr, ignore_index=cases.IGNORE)
    m = cases.make_curve_metric(kind, p, thr).cuda()
    for _ in range(2):  # twice: the device epoch protocol must close the first update
        m.update(*_dev(p, t))
    assert torch.equal(_state(m), 2 * want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("where", ["ignored", "kept"])
def test_ignore_normalise_order_functional_curves(where, dtype):
    """The functional curve API leaves the mask to the kernel on the GPU and normalises in
    torch: that range test must leave ignored samples out as well."""
    for kind, fn in (("binary_curve", oracle.binary_confmat), ("multiclass_curve", oracle.multiclass_confmat)):
        p, t, thr = cases.case(kind, where)
        p = p.to(dtype)
        want = fn(cases.normalised(kind, p, t), t, thr, ignore_index=cases.IGNORE)
        tps, fps, fns = want[..., 1, 1].double(), want[..., 0, 1].double(), want[..., 1, 0].double()
        if kind == "binary_curve":
            prec, rec, _ = ma.functional.classification.binary_precision_recall_curve(
                p.cuda().float(), t.cuda(), thresholds=thr.cuda(), ignore_index=cases.IGNORE)
            got_p, got_r = prec[:-1].cpu().double(), rec[:-1].cpu().double()
        else:
            prec, rec, _ = ma.functional.classification.multiclass_precision_recall_curve(
                p.cuda().float(), t.cuda(), num_classes=p.shape[1], thresholds=thr.cuda(), ignore_index=cases.IGNORE)
            got_p, got_r = prec[:, :-1].T.cpu().double(), rec[:, :-1].T.cpu().double()
        # a 0/0 follows the project's safe-divide convention; compare where the ratio exists
        has_pos = (tps + fns) > 0
        assert bool(has_pos.any())
        assert torch.allclose(got_r[has_pos], (tps / (tps + fns))[has_pos], atol=1e-6, rtol=0), kind
        has_pred = (tps + fps) > 0
        assert torch.allclose(got_p[has_pred], (tps / (tps + fps))[has_pred], atol=1e-6, rtol=0), kind


@pytest.mark.parametrize("onepass", [True, False], ids=["onepass", "two-kernel"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("where", ["ignored", "kept"])
def test_ignore_normalise_order_fused_collection(monkeypatch, where, dtype, onepass):
    C = 136
    p, t, thr = cases.multiclass_case(C, where, rows=8)
    assert int(((p < 0) | (p > 1)).sum()) == 1
    p = p.to(dtype)
    assert cases.reference_normalises("multiclass_curve", p, t) is (where == "kept")
    want = oracle.multiclass_confmat(cases.normalised("multiclass_curve", p, t), t, thr, ignore_index=cases.IGNORE)
    got = _fused_curve_state(monkeypatch, onepass, C, thr, cases.IGNORE, *_dev(p, t))
    assert torch.equal(got, 3 * want)


# =====================================================================
# d. random logits: interval check against the fp64 oracle
# =====================================================================
_MACHINE_EPS = 8 * 2.0 ** -24


def _rowinv_error(metric, logits):
    """Largest relative difference between the kernel's rowinv and fp64 1/sum(exp(x - max))."""
    buf = metric.__dict__["_hip_rowstats_buf"][:, : logits.shape[0]].cpu().double()
    x = logits.float().cpu().double()
    mx = x.max(1).values
    assert torch.equal(buf[0], mx)  # the online max is exact
    ref = 1.0 / torch.exp(x - mx[:, None]).sum(1)
    return float(((buf[1].abs() - ref).abs() / ref).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", [(257, 136, 200, 3.0), (257, 19, 100, 4.0)], ids=["C136-T200", "C19-T100"])
def test_random_logits_softmax_within_interval(shape, dtype):
    """Every GPU count lies in [certain, certain + ambiguous] of the fp64 oracle, where
    a score is ambiguous within a relative band eps around a threshold.

    eps = 4 * (largest relative error of the kernel's rowinv against fp64 1/sum(exp),
    measured here on these inputs) + 8 * 2^-24. The second term covers the rest of
    p = expf(x - rowmax) * rowinv: near the lowest positive threshold (1/199) the
    difference x - rowmax is above -8, so its rounding (half an ulp of a value below 8,
    2^-22) moves exp by about 2 * 2^-24 relative; expf is good to about 2 ulp
    (4 * 2^-24) and the product rounds once (2^-25).

    Measured on an MI355X, rowinv relative error: 1.92e-7 (C=136 fp32), 1.82e-7 (C=136
    bf16), 1.66e-7 (C=19 fp32), 1.67e-7 (C=19 bf16), so eps is 1.14e-6 .. 1.25e-6 and the
    ambiguous share came out at most 0.0002 % of the counted elements. The test fails,
    instead of widening the band, if eps exceeds 1e-5 or if more than 0.5 % of the
    counted elements are ambiguous (fp64 alone at eps = 1e-5 gave at most 0.3 %).
    """
    B, C, T, scale = shape
    g = torch.Generator().manual_seed(B + C + T)
    logits = (torch.randn(B, C, generator=g) * scale).to(dtype)
    target = torch.randint(0, C, (B,), generator=g)
    thr = torch.linspace(0, 1, T)
    m = ma.MulticlassPrecisionRecallCurve(num_classes=C, thresholds=thr).cuda()
    m.update(*_dev(logits, target))
    got = _state(m)
    measured = _rowinv_error(m, logits)
    eps = 4 * measured + _MACHINE_EPS
    print(f"rowinv relative error {measured:.3e}, eps {eps:.3e} ({shape}, {dtype})")
    assert eps <= 1e-5, (measured, eps)
    probs = torch.softmax(logits.float().double(), -1)
    certain, amb = oracle.multiclass_confmat_interval(probs, target, thr, eps)
    share = float(amb[:, :, :, 0].sum()) / (B * C * T)
    print(f"ambiguous share {share:.5%}")
    assert share <= 0.005, share
    oracle.assert_within(got, certain, amb)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_random_logits_sigmoid_within_interval(dtype):
    """(300, 12, 50) logits scaled by 3.5 through the multilabel curve. No row statistics
    are involved: eps = 8 * 2^-24 for expf, the add and the divide of 1/(1+expf(-x))."""
    B, C, T = 300, 12, 50
    g = torch.Generator().manual_seed(B + C + T)
    logits = (torch.randn(B, C, generator=g) * 3.5).to(dtype)
    target = torch.randint(0, 2, (B, C), generator=g)
    thr = torch.linspace(0, 1, T)
    m = ma.MultilabelPrecisionRecallCurve(num_labels=C, thresholds=thr).cuda()
    m.update(*_dev(logits, target))
    got = _state(m)
    probs = torch.sigmoid(logits.float().double())
    certain, amb = oracle.multilabel_confmat_interval(probs, target, thr, _MACHINE_EPS)
    share = float(amb[:, :, :, 0].sum()) / (B * C * T)
    print(f"ambiguous share {share:.5%}")
    assert share <= 0.005, share
    oracle.assert_within(got, certain, amb)


# =====================================================================
# e. large threshold counts
# =====================================================================
@pytest.mark.parametrize("T", [8192, 10240, 20000])
def test_large_threshold_counts_neither_raise_nor_differ(T):
    """8192 thresholds need 96 KiB (binary histogram) and 128 KiB (suffix) of dynamic LDS,
    more than any other test launches; 10240 is the first count whose suffix block no
    longer fits 160 KiB once its static words are counted, 20000 fits no kernel. Whatever
    path serves them, update and compute must not raise and the state must be exact."""
    thr = torch.linspace(0, 1, T)
    pool = oracle.value_pool(thr, torch.float32)
    N = 64
    pick = pool[torch.linspace(0, pool.numel() - 1, N).long()]
    target = (torch.arange(N) % 2).long()
    m = ma.BinaryPrecisionRecallCurve(thresholds=thr).cuda()
    m.update(*_dev(pick, target))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.compute()
    assert torch.equal(_state(m), oracle.binary_confmat(pick, target, thr))

    scores = pool[torch.linspace(0, pool.numel() - 1, N * 3).long()].reshape(N, 3)
    mc_t = (torch.arange(N) % 3).long()
    mc = ma.MulticlassPrecisionRecallCurve(num_classes=3, thresholds=thr).cuda()
    mc.update(*_dev(scores, mc_t))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mc.compute()
    assert torch.equal(_state(mc), oracle.multiclass_confmat(scores, mc_t, thr))
    assert _hip.curve_kernels_cover(T) is (T <= 10238)
