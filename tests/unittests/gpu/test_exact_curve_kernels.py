"""The exact (``thresholds=None``) curve kernels of csrc/clf_curve.hip
(``ma_binary_clf_curve``, ``ma_mc_clf_curve``, ``ma_retrieval_sort``) against
the definition oracle of ``tests/unittests/_exact_curve_oracle.py``, on the
case lists of ``tests/unittests/_exact_curve_cases.py``. The oracle and the
cases are held against the CPU path and the reference's record by
``tests/unittests/classification/test_exact_curve_oracle.py``.

``fps``, ``tps`` and the number of thresholds must be EXACT, thresholds
float-equal (never bitwise: which of two tied zeros is reported is arbitrary).
Weighted sums lie within 1 fp32 ulp of the fp64 oracle, curve values within 2
fp32 ulps of the fp64 ratio, areas within twice the CPU path's own error; the
derivations stand next to the constants in the case file and in docs/PARITY.md
("Exact curves"). The retrieval permutations must equal the stable torch
lexsort exactly.
"""
import warnings

import numpy as np
import pytest
import torch

import metrics_amd as ma
import metrics_amd.functional.classification as F
from metrics_amd.functional.classification.precision_recall_curve import (
    _binary_clf_curve,
    _binary_precision_recall_curve_compute,
    _multiclass_precision_recall_curve_compute,
)
from metrics_amd.functional.classification.roc import _binary_roc_compute, _multilabel_roc_compute
from metrics_amd.ops import _hip
from metrics_amd.retrieval.base import _group_by_query
from tests.unittests import _exact_curve_cases as cases
from tests.unittests import _exact_curve_oracle as oracle

pytestmark = pytest.mark.gpu

BINARY = cases.binary_cases()
as_f64, same_curve, same_floats = cases.as_f64, cases.same_curve, cases.same_floats


def _binary(s, t, pos_label=1, w=None):
    res = _hip.binary_clf_curve(s.cuda(), t.cuda(), None if w is None else w.cuda(), pos_label)
    assert res is not None
    return res


# =================================================================== binary
@pytest.mark.parametrize("cid,family,n,kind", BINARY, ids=[c[0] for c in BINARY])
def test_binary_kernel_against_the_definition(cid, family, n, kind):
    s, t, pos_label, want = cases.binary_case(family, n, kind)
    got = _binary(s, t, pos_label)
    assert all(x.dtype == torch.float32 for x in got)
    assert len(got[2]) == len(want[2]) and same_curve(got, want)


@pytest.mark.parametrize("n,family", [(cases.BINARY_LARGE[0], "quant50"), (cases.BINARY_LARGE[0], "distinct"),
                                      (cases.BINARY_LARGE[1], "distinct")])
def test_binary_kernel_beyond_one_block_of_rocprim(n, family):
    """2^17 + 3: merge-sort levels and look-back scans over many blocks with an
    odd tail. 2^20 + 1: the first size rocPRIM sorts with Onesweep."""
    s, t, pos_label, want = cases.binary_case(family, n, "random")
    assert same_curve(_binary(s, t, pos_label), want)


@pytest.mark.parametrize("n,kind", [(n, k) for n in (1, 257, 4097, 2 ** 17 + 3) for k in cases.WEIGHT_KINDS]
                         + [(2 ** 20 + 1, "rand")])
def test_binary_kernel_weighted_within_one_ulp(n, kind):
    s, t, pos_label, _ = cases.binary_case("quant50", n, "random")
    w = cases.weights(kind, n, seed=n % 1000)
    want = oracle.curve(s.numpy(), t.numpy(), pos_label, w.numpy())
    got = _binary(s, t, pos_label, w)
    assert same_floats(as_f64(got[2]), want[2])
    worst = max(oracle.ulps32(as_f64(g), e).max() for g, e in zip(got[:2], want[:2]))
    print(f"weighted n={n} {kind}: largest error {worst:.3f} fp32 ulps")
    assert worst <= cases.WEIGHTED_ULPS


def test_binary_kernel_counts_above_2_pow_24():
    """n = 2^24 + 3, every target positive, 8 distinct scores whose cumulative
    counts end at 2^24 - 9, -7, -5, -3, -1, +1, +2, +3. The outputs stay fp32:
    each must be float32(exact count), rounded to nearest (even on a tie), so
    2^24 + 1 reads 2^24 and 2^24 + 3 reads 2^24 + 4. docs/PARITY.md gives what
    that costs precision, recall and AUROC at this n."""
    n = 2 ** 24 + 3
    sizes = [2 ** 24 - 9, 2, 2, 2, 2, 2, 1, 1]
    values = [0.875, 0.75, 0.625, 0.5, 0.375, 0.25, 0.125, 0.0]
    assert sum(sizes) == n
    s = torch.full((n,), values[0])
    at = 1_000_003  # the small groups lie scattered inside the large one
    for v, k in zip(values[1:], sizes[1:]):
        for _ in range(k):
            s[at] = v
            at += 1_000_003
    assert at < n and (s != values[0]).sum() == sum(sizes[1:])
    exact = np.cumsum(sizes)
    assert exact[5] == 2 ** 24 + 1 and exact[7] == 2 ** 24 + 3
    fps, tps, thr = _hip.binary_clf_curve(s.cuda(), torch.ones(n, dtype=torch.long, device="cuda"))
    assert same_floats(as_f64(thr), values)
    assert np.array_equal(tps.cpu().numpy(), exact.astype(np.float32))  # int64 -> float32 rounds to nearest
    assert tps[5].item() == 2.0 ** 24 and tps[7].item() == 2.0 ** 24 + 4
    assert not fps.any()


# ================================================================== batched
def _check_batched(res, probs, target, multilabel):
    B, C = probs.shape
    assert len(res) == C
    off, base = 0, res[0][0].untyped_storage().data_ptr()
    for c, (fps, tps, thr, n_pos, n_neg) in enumerate(res):
        tc = target[:, c] if multilabel else target
        want = oracle.curve(probs[:, c].numpy(), tc.numpy(), 1 if multilabel else c)
        assert len(thr) == len(want[2]) and same_curve((fps, tps, thr), want), c
        assert n_pos == int((tc == (1 if multilabel else c)).sum()) and n_pos + n_neg == B, c
        # the slices tile the output: class c starts where the counts before it end
        for x in (fps, tps, thr):
            assert x.storage_offset() == off and len(x) == len(want[2])
        assert fps.untyped_storage().data_ptr() == base
        off += len(want[2])


@pytest.mark.parametrize("multilabel", [False, True], ids=["multiclass", "multilabel"])
@pytest.mark.parametrize("shape", cases.BATCHED_SHAPES + (cases.BATCHED_LARGE,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_batched_kernel_against_the_definition(shape, multilabel):
    """Constant columns, a column equal to its neighbour, a class without
    positives, a label every row has, multiclass rows with target -1, both
    zeros in one column; C of 255 / 256 / 257 is the second block of
    ``k_mc_counts``."""
    probs, mc, ml = cases.batched_case(*shape)
    target = ml if multilabel else mc
    res = _hip.mc_clf_curve(probs.cuda(), target.cuda(), multilabel=multilabel)
    _check_batched(res, probs, target, multilabel)


# ====================================================================== NaN
@pytest.mark.parametrize("cid,s,t,fps,tps,thr", cases.NAN_CASES, ids=[c[0] for c in cases.NAN_CASES])
def test_nan_scores_in_both_kernels_and_the_public_metrics(cid, s, t, fps, tps, thr):
    s, t = torch.tensor(s, dtype=torch.float32), torch.tensor(t)
    want = (fps, tps, thr)
    assert same_curve(_binary(s, t), want)
    # batched: the case as column 0, a finite column beside it
    other = torch.linspace(0, 1, len(s))
    probs = torch.stack([s, other], dim=1).contiguous()
    ml = torch.stack([t, 1 - t], dim=1).contiguous()
    want_other = oracle.curve(other.numpy(), (1 - t).numpy())
    for target, multilabel in ((ml, True), (1 - t, False)):  # multiclass: class 0 where t == 1
        res = _hip.mc_clf_curve(probs.cuda(), target.cuda(), multilabel=multilabel)
        assert same_curve(res[0][:3], want), multilabel
        assert same_curve(res[1][:3], want_other), multilabel
    # public metrics, from their states on: the CPU path's outcome. (Through the
    # front door the two devices part ways before any curve: the range test of
    # normalize_logits_if_needed counts a NaN as outside [0, 1] on CPU only, as
    # the reference's does. CHANGELOG.md lists it.)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fn, state, args in ((_binary_roc_compute, (s, t), (None,)),
                                (_binary_precision_recall_curve_compute, (s, t), (None,)),
                                (_multilabel_roc_compute, (probs, ml), (2, None)),
                                (_multiclass_precision_recall_curve_compute, (probs, 1 - t), (2, None))):
            cpu = fn(state, *args)
            gpu = fn(tuple(x.cuda() for x in state), *args)
            for a, b in zip(cpu, gpu):
                for x, y in zip(a, b) if isinstance(a, list) else ((a, b),):
                    assert same_floats(as_f64(y), as_f64(x)), (cid, fn.__name__)
        m = ma.BinaryROC(thresholds=None).to("cuda")
        m.preds, m.target = [s.cuda()], [t.cuda()]  # the state as update() would leave it, not normalised
        assert same_floats(as_f64(m.compute()[1]), as_f64(_binary_roc_compute((s, t), None)[1]))


# =========================================================== public surface
_columns, _close_curves = cases.column_curves, cases.check_curves


def _three_ways(fn, cls, args, kw):
    """The CPU functional, the GPU functional and the GPU modular metric over two updates."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield "cpu", fn(*args, **kw)
        gpu_args = tuple(a.cuda() for a in args)
        yield "gpu functional", fn(*gpu_args, **kw)
        m = cls(**kw).to("cuda")
        half = len(args[0]) // 2
        m.update(*(a[:half] for a in gpu_args))
        m.update(*(a[half:] for a in gpu_args))
        yield "gpu modular", m.compute()


@pytest.mark.parametrize("name", cases.PUBLIC_CASES)
def test_public_metrics_three_ways(name):
    """ROC, PR curve, AUROC (binary also with max_fpr = 0.5) and average
    precision (average none / macro / weighted) for binary, multiclass and
    multilabel: the oracle against the CPU path, the GPU functional and the GPU
    modular metric over two updates."""
    worst = 0.0
    for task, stem, args, kw, kind, want in cases.public_checks(name):
        cls = getattr(ma, task.capitalize() + cases.PUBLIC_CLASSES[stem])
        for how, got in _three_ways(getattr(F, f"{task}_{stem}"), cls, args, kw):
            what = (name, task, stem, kw.get("average"), kw.get("max_fpr"), how)
            if kind == "curve":
                _close_curves(got, want, what)
            else:
                err = cases.area_error(got, want)
                worst = max(worst, err) if how != "cpu" else worst
                assert err <= cases.AREA_BOUND, (what, err, got, want)
    print(f"{name}: largest GPU area error {worst:.3e} (bound {cases.AREA_BOUND:.1e})")


def test_public_planted_classes_without_positives_or_negatives():
    """Multilabel column 2 has no positive (warning, tpr zero), column 3 no
    negative (warning, fpr zero); column 0 ties both zeros across targets."""
    p, _, ml = cases.public_case("planted_6x5")
    with pytest.warns(UserWarning, match="No positive samples"):
        fpr, tpr, thr = F.multilabel_roc(p.cuda(), ml.cuda(), num_labels=5, thresholds=None)
    assert not tpr[2].any() and fpr[2][-1] == 1
    with pytest.warns(UserWarning, match="No negative samples"):
        fpr, tpr, thr = F.multilabel_roc(p.cuda(), ml.cuda(), num_labels=5, thresholds=None)
    assert not fpr[3].any() and tpr[3][-1] == 1
    assert same_floats(as_f64(thr[0]), [1.0, 1.0, 0.5, 0.0])  # ONE zero
    assert same_floats(as_f64(tpr[0]), [0, 0.25, 0.5, 1.0]) and same_floats(as_f64(fpr[0]), [0, 0, 0, 1.0])


def test_public_ignore_index():
    """Multilabel takes the per-label path (no batched kernel), multiclass and
    binary filter the rows first."""
    p, mc, ml = cases.public_case("families_300x5")
    mc, ml = mc.clone(), ml.clone()
    mc[::5] = -1
    ml[::3, 1] = -1
    ml[1::4, 0] = -1
    kw = {"thresholds": None, "ignore_index": -1}
    for how, got in _three_ways(F.binary_roc, ma.BinaryROC, (p[:, 0].contiguous(), ml[:, 0].contiguous()), kw):
        _close_curves([[g] for g in got], [oracle.roc(*_columns(p, ml, True, -1)[0])], ("binary ignore", how))
    for how, got in _three_ways(F.multiclass_roc, ma.MulticlassROC, (p, mc), {"num_classes": 5, **kw}):
        _close_curves(got, [oracle.roc(*c) for c in _columns(p, mc, False, -1)], ("multiclass ignore", how))
    for how, got in _three_ways(F.multilabel_roc, ma.MultilabelROC, (p, ml), {"num_labels": 5, **kw}):
        _close_curves(got, [oracle.roc(*c) for c in _columns(p, ml, True, -1)], ("multilabel ignore", how))
    for how, got in _three_ways(F.multilabel_precision_recall_curve, ma.MultilabelPrecisionRecallCurve, (p, ml),
                                {"num_labels": 5, **kw}):
        _close_curves(got, [oracle.precision_recall(*c) for c in _columns(p, ml, True, -1)],
                      ("multilabel PRC ignore", how))


def test_public_more_than_two_dimensions():
    p, mc, ml = cases.public_case("families_300x5")
    kw = {"thresholds": None}
    p3 = p.reshape(150, 2, 5).permute(0, 2, 1).contiguous()  # (N, C, d)
    for how, got in _three_ways(F.multiclass_roc, ma.MulticlassROC, (p3, mc.reshape(150, 2)),
                                {"num_classes": 5, **kw}):
        _close_curves(got, [oracle.roc(*c) for c in _columns(p, mc, False)], ("multiclass 3d", how))
    ml3 = ml.reshape(150, 2, 5).permute(0, 2, 1).contiguous()
    for how, got in _three_ways(F.multilabel_roc, ma.MultilabelROC, (p3, ml3), {"num_labels": 5, **kw}):
        _close_curves(got, [oracle.roc(*c) for c in _columns(p, ml, True)], ("multilabel 3d", how))
    s, t = p[:, 0].reshape(150, 2).contiguous(), ml[:, 0].reshape(150, 2).contiguous()
    for how, got in _three_ways(F.binary_precision_recall_curve, ma.BinaryPrecisionRecallCurve, (s, t), kw):
        _close_curves([[g] for g in got], [oracle.precision_recall(*_columns(p, ml, True)[0])], ("binary 2d", how))


def test_public_logits():
    """Scores outside [0, 1] are normalised first (sigmoid / softmax on the
    device); the curve is then the oracle's on those normalised scores."""
    p, mc, ml = cases.public_case("families_300x5")
    logits = (p * 8 - 4).contiguous()  # quantised columns stay tied
    kw = {"thresholds": None}
    sig = logits.cuda().sigmoid().cpu()
    soft = logits.cuda().softmax(1).cpu()
    got = F.binary_roc(logits[:, 0].cuda(), ml[:, 0].cuda(), **kw)
    _close_curves([[g] for g in got], [oracle.roc(*_columns(sig, ml, True)[0])], "binary logits")
    got = F.multilabel_precision_recall_curve(logits.cuda(), ml.cuda(), num_labels=5, **kw)
    _close_curves(got, [oracle.precision_recall(*c) for c in _columns(sig, ml, True)], "multilabel logits")
    got = F.multiclass_roc(logits.cuda(), mc.cuda(), num_classes=5, **kw)
    _close_curves(got, [oracle.roc(*c) for c in _columns(soft, mc, False)], "multiclass logits")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
def test_public_input_dtypes(dtype):
    """bf16 / fp16 widen exactly onto the kernels; fp64 is kept off them."""
    p, mc, ml = cases.public_case("families_300x5")
    q = p.to(dtype)
    kw = {"thresholds": None}
    before = _hip.exact_curve_calls()
    got = F.binary_roc(q[:, 0].cuda(), ml[:, 0].cuda(), **kw)
    _close_curves([[g] for g in got], [oracle.roc(*_columns(q, ml, True)[0])], ("binary", dtype))
    assert got[2].dtype == dtype
    got = F.multiclass_roc(q.cuda(), mc.cuda(), num_classes=5, **kw)
    _close_curves(got, [oracle.roc(*c) for c in _columns(q, mc, False)], ("multiclass", dtype))
    got = F.multilabel_precision_recall_curve(q.cuda(), ml.cuda(), num_labels=5, **kw)
    _close_curves(got, [oracle.precision_recall(*c) for c in _columns(q, ml, True)], ("multilabel", dtype))
    after = _hip.exact_curve_calls()
    if dtype == torch.float64:  # 1 binary + (1 batched + 5 columns) twice, none served
        assert after["kernel"] == before["kernel"] and after["kept_off"] == before["kept_off"] + 13
    else:
        assert after["kernel"] == before["kernel"] + 3 and after["kept_off"] == before["kept_off"]


def test_fp64_scores_one_ulp_apart_stay_apart():
    s, t = cases.ulp_apart_fp64()
    want = oracle.curve_by_definition(s.numpy(), t.numpy())
    assert len(want[2]) == 5
    before = _hip.exact_curve_calls()
    got = _binary_clf_curve(s.cuda(), t.cuda())
    assert got[2].dtype == torch.float64 and len(got[2]) == 5 and same_curve(got, want)
    fpr, tpr, thr = F.binary_roc(s.cuda(), t.cuda(), thresholds=None)
    assert len(thr) == 6 and same_floats(as_f64(thr)[1:], want[2])
    probs = torch.stack([s, 1 - s], dim=1)
    fprs, tprs, thrs = F.multilabel_roc(probs.cuda(), torch.stack([t, 1 - t], 1).cuda(), num_labels=2, thresholds=None)
    assert len(thrs[0]) == 6 and same_floats(as_f64(thrs[0])[1:], want[2])
    after = _hip.exact_curve_calls()
    assert after["kernel"] == before["kernel"] and after["kept_off"] > before["kept_off"]
    assert _hip.binary_clf_curve(s.cuda(), t.cuda()) is None
    assert _hip.mc_clf_curve(probs.cuda(), t.cuda()) is None


# ================================================================ retrieval
def _lexsort(idx, preds):
    o1 = torch.argsort(preds, descending=True, stable=True)
    o2 = torch.argsort(idx[o1], stable=True)
    return o1[o2], torch.argsort(idx, stable=True)


RETRIEVAL_SCORES = ("quant50", "zeros_denormals", "equal", "infs")


@pytest.mark.parametrize("queries", ["single", "own", "few", "up_to_2_pow_31"])
@pytest.mark.parametrize("n", [1, 2, 257, 2 ** 17 + 3])
def test_retrieval_sort_against_the_stable_lexsort(n, queries):
    g = torch.Generator().manual_seed(n)
    idx = {"single": torch.full((n,), 7), "own": torch.randperm(n, generator=g),
           "few": torch.randint(0, 5, (n,), generator=g),
           "up_to_2_pow_31": torch.randint(2 ** 31 - 40, 2 ** 31, (n,), generator=g)}[queries]
    if queries == "up_to_2_pow_31":
        idx[n // 2] = 2 ** 31 - 1
    for family in RETRIEVAL_SCORES:
        preds = cases.scores(family, n, seed=3)
        if family == "zeros_denormals" and n == 2:
            preds = torch.tensor([-0.0, 0.0])  # one query: the stable order keeps -0.0 in front
        got = _hip.retrieval_sort(idx.cuda(), preds.cuda())
        want = _lexsort(idx, preds)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), family


def test_retrieval_negative_indexes_are_kept_off_the_kernel():
    g = torch.Generator().manual_seed(5)
    n = 257
    idx = torch.randint(-3, 4, (n,), generator=g)
    preds, target = cases.scores("quant50", n, seed=9), torch.randint(0, 2, (n,), generator=g)
    before = _hip.exact_curve_calls()
    got = _group_by_query(idx.cuda(), preds.cuda(), target.cuda())
    assert _hip.exact_curve_calls() == before  # base.py never asked the kernel
    want = _group_by_query(idx, preds, target)
    for field in ("preds", "target", "preds_by_index", "target_by_index", "counts", "gid", "ranks"):
        assert torch.equal(getattr(got, field).cpu(), getattr(want, field)), field
    _group_by_query((idx + 3).cuda(), preds.cuda(), target.cuda())
    assert _hip.exact_curve_calls()["kernel"] == before["kernel"] + 1
    mg, mc_ = ma.retrieval.RetrievalMAP().to("cuda"), ma.retrieval.RetrievalMAP()
    mg.update(preds.cuda(), target.cuda(), indexes=idx.cuda())
    mc_.update(preds, target, indexes=idx)
    assert torch.allclose(mg.compute().cpu(), mc_.compute(), atol=1e-6)


# ============================================================= housekeeping
def test_call_counter_size_guard_and_repeats(monkeypatch):
    s, t, pos_label, want = cases.binary_case("quant50", 1025, "random")
    probs, mc, ml = cases.batched_case(257, 3)
    before = _hip.exact_curve_calls()
    _binary_clf_curve(s, t)  # CPU: neither counter moves
    assert _hip.exact_curve_calls() == before
    first = _binary(s, t, pos_label)
    again = _binary(s, t, pos_label)
    assert all(torch.equal(a, b) for a, b in zip(first, again))  # bit-identical repeats
    r1 = _hip.mc_clf_curve(probs.cuda(), mc.cuda())
    r2 = _hip.mc_clf_curve(probs.cuda(), mc.cuda())
    assert all(torch.equal(a, b) for x, y in zip(r1, r2) for a, b in zip(x[:3], y[:3]))
    idx = torch.randint(0, 9, (1025,), generator=torch.Generator().manual_seed(1)).cuda()
    o1, o2 = _hip.retrieval_sort(idx, s.cuda()), _hip.retrieval_sort(idx, s.cuda())
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1])
    mid = _hip.exact_curve_calls()
    assert mid == {"kernel": before["kernel"] + 6, "kept_off": before["kept_off"]}

    # the element limit, brought down: the same calls take the torch path
    assert _hip.EXACT_CURVE_MAX_ELEMENTS == 2 ** 31 - 1
    monkeypatch.setattr(_hip, "EXACT_CURVE_MAX_ELEMENTS", 1000)
    assert _hip.binary_clf_curve(s.cuda(), t.cuda()) is None
    assert _hip.retrieval_sort(idx, s.cuda()) is None
    assert _hip.mc_clf_curve(probs.repeat(2, 1).cuda(), mc.repeat(2).cuda()) is None  # 514 * 3 elements
    assert _hip.exact_curve_calls() == {"kernel": mid["kernel"], "kept_off": mid["kept_off"] + 3}
    assert same_curve(_binary_clf_curve(s.cuda(), t.cuda(), pos_label=pos_label), want)
    got = _group_by_query(idx, s.cuda(), t.cuda())
    want_g = _group_by_query(idx.cpu(), s, t)
    assert torch.equal(got.preds.cpu(), want_g.preds) and torch.equal(got.target.cpu(), want_g.target)
    # 514 x 3 is over the limit as a batch, each column of 514 is under it
    p2, t2 = probs.repeat(2, 1), ml.repeat(2, 1)
    at = _hip.exact_curve_calls()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, thr = F.multilabel_roc(p2.cuda(), t2.cuda(), num_labels=3, thresholds=None)
    assert _hip.exact_curve_calls() == {"kernel": at["kernel"] + 3, "kept_off": at["kept_off"] + 1}
    _close_curves((fpr, tpr, thr), [oracle.roc(*c) for c in _columns(p2, t2, True)], "size guard")
