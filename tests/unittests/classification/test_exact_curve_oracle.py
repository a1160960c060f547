"""The oracles of the exact curves (``tests/unittests/_exact_curve_oracle.py``)
held against each other, against the CPU functionals and, through a golden
tape, against the reference on the planted cases. The GPU tests
(``tests/unittests/gpu/test_exact_curve_kernels.py``) use the same oracles and
case lists, so what is established here is what the kernels are measured with.

Thresholds are compared with float ``==``, never bitwise: the reference's
unstable argsort makes the sign of a reported zero arbitrary.
"""
import warnings

import numpy as np
import pytest
import torch

from metrics_amd.functional.classification import (  # the functionals the oracle is held against
    binary_roc,
    multiclass_precision_recall_curve,
    multilabel_roc,
)
from metrics_amd.functional.classification.precision_recall_curve import _binary_clf_curve
from tests.unittests import _exact_curve_cases as cases
from tests.unittests import _exact_curve_oracle as oracle
from tests.unittests._golden import ref_module

BINARY = cases.binary_cases()


_np = cases.as_f64


_same_curve = cases.same_curve


def _ratios_ok(got, want, what):
    u = oracle.ulps32(_np(got), want)
    both_nan = np.isnan(_np(got)) & np.isnan(want)
    assert _np(got).shape == want.shape and np.all(both_nan | (u <= cases.RATIO_ULPS)), (what, np.nanmax(u))


def _area_ok(got, want):
    return cases.area_error(got, want) <= cases.AREA_BOUND


@pytest.mark.parametrize("cid,family,n,kind", BINARY, ids=[c[0] for c in BINARY])
def test_the_two_oracles_are_identical_and_meet_the_cpu_path(cid, family, n, kind):
    s, t, pos_label, _ = cases.binary_case(family, n, kind)
    by_def = oracle.curve_by_definition(s.numpy(), t.numpy(), pos_label)
    by_sort = oracle.curve_by_sort(s.numpy(), t.numpy(), pos_label)
    for a, b in zip(by_def, by_sort):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert by_def[0].dtype == np.int64 and by_def[2].dtype == np.float64
    if family == "infs" and n > 2:
        # the CPU path, like the reference, finds group ends with a subtraction:
        # inf - inf is NaN, so REPEATED infinities are one threshold each there.
        # The definition (and the kernels) tie them. CHANGELOG.md has the note.
        fps, tps, thr = _binary_clf_curve(s, t, pos_label=pos_label)
        assert len(thr) > len(by_def[2]) and set(thr.tolist()) == set(by_def[2].tolist())
        return
    assert _same_curve(_binary_clf_curve(s, t, pos_label=pos_label), by_def)


@pytest.mark.parametrize("kind", cases.WEIGHT_KINDS)
@pytest.mark.parametrize("n", [1, 257, 1025])
def test_weighted_oracles_agree(n, kind):
    s, t, pos_label, _ = cases.binary_case("quant50", n, "random")
    w = cases.weights(kind, n, seed=n)
    by_def = oracle.curve_by_definition(s.numpy(), t.numpy(), pos_label, w.numpy())
    by_sort = oracle.curve_by_sort(s.numpy(), t.numpy(), pos_label, w.numpy())
    assert np.array_equal(by_def[2], by_sort[2])
    for a, b in zip(by_def[:2], by_sort[:2]):  # two fp64 summation orders of fp32 weights
        assert np.allclose(a, b, rtol=n * 2.0 ** -52, atol=0)
    # the CPU path sums in fp32 (cumsum): n/2 ulps of the total at the most
    fps, tps, thr = _binary_clf_curve(s, t, sample_weights=w, pos_label=pos_label)
    assert cases.same_floats(_np(thr), by_def[2])
    for got, want in ((fps, by_def[0]), (tps, by_def[1])):
        assert np.abs(_np(got) - want).max() <= n * 2.0 ** -24 * max(want.max(), 1e-30)


@pytest.mark.parametrize("cid,s,t,fps,tps,thr", cases.NAN_CASES, ids=[c[0] for c in cases.NAN_CASES])
def test_nan_cases_are_what_the_cpu_path_gives(cid, s, t, fps, tps, thr):
    s = torch.tensor(s, dtype=torch.float32)
    if cid in ("negative_nan", "both_signs"):
        assert (s.view(torch.int32) < 0).any()  # the sign bit survived the list
    with pytest.raises(ValueError):
        oracle.curve_by_definition(s.numpy(), t)
    assert _same_curve(_binary_clf_curve(s, torch.tensor(t)), (fps, tps, thr))
    finite = ~torch.isnan(s)
    if finite.any():  # the finite part is the oracle's, shifted by the NaN rows in front
        k = int((~finite).sum())
        tt = torch.tensor(t)
        f0, t0, th0 = oracle.curve_by_definition(s[finite].numpy(), tt[finite].numpy())
        pos_nan = int(tt[~finite].sum())
        assert _same_curve((f0 + k - pos_nan, t0 + pos_nan, th0), (fps[k:], tps[k:], thr[k:]))


# -------------------------------------------------------------- public, CPU
import metrics_amd.functional.classification as F  # noqa: E402


def _column_curves(p, target, multilabel):
    return cases.column_curves(p, target, multilabel)


def _cpu(task, stem, args, kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(F, f"{task}_{stem}")(*args, **kw)


@pytest.mark.parametrize("name", cases.PUBLIC_CASES)
def test_cpu_functionals_meet_the_oracle(name):
    seen = set()
    for task, stem, args, kw, kind, want in cases.public_checks(name):
        if kind == "curve":
            cases.check_curves(_cpu(task, stem, args, kw), want, (name, task, stem))
            seen.add(f"{task}_{stem}")
    assert {"binary_roc", "multiclass_precision_recall_curve", "multilabel_roc"} <= seen
    assert {binary_roc, multiclass_precision_recall_curve, multilabel_roc} == {
        F.binary_roc, F.multiclass_precision_recall_curve, F.multilabel_roc}


def test_cpu_area_error_is_the_recorded_one():
    """The fp32 trapezoid / sum of the CPU path against the fp64 oracle, over
    every area the GPU tests bound (binary_auroc with and without max_fpr,
    multiclass_average_precision and the rest of ``cases.public_checks``): the
    GPU tests allow twice this (docs/PARITY.md "Exact curves")."""
    errs = {}
    for name in cases.PUBLIC_CASES:
        for task, stem, args, kw, kind, want in cases.public_checks(name):
            if kind == "area":
                errs[(name, task, stem, kw.get("average"), kw.get("max_fpr"))] = cases.area_error(
                    _cpu(task, stem, args, kw), want)
    assert ("planted_6x5", "multiclass", "average_precision", "none", None) in errs
    assert ("families_300x5", "binary", "auroc", None, 0.5) in errs
    worst = max(errs, key=errs.get)
    print(f"largest CPU-path area error: {errs[worst]:.3e} at {worst}")
    assert cases.CPU_AREA_ERROR / 2 < errs[worst] <= cases.CPU_AREA_ERROR


def test_cpu_path_keeps_fp64_scores_one_ulp_apart():
    s, t = cases.ulp_apart_fp64()
    want = oracle.curve_by_definition(s.numpy(), t.numpy())
    assert len(want[2]) == 5 and len(np.unique(s.numpy().astype(np.float32))) == 3
    got = _binary_clf_curve(s, t)
    assert got[2].dtype == torch.float64 and _same_curve(got, want)


# ---------------------------------------------------- the reference's record
def _planted():
    p, mc, ml = cases.public_case("planted_6x5")
    return p, mc, ml


def test_reference_binary_clf_curve_on_planted_columns():
    """Signed zeros, a column without positives, a column without negatives:
    the reference's ``_binary_clf_curve`` gives the oracle's counts."""
    ref = ref_module("torchmetrics.functional.classification.precision_recall_curve")
    p, _, ml = _planted()
    for c in range(5):
        want = oracle.curve_by_definition(p[:, c].numpy(), ml[:, c].numpy())
        assert _same_curve(ref._binary_clf_curve(p[:, c], ml[:, c]), want), c
    assert len(oracle.curve_by_definition(p[:, 0].numpy(), ml[:, 0].numpy())[2]) == 3  # 1.0, 0.5 and ONE zero


def test_reference_fp64_scores_one_ulp_apart():
    ref = ref_module("torchmetrics.functional.classification.precision_recall_curve")
    s, t = cases.ulp_apart_fp64()
    assert _same_curve(ref._binary_clf_curve(s, t), oracle.curve_by_definition(s.numpy(), t.numpy()))


def test_reference_public_curves_on_the_planted_case():
    tm = ref_module("torchmetrics")
    p, mc, ml = _planted()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fprs, tprs, thrs = tm.functional.classification.multilabel_roc(p, ml, num_labels=5, thresholds=None)
        for c, cur in enumerate(_column_curves(p, ml, True)):
            wf, wt, wth = oracle.roc(*cur)
            _ratios_ok(fprs[c], wf, ("ref ml fpr", c))
            _ratios_ok(tprs[c], wt, ("ref ml tpr", c))
            assert cases.same_floats(_np(thrs[c]), wth)
        prec, rec, thrs = tm.functional.classification.multiclass_precision_recall_curve(
            p, mc, num_classes=5, thresholds=None)
        for c, cur in enumerate(_column_curves(p, mc, False)):
            wp, wr, wth = oracle.precision_recall(*cur)
            _ratios_ok(prec[c], wp, ("ref mc precision", c))
            _ratios_ok(rec[c], wr, ("ref mc recall", c))
            assert cases.same_floats(_np(thrs[c]), wth)
        auroc = tm.functional.classification.multilabel_auroc(p, ml, num_labels=5, average="none", thresholds=None)
        for c, cur in enumerate(_column_curves(p, ml, True)):
            if ml[:, c].min() != ml[:, c].max():
                assert _area_ok(auroc[c], oracle.auroc(*cur)), c
