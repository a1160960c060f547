"""The curve oracle (tests/unittests/_curve_oracle.py) against the CPU ops, and
the ignore/normalise ordering of the reference, from its own record.

Runs without a GPU. The GPU edge tests (tests/unittests/gpu/test_curve_edges.py)
trust two things this file proves:

* the oracle agrees with ``ops.*_curve_confmat`` on CPU on the adversarial
  value pools (scores exactly on, just below and just above every threshold);
* ``_curve_cases.reference_normalises`` — which metric family tests which
  elements for "outside [0, 1]" — reproduces the reference's recorded answers
  (golden tape, see tests/unittests/_golden.py), for the out-of-range value on
  an ignored sample and, mirrored, on a kept one.
"""
from __future__ import annotations

import pytest
import torch

import metrics_amd as ma
from metrics_amd import ops
from tests.unittests import _curve_cases as cases
from tests.unittests import _curve_oracle as oracle
from tests.unittests._golden import ref_module

_SPECS = oracle.threshold_specs()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("spec", list(_SPECS))
def test_pool_holds_exact_hits_and_both_labels(spec, dtype):
    thr = _SPECS[spec]
    pool = oracle.value_pool(thr, dtype)
    assert float(pool.float().min()) >= 0.0 and float(pool.float().max()) <= 1.0
    assert not torch.isnan(pool.float()).any()
    pf = pool.float()
    if dtype == torch.float32:
        for v in thr.tolist():  # every threshold itself and both float32 neighbours inside [0, 1]
            assert (pf == v).any()
        assert (pf == torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))).any()
        assert (pf == 2.0 ** -149).any() and (pf == 2.0 ** -126).any()
    elif spec == "lin5":
        for v in (0.25, 0.5, 0.75):  # exact in bf16: real threshold hits
            assert (pf == v).any()
    assert (pf == 0).any() and torch.signbit(pf[pf == 0]).any() and (~torch.signbit(pf[pf == 0])).any()
    scores, labels = oracle.binary_layout(pool, 2 * pool.numel() + 1)
    assert oracle.coverage(scores, labels, pool) == [True, True]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("spec", list(_SPECS))
def test_oracle_matches_cpu_ops_binary(spec, dtype):
    thr = _SPECS[spec]
    pool = oracle.value_pool(thr, dtype)
    scores, labels = oracle.binary_layout(pool, 2 * pool.numel() + 3)
    assert torch.equal(ops.binary_curve_confmat(scores.float(), labels, thr), oracle.binary_confmat(scores, labels, thr))
    tgt = labels.clone()
    tgt[::3] = -1
    got = ops.binary_curve_confmat(scores.float(), tgt, thr, ignore_index=-1)
    assert torch.equal(got, oracle.binary_confmat(scores, tgt, thr, ignore_index=-1))
    assert int(got.sum()) == thr.numel() * int((tgt != -1).sum())
    # the weighted (deduplicated) form the large-N GPU case uses is the same oracle
    big_s, big_t = scores.repeat(5), tgt.repeat(5)
    assert torch.equal(oracle.binary_confmat(big_s, big_t, thr, ignore_index=-1, dedupe=True),
                       oracle.binary_confmat(big_s, big_t, thr, ignore_index=-1, dedupe=False))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 3, 17])
@pytest.mark.parametrize("spec", ["lin2", "lin5", "lin65", "list"])
def test_oracle_matches_cpu_ops_matrix(spec, C, dtype):
    thr = _SPECS[spec]
    pool = oracle.value_pool(thr, dtype)
    B = 63
    scores, ml = oracle.matrix_layout(pool, B, C)
    g = torch.Generator().manual_seed(C)
    tgt = torch.randint(0, C, (B,), generator=g)
    assert torch.equal(ops.multiclass_curve_confmat(scores.float(), tgt, thr),
                       oracle.multiclass_confmat(scores, tgt, thr))
    tgt[::4] = -1
    assert torch.equal(ops.multiclass_curve_confmat(scores.float(), tgt, thr, ignore_index=-1),
                       oracle.multiclass_confmat(scores, tgt, thr, ignore_index=-1))
    assert torch.equal(ops.multilabel_curve_confmat(scores.float(), ml, thr),
                       oracle.multilabel_confmat(scores, ml, thr))
    ml[torch.rand(B, C, generator=g) < 0.25] = -1
    assert torch.equal(ops.multilabel_curve_confmat(scores.float(), ml, thr, ignore_index=-1),
                       oracle.multilabel_confmat(scores, ml, thr, ignore_index=-1))


def test_oracle_nan_is_negative_everywhere():
    thr = torch.linspace(0, 1, 5)
    s = torch.tensor([float("nan"), float("nan"), 0.5])
    t = torch.tensor([0, 1, 1])
    cm = oracle.binary_confmat(s, t, thr)
    assert cm[:, 0, 0].tolist() == [1] * 5 and cm[:, 0, 1].tolist() == [0] * 5  # NaN, label 0: tn
    assert cm[:, 1, 0].tolist() == [1, 1, 1, 2, 2] and cm[:, 1, 1].tolist() == [1, 1, 1, 0, 0]
    assert torch.equal(ops.binary_curve_confmat(s, t, thr), cm)


def test_interval_oracle_brackets_the_exact_one():
    g = torch.Generator().manual_seed(5)
    s = torch.rand(64, 7, generator=g)
    t = torch.randint(0, 7, (64,), generator=g)
    thr = torch.linspace(0, 1, 11)
    s[0, 0] = thr[3] * (1 + 5e-7)  # inside the band: ambiguous
    exact = oracle.multiclass_confmat(s, t, thr)
    certain, amb = oracle.multiclass_confmat_interval(s, t, thr, eps=1e-6)
    oracle.assert_within(exact, certain, amb)
    assert int(amb.sum()) > 0 and int(amb[3, 0].sum()) >= 2
    zero_c, zero_a = oracle.multiclass_confmat_interval(s, t, thr, eps=0.0)
    # eps = 0: only exact hits are ambiguous, and the exact oracle counts them positive
    oracle.assert_within(exact, zero_c, zero_a)
    with pytest.raises(AssertionError):
        oracle.assert_within(exact + 1, certain, amb)


# ----------------------------------------------------------- reference tape
def _reference_answer(kind, p, t, thr):
    tm = ref_module("torchmetrics")
    if kind == "binary_stat":
        return tm.functional.classification.binary_stat_scores(
            p, t, threshold=cases.STAT_THRESHOLD, ignore_index=cases.IGNORE)
    if kind == "multilabel_stat":
        return tm.functional.classification.multilabel_stat_scores(
            p, t, num_labels=p.shape[1], threshold=cases.STAT_THRESHOLD, average=None, ignore_index=cases.IGNORE)
    if kind == "binary_curve":
        m = tm.classification.BinaryPrecisionRecallCurve(thresholds=thr, ignore_index=cases.IGNORE)
    elif kind == "multiclass_curve":
        m = tm.classification.MulticlassPrecisionRecallCurve(
            num_classes=p.shape[1], thresholds=thr, ignore_index=cases.IGNORE)
    else:
        m = tm.classification.MultilabelPrecisionRecallCurve(
            num_labels=p.shape[1], thresholds=thr, ignore_index=cases.IGNORE)
    m.update(p, t)
    return m.confmat


def _ours_cpu(kind, p, t, thr):
    if kind == "binary_stat":
        return ma.functional.classification.binary_stat_scores(
            p, t, threshold=cases.STAT_THRESHOLD, ignore_index=cases.IGNORE)
    if kind == "multilabel_stat":
        return ma.functional.classification.multilabel_stat_scores(
            p, t, num_labels=p.shape[1], threshold=cases.STAT_THRESHOLD, average=None, ignore_index=cases.IGNORE)
    m = cases.make_curve_metric(kind, p, thr)
    m.update(p, t)
    return m.confmat


@pytest.mark.parametrize("where", ["ignored", "kept"])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_ignore_normalise_order_is_the_references(kind, where):
    p, t, thr = cases.case(kind, where)
    assert int(((p < 0) | (p > 1)).sum()) == 1  # exactly one deciding value
    want = _reference_answer(kind, p, t, thr)
    # the reading of the reference's order, proved against its record
    scores = cases.normalised(kind, p, t)
    if kind.endswith("_stat"):
        mine = cases.stat_oracle(scores, t, multilabel=kind.startswith("multilabel"))
    else:
        fn = {"binary_curve": oracle.binary_confmat, "multiclass_curve": oracle.multiclass_confmat,
              "multilabel_curve": oracle.multilabel_confmat}[kind]
        mine = fn(scores, t, thr, ignore_index=cases.IGNORE)
    assert torch.equal(mine, want.long()), (kind, where, mine, want)
    # and the decision matters: the other choice gives another answer
    flipped = p.float() if cases.reference_normalises(kind, p, t) else (
        p.softmax(-1) if kind == "multiclass_curve" else p.sigmoid())
    if kind.endswith("_stat"):
        other = cases.stat_oracle(flipped, t, multilabel=kind.startswith("multilabel"))
    else:
        other = fn(flipped, t, thr, ignore_index=cases.IGNORE)
    assert not torch.equal(other, want.long())
    # this project's CPU path gives the reference's answer too
    assert torch.equal(_ours_cpu(kind, p, t, thr).long(), want.long())


@pytest.mark.parametrize("kind,expect", [
    ("binary_stat", True), ("multilabel_stat", True),
    ("binary_curve", False), ("multiclass_curve", False), ("multilabel_curve", True),
])
def test_reading_of_the_order(kind, expect):
    """ignored flavour: stat scores and the multilabel curve normalise, the
    binary and multiclass curves do not; the kept flavour always normalises."""
    p, t, _ = cases.case(kind, "ignored")
    assert cases.reference_normalises(kind, p, t) is expect
    p, t, _ = cases.case(kind, "kept")
    assert cases.reference_normalises(kind, p, t) is True
