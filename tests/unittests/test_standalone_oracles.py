"""The fp64 oracles of the stand-alone kernels (tests/unittests/_standalone_oracles.py)
against this project's CPU paths and against the reference's own record.

Runs without a GPU. The GPU edge tests (tests/unittests/gpu/test_ssim_edges.py,
test_standalone_edges.py) iterate the same case lists
(tests/unittests/_standalone_cases.py) and trust what this file proves:

* every oracle agrees with the CPU functional on every case, within the
  tolerance the GPU kernel is held to (docs/PARITY.md, "Stand-alone kernels");
  where the CPU path works in fp32 and the rule is an fp64 one, within the
  same rule at fp32 precision;
* every oracle agrees with the reference (golden tape, tests/unittests/_golden.py)
  on SSIM, MS-SSIM, calibration error, LogCosh, MAPE and, for the square
  structures the reference can run, erosion.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import metrics_amd as ma
from metrics_amd import ops
from metrics_amd.functional.classification.calibration_error import _binning_bucketize
from metrics_amd.functional.segmentation.utils import binary_erosion
from tests.unittests import _standalone_cases as cases
from tests.unittests import _standalone_oracles as oracle
from tests.unittests._golden import ref_module

F32 = 2.0 ** -24


# ---------------------------------------------------------------------- SSIM
def test_ssim_oracle_reflect_and_window_rules():
    assert oracle.reflect_index(6, 5).tolist() == [5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 4, 3, 2, 1, 0]
    wh, ww = oracle.ssim_window(True, (0.5, 2.0), 99)  # kernel_size ignored
    assert (len(wh), len(ww)) == (5, 15) and abs(wh.sum() - 1) < 1e-15 and abs(ww.sum() - 1) < 1e-15
    assert len(oracle.ssim_window(True, 3.7, 11)[0]) == 27 and len(oracle.ssim_window(True, 4.0, 11)[0]) == 29
    wh, ww = oracle.ssim_window(False, 1.5, (3, 9))
    assert wh.tolist() == [1 / 3] * 3 and ww.tolist() == [1 / 9] * 9
    # a transposed image under the transposed window gives the transposed map
    p, t, _ = cases.ssim_images("noisy_copy", (1, 1, 9, 14))
    _, _, a = oracle.ssim_oracle(p, t, sigma=(0.5, 1.0), data_range=1.0)
    _, _, b = oracle.ssim_oracle(p.transpose(2, 3), t.transpose(2, 3), sigma=(1.0, 0.5), data_range=1.0)
    assert np.abs(a - b.transpose(0, 1, 3, 2)).max() < 1e-13
    _, _, c = oracle.ssim_oracle(p, t, sigma=(1.0, 0.5), data_range=1.0)
    assert np.abs(a - c).max() > 1e-3  # and the orientation matters


@pytest.mark.parametrize("cid", list(cases.SSIM_CASES))
def test_ssim_cpu_path_meets_oracle(cid):
    """The CPU fp32 path defines the tolerance, so here it is held to its own
    measured size: at most 2e-4 on any family (docs/PARITY.md), far below the 1e-3
    a wrong reflect rule, axis or crop moves the mean by."""
    _, _, kw, want, cpu = cases.ssim_expected(cid)
    for w, c in zip(want, cpu):
        assert np.abs(oracle.as_f64(c) - w).max() <= 2e-4, (cid, c, w)
    family = cid.partition("family-")[2]
    if family in cases.SSIM_EXACT_ONE:
        assert torch.all(cpu[0] == 1.0) and np.abs(want[0] - 1).max() < 1e-12


def test_ssim_families_differ_by_more_than_a_tenth():
    _, _, _, want, _ = cases.ssim_expected("batch-3x2")
    s = np.sort(want[0])
    assert np.diff(s).min() > 0.1, s


@pytest.mark.parametrize("cid", ["family-noisy_copy", "family-ramp", "family-flat_bright", "family-int255",
                                 "family-zeros_ones", "win-sigma-0.5x2.0", "win-uniform-3x9", "shape-6x9",
                                 "shape-11x11-cs", "range-tuple", "lds-sigma-4.0-cs"])
def test_ssim_oracle_meets_reference(cid):
    tm = ref_module("torchmetrics")
    p, t, kw, want, cpu = cases.ssim_expected(cid)
    ref = cases.ssim_functional_outputs(tm.functional.image.structural_similarity_index_measure(p, t, **kw))
    for r, w, c in zip(ref, want, cpu):
        # the reference is the fp32 torch formulation the CPU path ports
        assert np.abs(oracle.as_f64(r).reshape(w.shape) - w).max() <= 2e-4, (cid, r, w)
        assert torch.allclose(r.reshape(-1), c, atol=1e-6, rtol=0), (cid, r, c)


@pytest.mark.parametrize("cid", list(cases.MS_SSIM_CASES))
def test_ms_ssim_oracle_meets_cpu_path_and_reference(cid):
    tm = ref_module("torchmetrics")
    p, t, kw, want, cpu = cases.ms_ssim_expected(cid)
    ref = tm.functional.image.multiscale_structural_similarity_index_measure(p, t, **kw)
    assert np.abs(oracle.as_f64(cpu) - want).max() <= 2e-4, (cpu, want)
    assert np.abs(oracle.as_f64(ref).reshape(-1) - want).max() <= 2e-4, (ref, want)


# ------------------------------------------------------------------- erosion
@pytest.mark.parametrize("shape", cases.EROSION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_erosion_oracle_equals_cpu_path(shape):
    for kind in cases.EROSION_IMAGES:
        img = cases.erosion_image(kind, shape)
        for name, strel, origin in cases.EROSION_STRUCTURES:
            st = torch.tensor(strel, dtype=torch.int32)
            for border in (0, 1):
                want = oracle.erosion_oracle(img, st, origin, border)
                got = binary_erosion(img, st, origin, border)
                assert got.dtype == torch.uint8
                assert np.array_equal(got.numpy(), want), (kind, name, border)
    # the all-zero structure on an all-one neighbourhood is the documented 2
    ones = cases.erosion_image("ones", shape)
    assert oracle.erosion_oracle(ones, torch.zeros(3, 3), (1, 1), 1).max() == 2


def test_erosion_oracle_meets_reference_on_square_structures():
    ref_erosion = ref_module("torchmetrics.functional.segmentation.utils").binary_erosion
    compared = 0
    for shape in ((2, 1, 5, 4), (1, 1, 3, 3)):  # one channel: the reference crashes on more
        img = cases.erosion_image("random", shape)
        for name, strel, origin in cases.EROSION_STRUCTURES:
            st = torch.tensor(strel, dtype=torch.int32)
            if st.shape[0] != st.shape[1]:
                continue  # the reference crashes on non-square structures
            for border in (0, 1):
                ref = ref_erosion(img, st, origin, border)
                assert np.array_equal(ref.numpy(), oracle.erosion_oracle(img, st, origin, border)), (name, border)
                compared += 1
    assert compared == 2 * 9 * 2


# --------------------------------------------------------------- calibration
def _calib_cpu(conf, acc, bounds):
    """Per-bin (count, conf sum, acc sum) recovered from the CPU path's means and proportions."""
    acc_bin, conf_bin, prop = _binning_bucketize(conf, acc, bounds)
    count = (prop.double() * conf.numel()).round()
    return count.numpy().astype(np.int64), (conf_bin.double() * count).numpy(), (acc_bin.double() * count).numpy()


@pytest.mark.parametrize("kind,n_bins", [("uniform", b) for b in cases.CALIB_N_BINS + (cases.CALIB_FALLBACK_BINS,)]
                         + [("sqrt", 15), ("sqrt", 99), ("bf16", 99)])
def test_calib_oracle_meets_cpu_path(kind, n_bins):
    bounds = cases.calib_bounds(kind, n_bins)
    if kind == "bf16":
        # rounded boundaries: unevenly spaced (and, should a linspace ever repeat one, an empty bin)
        assert not torch.equal(bounds, cases.calib_bounds("uniform", n_bins))
    conf, acc = cases.calib_inputs(bounds, 3 * (n_bins + 1) + 2 + 257)
    assert conf.min() < 0 and conf.max() > 1 and (conf == 0).any() and (conf == 1).any()
    count, conf_sum, acc_sum = oracle.calib_oracle(conf, acc, bounds)
    assert count.sum() == conf.numel()
    c_count, c_conf, c_acc = _calib_cpu(conf, acc, bounds)
    assert np.array_equal(c_count, count)
    # the CPU path returns fp32 means of fp32 sums: n_j roundings of at most 2^-24 * sum each
    assert np.all(np.abs(c_conf - conf_sum) <= (count + 2) * F32 * np.abs(conf_sum) + 1e-30)
    assert np.all(np.abs(c_acc - acc_sum) <= (count + 2) * F32 * np.abs(acc_sum) + 1e-30)


def _ece_from_oracle(conf, acc, bounds, norm):
    count, conf_sum, acc_sum = oracle.calib_oracle(conf, acc, bounds)
    nz = count > 0
    gap = np.zeros(len(count))
    gap[nz] = np.abs(acc_sum[nz] / count[nz] - conf_sum[nz] / count[nz])
    prop = count / count.sum()
    if norm == "l1":
        return float((gap * prop).sum())
    if norm == "max":
        return float(gap.max())
    return float(np.sqrt((gap ** 2 * prop).sum()))


@pytest.mark.parametrize("norm", ["l1", "l2", "max"])
@pytest.mark.parametrize("n_bins", [1, 10, 15, 99])
def test_calib_oracle_meets_reference(n_bins, norm):
    tm = ref_module("torchmetrics")
    bounds = cases.calib_bounds("uniform", n_bins)
    conf, acc = cases.calib_inputs(bounds, 3 * (n_bins + 1) + 2 + 257)
    # probabilities below 1: outside [0, 1] the functional takes a sigmoid, and the reference
    # counts confidence 1.0 in a bin of its own past the last one, where this project (and
    # the oracle) clamp it into the last bin (docs/PARITY.md)
    keep = (conf >= 0) & (conf < 1)
    conf, acc = conf[keep], acc[keep]
    assert (conf == 0).any() and (conf == bounds[n_bins // 2]).any()
    ref = tm.functional.classification.binary_calibration_error(conf, acc.long(), n_bins=n_bins, norm=norm)
    ours = ma.functional.classification.binary_calibration_error(conf, acc.long(), n_bins=n_bins, norm=norm)
    want = _ece_from_oracle(conf, acc, bounds, norm)
    # fp32 sums of at most n terms in [0, 1]
    tol = conf.numel() * F32
    assert abs(float(ref) - want) <= tol and abs(float(ours) - want) <= tol, (ref, ours, want)


# ---------------------------------------------------------- error reductions
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [n for n in cases.ERR_SIZES])
@pytest.mark.parametrize("op", oracle.ERR_OPS)
def test_err_oracle_meets_cpu_ops(op, N, dtype):
    x, y = cases.err_inputs(op, N, dtype)
    want, sum_abs = oracle.err_oracle(x, y, op)
    got = ops.err_reduce_sum(x, y, op).numpy()
    assert np.all(np.isfinite(want))
    assert np.all(np.abs(got - want) <= cases.err_tol(N, sum_abs)), (op, N, got, want)


def test_logcosh_oracle_is_linear_far_out():
    want, _ = oracle.err_oracle(torch.tensor([0.0, 400.0]), torch.tensor([400.0, 0.0]), "logcosh")
    assert want[0] == 2 * (400.0 - oracle.LN2)
    assert float(ma.functional.log_cosh_error(torch.tensor([0.0]), torch.tensor([400.0]))) == pytest.approx(
        400.0 - oracle.LN2, rel=2 ** -23)


@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("name", list(cases.FUNCTIONAL_OPS))
def test_err_oracle_meets_cpu_functionals(name, N):
    """The CPU functionals work in fp32: the rule of the kernel at fp32 precision."""
    op = cases.FUNCTIONAL_OPS[name]
    x, y = cases.err_inputs(op, N)
    want, sum_abs = oracle.err_oracle(x, y, op)
    got = float(getattr(ma.functional, name)(x, y))
    tol = ((N + 16) * 2 * F32 * sum_abs[0] + 2 * F32 * abs(want[0])) / N
    assert abs(got - want[0] / N) <= tol, (name, N, got, want[0] / N, tol)


@pytest.mark.parametrize("name", ["log_cosh_error", "mean_absolute_percentage_error"])
def test_err_oracle_meets_reference(name):
    tm = ref_module("torchmetrics")
    op = cases.FUNCTIONAL_OPS[name]
    N = 257
    # the reference's log((e^d + e^-d) / 2) overflows fp32 past |d| = 88: no planted differences for it
    x, y = cases.err_inputs("abs_err" if op == "logcosh" else op, N)
    want, sum_abs = oracle.err_oracle(x, y, op)
    ref = float(getattr(tm.functional, name)(x, y))
    tol = ((N + 16) * 2 * F32 * sum_abs[0] + 2 * F32 * abs(want[0])) / N
    assert abs(ref - want[0] / N) <= tol, (name, ref, want[0] / N, tol)


# -------------------------------------------------------------------- box IoU
def test_box_grid_is_exact_in_fp32():
    b = cases.random_boxes(257, 3)
    assert torch.equal(b * 4, (b * 4).round()) and float(b.max()) < 512 and float(b.min()) >= 0
    assert (b[:, 2] == b[:, 0]).any() and (b[:, 3] == b[:, 1]).any() and (b[:, 2:] >= b[:, :2]).all()


@pytest.mark.parametrize("variant", oracle.IOU_VARIANTS)
def test_box_oracle_meets_cpu_path(variant):
    names, p1, p2 = cases.planted_boxes()
    for b1, b2 in ((p1, p2), (cases.random_boxes(65, 1), cases.random_boxes(257, 2))):
        cpu = ops.box_iou_pairwise(b1, b2, variant)
        want, tol = cases.box_tol(variant, b1, b2, cpu)
        assert np.all(np.isfinite(want))
        if variant in ("iou", "giou"):
            assert np.all(np.abs(cpu.double().numpy() - want) <= tol), variant
        else:  # the CPU fp32 path defines the tolerance: hold it to a fixed 1e-5
            assert np.abs(cpu.double().numpy() - want).max() <= 1e-5, variant
    if variant == "iou":
        cpu = ops.box_iou_pairwise(p1, p2, "iou")
        for i, n in enumerate(names):
            if n in cases.IOU_EXACT:
                assert float(cpu[i, i]) == cases.IOU_EXACT[n] == oracle.box_iou_oracle(p1, p2, "iou")[i, i], n
        i = names.index("zero-area-same-point")
        assert float(cpu[i, i]) == 0.0  # union 0
