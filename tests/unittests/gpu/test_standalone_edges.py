"""Erosion, calibration bins, error reductions and box IoU kernels at their
edges, against the fp64 oracles (tests/unittests/_standalone_oracles.py).

The case lists and tolerances are tests/unittests/_standalone_cases.py, the ones
tests/unittests/test_standalone_oracles.py runs on CPU. Erosion and the
calibration counts are held to exact equality.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_amd as ma
from metrics_amd import ops
from metrics_amd.functional.classification.calibration_error import _binning_bucketize
from metrics_amd.functional.segmentation.utils import binary_erosion
from metrics_amd.ops import _hip
from tests.unittests import _standalone_cases as cases
from tests.unittests import _standalone_oracles as oracle

F32 = 2.0 ** -24


@pytest.fixture(autouse=True)
def _require_hip():
    assert torch.cuda.is_available()
    assert ops.hip_available(), "HIP kernel library must be built and loadable on a GPU box"


def _counted(monkeypatch, name):
    calls = {"entered": 0, "ran": 0}
    real = getattr(_hip, name)

    def counted(*args, **kwargs):
        calls["entered"] += 1
        out = real(*args, **kwargs)
        calls["ran"] += 1
        return out

    monkeypatch.setattr(_hip, name, counted)
    return calls


# ------------------------------------------------------------------- erosion
@pytest.mark.parametrize("shape", cases.EROSION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_erosion_equals_oracle_and_cpu_path(shape, monkeypatch):
    calls = _counted(monkeypatch, "binary_erosion2d")
    n = 0
    for kind in cases.EROSION_IMAGES:
        img = cases.erosion_image(kind, shape)
        dev = img.cuda()
        for name, strel, origin in cases.EROSION_STRUCTURES:
            st = torch.tensor(strel, dtype=torch.int32)
            for border in (0, 1):
                got = binary_erosion(dev, st.cuda(), origin, border)
                n += 1
                assert got.dtype == torch.uint8 and got.shape == img.shape
                assert np.array_equal(got.cpu().numpy(), oracle.erosion_oracle(img, st, origin, border)), (
                    kind, name, border)
                assert torch.equal(got.cpu(), binary_erosion(img, st, origin, border)), (kind, name, border)
    assert calls == {"entered": n, "ran": n}


@pytest.mark.parametrize("dtype", cases.EROSION_DTYPES, ids=lambda d: str(d)[6:])
def test_erosion_input_dtypes(dtype):
    img = cases.erosion_image("random", (2, 3, 5, 4))
    st = torch.tensor([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=torch.int32)
    for border in (0, 1):
        got = binary_erosion(img.to(dtype).cuda(), st.cuda(), (1, 1), border)
        assert got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), oracle.erosion_oracle(img, st, (1, 1), border))
        assert torch.equal(got.cpu(), binary_erosion(img.to(dtype), st, (1, 1), border))
    # the default structure and origin
    assert np.array_equal(binary_erosion(img.to(dtype).cuda()).cpu().numpy(),
                          oracle.erosion_oracle(img, st, (1, 1), 0))


# --------------------------------------------------------------- calibration
def _check_calib_bins(conf, acc, bounds):
    count, conf_sum, acc_sum = oracle.calib_oracle(conf, acc, bounds)
    g_acc, g_conf, g_count = _hip.calib_bins(conf.cuda(), acc.cuda(), bounds.cuda())
    # a single mis-binned element fails this
    assert np.array_equal(g_count.cpu().numpy().astype(np.int64), count)
    for got, want in ((g_conf, conf_sum), (g_acc, acc_sum)):
        err = np.abs(oracle.as_f64(got) - want)
        assert np.all(err <= cases.calib_sum_tol(count, want)), (err.max(), want[err.argmax()])
    return count


@pytest.mark.parametrize("kind,n_bins", [("uniform", b) for b in cases.CALIB_N_BINS]
                         + [("sqrt", 15), ("sqrt", 99), ("bf16", 99)])
def test_calib_bins_planted_boundaries(kind, n_bins):
    bounds = cases.calib_bounds(kind, n_bins)
    _hip._UNIFORM_CACHE.clear()  # keyed by address: a freed tensor's entry must not answer for this one
    # evenly spaced bounds take the O(1) guess and its fix-up loops, the others the binary search
    assert _hip._uniform_params(bounds.cuda())[0] == (1 if kind == "uniform" else 0)
    dtype = torch.bfloat16 if kind == "bf16" else torch.float32
    conf, acc = cases.calib_inputs(bounds, 3 * (n_bins + 1) + 2 + 257, dtype=dtype)
    count = _check_calib_bins(conf, acc, bounds)
    assert count.sum() == conf.numel()


@pytest.mark.parametrize("n", cases.CALIB_SIZES)
def test_calib_bins_sizes(n):
    bounds = cases.calib_bounds("uniform", 15)
    conf, acc = cases.calib_inputs(bounds, n, seed=n % 7)
    assert conf.numel() == n
    _check_calib_bins(conf, acc, bounds)


@pytest.mark.parametrize("n_bins", [1, 15, 2048, cases.CALIB_FALLBACK_BINS])
def test_binning_bucketize_and_its_fallback(n_bins, monkeypatch):
    """Through the functional's binning. Above 2048 bins the kernel does not fit its
    LDS and the torch branch runs, as on CPU, instead of raising."""
    calls = _counted(monkeypatch, "calib_bins")
    bounds = cases.calib_bounds("uniform", n_bins)
    conf, acc = cases.calib_inputs(bounds, 3 * (n_bins + 1) + 2 + 257)
    n = conf.numel()
    count, conf_sum, acc_sum = oracle.calib_oracle(conf, acc, bounds)
    acc_bin, conf_bin, prop = _binning_bucketize(conf.cuda(), acc.cuda(), bounds.cuda())
    fits = n_bins <= 2048
    assert calls == {"entered": 1, "ran": 1 if fits else 0}
    want_prop = torch.from_numpy(count).float() / torch.tensor(float(n))
    assert torch.equal(prop.cpu(), want_prop)  # counts exact
    nz = count > 0
    for got, total in ((conf_bin, conf_sum), (acc_bin, acc_sum)):
        mean = np.where(nz, total / np.maximum(count, 1), 0.0)
        if fits:  # the kernel's sums, then one fp32 division
            tol = cases.calib_sum_tol(count, total) / np.maximum(count, 1) + 2 * F32 * np.abs(mean)
        else:     # fp32 sums of n_j terms, as on CPU
            tol = (count + 2) * F32 * np.abs(mean)
        assert np.all(np.abs(oracle.as_f64(got) - mean) <= tol)
    # and the metric built on it, against the CPU path
    p, t = conf.clamp(0, 1), acc.long()
    for norm in ("l1", "l2", "max"):
        g = ma.functional.classification.binary_calibration_error(p.cuda(), t.cuda(), n_bins=n_bins, norm=norm)
        c = ma.functional.classification.binary_calibration_error(p, t, n_bins=n_bins, norm=norm)
        assert abs(float(g) - float(c)) <= n * F32, (norm, g, c)


# ---------------------------------------------------------- error reductions
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", cases.ERR_SIZES)
@pytest.mark.parametrize("op", oracle.ERR_OPS)
def test_err_reduce_meets_oracle(op, N, dtype):
    x, y = cases.err_inputs(op, N, dtype)
    want, sum_abs = oracle.err_oracle(x, y, op)
    got = ops.err_reduce_sum(x.cuda(), y.cuda(), op)
    assert got.dtype == torch.float64 and got.shape == want.shape
    got = got.cpu().numpy()
    assert np.all(np.isfinite(got)), (op, N, got)
    assert np.all(np.abs(got - want) <= cases.err_tol(N, sum_abs)), (op, N, got, want)


def test_logcosh_far_negative_difference_is_linear():
    """d = -400: exp(-2d) overflows a double; |d| + log1p(exp(-2|d|)) - ln 2 does not."""
    x, y = torch.tensor([0.0, 0.0, -1e4]), torch.tensor([355.0, 400.0, 0.0])
    want, sum_abs = oracle.err_oracle(x, y, "logcosh")
    got = ops.err_reduce_sum(x.cuda(), y.cuda(), "logcosh").cpu().numpy()
    assert np.isfinite(got).all() and abs(got[0] - want[0]) <= cases.err_tol(3, sum_abs)[0], (got, want)
    assert float(ma.functional.log_cosh_error(x[1:2].cuda(), y[1:2].cuda())) == pytest.approx(
        400.0 - oracle.LN2, rel=2 ** -23)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("name", list(cases.FUNCTIONAL_OPS))
def test_regression_functionals_meet_oracle(name, N, dtype, monkeypatch):
    calls = _counted(monkeypatch, "err_reduce")
    op = cases.FUNCTIONAL_OPS[name]
    x, y = cases.err_inputs(op, N, dtype)
    want, sum_abs = oracle.err_oracle(x, y, op)
    got = getattr(ma.functional, name)(x.cuda(), y.cuda())
    assert calls == {"entered": 1, "ran": 1}
    tol = (cases.err_tol(N, sum_abs)[0] + 2 * F32 * abs(want[0])) / N  # the fp32 the functional returns
    assert abs(float(got) - want[0] / N) <= tol, (name, N, float(got), want[0] / N, tol)


@pytest.mark.parametrize("p_dtype,t_dtype", [(torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16),
                                             (torch.float32, torch.int64)], ids=["bf16-fp32", "fp32-bf16", "fp32-int64"])
def test_logcosh_mixed_dtypes_take_the_torch_path(p_dtype, t_dtype, monkeypatch):
    """The kernel reads both buffers as ``preds``' type: a pair of two dtypes must
    not reach it. The torch path works in the promoted dtype, fp32."""
    calls = _counted(monkeypatch, "err_reduce")
    N = 257
    x, y = cases.err_inputs("logcosh", N)
    x = x.to(p_dtype)
    y = (y * 2).round().long() if t_dtype == torch.int64 else y.to(t_dtype)
    want, sum_abs = oracle.err_oracle(x, y, "logcosh")
    got = ma.functional.log_cosh_error(x.cuda(), y.cuda())
    assert calls["entered"] == 0
    tol = ((N + 16) * 2 * F32 * sum_abs[0] + 2 * F32 * abs(want[0])) / N
    assert abs(float(got) - want[0] / N) <= tol, (float(got), want[0] / N, tol)


def test_err_reduce_refuses_two_dtypes_or_sizes():
    """Checked on the host, before any launch."""
    x = torch.zeros(8, device="cuda")
    with pytest.raises(TypeError):
        _hip.err_reduce(x, x.bfloat16(), "sq_err")
    with pytest.raises(TypeError):
        _hip.err_reduce(x, x[:4], "sq_err")


# -------------------------------------------------------------------- box IoU
@pytest.mark.parametrize("variant", oracle.IOU_VARIANTS)
def test_box_iou_tile_edges(variant):
    for N in cases.BOX_N:
        b1 = cases.random_boxes(N, N)
        for M in cases.BOX_M:
            b2 = cases.random_boxes(M, 100 + M)
            got = ops.box_iou_pairwise(b1.cuda(), b2.cuda(), variant)
            assert got.shape == (N, M) and got.dtype == torch.float32
            want, tol = cases.box_tol(variant, b1, b2, ops.box_iou_pairwise(b1, b2, variant))
            err = np.abs(oracle.as_f64(got) - want)
            assert np.all(err <= tol), (variant, N, M, float(err.max()), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("variant", oracle.IOU_VARIANTS)
def test_box_iou_planted_pairs(variant):
    names, b1, b2 = cases.planted_boxes()
    got = ops.box_iou_pairwise(b1.cuda(), b2.cuda(), variant).cpu()
    want, tol = cases.box_tol(variant, b1, b2, ops.box_iou_pairwise(b1, b2, variant))
    assert np.all(np.isfinite(want)) and torch.isfinite(got).all()
    err = np.abs(oracle.as_f64(got) - want)
    assert np.all(err <= tol), (variant, err, tol)
    if variant == "iou":
        for i, n in enumerate(names):
            if n in cases.IOU_EXACT:
                assert float(got[i, i]) == cases.IOU_EXACT[n], n
        assert float(got[names.index("zero-area-same-point"), names.index("zero-area-same-point")]) == 0.0
