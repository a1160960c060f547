"""Case lists of the stand-alone kernels (fused SSIM, erosion, calibration bins,
error reductions, box IoU), shared by the CPU oracle test
(``tests/unittests/test_standalone_oracles.py``) and the GPU edge tests
(``tests/unittests/gpu/test_*_edges.py``): both iterate the same cases.

Everything here is seeded, on CPU, and small: every case is the smallest that
reaches its branch. Tolerances are the ones of docs/PARITY.md ("Stand-alone
kernels"); none is taken from a kernel's output.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import numpy as np
import torch

from tests.unittests import _standalone_oracles as oracle

F32_EPS = 2.0 ** -24  # half an ulp of 1.0f


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ====================================================================== SSIM
SSIM_FAMILIES = ("noise", "noisy_copy", "flat_bright", "ramp", "int255", "equal_zero", "equal_half",
                 "equal_noise", "zeros_ones")
# families whose result is 1.0 bit for bit on every path: all-zero images give
# (c1*c2)/(c1*c2), equal textured images give cov == var well above the clamp.
# A non-zero constant does not: the rounded window weights sum to 1 + d, the
# variance estimate becomes -v^2*d and only the variances are clamped.
SSIM_EXACT_ONE = ("equal_zero", "equal_noise")


def ssim_images(family: str, shape: Tuple[int, int, int, int], seed: int = 0):
    """(preds, target, data_range) float32 of one content family."""
    g = _gen(1000 + seed)
    B, C, H, W = shape
    if family == "noise":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g), None
    if family == "noisy_copy":
        t = torch.rand(shape, generator=g)
        return t + 0.05 * torch.randn(shape, generator=g), t, None
    if family == "flat_bright":
        return (0.9 + 0.001 * (2 * torch.rand(shape, generator=g) - 1),
                0.9 + 0.001 * (2 * torch.rand(shape, generator=g) - 1), 1.0)
    if family == "ramp":
        yy = torch.arange(H, dtype=torch.float32)[:, None]
        xx = torch.arange(W, dtype=torch.float32)[None, :]
        t = ((yy + xx) / max(H + W - 2, 1)).expand(shape).contiguous()
        return 0.8 * t + 0.1, t, 1.0
    if family == "int255":
        t = torch.randint(0, 256, shape, generator=g).float()
        p = (t + torch.randint(-20, 21, shape, generator=g).float()).clamp(0, 255)
        return p, t, 255.0
    if family == "equal_zero":
        return torch.zeros(shape), torch.zeros(shape), 1.0
    if family == "equal_half":
        return torch.full(shape, 0.5), torch.full(shape, 0.5), 1.0
    if family == "equal_noise":
        t = torch.rand(shape, generator=g)
        return t.clone(), t, 1.0
    assert family == "zeros_ones", family
    return torch.zeros(shape), torch.ones(shape), 1.0


def _mixed_batch(H: int, W: int, C: int = 2):
    """Three images of different content: independent noise (SSIM about 0), a noisy
    copy (0.97) and a copy under heavy noise (about 0.6), so a wrong plane-to-image
    mapping moves a per-image result by more than 0.1."""
    parts = [ssim_images(f, (1, C, H, W), seed=7 + i)[:2] for i, f in enumerate(("noise", "noisy_copy", "noise"))]
    base = parts[2][1]
    parts[2] = (base + 0.3 * torch.randn(base.shape, generator=_gen(8)), base)
    return torch.cat([p for p, _ in parts]), torch.cat([t for _, t in parts])


def _ssim_case_table() -> Dict[str, dict]:
    """id -> dict(make=() -> (p, t), kw=functional kwargs, path='kernel' | 'torch')."""
    cases: Dict[str, dict] = {}

    def add(cid, make, path="kernel", **kw):
        kw.setdefault("reduction", "none")
        cases[cid] = {"make": make, "kw": kw, "path": path}

    def fam(family, shape, seed=0):
        return lambda: ssim_images(family, shape, seed)[:2]

    # shapes against the 32-wide tile, default window (radius 5)
    for H, W in ((6, 9), (12, 12), (32, 32), (33, 31), (64, 65), (57, 83)):
        add(f"shape-{H}x{W}", fam("noisy_copy", (2, 1, H, W), seed=H))
    add("shape-11x11-cs", fam("noisy_copy", (2, 1, 11, 11), seed=11), return_contrast_sensitivity=True)
    add("batch-3x2", lambda: _mixed_batch(33, 31))
    add("batch-3x2-cs", lambda: _mixed_batch(33, 31), return_contrast_sensitivity=True)
    # windows: orientation matters on a non-square image with directional content
    win = lambda: _mixed_batch(33, 31)  # noqa: E731
    add("win-sigma-0.5x2.0", win, sigma=(0.5, 2.0), return_contrast_sensitivity=True)
    add("win-sigma-2.0x0.5", win, sigma=(2.0, 0.5), return_contrast_sensitivity=True)
    add("win-uniform-3x9", win, gaussian_kernel=False, kernel_size=(3, 9), return_contrast_sensitivity=True)
    add("win-uniform-9x3", win, gaussian_kernel=False, kernel_size=(9, 3), return_contrast_sensitivity=True)
    add("win-uniform-1", win, gaussian_kernel=False, kernel_size=1)
    add("win-uniform-7", win, gaussian_kernel=False, kernel_size=7)
    add("win-gauss-ignores-kernel-size", win, sigma=1.0, kernel_size=(3, 5))
    # both sides of the LDS gate: radius 13 is the last window that fits
    for s, path in ((3.7, "kernel"), (4.0, "torch")):
        add(f"lds-sigma-{s}", fam("noisy_copy", (2, 2, 30, 30), seed=3), path=path, sigma=s)
        add(f"lds-sigma-{s}-cs", fam("noisy_copy", (2, 2, 30, 30), seed=3), path=path, sigma=s,
            return_contrast_sensitivity=True)
    # content families at 57x83
    for f in SSIM_FAMILIES:
        dr = ssim_images(f, (1, 1, 2, 2))[2]
        add(f"family-{f}", fam(f, (2, 2, 57, 83), seed=5), data_range=dr)
    # data_range: None is covered above; a float; a tuple that clamps real outliers
    add("range-float", fam("noisy_copy", (2, 1, 33, 31), seed=9), data_range=2.5)

    def outliers():
        p, t = ssim_images("noisy_copy", (2, 1, 33, 31), seed=9)[:2]
        p, t = p.clone(), t.clone()
        p[0, 0, 3, 4], p[1, 0, 20, 30], t[0, 0, 0, 0], t[1, 0, 32, 0] = 3.0, -2.0, -1.5, 7.0
        return p, t

    # bounds exact in bf16 and fp16, so every dtype clamps at the same values
    add("range-tuple", outliers, data_range=(0.125, 0.875), return_contrast_sensitivity=True)
    add("elementwise-mean", lambda: _mixed_batch(33, 31), reduction="elementwise_mean")
    return cases


SSIM_CASES = _ssim_case_table()
SSIM_DTYPE_CASES = ("shape-33x31", "range-tuple", "family-int255")  # run again in bf16 / fp16 / fp64
MS_SSIM_CASES: Dict[str, dict] = {
    "ms-176x180-defaults": {"make": lambda: ssim_images("noisy_copy", (1, 1, 176, 180), seed=21)[:2],
                            "kw": {"reduction": "none"}},
    "ms-two-betas-16x20": {"make": lambda: ssim_images("noisy_copy", (2, 2, 16, 20), seed=22)[:2],
                           "kw": {"reduction": "none", "kernel_size": 5, "sigma": 0.5, "betas": (0.4, 0.6)}},
}
# more planes than grid.z holds (65535): 6x6 images, sigma 0.5 (radius 2)
SSIM_PLANE_COUNTS = ((13107, 5), (13108, 5))  # B*C = 65535, 65540


def ssim_plane_images(B: int, C: int):
    """(B, C, 6, 6) noisy copies whose noise level grows with the image index, so
    every image has its own value."""
    g = _gen(77)
    t = torch.rand(B, C, 6, 6, generator=g)
    level = torch.linspace(0.01, 0.3, B)[:, None, None, None]
    return t + level * torch.randn(B, C, 6, 6, generator=g), t


def _oracle_kwargs(kw: dict) -> dict:
    out = {"gaussian": kw.get("gaussian_kernel", True), "sigma": kw.get("sigma", 1.5),
           "kernel_size": kw.get("kernel_size", 11), "data_range": kw.get("data_range"),
           "k1": kw.get("k1", 0.01), "k2": kw.get("k2", 0.03)}
    return out


def ssim_tol(cpu_fp32, want) -> float:
    """Per case: max(4 * |CPU fp32 path - oracle|, 8 * 2^-24 * max(1, |oracle|)), the
    largest over the outputs of the case (a per-image result of a small image is a
    mean of few pixels, and its fp32 error is a draw: the CPU path's error on one
    image says nothing about the kernel's on the same image, its largest does)."""
    want = np.asarray(want, dtype=np.float64)
    cpu = oracle.as_f64(cpu_fp32).reshape(want.shape)
    return float(max(4 * np.abs(cpu - want).max(), 8 * F32_EPS * max(1.0, np.abs(want).max())))


def _reduced(x: np.ndarray, kw: dict) -> np.ndarray:
    return x.mean(keepdims=True) if kw.get("reduction") == "elementwise_mean" else x


def ssim_functional_outputs(out) -> List[torch.Tensor]:
    """[sim] or [sim, cs] of the functional's return value."""
    return list(out) if isinstance(out, tuple) else [out]


@functools.lru_cache(maxsize=None)
def ssim_expected(cid: str, dtype: torch.dtype = torch.float32):
    """(p, t, kw, [oracle sim(, cs)], [CPU fp32 path sim(, cs)]) of a case; p and t
    are rounded to ``dtype``, and the oracle and the CPU path (run in fp32) see
    the rounded values. Computed once, shared, never modified."""
    from metrics_amd.functional.image import structural_similarity_index_measure as ssim

    case = SSIM_CASES[cid]
    p, t = case["make"]()
    p, t = p.to(dtype), t.to(dtype)
    kw = dict(case["kw"])
    sim, cs, _ = oracle.ssim_oracle(p, t, **_oracle_kwargs(kw))
    want = [_reduced(sim, kw)] + ([cs] if kw.get("return_contrast_sensitivity") else [])
    cpu = ssim_functional_outputs(ssim(p.float(), t.float(), **kw))
    return p, t, kw, want, [c.reshape(-1) for c in cpu]


@functools.lru_cache(maxsize=None)
def ms_ssim_expected(cid: str):
    from metrics_amd.functional.image import multiscale_structural_similarity_index_measure as ms_ssim

    case = MS_SSIM_CASES[cid]
    p, t = case["make"]()
    kw = dict(case["kw"])
    okw = _oracle_kwargs(kw)
    if "betas" in kw:
        okw["betas"] = kw["betas"]
    want = oracle.ms_ssim_oracle(p, t, **okw)
    return p, t, kw, want, ms_ssim(p, t, **kw).reshape(-1)


def assert_ssim_close(got, want, cpu, label, out_dtype: torch.dtype = torch.float32) -> float:
    """got within ssim_tol of the oracle; returns the largest |got - oracle|.

    A bf16 / fp16 result is the kernel's value rounded to that format. Rounding is
    monotonic, so the value was within the tolerance iff the result lies between
    the roundings of oracle - tol and oracle + tol: that is what is asserted, and
    it allows nothing but the output format on top of the rule."""
    got = oracle.as_f64(got).reshape(np.shape(want))
    err = np.abs(got - want)
    tol = ssim_tol(cpu, want)
    if out_dtype in (torch.bfloat16, torch.float16):
        lo = oracle.as_f64(torch.from_numpy(want - tol).to(out_dtype))
        hi = oracle.as_f64(torch.from_numpy(want + tol).to(out_dtype))
        assert np.all((got >= lo) & (got <= hi)), (label, got, lo, hi)
    else:
        assert np.all(err <= tol), (label, float(err.max()), tol, got, want)
    return float(err.max())


# =================================================================== erosion
EROSION_SHAPES = ((1, 1, 1, 1), (1, 1, 1, 7), (1, 1, 7, 1), (2, 3, 5, 4), (1, 2, 17, 300), (1, 1, 3, 3))
EROSION_STRUCTURES: Tuple[Tuple[str, List[List[int]], Tuple[int, int]], ...] = (
    ("1x1", [[1]], (0, 0)),
    ("3x3-full", [[1, 1, 1]] * 3, (1, 1)),
    ("cross", [[0, 1, 0], [1, 1, 1], [0, 1, 0]], (1, 1)),
    ("1x3", [[1, 1, 1]], (0, 1)),
    ("3x1", [[1], [1], [1]], (1, 0)),
    ("5x3-origin-2-1", [[1, 1, 1]] * 5, (2, 1)),
    ("2x2-origin-0-0", [[1, 1], [0, 1]], (0, 0)),
    ("2x2-origin-1-1", [[1, 1], [0, 1]], (1, 1)),
    ("3x3-origin-0-0", [[1, 1, 0], [1, 1, 1], [0, 1, 1]], (0, 0)),
    ("3x3-origin-2-2", [[1, 1, 0], [1, 1, 1], [0, 1, 1]], (2, 2)),
    ("5x5", [[1] * 5] * 5, (2, 2)),
    ("3x3-all-zero", [[0] * 3] * 3, (1, 1)),
)
EROSION_IMAGES = ("ones", "zeros", "checker", "random")
EROSION_DTYPES = (torch.bool, torch.uint8, torch.int32, torch.int64, torch.float32)


def erosion_image(kind: str, shape) -> torch.Tensor:
    N, C, H, W = shape
    if kind == "ones":
        return torch.ones(shape, dtype=torch.int32)
    if kind == "zeros":
        return torch.zeros(shape, dtype=torch.int32)
    if kind == "checker":
        yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
        return ((yy + xx) % 2).int().expand(shape).contiguous()
    return (torch.rand(shape, generator=_gen(H * 1000 + W)) > 0.3).int()  # mostly ones: erosion has work to do


# =============================================================== calibration
CALIB_N_BINS = (1, 2, 10, 15, 99, 2048)
CALIB_FALLBACK_BINS = 2049  # 3 * 2049 int64 counters exceed the kernel's 48 KB of LDS
CALIB_SIZES = (1, 255, 256, 257, 2048 * 256 + 1)  # the last wraps the grid-stride loop (2048 blocks of 256)


def calib_bounds(kind: str, n_bins: int) -> torch.Tensor:
    """float32 boundaries. 'uniform' is what the metric builds; 'sqrt' is
    non-uniform (binary-search branch); 'bf16' is linspace computed in bf16, whose
    rounded boundaries are unevenly spaced."""
    if kind == "uniform":
        return torch.linspace(0, 1, n_bins + 1)
    if kind == "sqrt":
        return torch.linspace(0, 1, n_bins + 1).sqrt()
    assert kind == "bf16"
    return torch.linspace(0, 1, n_bins + 1, dtype=torch.bfloat16).float()


def calib_inputs(bounds: torch.Tensor, n: int, seed: int = 0, dtype=torch.float32):
    """(conf, acc) of length n: every boundary, its float neighbours on both sides
    (so just below 0 and just above 1 too), 0.0 and 1.0, then a seeded random fill.
    Planted values come first in a seeded shuffle of themselves, so a short n still
    holds boundaries."""
    g = _gen(300 + seed)
    b = bounds.to(dtype)
    inf = torch.tensor(float("inf"), dtype=dtype)
    planted = torch.cat([b, torch.nextafter(b, inf), torch.nextafter(b, -inf),
                         torch.tensor([0.0, 1.0], dtype=dtype)])
    planted = planted[torch.randperm(planted.numel(), generator=g)]
    fill = torch.rand(max(n - planted.numel(), 0), generator=g).to(dtype)
    conf = torch.cat([planted, fill])[:n]
    acc = (torch.rand(n, generator=g) > 0.4).float()
    return conf, acc


def calib_sum_tol(count: np.ndarray, want: np.ndarray) -> np.ndarray:
    """n_j * 2^-34 (2^33 fixed-point quantisation) + 2^-23 * |oracle| (returned as fp32)."""
    return count * 2.0 ** -34 + 2.0 ** -23 * np.abs(want)


# ========================================================== error reductions
ERR_SIZES = (0, 1, 255, 256, 257, 2048 * 256 + 3)
LOGCOSH_PLANTS = (1e-4, 20.0, 354.0, 355.0, 400.0, 1e4)  # exp(2 * 354.9) is the last finite double
FUNCTIONAL_OPS = {  # functional name -> op of the kernel
    "mean_squared_error": "sq_err", "mean_absolute_error": "abs_err",
    "mean_absolute_percentage_error": "ape", "mean_squared_log_error": "sq_log_err",
    "log_cosh_error": "logcosh",
}


def err_inputs(op: str, N: int, dtype=torch.float32, seed: int = 0):
    """(x, y) of length N in ``dtype`` with the op's edge values planted up front."""
    g = _gen(500 + seed + N % 1000)
    x = torch.randn(N, generator=g)
    y = torch.randn(N, generator=g)
    if op == "sq_log_err":
        x, y = x.abs(), y.abs()
        for i, (a, b) in enumerate(((0.0, 1.5), (2.0, 0.0), (0.0, 0.0))):
            if i + 1 < N:
                x[i + 1], y[i + 1] = a, b
    elif op == "ape":  # targets at 0 and below eps = 1.17e-6, both signs
        for i, b in enumerate((0.0, 1e-7, -1e-7, 1e-6, -0.0)):
            if i + 1 < N:
                y[i + 1] = b
    elif op == "logcosh":
        plants = [s * d for d in LOGCOSH_PLANTS for s in (1.0, -1.0)]
        for i, d in enumerate(plants):
            if i + 1 < N:
                x[i + 1], y[i + 1] = (d, 0.0) if i % 4 < 2 else (0.0, -d)
    return x.to(dtype), y.to(dtype)


def err_tol(N: int, sum_abs: np.ndarray) -> np.ndarray:
    """(N + 16) * 2^-52 * sum |term|: fp64 accumulation in any order plus a few
    ulps per device log1p / exp."""
    return (N + 16) * 2.0 ** -52 * sum_abs


# =================================================================== box IoU
BOX_N = (1, 63, 64, 65)    # rows: 64 per block
BOX_M = (1, 255, 256, 257)  # columns: 256 per block


def random_boxes(n: int, seed: int) -> torch.Tensor:
    """(n, 4) xyxy boxes on the grid of multiples of 0.25 below 512, so widths and
    heights have at most 11 bits, areas 22, and unions and enclosing areas at most
    24: every term of 'iou' and 'giou' before the division is exact in fp32. Every
    7th box has zero width and every 11th zero height; inverted boxes are among
    the planted pairs only."""
    g = _gen(900 + seed)
    xy = torch.randint(0, 1024, (n, 2), generator=g).float() * 0.25
    wh = torch.randint(1, 1024, (n, 2), generator=g).float() * 0.25
    b = torch.cat([xy, torch.minimum(xy + wh, torch.tensor(511.75))], 1)
    b[6::7, 2] = b[6::7, 0]
    b[10::11, 3] = b[10::11, 1]
    return b


PLANTED_PAIRS = {  # name -> (box1, box2)
    "identical": ((10.0, 20.0, 50.0, 80.0), (10.0, 20.0, 50.0, 80.0)),
    "nested": ((10.0, 20.0, 50.0, 80.0), (20.0, 30.0, 30.0, 40.0)),
    "touching-edge": ((10.0, 20.0, 50.0, 80.0), (50.0, 20.0, 70.0, 80.0)),
    "touching-corner": ((10.0, 20.0, 50.0, 80.0), (50.0, 80.0, 60.0, 90.0)),
    "far-apart": ((0.0, 0.0, 1.25, 2.5), (400.0, 500.0, 410.0, 511.75)),
    "zero-width": ((10.0, 20.0, 10.0, 80.0), (5.0, 20.0, 40.0, 80.0)),
    "zero-area-same-point": ((7.5, 7.5, 7.5, 7.5), (7.5, 7.5, 7.5, 7.5)),
    "inverted": ((50.0, 20.0, 10.0, 80.0), (20.0, 30.0, 60.0, 70.0)),
}
IOU_EXACT = {"identical": 1.0, "touching-edge": 0.0, "touching-corner": 0.0, "far-apart": 0.0}


def planted_boxes():
    names = list(PLANTED_PAIRS)
    b1 = torch.tensor([PLANTED_PAIRS[n][0] for n in names])
    b2 = torch.tensor([PLANTED_PAIRS[n][1] for n in names])
    return names, b1, b2


def box_tol(variant: str, b1, b2, cpu_fp32) -> Tuple[np.ndarray, np.ndarray]:
    """(oracle, tolerance). 'iou' is one correctly rounded division of exact
    terms and 'giou' two and a subtraction: 2 ulp of fp32, taken at the largest
    term (the value itself for 'iou'), per element. 'diou' and 'ciou' follow the
    SSIM rule, per (N, M) case."""
    want, mag = oracle.box_iou_parts(b1, b2, variant)
    if variant in ("iou", "giou"):
        return want, 2 * np.spacing(mag.astype(np.float32)).astype(np.float64)
    return want, ssim_tol(cpu_fp32, want)
