"""fp64 oracles for the stand-alone kernels, written from the definitions.

Plain numpy: no torch convolution, no call into ``metrics_amd``. Each function
takes torch tensors or arrays, works on their values in float64 and returns
numpy. A low-precision input (bf16, fp16) is judged on its rounded values: the
caller passes the rounded tensor, the oracle widens it exactly.

* :func:`ssim_oracle` / :func:`ms_ssim_oracle` - windowed SSIM, reflect padding
* :func:`erosion_oracle` - ``min over window (v - strel) + 1``
* :func:`calib_oracle` - ``searchsorted(..., 'right') - 1`` binning
* :func:`err_oracle` - the six elementwise-error reductions, exactly summed
* :func:`box_iou_oracle` - IoU / GIoU / DIoU / CIoU, the formulas of
  ``ops._box_iou_torch``
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np

LN2 = math.log(2.0)
ERR_OPS = ("sq_err", "abs_err", "ape", "sq_log_err", "moments", "logcosh")
IOU_VARIANTS = ("iou", "giou", "diou", "ciou")


def as_f64(x) -> np.ndarray:
    """The values of a tensor or array, widened exactly to float64."""
    if hasattr(x, "detach"):
        x = x.detach().cpu()
        x = x.double() if x.is_floating_point() else x.long()
        return x.numpy().astype(np.float64)
    return np.asarray(x, dtype=np.float64)


# ---------------------------------------------------------------------- SSIM
def _pair(v) -> Tuple:
    return tuple(v) if isinstance(v, (list, tuple)) else (v, v)


def ssim_window(gaussian: bool, sigma, kernel_size) -> Tuple[np.ndarray, np.ndarray]:
    """(vertical, horizontal) 1-D weights. A gaussian window's size follows
    sigma (``2*int(3.5*sigma+0.5)+1`` per axis) and ignores ``kernel_size``."""
    out = []
    for s, k in zip(_pair(sigma), _pair(kernel_size)):
        if gaussian:
            k = 2 * int(3.5 * s + 0.5) + 1
            d = np.arange(k, dtype=np.float64) - (k - 1) / 2
            w = np.exp(-((d / s) ** 2) / 2)
            out.append(w / w.sum())
        else:
            out.append(np.full(k, 1.0 / k))
    return out[0], out[1]


def reflect_index(n: int, pad: int) -> np.ndarray:
    """Source index of every cell of an axis of length n padded by ``pad`` on both
    sides, mirror without repeating the edge: -1 -> 1, n -> n - 2."""
    assert 0 <= pad < n, "reflect padding needs pad < n"
    i = np.arange(-pad, n + pad)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _window_mean(x: np.ndarray, wh: np.ndarray, ww: np.ndarray) -> np.ndarray:
    """Mean of x (..., H, W) under the 2-D window outer(wh, ww), reflect padded."""
    H, W = x.shape[-2:]
    ph, pw = (len(wh) - 1) // 2, (len(ww) - 1) // 2
    xp = x[..., reflect_index(H, ph)[:, None], reflect_index(W, pw)[None, :]]
    w2 = np.outer(wh, ww)
    out = np.zeros_like(x)
    for dy in range(len(wh)):
        for dx in range(len(ww)):
            out += w2[dy, dx] * xp[..., dy:dy + H, dx:dx + W]
    return out


def ssim_oracle(p, t, *, gaussian: bool = True, sigma=1.5, kernel_size=11,
                data_range: Optional[Union[float, Tuple[float, float]]] = None,
                k1: float = 0.01, k2: float = 0.03):
    """(sim (B,), cs (B,), full map (B, C, H, W)) of (B, C, H, W) images.

    ``sim`` is the mean of the whole map, ``cs`` the mean of the contrast term
    over the map cropped by the pad (NaN where nothing is left)."""
    p, t = as_f64(p), as_f64(t)
    assert p.shape == t.shape and p.ndim == 4
    if data_range is None:
        dr = max(p.max() - p.min(), t.max() - t.min())
    elif isinstance(data_range, tuple):
        p, t = np.clip(p, *data_range), np.clip(t, *data_range)
        dr = data_range[1] - data_range[0]
    else:
        dr = data_range
    c1, c2 = (k1 * dr) ** 2, (k2 * dr) ** 2
    wh, ww = ssim_window(gaussian, sigma, kernel_size)
    ph, pw = (len(wh) - 1) // 2, (len(ww) - 1) // 2
    mu_p, mu_t = _window_mean(p, wh, ww), _window_mean(t, wh, ww)
    var_p = np.maximum(_window_mean(p * p, wh, ww) - mu_p * mu_p, 0.0)
    var_t = np.maximum(_window_mean(t * t, wh, ww) - mu_t * mu_t, 0.0)
    cov = _window_mean(p * t, wh, ww) - mu_p * mu_t
    upper, lower = 2 * cov + c2, var_p + var_t + c2
    full = ((2 * mu_p * mu_t + c1) * upper) / ((mu_p * mu_p + mu_t * mu_t + c1) * lower)
    B, _, H, W = p.shape
    sim = full.reshape(B, -1).mean(-1)
    if H > 2 * ph and W > 2 * pw:
        cs = (upper / lower)[..., ph:H - ph, pw:W - pw].reshape(B, -1).mean(-1)
    else:
        cs = np.full(B, np.nan)
    return sim, cs, full


def _avg_pool2(x: np.ndarray) -> np.ndarray:
    H, W = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    x = x[..., :H, :W]
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) / 4


def ms_ssim_oracle(p, t, *, betas: Sequence[float] = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333),
                   normalize: Optional[str] = "relu", **ssim_kwargs) -> np.ndarray:
    """Per-image multi-scale SSIM: contrast terms of all scales but the last,
    the similarity of the last, 2x2 mean pooling between scales."""
    p, t = as_f64(p), as_f64(t)
    terms = []
    for i in range(len(betas)):
        sim, cs, _ = ssim_oracle(p, t, **ssim_kwargs)
        terms.append(sim if i == len(betas) - 1 else cs)
        if i < len(betas) - 1:
            p, t = _avg_pool2(p), _avg_pool2(t)
    m = np.stack(terms)
    if normalize == "relu":
        m = np.maximum(m, 0.0)
    elif normalize == "simple":
        m = (m + 1) / 2
    return np.prod(m ** np.asarray(betas, dtype=np.float64)[:, None], axis=0)


# ------------------------------------------------------------------- erosion
def erosion_oracle(img, strel, origin: Tuple[int, int], border_value: int = 0) -> np.ndarray:
    """``min over the window of (v - strel) + 1`` of a (N, C, H, W) 0/1 image, where
    the window cell (dy, dx) of output (y, x) is input (y + dy - origin[0],
    x + dx - origin[1]) and reads ``border_value`` outside the image. An all-zero
    structure gives 2 on an all-one neighbourhood."""
    img = as_f64(img).astype(np.int64)
    strel = as_f64(strel).astype(np.int64)
    N, C, H, W = img.shape
    kh, kw = strel.shape
    oy, ox = origin
    big = np.full((N, C, H + kh, W + kw), int(border_value), dtype=np.int64)
    big[:, :, oy:oy + H, ox:ox + W] = img  # big[y + oy, x + ox] = img[y, x]
    mn = None
    for dy in range(kh):
        for dx in range(kw):
            d = big[:, :, dy:dy + H, dx:dx + W] - strel[dy, dx]
            mn = d if mn is None else np.minimum(mn, d)
    return (mn + 1).astype(np.uint8)


# --------------------------------------------------------------- calibration
def calib_oracle(conf, acc, bounds):
    """(count int64, sum of conf, sum of acc) per bin. Bin of c is the index of
    the last boundary <= c, clamped to [0, n_bins - 1]."""
    conf, acc, bounds = as_f64(conf).ravel(), as_f64(acc).ravel(), as_f64(bounds).ravel()
    n_bins = len(bounds) - 1
    idx = np.clip(np.searchsorted(bounds, conf, side="right") - 1, 0, n_bins - 1)
    count = np.bincount(idx, minlength=n_bins).astype(np.int64)
    conf_sum = np.bincount(idx, weights=conf, minlength=n_bins)
    acc_sum = np.bincount(idx, weights=acc, minlength=n_bins)
    return count, conf_sum, acc_sum


# ---------------------------------------------------------- error reductions
def err_terms(x, y, op: str, eps: float = 1.17e-6) -> np.ndarray:
    """The per-element terms of ``op``: (N,) or, for ``moments``, (6, N) in the
    order sum_x, sum_x2, sum_y, sum_y2, sum_xy, n."""
    x, y = as_f64(x).ravel(), as_f64(y).ravel()
    d = x - y
    if op == "sq_err":
        return d * d
    if op == "abs_err":
        return np.abs(d)
    if op == "ape":
        return np.abs(d) / np.maximum(np.abs(y), eps)
    if op == "sq_log_err":
        return (np.log1p(x) - np.log1p(y)) ** 2
    if op == "logcosh":
        a = np.abs(d)
        return a + np.log1p(np.exp(-2 * a)) - LN2
    if op == "moments":
        return np.stack([x, x * x, y, y * y, x * y, np.ones_like(x)])
    raise ValueError(op)


def err_oracle(x, y, op: str, eps: float = 1.17e-6) -> Tuple[np.ndarray, np.ndarray]:
    """(sums, sums of |term|), each of shape (n_out,), exactly rounded (fsum)."""
    terms = np.atleast_2d(err_terms(x, y, op, eps))
    return (np.array([math.fsum(r) for r in terms]),
            np.array([math.fsum(np.abs(r)) for r in terms]))


# -------------------------------------------------------------------- box IoU
def box_iou_oracle(b1, b2, variant: str) -> np.ndarray:
    """(N, M) all-pairs value for xyxy boxes; degenerate and inverted boxes give
    whatever the formulas give."""
    return box_iou_parts(b1, b2, variant)[0]


def box_iou_parts(b1, b2, variant: str) -> Tuple[np.ndarray, np.ndarray]:
    """(value, largest magnitude among the value and the terms it is the sum of)."""
    b1, b2 = as_f64(b1), as_f64(b2)
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt = np.maximum(b1[:, None, :2], b2[None, :, :2])
    rb = np.minimum(b1[:, None, 2:], b2[None, :, 2:])
    wh = np.maximum(rb - lt, 0.0)
    inter = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, inter / union, 0.0)
        if variant == "iou":
            return iou, np.abs(iou)
        whc = np.maximum(b1[:, None, 2:], b2[None, :, 2:]) - np.minimum(b1[:, None, :2], b2[None, :, :2])
        if variant == "giou":
            carea = whc[..., 0] * whc[..., 1]
            pen = np.where(carea > 0, (carea - union) / carea, 0.0)
            out = iou - pen
            return out, np.maximum(np.maximum(np.abs(iou), np.abs(pen)), np.abs(out))
        cdiag = whc[..., 0] ** 2 + whc[..., 1] ** 2 + 1e-7
        cent1, cent2 = (b1[:, :2] + b1[:, 2:]) / 2, (b2[:, :2] + b2[:, 2:]) / 2
        dist = ((cent1[:, None, :] - cent2[None, :, :]) ** 2).sum(-1)
        if variant == "diou":
            out = iou - dist / cdiag
            return out, np.maximum(np.abs(iou), np.abs(out))
        assert variant == "ciou"
        w1, h1 = b1[:, 2] - b1[:, 0], b1[:, 3] - b1[:, 1]
        w2, h2 = b2[:, 2] - b2[:, 0], b2[:, 3] - b2[:, 1]
        v = (4 / math.pi ** 2) * (np.arctan(w2 / (h2 + 1e-7))[None, :] - np.arctan(w1 / (h1 + 1e-7))[:, None]) ** 2
        alpha = v / (1 - iou + v + 1e-7)
        out = iou - dist / cdiag - alpha * v
        return out, np.maximum(np.abs(iou), np.abs(out))
