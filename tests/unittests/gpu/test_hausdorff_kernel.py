"""The Hausdorff kernels (csrc/hausdorff.hip) against a numpy oracle written from
the definition: edge pixels by the four-neighbour rule with everything outside
the image counting as "not the class", all pairs in fp64, spacing rounded to
fp32 first.

Unit spacing must be EXACT: float32(sqrt(k)) for euclidean (k the integer
squared distance; the fp64 sqrt rounded to fp32 is the correctly rounded fp32
sqrt) and the integer for chessboard / taxicab. Any other spacing is held to a
relative 4 * 2**-24: the fp32 chain is two products, two squares, an add and a
sqrt, at most 3 units of 2**-24 once the sqrt has halved the error of its
argument, plus one of margin. inf must match exactly.
"""
import functools
import math

import numpy as np
import pytest
import torch

import metrics_amd as ma
from metrics_amd.functional.segmentation import hausdorff_distance
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "chessboard", "taxicab")


def _edge_points(mask):
    p = np.pad(mask, 1)
    inside = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return np.argwhere(mask & ~inside).astype(np.float64)


def _directed(a, b, metric, s):
    worst = 0.0
    for i in range(0, len(a), 512):  # chunks of A keep the pair matrix small
        dy = np.abs(a[i:i + 512, None, 0] - b[None, :, 0]) * s[0]
        dx = np.abs(a[i:i + 512, None, 1] - b[None, :, 1]) * s[1]
        d = {"euclidean": np.sqrt(dy * dy + dx * dx), "chessboard": np.maximum(dy, dx), "taxicab": dy + dx}[metric]
        worst = max(worst, d.min(1).max())
    return worst


def _oracle_arrays(p, t, C, include_background, metric, spacing, directed):
    """p, t: (N, H, W) label maps. (N, C') fp64; nan where both sides are empty."""
    s = np.asarray(spacing or [1, 1], dtype=np.float32).astype(np.float64)
    classes = range(1 if (not include_background and C > 1) else 0, C)
    out = np.empty((len(p), len(classes)))
    for n in range(len(p)):
        for j, c in enumerate(classes):
            a, b = _edge_points(p[n] == c), _edge_points(t[n] == c)
            if len(a) == 0 or len(b) == 0:
                out[n, j] = np.nan if len(a) == len(b) else np.inf
            else:
                out[n, j] = _directed(a, b, metric, s)
                if not directed:
                    out[n, j] = max(out[n, j], _directed(b, a, metric, s))
    return out


def _checker(s):
    return (np.indices((s, s)).sum(0) % 2).astype(np.int64)


def _tile_case(tile):
    """A checkerboard class (every pixel of it an edge pixel) with just more
    than ``tile`` pixels against the same board with a corner cut out."""
    s = math.isqrt(2 * tile) + 1
    p = _checker(s)[None]
    t = p.copy()
    t[0, : s // 2, : s // 3] = 0
    return p, t, 2, False


def _early_case(first):
    """Two identical boards of more than a B tile, and one far pixel in preds only."""
    s = math.isqrt(2 * _hip.HAUSDORFF_B_TILE) + 1
    t = np.zeros((1, s + 1, s + 40), dtype=np.int64)
    t[0, :s, 20:20 + s] = _checker(s)
    p = t.copy()
    p[0, 0 if first else s, 0 if first else s + 39] = 1
    return p, t, 2, False


def _boxes(H, W, a, b):
    p, t = np.zeros((1, H, W), dtype=np.int64), np.zeros((1, H, W), dtype=np.int64)
    p[0, a[0]:a[1], a[2]:a[3]] = 1
    t[0, b[0]:b[1], b[2]:b[3]] = 1
    return p, t, 2, False


def _ballot_case(W):
    """Class 1 fills preds (only border pixels are edges, class 0 is absent: inf);
    the target's class 1 touches the last column and the last row."""
    p = np.ones((1, 18, W), dtype=np.int64)
    t = np.zeros((1, 18, W), dtype=np.int64)
    t[0, 10:, W - 3:] = 1
    return p, t, 2, True


def _planes_case(include_background):
    rng = np.random.default_rng(5)
    p = np.kron(rng.integers(0, 4, (3, 5, 6)), np.ones((4, 4), dtype=np.int64))[:, :, :23]
    t = np.kron(rng.integers(0, 4, (3, 5, 6)), np.ones((4, 4), dtype=np.int64))[:, :, :23]
    p[1][p[1] == 3] = 2  # class 3 of sample 1 is absent from preds only
    return p, t, 4, include_background


CASES = {
    "wide_5x37": lambda: _boxes(5, 37, (1, 4, 2, 8), (0, 3, 20, 30)),
    "tall_37x5": lambda: _boxes(37, 5, (2, 8, 1, 4), (20, 30, 0, 3)),
    "ballot_w63": lambda: _ballot_case(63),
    "ballot_w64": lambda: _ballot_case(64),
    "ballot_w65": lambda: _ballot_case(65),
    "checker_24": lambda: (_checker(24)[None], 1 - _checker(24)[None], 2, True),
    "over_a_tile": lambda: _tile_case(_hip.HAUSDORFF_A_TILE),
    "over_b_tile": lambda: _tile_case(_hip.HAUSDORFF_B_TILE),
    "pixel_vs_pixel": lambda: _boxes(12, 33, (3, 4, 4, 5), (10, 11, 30, 31)),
    "pixel_vs_ring": lambda: _boxes(40, 40, (20, 21, 20, 21), (2, 38, 2, 38)),
    "early_exit_first": lambda: _early_case(True),
    "early_exit_last": lambda: _early_case(False),
    "planes_background": lambda: _planes_case(True),
    "planes_no_background": lambda: _planes_case(False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _oracle(name, metric, spacing, directed):
    p, t, C, bg = _case(name)
    return _oracle_arrays(p, t, C, bg, metric, list(spacing) if spacing else None, directed)


def _tensor(x, C, fmt, dtype):
    x = torch.from_numpy(x)
    if fmt == "one-hot":
        x = torch.nn.functional.one_hot(x, C).movedim(-1, 1)
    return x.to(dtype).cuda()


def _run(name, fmt, metric, spacing=None, directed=False):
    p, t, C, bg = _case(name)
    fp, ft = ("one-hot", "index") if fmt == "mixed" else (fmt, fmt)
    pd, td = (torch.bool, torch.uint8) if fmt == "one-hot" else (torch.int64, torch.int32)
    before = _hip.hausdorff_kernel_calls()
    got = hausdorff_distance(_tensor(p, C, fp, pd), _tensor(t, C, ft, td), C, bg, metric, spacing, directed, fmt)
    assert _hip.hausdorff_kernel_calls() == before + 1
    return got


def _assert_matches(got, exp, unit):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == exp.shape
    got = got.cpu().numpy().astype(np.float64)
    print("got", got.ravel(), "expected", exp.ravel())
    assert not np.isnan(exp).any()
    inf = np.isinf(exp)
    assert (np.isinf(got) == inf).all()
    if unit:
        assert (got[~inf] == exp[~inf].astype(np.float32)).all()
    else:
        assert (np.abs(got[~inf] - exp[~inf]) <= 4 * 2.0**-24 * exp[~inf]).all()


@pytest.mark.parametrize("fmt", ["index", "one-hot"])
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", list(CASES))
def test_matches_oracle(name, metric, directed, fmt):
    _assert_matches(_run(name, fmt, metric, None, directed), _oracle(name, metric, None, directed), unit=True)


@pytest.mark.parametrize("fmt", ["index", "one-hot"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("spacing", [(2, 3), (0.5, 1.5), (0.7, 1.3)])
@pytest.mark.parametrize("name", ["wide_5x37", "over_a_tile", "planes_no_background"])
def test_spacing(name, spacing, metric, fmt):
    _assert_matches(_run(name, fmt, metric, list(spacing)), _oracle(name, metric, spacing, False), unit=False)


def test_mixed_format_and_the_absent_class():
    exp = _oracle("planes_background", "euclidean", None, False)
    assert np.isinf(exp).sum() == 1 and np.isinf(exp[1, 3])  # absent from preds only: inf there, finite elsewhere
    _assert_matches(_run("planes_background", "mixed", "euclidean"), exp, unit=True)


def test_raises_like_the_torch_path():
    absent = torch.zeros(1, 9, 9, dtype=torch.long, device="cuda")
    with pytest.raises(RuntimeError):
        hausdorff_distance(absent, absent, 2, input_format="index")
    two = torch.zeros(1, 2, 9, 9, dtype=torch.long, device="cuda")
    two[0, 1, 3:5, 3:5] = 1
    bad = two.clone()
    bad[0, 1, 4, 4] = 2
    with pytest.raises(ValueError, match="binarized"):
        hausdorff_distance(bad, two, 2)


@pytest.mark.parametrize("metric", METRICS)
def test_square_random_masks_equal_the_cpu_path(metric):
    gen = torch.Generator().manual_seed(36)
    p = torch.randint(0, 2, (2, 2, 32, 32), generator=gen)
    t = torch.randint(0, 2, (2, 2, 32, 32), generator=gen)
    got = hausdorff_distance(p.cuda(), t.cuda(), 2, distance_metric=metric)
    assert torch.equal(got.cpu(), hausdorff_distance(p, t, 2, distance_metric=metric))


def test_path_and_determinism(monkeypatch):
    first = _run("planes_background", "index", "euclidean")
    assert torch.equal(first, _run("planes_background", "index", "euclidean"))
    sq = torch.zeros(1, 12, 12, dtype=torch.long)
    sq[0, 2:5, 2:6] = 1
    moved = sq.roll(3, 2)
    before = _hip.hausdorff_kernel_calls()
    assert hausdorff_distance(sq, moved, 2, input_format="index").item() == 3.0  # a CPU input
    monkeypatch.setenv(_hip.HAUSDORFF_KERNEL_ENV, "0")
    assert hausdorff_distance(sq.cuda(), moved.cuda(), 2, input_format="index").item() == 3.0
    assert _hip.hausdorff_kernel_calls() == before
    monkeypatch.setenv(_hip.HAUSDORFF_KERNEL_ENV, "1")
    assert hausdorff_distance(sq.cuda(), moved.cuda(), 2, input_format="index").item() == 3.0
    assert _hip.hausdorff_kernel_calls() == before + 1


def test_modular_metric_over_two_updates():
    m = ma.segmentation.HausdorffDistance(num_classes=2, input_format="index").to("cuda")
    total = np.float32(0.0)
    for name in ("wide_5x37", "pixel_vs_ring"):  # one plane each
        p, t, _, _ = _case(name)
        m.update(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda())
        total = total + np.float32(_oracle(name, "euclidean", None, False).item())
    assert m.compute().item() == float(total / np.float32(2.0))
