"""Case lists of the exact (``thresholds=None``) curve kernels
(``metrics_amd/csrc/clf_curve.hip``), shared by the CPU oracle test
(``tests/unittests/classification/test_exact_curve_oracle.py``) and the GPU
tests (``tests/unittests/gpu/test_exact_curve_kernels.py``).

Everything is seeded, on CPU and small. Expected values come from
``tests/unittests/_exact_curve_oracle.py``; the NaN cases carry theirs written
out by hand. No bound here is taken from a kernel's output.
"""
from __future__ import annotations

import functools
from typing import List, Tuple

import numpy as np
import torch

from tests.unittests import _exact_curve_oracle as oracle

NAN = float("nan")
INF = float("inf")
NEG_NAN = torch.tensor([0xFFC00000 - 2**32], dtype=torch.int32).view(torch.float32).item()  # sign bit set

# ------------------------------------------------------------------ bounds
# Counts are exact. A curve value is one fp32 division of two exact counts (or a
# sum of two first): within 2 fp32 ulps of the fp64 ratio.
RATIO_ULPS = 2.0
# Weighted sums: the kernel scans in fp64 and rounds to fp32 once, so half an
# ulp plus a scan error of at most n * 2^-53 relative, negligible for n <= 2^20.
WEIGHTED_ULPS = 1.0
# Areas: twice the largest error of the CPU path's own fp32 trapezoid / sum
# against the fp64 oracle over PUBLIC_CASES (measured by
# test_exact_curve_oracle.py::test_cpu_area_error_is_the_recorded_one, recorded
# in docs/PARITY.md "Exact curves"). Not taken from the kernel.
CPU_AREA_ERROR = 7.0e-8
AREA_BOUND = 2 * CPU_AREA_ERROR

# ---------------------------------------------------------- score families
FAMILIES = ("distinct", "equal", "two_values", "quant50", "ramp_up", "ramp_down", "bf16", "fp16", "zeros_denormals",
            "infs", "neighbours")
_DENORMAL = 2.0 ** -149
_PLANTED = {
    "zeros_denormals": [0.0, -0.0, _DENORMAL, -_DENORMAL, 2.0 ** -127, -(2.0 ** -127), 0.0, -0.0],
    "infs": [INF, -INF, 0.25, 0.75, 1.0, 0.0],
}


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def scores(family: str, n: int, seed: int = 0) -> torch.Tensor:
    """n float32 scores of one family, in a seeded random order (the ramps keep theirs)."""
    g = _gen(17 * seed + 1)
    if family == "distinct":  # i / n is distinct in fp32 up to n = 2^24
        return (torch.randperm(n, generator=g).double() / n).float()
    if family == "equal":
        return torch.full((n,), 0.375)
    if family == "two_values":
        return torch.where(torch.rand(n, generator=g) < 0.5, 0.25, 0.75)
    if family == "quant50":
        return (torch.rand(n, generator=g) * 50).round() / 50
    if family == "ramp_up":
        return (torch.arange(n).double() / n).float()
    if family == "ramp_down":
        return (torch.arange(n - 1, -1, -1).double() / n).float()
    if family == "bf16":
        return torch.rand(n, generator=g).bfloat16().float()
    if family == "fp16":
        return torch.rand(n, generator=g).half().float()
    if family in _PLANTED:
        vals = torch.tensor(_PLANTED[family], dtype=torch.float32)
        return vals[torch.randint(0, len(vals), (n,), generator=g)] if n > 1 else vals[:1].clone()
    if family == "neighbours":  # 0, 0.5, 1 and the float32 on either side of each
        base = np.array([0.0, 0.5, 1.0], dtype=np.float32)
        vals = np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-2))])
        vals = torch.from_numpy(vals)
        return vals[torch.randint(0, len(vals), (n,), generator=g)]
    raise ValueError(family)


TARGET_KINDS = ("random", "all_pos", "all_neg", "one_pos_best", "one_pos_worst", "label0_of5", "label3_of5")


def targets(kind: str, s: torch.Tensor, seed: int = 0) -> Tuple[torch.Tensor, int]:
    """(int64 targets, pos_label) for the scores ``s``."""
    n, g = s.numel(), _gen(31 * seed + 7)
    if kind == "random":
        return torch.randint(0, 2, (n,), generator=g), 1
    if kind == "all_pos":
        return torch.ones(n, dtype=torch.long), 1
    if kind == "all_neg":
        return torch.zeros(n, dtype=torch.long), 1
    if kind in ("one_pos_best", "one_pos_worst"):
        t = torch.zeros(n, dtype=torch.long)
        t[int(s.argmax() if kind == "one_pos_best" else s.argmin())] = 1
        return t, 1
    if kind in ("label0_of5", "label3_of5"):
        return torch.randint(0, 5, (n,), generator=g), int(kind[5])
    raise ValueError(kind)


def weights(kind: str, n: int, seed: int = 0) -> torch.Tensor:
    g = _gen(13 * seed + 3)
    if kind == "rand":
        return torch.rand(n, generator=g)
    if kind == "zero":
        return torch.zeros(n)
    if kind == "tiny_next_to_huge":
        w = torch.full((n,), 1e-6)
        w[torch.randperm(n, generator=g)[: max(1, n // 64)]] = 1e4
        return w
    raise ValueError(kind)


WEIGHT_KINDS = ("rand", "zero", "tiny_next_to_huge")

# Binary sizes. rocPRIM's radix sort runs in a single block up to 256 * 4 = 1024
# items, as block sort + merge levels up to 2^20 and as Onesweep above; its scans
# run in a single block up to block size * items per thread (4096 at the most
# for the int and double scans here) and with a look-back chain above.
#   255 / 256 / 257     one block of the element kernels (256 threads)
#   1023 / 1024 / 1025  the last single-block sort and the first merge sort
#   4095 / 4096 / 4097  past every single-block scan
#   2^17 + 3            many blocks of every stage, merge levels, odd tail
#   2^20 + 1            the first Onesweep sort
BINARY_SIZES = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
BINARY_LARGE = (2 ** 17 + 3, 2 ** 20 + 1)


def binary_cases() -> List[Tuple[str, str, int, str]]:
    """(id, family, n, target kind): every size on quantised scores, every family
    at two sizes around the block and the single-block sort, every target kind."""
    out = [(f"n{n}-quant50-random", "quant50", n, "random") for n in BINARY_SIZES]
    for n in (257, 1025):
        out += [(f"n{n}-{f}-random", f, n, "random") for f in FAMILIES if f != "quant50"]
    out += [(f"n257-quant50-{k}", "quant50", 257, k) for k in TARGET_KINDS if k != "random"]
    out += [("n3-zeros_denormals-one_pos_best", "zeros_denormals", 3, "one_pos_best"),
            ("n2-infs-random", "infs", 2, "random")]
    return out


@functools.lru_cache(maxsize=None)
def binary_case(family: str, n: int, kind: str):
    """(scores, target, pos_label, (fps, tps, thr) of the oracle), built once."""
    s = scores(family, n, seed=n % 1000)
    t, pos_label = targets(kind, s, seed=n % 1000)
    return s, t, pos_label, oracle.curve(s.numpy(), t.numpy(), pos_label)


# ------------------------------------------------------------------ batched
BATCHED_SHAPES = ((1, 1), (1, 7), (2, 300), (257, 3), (64, 65), (5000, 9), (5, 255), (5, 256), (5, 257))
BATCHED_LARGE = (2 ** 17 + 3, 2)


@functools.lru_cache(maxsize=None)
def batched_case(B: int, C: int):
    """(probs (B, C) float32, multiclass target (B,), multilabel target (B, C)).

    Columns cycle through the score families; then, where there is room: column
    1 repeats column 0 (equal scores in different classes must not merge), the
    last column is constant, class 2 has no positive row, and every row belongs
    to label 0 (multiclass C = 1 gives the same for class 0). Every fourth
    multiclass row has target -1: a negative for every class."""
    g = _gen(1000 * B + C)
    fams = ("quant50", "zeros_denormals", "two_values", "neighbours", "bf16", "infs", "distinct", "equal")
    probs = torch.stack([scores(fams[c % len(fams)], B, seed=c) for c in range(C)], dim=1)
    if C > 1:
        probs[:, 1] = probs[:, 0]
    probs[:, C - 1] = 0.625
    mc = torch.randint(0, C, (B,), generator=g)
    ml = torch.randint(0, 2, (B, C), generator=g)
    if C > 2:
        mc[mc == 2] = 0
        ml[:, 2] = 0
    ml[:, 0] = 1
    mc[3::4] = -1
    return probs.contiguous(), mc, ml.contiguous()


# ---------------------------------------------------------------------- NaN
# (id, scores, targets, expected fps, expected tps, expected thresholds) with
# pos_label 1. Every NaN sorts in front, whatever its sign, and is a threshold
# of its own; the finite part follows as the definition gives it (the rows
# behind the NaNs all count as "score >= t"). This is what the CPU path does:
# torch.argsort(descending=True) puts NaN first and a NaN differs from its
# neighbour. Rows with NaN share one target value within a case, so that the
# order among them cannot matter.
NAN_CASES = (
    ("one_nan", [0.5, NAN, 0.25, 0.5], [1, 1, 0, 0], [0, 1, 2], [1, 2, 2], [NAN, 0.5, 0.25]),
    ("same_nan_three_times", [NAN, 0.5, NAN, 0.25, NAN], [0, 1, 0, 1, 0], [1, 2, 3, 3, 3], [0, 0, 0, 1, 2],
     [NAN, NAN, NAN, 0.5, 0.25]),
    ("negative_nan", [0.5, NEG_NAN, 0.25, 0.5], [1, 1, 0, 0], [0, 1, 2], [1, 2, 2], [NAN, 0.5, 0.25]),
    ("both_signs", [NEG_NAN, 0.75, NAN], [1, 0, 1], [0, 0, 1], [1, 2, 2], [NAN, NAN, 0.75]),
    ("only_a_nan", [NAN], [1], [0], [1], [NAN]),
)


def same_floats(a, b) -> bool:
    """Float ==, elementwise over equal shapes, with NaN equal to NaN (any sign,
    any payload) and +0.0 equal to -0.0. Never bitwise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def as_f64(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def same_curve(got, want) -> bool:
    """(fps, tps, thresholds): counts exactly, thresholds float-equal."""
    return len(got) == len(want) and all(same_floats(as_f64(g), as_f64(w)) for g, w in zip(got, want))


# ------------------------------------------------------------------- public
@functools.lru_cache(maxsize=None)
def public_case(name: str):
    """(scores (N, 5) float32 in [0, 1], multiclass target, multilabel target)."""
    if name == "families_300x5":
        fams = ("quant50", "zeros_denormals", "neighbours", "bf16", "two_values")
        p = torch.stack([scores(f, 300, seed=40 + i) for i, f in enumerate(fams)], dim=1).abs().clamp(0, 1)
        p[::7, 1] = -0.0  # abs() above removed the negative zero: plant it next to +0.0 again
        p[1::7, 1] = 0.0
        g = _gen(77)
        return p.contiguous(), torch.randint(0, 5, (300,), generator=g), torch.randint(0, 2, (300, 5), generator=g)
    if name == "planted_6x5":
        # column 0: both zeros tied across a positive and a negative; column 1:
        # all equal; column 2: no positive (multiclass and multilabel); column 3:
        # every multilabel row positive; column 4: distinct
        p = torch.tensor([[0.0, 0.5, 0.1, 0.9, 0.1],
                          [-0.0, 0.5, 0.7, 0.2, 0.2],
                          [0.5, 0.5, 0.3, 0.2, 0.3],
                          [-0.0, 0.5, 0.7, 0.4, 0.4],
                          [0.0, 0.5, 0.2, 0.9, 0.6],
                          [1.0, 0.5, 0.1, 0.1, 0.5]], dtype=torch.float32)
        mc = torch.tensor([0, 1, 4, 3, 0, 1])
        ml = torch.tensor([[1, 0, 0, 1, 1], [0, 1, 0, 1, 0], [1, 1, 0, 1, 0], [1, 0, 0, 1, 1], [0, 0, 0, 1, 1],
                           [1, 1, 0, 1, 0]])
        return p, mc, ml
    raise ValueError(name)


PUBLIC_CASES = ("families_300x5", "planted_6x5")
PUBLIC_CLASSES = {"roc": "ROC", "precision_recall_curve": "PrecisionRecallCurve", "auroc": "AUROC",
                  "average_precision": "AveragePrecision"}


def column_curves(p, target, multilabel: bool, ignore_index=None):
    """The oracle's (fps, tps, thresholds) of every column of ``p`` (N, C)."""
    out = []
    for c in range(p.shape[1]):
        tc = target[:, c] if multilabel else target
        keep = torch.ones_like(tc, dtype=torch.bool) if ignore_index is None else tc != ignore_index
        out.append(oracle.curve(p[keep, c].double().numpy(), tc[keep].numpy(), 1 if multilabel else c))
    return out


def _average(per_class, average, support):
    """``_reduce_auroc`` / ``_reduce_average_precision`` in fp64: NaN classes are left out."""
    per_class = np.asarray(per_class, np.float64)
    if average == "none":
        return per_class
    ok = ~np.isnan(per_class)
    if average == "macro":
        return per_class[ok].mean()
    return (per_class[ok] * support[ok] / support[ok].sum()).sum()


@functools.lru_cache(maxsize=None)
def public_checks(name: str):
    """Every public check of one case: (task, functional stem, args, kwargs,
    "curve" | "area", expected). A curve's expected value is a list per class of
    (x, y, thresholds), an area's a float or a per-class array."""
    p, mc, ml = public_case(name)
    kw = {"thresholds": None}
    s, t = p[:, 0].contiguous(), ml[:, 0].contiguous()
    cur = oracle.curve(s.numpy(), t.numpy())
    out = [("binary", "roc", (s, t), kw, "curve", [oracle.roc(*cur)]),
           ("binary", "precision_recall_curve", (s, t), kw, "curve", [oracle.precision_recall(*cur)]),
           ("binary", "auroc", (s, t), kw, "area", oracle.auroc(*cur)),
           ("binary", "auroc", (s, t), {"max_fpr": 0.5, **kw}, "area", oracle.auroc(*cur, max_fpr=0.5)),
           ("binary", "average_precision", (s, t), kw, "area", oracle.average_precision(*cur))]
    for task, target, size in (("multiclass", mc, "num_classes"), ("multilabel", ml, "num_labels")):
        multilabel = task == "multilabel"
        curves = column_curves(p, target, multilabel)
        support = np.array([float((target[:, c] == 1).sum() if multilabel else (target == c).sum()) for c in range(5)])
        kw = {size: 5, "thresholds": None}
        out.append((task, "roc", (p, target), kw, "curve", [oracle.roc(*c) for c in curves]))
        out.append((task, "precision_recall_curve", (p, target), kw, "curve",
                    [oracle.precision_recall(*c) for c in curves]))
        for average in ("none", "macro", "weighted"):
            out.append((task, "auroc", (p, target), {"average": average, **kw}, "area",
                        _average([oracle.auroc(*c) for c in curves], average, support)))
            out.append((task, "average_precision", (p, target), {"average": average, **kw}, "area",
                        _average([oracle.average_precision(*c) for c in curves], average, support)))
    return out


def check_curves(got, wants, what) -> None:
    """got: (x, y, thresholds), each a list per class (or one tensor, binary);
    every x and y within RATIO_ULPS fp32 ulps of the fp64 ratio, NaN where it is
    NaN, thresholds float-equal. ``Metric.compute`` squeezes a one-element
    tensor to 0-d, as the reference's does: a one-point curve is read as (1,)."""
    if isinstance(got[0], torch.Tensor) and len(wants) == 1 and got[0].ndim <= 1:
        got = [[g] for g in got]
    assert len(got[0]) == len(wants), what
    for c, want in enumerate(wants):
        for k in (0, 1):
            g = np.atleast_1d(as_f64(got[k][c]))
            assert g.shape == want[k].shape, (what, c, k)
            u = oracle.ulps32(g, want[k])
            assert np.all((np.isnan(g) & np.isnan(want[k])) | (u <= RATIO_ULPS)), (what, c, k, np.nanmax(u))
        assert same_floats(np.atleast_1d(as_f64(got[2][c])), want[2]), (what, c)


def area_error(got, want) -> float:
    """Largest |got - want|; inf where the shapes or the NaN positions differ."""
    got, want = as_f64(got), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    err = np.abs(got - want)[~np.isnan(want)]
    return float(err.max()) if err.size else 0.0


def ulp_apart_fp64():
    """fp64 scores one fp64 ulp apart (one fp32 value, three fp64 values) and
    their targets: three thresholds in fp64, one after a cast to fp32."""
    mid = np.float64(0.3)
    s = np.array([mid, np.nextafter(mid, 1.0), np.nextafter(mid, 0.0), 0.75, mid, 0.125], dtype=np.float64)
    t = np.array([1, 0, 1, 0, 0, 1])
    return torch.from_numpy(s), torch.from_numpy(t)
