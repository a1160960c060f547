"""Independent oracle for the threshold-curve confusion matrices.

Plain torch on CPU, no ``metrics_amd.ops`` call anywhere. Scores are float32
values (bf16 upcasts exactly) and thresholds are float32; both are cast to
float64, which represents every float32 exactly, so ``score >= thr`` decides
exactly what the float32 comparison decides. A NaN score compares false at
every threshold: it counts as predicted negative.

``confmat[t] = [[tn, fp], [fn, tp]]`` — layout ``[t][target][pred]``, the
metric state layout. Binary gives (T, 2, 2); multiclass one-vs-rest and
multilabel give (T, C, 2, 2).

The ``*_interval`` variants serve inputs the kernels normalise in float32
(softmax / sigmoid of logits): a score within a relative band ``eps`` of a
threshold may legitimately fall on either side. Per cell they return the count
that is certain and the count that is ambiguous; a correct kernel's count lies
in ``[certain, certain + ambiguous]``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch
from torch import Tensor

_FLT_MIN = 2.0 ** -126
_DENORM_MIN = 2.0 ** -149


def _f64(x: Tensor) -> Tensor:
    assert x.dtype in (torch.float32, torch.bfloat16, torch.float64), x.dtype
    return x.detach().cpu().to(torch.float64)


def _cells(pred: Tensor, label: Tensor, keep: Tensor, weight: Optional[Tensor] = None) -> Tensor:
    """pred (N, T) bool, label/keep (N,) bool -> (T, 2, 2) counts; ``weight`` (N,) int64
    counts how many identical samples a row stands for."""
    label = label.reshape(-1, 1)
    keep = keep.reshape(-1, 1)
    w = torch.ones_like(label, dtype=torch.long) if weight is None else weight.reshape(-1, 1)
    tp = ((pred & label & keep) * w).sum(0)
    fp = ((pred & ~label & keep) * w).sum(0)
    fn = ((~pred & label & keep) * w).sum(0)
    tn = ((~pred & ~label & keep) * w).sum(0)
    return torch.stack([torch.stack([tn, fp], -1), torch.stack([fn, tp], -1)], -2)


def binary_confmat(scores: Tensor, target: Tensor, thr: Tensor, ignore_index: Optional[int] = None,
                   dedupe: Optional[bool] = None) -> Tensor:
    """``dedupe`` (default: above 65536 samples) folds identical (score bits, target)
    pairs into one weighted row first — the same comparison, made once per distinct pair."""
    s32, t, th = scores.detach().cpu().float().flatten(), target.detach().cpu().flatten().long(), _f64(thr)
    weight = None
    if dedupe if dedupe is not None else s32.numel() > 65536:
        # one int64 key per (score bit pattern, target): NaN and -0.0 stay themselves
        assert int(t.min()) >= -128 and int(t.max()) < 128
        key = (s32.contiguous().view(torch.int32).long() & 0xFFFFFFFF) * 256 + (t + 128)
        uniq, weight = torch.unique(key, return_counts=True)
        bits = uniq // 256
        s32 = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)
        t = uniq % 256 - 128
    s = s32.to(torch.float64)
    keep = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != ignore_index
    return _cells(s[:, None] >= th[None, :], t == 1, keep, weight)


def multiclass_confmat(scores: Tensor, target: Tensor, thr: Tensor, ignore_index: Optional[int] = None) -> Tensor:
    """One-vs-rest: label of (row, c) is target[row] == c; an ignored row drops all its C elements."""
    s, t, th = _f64(scores), target.detach().cpu(), _f64(thr)
    B, C = s.shape
    keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else t != ignore_index
    out = []
    for c in range(C):
        out.append(_cells(s[:, c, None] >= th[None, :], t == c, keep))
    return torch.stack(out, 1)  # (T, C, 2, 2)


def multilabel_confmat(scores: Tensor, target: Tensor, thr: Tensor, ignore_index: Optional[int] = None) -> Tensor:
    """target (B, C) of 0/1; an element equal to ignore_index drops that element alone."""
    s, t, th = _f64(scores), target.detach().cpu(), _f64(thr)
    B, C = s.shape
    out = []
    for c in range(C):
        keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else t[:, c] != ignore_index
        out.append(_cells(s[:, c, None] >= th[None, :], t[:, c] == 1, keep))
    return torch.stack(out, 1)


# ---------------------------------------------------------------- interval
def _interval_cells(s: Tensor, label: Tensor, keep: Tensor, th: Tensor, eps: float) -> Tuple[Tensor, Tensor]:
    """s (N,) float64. Returns (certain, ambiguous), each (T, 2, 2)."""
    band = eps * th.abs()
    hi = s[:, None] >= (th + band)[None, :]  # positive whatever the rounding
    lo = s[:, None] < (th - band)[None, :]  # negative whatever the rounding
    nan = torch.isnan(s)[:, None]
    lo = lo | nan  # NaN: negative, and certain
    amb = ~(hi | lo)
    label = label.reshape(-1, 1)
    keep = keep.reshape(-1, 1)
    tp = (hi & label & keep).sum(0)
    fp = (hi & ~label & keep).sum(0)
    fn = (lo & label & keep).sum(0)
    tn = (lo & ~label & keep).sum(0)
    a1 = (amb & label & keep).sum(0)  # either fn or tp
    a0 = (amb & ~label & keep).sum(0)  # either tn or fp
    certain = torch.stack([torch.stack([tn, fp], -1), torch.stack([fn, tp], -1)], -2)
    ambiguous = torch.stack([torch.stack([a0, a0], -1), torch.stack([a1, a1], -1)], -2)
    return certain, ambiguous


def binary_confmat_interval(scores, target, thr, eps: float, ignore_index: Optional[int] = None):
    s = scores.detach().cpu().to(torch.float64).flatten()
    t, th = target.detach().cpu().flatten(), _f64(thr)
    keep = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != ignore_index
    return _interval_cells(s, t == 1, keep, th, eps)


def multiclass_confmat_interval(scores, target, thr, eps: float, ignore_index: Optional[int] = None):
    s = scores.detach().cpu().to(torch.float64)
    t, th = target.detach().cpu(), _f64(thr)
    B, C = s.shape
    keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else t != ignore_index
    cs, As = zip(*[_interval_cells(s[:, c], t == c, keep, th, eps) for c in range(C)])
    return torch.stack(cs, 1), torch.stack(As, 1)


def multilabel_confmat_interval(scores, target, thr, eps: float, ignore_index: Optional[int] = None):
    s = scores.detach().cpu().to(torch.float64)
    t, th = target.detach().cpu(), _f64(thr)
    B, C = s.shape
    cs, As = [], []
    for c in range(C):
        keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else t[:, c] != ignore_index
        ce, am = _interval_cells(s[:, c], t[:, c] == 1, keep, th, eps)
        cs.append(ce)
        As.append(am)
    return torch.stack(cs, 1), torch.stack(As, 1)


def assert_within(got: Tensor, certain: Tensor, ambiguous: Tensor) -> None:
    got = got.detach().cpu()
    bad = (got < certain) | (got > certain + ambiguous)
    assert not bool(bad.any()), (
        f"{int(bad.sum())} cells outside [certain, certain+ambiguous]; first at "
        f"{bad.nonzero()[0].tolist()}: got {int(got[bad][0])}, certain {int(certain[bad][0])}, "
        f"ambiguous {int(ambiguous[bad][0])}"
    )


# ------------------------------------------------------------- value pools
def _nextafter32(x: Tensor, toward: float) -> Tensor:
    return torch.nextafter(x.float(), torch.full_like(x.float(), toward))


def _bf16_round_both(x: Tensor) -> Tensor:
    """Every float32 in x rounded to bf16 downwards and upwards (by magnitude bits)."""
    bits = x.float().contiguous().view(torch.int32)
    down = (bits & ~0xFFFF).view(torch.float32)  # truncation: toward zero, x >= 0 here
    up = torch.where((bits & 0xFFFF) != 0, (bits & ~0xFFFF) + 0x10000, bits).view(torch.float32)
    return torch.cat([down, up])


def _bf16_neighbours(x: Tensor) -> Tensor:
    """bf16 predecessor and successor of each bf16-representable value in x (x >= 0)."""
    bits = x.float().contiguous().view(torch.int32)
    return torch.cat([(bits - 0x10000).clamp(min=0).view(torch.float32), (bits + 0x10000).view(torch.float32)])


def value_pool(thr: Tensor, dtype: torch.dtype = torch.float32) -> Tensor:
    """Adversarial scores for the threshold tensor ``thr``: every threshold, its
    neighbours on either side, signed zeros, 1, the float below 1, the smallest
    denormal and FLT_MIN — clipped to [0, 1]. The bf16 flavour holds each
    threshold rounded to bf16 in both directions plus the bf16 neighbours."""
    thr = thr.detach().cpu().float().flatten()
    fixed = torch.tensor([0.0, -0.0, 1.0, math.nextafter(1.0, 0.0), _DENORM_MIN, _FLT_MIN], dtype=torch.float64).float()
    fixed[3] = _nextafter32(torch.ones(1), 0.0)[0]
    if dtype == torch.float32:
        vals = torch.cat([thr, _nextafter32(thr, math.inf), _nextafter32(thr, -math.inf), fixed])
    else:
        assert dtype == torch.bfloat16
        r = _bf16_round_both(thr.clamp(0.0, 1.0))
        below_one = torch.tensor([1.0 - 2.0 ** -8])  # bf16 predecessor of 1
        vals = torch.cat([r, _bf16_neighbours(r), fixed[:3], below_one,
                          _bf16_round_both(fixed[4:]).clamp(min=0.0)])
    vals = vals.clamp(0.0, 1.0)  # keeps -0.0 (clamp returns the input when it compares equal)
    out = vals.to(dtype)
    assert torch.equal(out.float(), vals) or dtype == torch.bfloat16
    return out


def binary_layout(pool: Tensor, n: int) -> Tuple[Tensor, Tensor]:
    """n scores cycling through the pool; sample i has label (i // len(pool)) % 2,
    so with n >= 2 * len(pool) every value appears with label 0 and with label 1."""
    P = pool.numel()
    i = torch.arange(n)
    return pool[i % P].clone(), ((i // P) % 2).long()


def matrix_layout(pool: Tensor, B: int, C: int) -> Tuple[Tensor, Tensor]:
    """(B, C) scores and 0/1 labels. Element e = row * C + c takes slot
    (e * stride) % M with M >= 2P the first modulus coprime to C: slot s < 2P holds
    value pool[s % P] with label s // P, the few slots from 2P on repeat the first
    pool values with label 0. The stride is coprime to C and to M, so any M
    consecutive elements meet every (value, label) pair, and (M coprime to C) each
    pair visits every column, hence different lanes and rows."""
    P = pool.numel()
    M = next(m for m in range(2 * P, 2 * P + 10 ** 4) if math.gcd(m, C) == 1)
    # a stride near M / golden ratio spreads even one row's C elements over the whole pool
    stride = next(s for s in range(max(int(M * 0.618), C + 1), 10 ** 6) if math.gcd(s, C) == 1 and math.gcd(s, M) == 1)
    slot = (torch.arange(B * C) * stride) % M
    label = torch.where(slot < 2 * P, slot // P, torch.zeros_like(slot))
    return pool[slot % P].reshape(B, C).clone(), label.reshape(B, C).long()


UNIFORM_T = (1, 2, 5, 64, 65, 200)
NONUNIFORM = (0.05, 0.05, 0.2, 0.35, 0.35, 0.35, 0.6, 0.95)  # duplicates, first > 0, last < 1


def threshold_specs() -> dict:
    """name -> float32 threshold tensor: the uniform grids and the non-uniform list."""
    specs = {f"lin{T}": torch.linspace(0, 1, T) for T in UNIFORM_T}
    specs["list"] = torch.tensor(NONUNIFORM)
    return specs


def coverage(scores: Tensor, labels: Tensor, pool: Tensor) -> List[bool]:
    """[every pool value met with label 0, every pool value met with label 1] (by bit pattern)."""
    def bits(x):
        x = x.float().contiguous().view(torch.int32)
        return x

    pb = set(bits(pool).tolist())
    out = []
    for lab in (0, 1):
        seen = set(bits(scores.flatten()[labels.flatten() == lab]).tolist())
        out.append(pb <= seen)
    return out
