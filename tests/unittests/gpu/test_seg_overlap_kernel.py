"""The overlap kernels (csrc/seg_overlap.hip) against numpy from the definition:
for label maps a bincount per sample over the labels inside [0, C), and over the
labels where both sides agree; for planes Python-int sums of p * t, p and t. The
three counts must match EXACTLY.

The public functions on the GPU must equal the switched-off path bit for bit
(same integers, same torch tail) and lie within a relative 4 * 2**-24 of the CPU
path: the tail is one fp32 division, for the averaged forms also a product and a
sum over C = 5 terms of one sign. Measured on these inputs, the CPU path lies at
most 2.9 units of 2**-24 from an fp64 evaluation of the same formulas
(generalized dice, simple weights), so the 4 units stand.
"""
import numpy as np
import pytest
import torch

import metrics_amd as ma
from metrics_amd.functional.segmentation import dice_score, generalized_dice_score, mean_iou
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
CHUNK, SMALL_S, ROUNDS, WAVES, MAX_C, MAX_GRID = (
    _hip.SEG_OVERLAP_CHUNK, _hip.SEG_OVERLAP_SMALL_S, _hip.SEG_OVERLAP_ROUNDS, _hip.SEG_OVERLAP_WAVES,
    _hip.SEG_OVERLAP_MAX_C, _hip.SEG_OVERLAP_MAX_GRID)
RTOL = 4 * 2.0**-24


def _label_oracle(p, t, C):
    """p, t: (N, S) int64 arrays. (3, N, C) int64."""
    N = len(p)
    row = np.arange(N)[:, None] * C

    def count(x, keep):
        return np.bincount((row + x)[keep], minlength=N * C).reshape(N, C)

    p_in, t_in = (p >= 0) & (p < C), (t >= 0) & (t < C)
    return np.stack([count(p, p_in & (p == t)), count(p, p_in), count(t, t_in)])


def _plane_oracle(p, t):
    """p, t: (N, C, S) integer arrays. (3, N, C) int64 from Python-int sums."""
    p, t = p.astype(object), t.astype(object)
    return np.stack([(p * t).sum(-1), p.sum(-1), t.sum(-1)]).astype(np.int64)


def _planes(labels, C):
    return (labels[:, None, :] == np.arange(C)[None, :, None]).astype(np.int64)


def _labels(pattern, N, S, C, rng):
    """Two (N, S) int64 label maps that agree on about two elements in three."""
    i = np.arange(N * S)
    if pattern == "const":
        p = np.full(N * S, C - 1)
    elif pattern == "runs":  # blobs: runs of 37, too long for a wave to see many labels
        p = np.repeat(rng.integers(0, C, N * S // 37 + 1), 37)[: N * S]
    elif pattern == "random":  # per pixel: the LDS-atomic fall-through
        p = rng.integers(0, C, N * S)
    else:  # ("stripes", width, k): a wave's slot holds exactly k labels when width is its vector
        p = (i // pattern[1]) % pattern[2]
    t = np.where(i % 3 == 0, (p + 1) % C, p)
    return p.reshape(N, S), t.reshape(N, S)


def _run(p, t, C, fmt, dp, dt, expect):
    calls = _hip.seg_overlap_kernel_calls()
    got = _hip.seg_overlap(torch.from_numpy(p).to("cuda", dp), torch.from_numpy(t).to("cuda", dt), C, fmt)
    assert _hip.seg_overlap_kernel_calls() == calls + 1
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(expect))


VEC_SPAN = 64 * 2  # int64 elements of one 16-byte load per lane of a wave
LABEL_CASES = [(3, S, 3, "runs", I64, I64) for S in (
    1, 63, 64, 65, VEC_SPAN - 1, VEC_SPAN, VEC_SPAN + 1, SMALL_S - 1, SMALL_S, SMALL_S + 1,
    CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)]
LABEL_CASES += [(3, S, 3, "runs", dt, dt) for dt in (U8, I32) for S in (17, SMALL_S - 1, CHUNK + 1)]
LABEL_CASES += [(2, S, C, "random", I64, I64) for C in (1, 2, 19, MAX_C) for S in (300, CHUNK + 77)]
LABEL_CASES += [(2, CHUNK + 5, 7, pat, I64, I32) for pat in ("const", "runs", "random")]
LABEL_CASES += [(2, S, 6, ("stripes", w, k), dt, dt) for dt, w in ((I64, 2), (I32, 4), (U8, 16), (I64, 1))
                for k in (ROUNDS, ROUNDS + 1) for S in (SMALL_S - 3, CHUNK + 3)]
# the wave mapping: samples around a block's worth, and enough to wrap the capped grid
LABEL_CASES += [(N, 33, 4, "runs", U8, I64) for N in (1, WAVES - 1, WAVES, WAVES + 1, WAVES * MAX_GRID + 1)]


@pytest.mark.parametrize("N,S,C,pattern,dp,dt", LABEL_CASES)
def test_label_maps(N, S, C, pattern, dp, dt):
    p, t = _labels(pattern, N, S, C, np.random.default_rng(S + C))
    _run(p, t, C, "index", dp, dt, _label_oracle(p, t, C))


@pytest.mark.parametrize("S,dtype,planted", [(SMALL_S - 5, I64, (-1, 5, 255)), (CHUNK + 9, I32, (-1, 5, 255)),
                                             (CHUNK + 9, U8, (5, 255))])
def test_labels_out_of_range_are_counted_nowhere(S, dtype, planted):
    rng = np.random.default_rng(S)
    p, t = _labels("runs", 2, S, 5, rng)
    for x in (p, t):
        x.reshape(-1)[rng.integers(0, x.size, 200)] = rng.choice(planted, 200)
    t[0, :7], p[0, :7] = 255, 255  # equal on both sides and still no intersection
    _run(p, t, 5, "index", dtype, dtype, _label_oracle(p, t, 5))


def test_counts_past_32_bits():
    """(1, 2^31 + 64) constant uint8 labels: the 64-bit flush and element offsets past 2^31."""
    S = 2**31 + 64
    p = torch.full((1, S), 1, dtype=U8, device="cuda")
    got = _hip.seg_overlap(p, p, 2, "index")
    assert got.tolist() == [[[0, S]]] * 3


def _plane_case(name):
    rng = np.random.default_rng(len(name))
    if name == "bool-i64":
        return rng.integers(0, 2, (2, 3, 1001)), rng.integers(0, 2, (2, 3, 1001)), torch.bool, I64
    if name == "u8-binary":
        return rng.integers(0, 2, (2, 3, CHUNK + 5)), rng.integers(0, 2, (2, 3, CHUNK + 5)), U8, U8
    if name == "u8-255":  # 255 * 255 * 70000 > 2^32: no 32-bit partial sum may hold it
        return np.full((1, 1, 70000), 255), np.full((1, 1, 70000), 255), U8, U8
    if name == "i64-0to3":
        return rng.integers(0, 4, (2, 3, CHUNK + 5)), rng.integers(0, 4, (2, 3, CHUNK + 5)), I64, I64
    S = int(name.split("-")[1])  # "bool-S"
    return rng.integers(0, 2, (2, 3, S)), rng.integers(0, 2, (2, 3, S)), torch.bool, torch.bool


@pytest.mark.parametrize("name", ["bool-15", "bool-16", "bool-17", f"bool-{CHUNK + 17}", "u8-binary", "u8-255",
                                  "i64-0to3", "bool-i64"])
def test_planes(name):
    p, t, dp, dt = _plane_case(name)
    _run(p, t, p.shape[1], "one-hot", dp, dt, _plane_oracle(p, t))


@pytest.mark.parametrize("planes_first", [True, False])
@pytest.mark.parametrize("dl,dpl", [(I64, torch.bool), (U8, U8), (I32, I64)])
def test_mixed(planes_first, dl, dpl):
    p, t = _labels("runs", 2, CHUNK + 11, 4, np.random.default_rng(3))
    t[t == 2] = 0  # class 2 is absent from one side
    expect = _label_oracle(p, t, 4)
    if planes_first:
        _run(_planes(p, 4), t, 4, "mixed", dpl, dl, expect)
    else:
        _run(p, _planes(t, 4), 4, "mixed", dl, dpl, expect)


def test_views_and_spatial_ranks():
    rng = np.random.default_rng(5)
    p, t = rng.integers(0, 4, (2, 5, 6, 7)), rng.integers(0, 4, (2, 5, 6, 7))
    expect = torch.from_numpy(_label_oracle(p.reshape(2, -1), t.reshape(2, -1), 4))
    dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    assert torch.equal(_hip.seg_overlap(dp, dt, 4, "index").cpu(), expect)  # 3-D volumes
    assert torch.equal(_hip.seg_overlap(dp.flatten(1), dt.flatten(1), 4, "index").cpu(), expect)  # 1-D
    swapped = _hip.seg_overlap(dp.transpose(1, 3), dt.transpose(1, 3), 4, "index")  # not contiguous
    assert torch.equal(swapped.cpu(), expect)
    # a contiguous view that starts 8 bytes off its partner's alignment: the all-scalar run
    off = torch.from_numpy(np.concatenate([[0], p.reshape(-1)])).cuda()[1:].view(2, -1)
    assert off.is_contiguous() and off.data_ptr() % 16 != dt.data_ptr() % 16
    assert torch.equal(_hip.seg_overlap(off, dt.flatten(1), 4, "index").cpu(), expect)


def _public_inputs():
    p, t = _labels("runs", 3, 40 * 50, 5, np.random.default_rng(11))
    t[1][t[1] == 3] = 0  # an absent class: the zero-division branches of the tails
    return torch.from_numpy(p).view(3, 40, 50), torch.from_numpy(t).view(3, 40, 50)


FUNCTIONALS = [(mean_iou, {"per_class": v}) for v in (True, False)]
FUNCTIONALS += [(dice_score, {"average": v}) for v in ("micro", "macro", "weighted", "none")]
FUNCTIONALS += [(generalized_dice_score, {"weight_type": v}) for v in ("square", "simple", "linear")]


@pytest.mark.parametrize("C,include_background", [(5, True), (5, False), (1, False)])
@pytest.mark.parametrize("fn,kwargs", FUNCTIONALS, ids=lambda v: getattr(v, "__name__", None) or "-".join(map(str, v.values())))
def test_functionals(fn, kwargs, C, include_background, monkeypatch):
    p, t = _public_inputs()
    if C == 1:
        p, t = torch.zeros_like(p), torch.zeros_like(t)
    kwargs = dict(kwargs, num_classes=C, include_background=include_background, input_format="index")
    calls = _hip.seg_overlap_kernel_calls()
    got = fn(p.cuda(), t.cuda(), **kwargs)
    assert _hip.seg_overlap_kernel_calls() == calls + 1
    torch.testing.assert_close(got.cpu(), fn(p, t, **kwargs), rtol=RTOL, atol=0, equal_nan=True)
    monkeypatch.setenv(_hip.SEG_OVERLAP_KERNEL_ENV, "0")
    off = fn(p.cuda(), t.cuda(), **kwargs)
    assert _hip.seg_overlap_kernel_calls() == calls + 1
    assert got.dtype == off.dtype and torch.equal(got.isnan(), off.isnan()) and torch.equal(got.nan_to_num(), off.nan_to_num())


@pytest.mark.parametrize("cls,kwargs", [(ma.segmentation.MeanIoU, {"per_class": True}),
                                        (ma.segmentation.DiceScore, {"average": "macro"}),
                                        (ma.segmentation.GeneralizedDiceScore, {"weight_type": "simple"})])
def test_modular_over_two_updates(cls, kwargs, monkeypatch):
    p, t = _public_inputs()

    def run(device):
        m = cls(num_classes=5, input_format="index", **kwargs).to(device)
        m.update(p[:2].to(device), t[:2].to(device))
        m.update(p[2:].to(device), t[2:].to(device))
        return m.compute().cpu()

    calls = _hip.seg_overlap_kernel_calls()
    got = run("cuda")
    assert _hip.seg_overlap_kernel_calls() == calls + 2
    torch.testing.assert_close(got, run("cpu"), rtol=RTOL, atol=0, equal_nan=True)
    monkeypatch.setenv(_hip.SEG_OVERLAP_KERNEL_ENV, "0")
    assert torch.equal(got.nan_to_num(), run("cuda").nan_to_num())


def test_dispatch(monkeypatch):
    p, t = (x.cuda() for x in _public_inputs())
    calls = _hip.seg_overlap_kernel_calls()
    hot = torch.nn.functional.one_hot(p, 5).movedim(-1, 1)
    assert _hip.seg_overlap(p.cpu(), t.cpu(), 5, "index") is None
    assert _hip.seg_overlap(hot.float(), hot.float(), 5, "one-hot") is None
    assert _hip.seg_overlap(hot, t, 4, "mixed") is None and _hip.seg_overlap(p, t, 5, "mixed") is None
    assert _hip.seg_overlap(p, t[:, :-1], 5, "index") is None
    big = torch.full((1, 8), MAX_C, device="cuda")  # one class too many: the torch chain serves it
    assert _hip.seg_overlap(big, big, MAX_C + 1, "index") is None
    assert mean_iou(big, big, MAX_C + 1, per_class=True, input_format="index")[0, MAX_C] == 1
    assert mean_iou(hot.float(), hot.float(), 5).shape == (3,)
    assert _hip.seg_overlap_kernel_calls() == calls
    with monkeypatch.context() as m:
        m.setenv(_hip.SEG_OVERLAP_KERNEL_ENV, "0")
        assert _hip.seg_overlap(p, t, 5, "index") is None
    assert _hip.seg_overlap_kernel_calls() == calls


def test_no_host_sync():
    p, t = (x.cuda() for x in _public_inputs())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _hip.seg_overlap(p, t, 5, "index")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got.shape == (3, 3, 5)
