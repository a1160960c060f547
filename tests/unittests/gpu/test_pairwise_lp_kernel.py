"""The pairwise L_p kernel (csrc/pairwise_lp.hip) through the two public
functions against numpy fp64 from the definition, on the inputs as the kernel
sees them (already rounded to bf16 / fp16).

Bounds on |got - want| relative to want, u = 2**-24, for fp32 accumulation of D
non-negative terms in any order: (D + 2) u for p = 1, (D + 4) u for p = 2,
(D + 2p + 4) u for p = 3, 4; plus one output rounding (2**-8 bf16, 2**-11 fp16).
A reduced output: the same bound on the row sum plus (tiles + 1) u, and for the
16-bit dtypes one more output rounding (the elements are rounded before the
fold). Non-integer exponents go through powf: the kernel's largest relative
error must not exceed twice that of the switched-off torch chain on the same
case (measured pairs in docs/PARITY.md).
"""
import math

import numpy as np
import pytest
import torch

from metrics_amd.functional.pairwise import pairwise_manhattan_distance, pairwise_minkowski_distance
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

TN, TM, KC = _hip.PAIRWISE_TILE_N, _hip.PAIRWISE_TILE_M, _hip.PAIRWISE_CHUNK_K
U = 2.0**-24
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
OUT_ROUNDING = {F32: 0.0, BF16: 2.0**-8, F16: 2.0**-11}


def _randn(shape, seed, dtype=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to("cuda", dtype)


def _call(x, y, p, **kwargs):
    """p == "manhattan": that function; a number: minkowski of that order."""
    if p == "manhattan":
        return pairwise_manhattan_distance(x, y, **kwargs)
    return pairwise_minkowski_distance(x, y, exponent=p, **kwargs)


def _oracle(x, y, p, zero_diagonal, reduction=None):
    p = 1 if p == "manhattan" else p
    x, y = (t.detach().double().cpu().numpy() for t in (x, x if y is None else y))
    with np.errstate(invalid="ignore"):
        want = (np.abs(x[:, None, :] - y[None, :, :]) ** p).sum(-1) ** (1 / p)
    if zero_diagonal:
        np.fill_diagonal(want, 0)
    if reduction in ("sum", "mean"):
        want = want.sum(-1) / (want.shape[1] if reduction == "mean" else 1)
    return want


def _bound(p, D, M, dtype, reduction=None):
    p = 1 if p == "manhattan" else p
    rel = {1: D + 2, 2: D + 4}.get(p, D + 2 * p + 4) * U + OUT_ROUNDING[dtype]
    if reduction in ("sum", "mean"):
        rel += (math.ceil(M / TM) + 1) * U + OUT_ROUNDING[dtype]
    return rel


def _check(x, y, p, zero_diagonal=None, reduction=None):
    calls = _hip.pairwise_kernel_calls()
    got = _call(x, y, p, zero_diagonal=zero_diagonal, reduction=reduction)
    assert _hip.pairwise_kernel_calls() == calls + 1
    want = _oracle(x, y, p, (y is None) if zero_diagonal is None else zero_diagonal, reduction)
    assert got.dtype == x.dtype and got.shape == want.shape
    err = np.abs(got.double().cpu().numpy() - want)
    rel = _bound(p, x.shape[1], (x if y is None else y).shape[0], x.dtype, reduction)
    worst = (err / np.maximum(want, 1e-300)).max()
    print(f"p={p} {tuple(x.shape)} {x.dtype} {reduction}: worst {worst / U:.2f} u, bound {rel / U:.2f} u")
    assert (err <= rel * want).all()


# N and M around one and two tiles, crossed sparsely; D over the scalar and the
# vector loads, the chunk tail and an odd number of chunks
SHAPES = [(1, 1, 1), (TN - 1, TM + 1, 3), (TN, TM - 1, 4), (TN + 1, 1, 5), (2 * TN + 1, 2 * TM + 1, 8),
          (1, TM + 1, KC - 1), (TN - 1, 2 * TM + 1, KC), (TN + 1, TM - 1, KC + 1), (TN, 2 * TM + 1, 2 * KC + 3),
          (2 * TN + 1, TM - 1, KC + 1), (TN + 1, TM + 1, 2 * KC)]


@pytest.mark.parametrize("p", ["manhattan", 2])
@pytest.mark.parametrize("N,M,D", SHAPES)
def test_shapes(N, M, D, p):
    _check(_randn((N, D), N + D), _randn((M, D), M + D + 1), p)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("p", ["manhattan", 1, 2, 3, 4])
@pytest.mark.parametrize("N,M,D", [(TN + 1, TM + 1, 2 * KC + 3), (5, TM + 1, 8), (TN - 1, 3, 2 * KC)])
def test_exponents_and_dtypes(N, M, D, p, dtype):
    _check(_randn((N, D), 1, dtype), _randn((M, D), 2, dtype), p)


@pytest.mark.parametrize("p", [1.5, 0.5])
def test_non_integer_exponents_against_the_chain(p, monkeypatch):
    x, y = _randn((TN + 1, KC + 1), 3), _randn((TM + 1, KC + 1), 4)
    want = _oracle(x, y, p, False)
    calls = _hip.pairwise_kernel_calls()
    got = pairwise_minkowski_distance(x, y, exponent=p)
    assert _hip.pairwise_kernel_calls() == calls + 1
    monkeypatch.setenv(_hip.PAIRWISE_KERNEL_ENV, "0")
    chain = pairwise_minkowski_distance(x, y, exponent=p)
    assert _hip.pairwise_kernel_calls() == calls + 1
    e_kernel, e_chain = (np.abs(v.double().cpu().numpy() / want - 1).max() for v in (got, chain))
    print(f"p={p}: kernel {e_kernel / U:.2f} u, chain {e_chain / U:.2f} u")
    assert e_kernel <= 2 * e_chain


def test_views():
    N, M, D = TN + 1, 7, 2 * KC
    x, y = _randn((N, D), 5), _randn((M, D), 6)
    off = torch.cat([x.new_zeros(1), x.reshape(-1)])[1:].view(N, D)  # contiguous, 4 bytes off 16-byte alignment
    assert off.is_contiguous() and off.data_ptr() % 16 != 0 and y.data_ptr() % 16 == 0
    _check(off, y, 2)
    _check(y, off, "manhattan")
    transposed = x.T.contiguous().T
    assert not transposed.is_contiguous()
    _check(transposed, y, 3)


@pytest.mark.parametrize("N,M", [(2 * TN + 1, 5), (5, 2 * TM + 1)])
@pytest.mark.parametrize("p", ["manhattan", 3])
def test_zero_diagonal(N, M, p):
    x = _randn((N, 9), 7)
    _check(x, _randn((M, 9), 8), p, zero_diagonal=True)  # tall and wide: min(N, M) zeros
    _check(x, None, p)  # y = None: the same rows, the diagonal zeroed by default
    _check(x, None, p, zero_diagonal=False)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("reduction", [None, "sum", "mean"])
@pytest.mark.parametrize("M", [TM - 3, 2 * TM + 1])  # one and three column tiles
@pytest.mark.parametrize("p", ["manhattan", 2, 4])
def test_reductions(p, M, reduction, dtype):
    x, y = _randn((TN + 5, KC + 1), 9, dtype), _randn((M, KC + 1), 10, dtype)
    _check(x, y, p, reduction=reduction)
    _check(x, y, p, zero_diagonal=True, reduction=reduction)


@pytest.mark.parametrize("reduction", [None, "sum"])
@pytest.mark.parametrize("p", ["manhattan", 2, 3, 1.5])
def test_planted_values(p, reduction):
    x, y = _randn((TN + 2, KC + 3), 11), _randn((TM + 2, KC + 3), 12)
    y[TM] = x[3]  # an equal pair: exactly 0
    x[TN, 2] = math.inf  # inf along that row of the output,
    y[5, 2] = math.inf  # nan where both sides hold it
    y[9, 2] = -math.inf
    got = _call(x, y, p, reduction=reduction).cpu().numpy()
    want = _oracle(x, y, p, False, reduction).astype(np.float32)
    np.testing.assert_array_equal(got[TN], want[TN])  # nan == nan here
    if reduction is None:
        assert np.isnan(got[TN, 5]) and got[TN, 9] == math.inf and got[TN, 0] == math.inf
        assert got[3, TM] == 0 and want[3, TM] == 0


def test_repeats_are_bit_identical_and_nothing_syncs():
    x, y = _randn((2 * TN + 1, 40), 13), _randn((2 * TM + 1, 40), 14)
    first = pairwise_minkowski_distance(x, y, exponent=3, reduction="mean")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = pairwise_minkowski_distance(x, y, exponent=3, reduction="mean")
        full = pairwise_manhattan_distance(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, again) and full.shape == (2 * TN + 1, 2 * TN + 1)


def test_dispatch(monkeypatch):
    def chain(x, y):
        return (x.unsqueeze(1) - y.unsqueeze(0)).abs().pow(3).sum(-1).pow(1.0 / 3)

    x, y = _randn((20, 7), 15), _randn((15, 7), 16)
    calls = _hip.pairwise_kernel_calls()
    pairwise_minkowski_distance(x, y, exponent=3)
    assert _hip.pairwise_kernel_calls() == calls + 1
    xg = x.clone().requires_grad_()
    for a, b in [(x.cpu(), y.cpu()), (x.double(), y.double()), (xg, y)]:
        assert torch.equal(pairwise_minkowski_distance(a, b, exponent=3), chain(a, b))
    pairwise_minkowski_distance(xg, y, exponent=3).sum().backward()
    assert xg.grad is not None and _hip.pairwise_lp(x, y.half(), 3, False, None) is None
    assert _hip.pairwise_lp(x, y, math.inf, False, None) is None and _hip.pairwise_lp(x[:0], y, 3, False, None) is None
    with monkeypatch.context() as m:
        m.setenv(_hip.PAIRWISE_KERNEL_ENV, "0")
        assert torch.equal(pairwise_minkowski_distance(x, y, exponent=3), chain(x, y))
        assert torch.equal(pairwise_manhattan_distance(x, y), (x.unsqueeze(1) - y.unsqueeze(0)).abs().sum(-1))
    assert _hip.pairwise_kernel_calls() == calls + 1


@pytest.mark.parametrize("reduction", [None, "sum"])
@pytest.mark.parametrize("p", ["manhattan", 3])
def test_peak_memory(p, reduction):
    """The torch chain needs 64 times the output matrix here."""
    x, y = _randn((1024, 64), 17), _randn((1024, 64), 18)
    matrix_bytes = 1024 * 1024 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _call(x, y, p, reduction=reduction)
    rise = torch.cuda.max_memory_allocated() - before
    assert out.shape == ((1024, 1024) if reduction is None else (1024,))
    assert rise < (2 * matrix_bytes if reduction is None else matrix_bytes)
