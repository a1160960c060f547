"""The Spearman kernels (csrc/spearman.hip) against a numpy oracle: a stable
sort of the order-mapped values (``-0.0`` on ``+0.0``, every NaN one word above
``+inf``), run bounds ``f``, ``l`` from head flags (a NaN is always a head), the
centred twice-rank ``a = f + l + 1 - n``, the sums of ``a*b``, ``a*a``, ``b*b``
as Python ints, then the formula of ``_spearman_corrcoef_compute`` in fp64.

The three sums and the two run counts of the record must be EQUAL to the
oracle's. rho (fp32) must lie within one fp32 ulp of the oracle's fp64 value
rounded to fp32: the sums are exact and the tail is fp64, so only the last
rounding can differ. The functional must return ``rho.to(input dtype)``.
"""
import functools
import math

import numpy as np
import pytest
import torch

import metrics_amd as ma
from metrics_amd.functional.regression.spearman import spearman_corrcoef
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

TILE = _hip.SPEARMAN_TILE
NAN_WORD = 0xFFFFFFFF


def _twice_ranks(v):
    """v: fp32 numpy. (a, run count)."""
    b = np.ascontiguousarray(v).view(np.uint32).astype(np.int64)
    b = np.where((b & 0x7FFFFFFF) == 0, 0, b)
    u = np.where(np.isnan(v), NAN_WORD, np.where(b >> 31, ~b & 0xFFFFFFFF, b | 0x80000000))
    n = len(u)
    idx = np.argsort(u, kind="stable")
    s = u[idx]
    head = np.ones(n, bool)
    head[1:] = (s[1:] != s[:-1]) | (s[1:] == NAN_WORD)
    first = np.flatnonzero(head)
    last = np.append(first[1:], n) - 1
    run = np.cumsum(head) - 1
    a = np.empty(n, np.int64)
    a[idx] = first[run] + last[run] + 1 - n
    return a, len(first)


def _exact_sum(p):  # int64 products below 2^46 each: chunks of 2^16 stay below 2^62, the total is a Python int
    return sum(int(c) for c in np.add.reduceat(p, np.arange(0, len(p), 65536)))


def _rho(sab, saa, sbb, n):
    m = 4.0 * n
    rho = (sab / m) / (math.sqrt(saa / m) * math.sqrt(sbb / m) + 1e-6)
    return min(max(rho, -1.0), 1.0)


def _oracle(x, y):
    """x, y: 1-D CPU tensors of any float dtype (widened to fp32, exact)."""
    (a, rx), (b, ry) = (_twice_ranks(t.float().numpy()) for t in (x, y))
    o = {"sab": _exact_sum(a * b), "saa": _exact_sum(a * a), "sbb": _exact_sum(b * b), "runs_x": rx, "runs_y": ry}
    assert int(a.sum()) == 0 and int(b.sum()) == 0
    return o, _rho(o["sab"], o["saa"], o["sbb"], len(a))


def _assert_rho(got, want):
    want = np.float32(want)
    print("rho", got, want)
    assert abs(np.float32(got) - want) <= np.spacing(abs(want))


def _run(x, y):
    """Kernel and functional on the GPU copy of CPU (n,) / (n, D) tensors, every column against the oracle."""
    xg, yg = x.cuda(), y.cuda()
    res = _hip.spearman_ranks(xg, yg)
    sums = res.sums()
    for d, (cx, cy) in enumerate(zip(x.reshape(len(x), -1).T, y.reshape(len(y), -1).T)):
        want, rho = _oracle(cx, cy)
        got = {k: sums[d][k] for k in want}
        print(d, got, want)
        assert got == want
        _assert_rho(res.rho[d].item(), rho)
    out = spearman_corrcoef(xg, yg)
    assert out.shape == x.shape[1:] and torch.equal(out, res.rho.to(x.dtype).reshape(out.shape))
    return res


@functools.lru_cache(maxsize=None)
def _inputs(n, kind, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + n % 997)
    if kind == "cont":
        return torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    return tuple(torch.randint(0, k, (n,), generator=gen).float() for k in (7, 5))  # "tied"


@pytest.mark.parametrize("kind", ["cont", "tied"])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_small_sizes(n, kind):
    _run(*_inputs(n, kind))


@pytest.mark.parametrize("how", ["wave_boundary", "three_tiles", "constant_x", "identical"])
def test_planted_runs(how):
    n = {"wave_boundary": 200, "three_tiles": 3 * TILE + 2}.get(how, TILE + 77)
    y = _inputs(n, "cont", 3)[1]
    x = torch.arange(n, dtype=torch.float32)
    if how == "wave_boundary":
        x[64] = 63.0  # sorted positions 63 and 64: the last lane of one wave, the first of the next
    elif how == "three_tiles":
        x = torch.cat([torch.tensor([-1.0]), torch.zeros(3 * TILE), torch.tensor([1.0])])  # positions 1 .. 3 TILE
    elif how == "constant_x":
        x = torch.full((n,), 2.5)
    else:
        x = y
    x = x[torch.randperm(n, generator=torch.Generator().manual_seed(5))] if how != "identical" else x
    res = _run(x, y)
    if how == "constant_x":
        assert res.rho.item() == 0.0 and res.sums()[0]["runs_x"] == 1
    if how == "identical":
        assert res.rho.item() == pytest.approx(1.0, abs=1e-5)


@pytest.mark.parametrize("n,D", [(5, 1000), (TILE // 2 + 1, 3), (64, 64)])
def test_packed_columns(n, D):
    assert _hip.spearman_layout(n, D)[5] == 1 and _hip.spearman_layout(TILE, D)[5] == 0
    gen = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, D, generator=gen), torch.randint(0, 4, (n, D), generator=gen).float()
    if (n, D) == (64, 64):  # the last value of column d is the first of column d + 1, in x and in y
        x = (torch.arange(64.0)[:, None] + 63.0 * torch.arange(64.0)[None, :])[torch.randperm(64, generator=gen)]
        y = (torch.arange(64.0)[:, None] + 63.0 * torch.arange(64.0)[None, :])[torch.randperm(64, generator=gen)]
    res = _run(x, y)
    xt, yt = x.cuda().t().contiguous().t(), y.cuda().t().contiguous().t()  # (D, n).T views
    assert not xt.is_contiguous()
    again = _hip.spearman_ranks(xt, yt)
    assert torch.equal(again.record, res.record) and torch.equal(again.rho, res.rho)


@pytest.mark.parametrize("n,sign", [(2**22 + 1, 1), (2**22 + 1, -1), (TILE + 1, -1)])
def test_closed_forms(n, sign):
    x = torch.arange(n, dtype=torch.float32, device="cuda")
    res = _hip.spearman_ranks(x, sign * x)
    s = res.sums()[0]
    third = (n**3 - n) // 3  # above 2^63 at the large size: the high words count
    assert (s["sab"], s["saa"], s["sbb"], s["runs_x"], s["runs_y"]) == (sign * third, third, third, n, n)
    assert (third > 2**63) == (n > TILE + 1)
    _assert_rho(res.rho.item(), _rho(sign * third, third, third, n))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_special_values(dtype):
    den = torch.finfo(dtype).smallest_normal / 4  # a denormal of the dtype
    vals = torch.tensor([-0.0, 0.0, den, -den, math.inf, -math.inf, 1.0, -1.0, 2 * den, 3.0]).to(dtype)
    assert (vals[2] != 0) and (vals[2] != vals[8])
    gen = torch.Generator().manual_seed(11)
    x, y = (vals[torch.randint(0, len(vals), (517,), generator=gen)] for _ in range(2))
    s = _run(x, y).sums()[0]
    assert (s["runs_x"], s["runs_y"], s["nan"]) == (9, 9, 0)  # -0.0 ties with +0.0, the denormals stay apart


def test_bf16_where_the_torch_chain_has_no_ranks(monkeypatch):
    x, y = (t.bfloat16() for t in _inputs(1000, "cont", 7))
    res = _run(x, y)
    want = _oracle(x, y)[1]
    monkeypatch.setenv(_hip.SPEARMAN_KERNEL_ENV, "0")
    off = spearman_corrcoef(x.cuda(), y.cuda())  # ranks above 256 are not bf16 numbers
    ulp = np.spacing(np.float32(abs(want))) * 2**16  # of bf16
    print("bf16", want, res.rho.item(), off.item(), ulp)
    assert abs(spearman_corrcoef(x, y).item() - want) > ulp and abs(off.item() - want) > ulp
    assert abs(res.rho.to(torch.bfloat16).item() - want) <= ulp


@pytest.mark.parametrize("where", ["x", "y", "both"])
def test_nan_ranks_last_in_index_order(where):
    n = 300
    cols = [_inputs(n, kind, seed) for kind, seed in (("cont", 1), ("tied", 2), ("cont", 3))]
    x, y = (torch.stack([c[i] for c in cols], 1) for i in (0, 1))
    if where in ("x", "both"):
        x[[299, 17, 40], 1] = math.nan
    if where in ("y", "both"):
        y[[40, 5], 1] = -math.nan
    res = _run(x, y)  # the oracle ranks NaNs last, apart and by index
    s = res.sums()
    assert [c["nan"] for c in s] == [0, 1, 0]
    assert s[1]["runs_x"] == (7 + 3 if where != "y" else 7) and not res.rho.isnan().any()


def test_modular_metric_over_two_updates():
    x, y = (torch.stack([_inputs(TILE + 1, "tied", s)[i] for s in range(3)], 1).cuda() for i in (0, 1))
    m = ma.SpearmanCorrCoef(num_outputs=3).to("cuda")
    before = _hip.spearman_kernel_calls()
    m.update(x[:1000], y[:1000])
    m.update(x[1000:], y[1000:])
    assert torch.equal(m.compute(), spearman_corrcoef(x, y))
    assert _hip.spearman_kernel_calls() == before + 2 and "_hip_spearman_scratch" in m.__dict__


def test_dispatch_and_determinism(monkeypatch):
    x, y = _inputs(3 * TILE + 5, "cont")
    xg, yg = x.cuda(), y.cuda()
    before = _hip.spearman_kernel_calls()
    first, again = _hip.spearman_ranks(xg, yg), _hip.spearman_ranks(xg, yg)
    assert torch.equal(first.record, again.record) and torch.equal(first.rho, again.rho)  # bit-identical
    rho = spearman_corrcoef(xg, yg)
    assert _hip.spearman_kernel_calls() == before + 3
    cpu = spearman_corrcoef(x, y)  # CPU inputs
    f64 = spearman_corrcoef(xg.double(), yg.double())  # fp64 inputs
    assert _hip.spearman_ranks(xg[:1], yg[:1]) is None and _hip.spearman_ranks(xg, yg[:-1]) is None
    monkeypatch.setenv(_hip.SPEARMAN_KERNEL_ENV, "0")
    off = spearman_corrcoef(xg, yg)  # the switch
    assert _hip.spearman_kernel_calls() == before + 3
    want = _oracle(x, y)[1]
    err = abs(cpu.item() - want)  # the torch chain's own fp32 error
    print("cpu", cpu.item(), "off", off.item(), "kernel", rho.item(), "oracle", want, "f64", f64.item())
    assert abs(rho.item() - cpu.item()) <= 2 * err + np.spacing(np.float32(abs(want)))
    # the three still are the torch chain: fp32 sums over 6149 ranks, fp64 for fp64
    assert off.is_cuda and f64.dtype == torch.float64 and err <= 1e-4
    assert abs(off.item() - want) <= 1e-4 and abs(f64.item() - want) <= 1e-9


def test_no_host_sync(monkeypatch):
    x, y = (torch.stack([_inputs(4096, "tied", s)[i] for s in (0, 1)], 1).cuda() for i in (0, 1))
    spearman_corrcoef(x, y)  # allocates the scratch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rho = spearman_corrcoef(x, y)
        monkeypatch.setenv(_hip.SPEARMAN_KERNEL_ENV, "0")
        with pytest.raises(RuntimeError):  # the control: the torch chain waits for the host
            spearman_corrcoef(x, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rho.shape == (2,) and not rho.isnan().any()
