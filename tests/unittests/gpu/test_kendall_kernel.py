"""The Kendall kernels (csrc/kendall.hip) against an all-pairs numpy oracle:
every pair by direct comparison, ``(a > b) - (a < b)`` (not a subtraction:
``inf - inf`` is NaN), in chunks, integer counts. Above ``2 * KENDALL_TILE + 1``
elements con / dis / ties come from the CPU path (``_count_pairs``), exact
integer arithmetic too.

The seven integer counts of the record must be EXACT. tau must lie within one
fp32 ulp of the fp64 formula on the oracle's counts (the fp64 chain errs far
below half an fp32 ulp, so only a rounding boundary can move it by one), the
fp32 p-value within rtol 1e-5 of the same formula on the oracle's t-value.
"""
import functools
import math

import numpy as np
import pytest
import torch

import metrics_amd as ma
from metrics_amd.functional.regression.kendall import _count_pairs, _p_value, kendall_rank_corrcoef
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

TILE = _hip.KENDALL_TILE
INTS = ("con", "dis", "x_ties", "y_ties", "xy_ties", "unique_x", "unique_y")


def _sign(a, b):
    return (a[:, None] > b[None, :]).astype(np.int8) - (a[:, None] < b[None, :]).astype(np.int8)


def _oracle(x, y):
    """x, y: fp64 numpy. The integer counts and the p1 / p2 tie sums."""
    n = len(x)
    out = {}
    if n <= 2 * TILE + 1:
        tot = dict.fromkeys(("con", "dis", "x_ties", "y_ties", "xy_ties"), 0)
        for i in range(0, n, 1024):
            sx, sy = _sign(x[i:i + 1024], x), _sign(y[i:i + 1024], y)
            for k, m in (("con", sx * sy > 0), ("dis", sx * sy < 0), ("x_ties", sx == 0), ("y_ties", sy == 0),
                         ("xy_ties", (sx == 0) & (sy == 0))):
                tot[k] += int(m.sum())
        out = {k: (v - (n if "ties" in k else 0)) // 2 for k, v in tot.items()}  # ordered pairs, less the diagonal
    else:
        con, dis, xt, yt, _, _ = _count_pairs(torch.from_numpy(x), torch.from_numpy(y))
        out = {"con": int(con), "dis": int(dis), "x_ties": int(xt), "y_ties": int(yt)}
        out["xy_ties"] = out["con"] + out["dis"] - n * (n - 1) // 2 + out["x_ties"] + out["y_ties"]
    for name, v in (("x", x), ("y", y)):
        t = [int(c) for c in np.unique(v, return_counts=True)[1]]
        out["unique_" + name] = len(t)
        out["p1_" + name] = float(sum(c * (c - 1) * (c - 2) for c in t))
        out["p2_" + name] = float(sum(c * (c - 1) * (2 * c + 5) for c in t))
    return out


def _formula(o, n, variant):
    """(tau, t-value) in fp64, the chain of ``_kendall_corrcoef_compute``."""
    con, dis, xt, yt = (np.float64(o[k]) for k in ("con", "dis", "x_ties", "y_ties"))
    n0 = n * (n - 1) / 2
    with np.errstate(all="ignore"):
        if variant == "a":
            tau = (con - dis) / (con + dis)
        elif variant == "b":
            tau = (con - dis) / np.sqrt((n0 - xt) * (n0 - yt))
        else:
            m = min(o["unique_x"], o["unique_y"])
            tau = 2 * (con - dis) / np.float64(n**2 * (m - 1) / m)
        base = n * (n - 1) * (2 * n + 5)
        if variant == "a":
            return tau, 3 * (con - dis) / math.sqrt(base / 2)
        mm = n * (n - 1)
        denom = (base - o["p2_x"] - o["p2_y"]) / 18 + (2 * xt * yt) / mm
        denom += o["p1_x"] * o["p1_y"] / (9 * mm * (n - 2)) if n != 2 else float("nan")
        return tau, ((con - dis) / math.sqrt(denom) if denom > 0 else float("nan"))


@functools.lru_cache(maxsize=None)
def _inputs(n, kind, seed=0):
    """(x, y) as fp32 CPU tensors and their oracle."""
    gen = torch.Generator().manual_seed(1000 * seed + n % 997)
    if kind == "cont":
        x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    elif kind == "tied":
        x, y = (torch.randint(0, k, (n,), generator=gen).float() for k in (7, 300))
    elif kind == "interleave":  # x ascending; a sparse sorted half of y against a dense one: a chunk of the
        h = (n // 2) & -TILE     # sparse half interleaves with 8 * KENDALL_CHUNK > KENDALL_STAGE dense keys
        x = torch.arange(n, dtype=torch.float32)
        y = torch.cat([8.0 * torch.arange(h), torch.arange(h) + 0.5, torch.tensor([-1.0, 1e6, 7.25])[: n - 2 * h]])
    elif kind == "planted":
        vals = torch.tensor([-0.0, 0.0, 1e-45, -1e-45, math.inf, -math.inf, 1.0, -1.0, 3e-39, 65504.0])
        x = vals[torch.randint(0, len(vals), (n,), generator=gen)]
        y = vals[torch.randint(0, len(vals), (n,), generator=gen)]
    x, y = x.contiguous(), y.contiguous()
    return x, y, _oracle(x.double().numpy(), y.double().numpy())


def _assert_record(res, col, oracle, n, variant="b"):
    f = {k: v[col].item() for k, v in res.fields().items()}
    print({k: (f[k], oracle[k]) for k in INTS})
    assert all(f[k] == oracle[k] for k in INTS)
    tau = np.float32(_formula(oracle, n, variant)[0])
    got = np.float32(res.tau[col].item())
    print("tau", got, tau, "routes", f["lds_chunks"], f["global_chunks"])
    assert (np.isnan(tau) and np.isnan(got)) or abs(got - tau) <= np.spacing(abs(tau))
    return f


SMALL = [2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


@pytest.mark.parametrize("kind", ["cont", "tied"])
@pytest.mark.parametrize("n", SMALL)
def test_small_against_all_pairs(n, kind):
    x, y, oracle = _inputs(n, kind)
    _assert_record(_hip.kendall_counts(x.cuda(), y.cuda(), "b"), 0, oracle, n)


@pytest.mark.parametrize("n,kind", [
    (3 * TILE + 5, "cont"), (3 * TILE + 5, "tied"), (5 * TILE + 17, "cont"), (5 * TILE + 17, "tied"),
    (2**17 + 3, "cont"), (2**17 + 3, "tied"), (2**17 + 3, "interleave"),
])
def test_global_levels_against_the_cpu_path(n, kind):
    x, y, oracle = _inputs(n, kind)
    lay = _hip.kendall_layout(n)
    assert lay[7] == math.ceil(math.log2(n / TILE)) and lay[2] == _hip.KENDALL_STAGE < 8 * lay[3]
    f = _assert_record(_hip.kendall_counts(x.cuda(), y.cuda(), "b"), 0, oracle, n)
    if (n, kind) == (3 * TILE + 5, "cont"):
        assert f["global_chunks"] == 0 and f["lds_chunks"] > 0  # every chunk searched its stage in LDS
    if kind == "interleave":
        assert f["global_chunks"] >= 8 and f["lds_chunks"] > 0  # the sparse half's first chunks went to global memory


@pytest.mark.parametrize("how", ["ascending", "descending", "constant_x"])
def test_closed_forms(how):
    n = 2**20 + 1 if how == "descending" else 1000
    x = torch.arange(n, dtype=torch.float32, device="cuda")
    y = {"ascending": x, "descending": -x, "constant_x": x}[how]
    x = torch.ones_like(x) if how == "constant_x" else x
    res = _hip.kendall_counts(x, y, "b")
    f = {k: v[0].item() for k, v in res.fields().items()}
    tot = n * (n - 1) // 2  # 2^39 at the large size: 32-bit sums of the merge levels would wrap
    want = {"ascending": (tot, 0, 1.0), "descending": (0, tot, -1.0), "constant_x": (0, 0, math.nan)}[how]
    assert (f["con"], f["dis"]) == want[:2]
    assert res.tau[0].item() == want[2] or (math.isnan(want[2]) and math.isnan(res.tau[0].item()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_planted_values_and_dtypes(dtype):
    n = 517
    x, y, oracle = _inputs(n, "planted" if dtype == torch.float32 else "cont")
    if dtype != torch.float32:
        x, y = x.to(dtype), y.to(dtype)
        oracle = _oracle(x.double().numpy(), y.double().numpy())
        assert oracle["x_ties"] > 0  # the narrow format ties some values
    f = _assert_record(_hip.kendall_counts(x.cuda(), y.cuda(), "b"), 0, oracle, n)
    assert f["nan"] == 0
    if dtype == torch.float32:
        assert oracle["unique_x"] == 9  # -0.0 ties with +0.0, the denormals stay apart


@pytest.mark.parametrize("variant", ["a", "b", "c"])
@pytest.mark.parametrize("transposed", [False, True])
def test_columns_variants_and_nan(variant, transposed):
    n = 300
    cols = [_inputs(n, kind, seed) for kind, seed in (("cont", 1), ("tied", 2), ("cont", 3))]
    x, y = (torch.stack([c[i] for c in cols], 1) for i in (0, 1))
    x[17, 1] = math.nan
    x, y = x.cuda(), y.cuda()
    if transposed:
        x, y = x.t().contiguous().t(), y.t().contiguous().t()
        assert not x.is_contiguous()
    res = _hip.kendall_counts(x, y, variant)
    for col in (0, 2):
        _assert_record(res, col, cols[col][2], n, variant)
    assert res.fields()["nan"].tolist() == [0, 1, 0]
    tau = kendall_rank_corrcoef(x, y, variant=variant)
    assert torch.equal(tau[[0, 2]], res.tau[[0, 2]]) and tau.isnan().tolist() == [False, True, False]


@pytest.mark.parametrize("alternative", ["two-sided", "greater", "less"])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_t_test(variant, alternative):
    n = 300
    x, y, oracle = _inputs(n, "tied", 2)
    tau, p = kendall_rank_corrcoef(x.cuda(), y.cuda(), variant=variant, t_test=True, alternative=alternative)
    want = _p_value([_formula(oracle, n, variant)[1]], alternative)
    print("p", p, want)
    assert tau.is_cuda and p.dtype == torch.float32 and p.device == want.device and p.shape == want.shape
    torch.testing.assert_close(p, want, rtol=1e-5, atol=0.0)
    # n == 2: the t-value of variant b is NaN by definition
    _, p2 = kendall_rank_corrcoef(x[:2].cuda(), y[:2].cuda(), variant="b", t_test=True, alternative=alternative)
    assert p2.isnan().item()


def test_modular_metric_over_two_updates():
    x, y, _ = _inputs(TILE + 1, "tied")
    m = ma.KendallRankCorrCoef().to("cuda")
    before = _hip.kendall_kernel_calls()
    m.update(x[:1000].cuda(), y[:1000].cuda())
    m.update(x[1000:].cuda(), y[1000:].cuda())
    assert torch.equal(m.compute(), kendall_rank_corrcoef(x.cuda(), y.cuda()))
    assert _hip.kendall_kernel_calls() == before + 2


def test_dispatch_and_determinism(monkeypatch):
    x, y, _ = _inputs(3 * TILE + 5, "tied")
    xg, yg = x.cuda(), y.cuda()
    before = _hip.kendall_kernel_calls()
    first = _hip.kendall_counts(xg, yg, "b")
    again = _hip.kendall_counts(xg, yg, "b")
    assert torch.equal(first.record, again.record) and torch.equal(first.tau, again.tau)  # bit-identical
    tau = kendall_rank_corrcoef(xg, yg)
    assert _hip.kendall_kernel_calls() == before + 3
    cpu = kendall_rank_corrcoef(x, y)  # CPU inputs
    f64 = kendall_rank_corrcoef(xg.double(), yg.double())  # fp64 inputs
    assert _hip.kendall_counts(xg[:1], yg[:1], "b") is None  # n < 2
    monkeypatch.setenv(_hip.KENDALL_KERNEL_ENV, "0")
    off = kendall_rank_corrcoef(xg, yg)  # the switch
    assert _hip.kendall_kernel_calls() == before + 3
    for other in (cpu, f64, off):
        assert abs(other.item() - tau.item()) <= np.spacing(np.float32(abs(tau.item())))


def test_no_host_sync_without_t_test():
    x, y, _ = _inputs(2 * TILE + 1, "cont")
    x, y = torch.stack([x, y], 1).cuda(), torch.stack([y, x], 1).cuda()
    kendall_rank_corrcoef(x, y)  # allocates the scratch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tau = kendall_rank_corrcoef(x, y, variant="c")
        with pytest.raises(RuntimeError):  # the control: the mode does catch a wait
            tau[0].item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(tau[0], tau[1])  # the pair counts are symmetric in (x, y)
