"""The language-model NLL kernel (``csrc/lm_nll.hip``) behind ``Perplexity``.

ORACLE: per kept row, fp64 on the CPU, ``logsumexp(x) - x[t]`` over the exact
values of the inputs; rows are added in numpy. A kept row with a target outside
[0, V) is NaN.

TOLERANCE, per case: E is the largest per-row error of the reference's own
formula, ``-log(softmax(x.float(), -1))[t]`` in fp32 on the CPU, against the
oracle, over the rows where both are finite. The kernel forms the same fp32
sum with a fast exp and finishes in fp64: it gets 4 * E per kept row, so the
bound on ``perplexity_sums()[0]`` is 4 * E * kept. The count is exact. A
non-finite oracle total must be matched in kind (NaN, +inf).
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import metrics_amd as ma
from metrics_amd.functional.text.misc import perplexity
from metrics_amd.ops import _hip, perplexity_sums

pytestmark = pytest.mark.gpu

FP32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [FP32, BF16, FP16]
MANTISSA = {FP32: 23, BF16: 7, FP16: 10}


def _id(v):
    return str(v).replace("torch.", "")


def _inputs(B, T, V, dtype, seed=0, ig=None, ignored=0.0):
    gen = torch.Generator().manual_seed(seed * 1000003 + V)
    x = (torch.randn(B, T, V, generator=gen) * 4).to(dtype)
    t = torch.randint(0, V, (B, T), generator=gen)
    if ig is not None and ignored > 0:
        t[torch.rand(B, T, generator=gen) < ignored] = ig
    return x, t


def _oracle(x, t, ig):
    """(fp64 nll per kept row, E of the case) from CPU tensors or views."""
    V = x.shape[-1]
    x64 = x.double().reshape(-1, V).numpy()
    tt = t.reshape(-1).numpy()
    keep = np.ones_like(tt, dtype=bool) if ig is None else tt != ig
    ref32 = -torch.log(torch.softmax(x.float().reshape(-1, V), -1)).numpy()
    rows, E = [], 0.0
    with np.errstate(all="ignore"):
        for r in np.nonzero(keep)[0]:
            if not 0 <= tt[r] < V:
                rows.append(np.nan)
                continue
            m = x64[r].max()
            v = m + np.log(np.exp(x64[r] - m).sum()) - x64[r, tt[r]]
            rows.append(v)
            if np.isfinite(v) and np.isfinite(ref32[r, tt[r]]):
                E = max(E, abs(float(ref32[r, tt[r]]) - v))
    return np.array(rows, dtype=np.float64), E


def _check(x, t, ig, base=None):
    """``x`` / ``t`` are device tensors or views; ``base`` = (CPU x, CPU t) where
    copying the views back is not wanted. Returns what the kernel gave."""
    cx, ct = base if base is not None else (x.cpu(), t.cpu())
    rows, E = _oracle(cx, ct, ig)
    got = perplexity_sums(x, t, ig)
    assert got is not None, "the kernel must cover this call"
    total, count = (float(v) for v in got.cpu())
    want = float(rows.sum()) if len(rows) else 0.0
    print(f"shape {tuple(x.shape)} {x.dtype}: kept {len(rows)} E {E:.3e} error {abs(total - want):.3e}")
    assert count == len(rows)
    if math.isnan(want):
        assert math.isnan(total)
    elif math.isinf(want):
        assert total == want
    else:
        assert abs(total - want) <= 4 * E * len(rows)
    return got


def _bt(rows):
    return next(((rows // T, T) for T in (7, 5, 3, 2) if rows % T == 0), (rows, 1))


def _row_lengths():
    lay = _hip.lm_nll_layout(3, 64, FP32)
    B1, B2 = lay.last_group_v, lay.last_wave_v
    return [1, 7, 8, 9, 63, 64, 65, B1 - 1, B1, B1 + 1, B2, B2 + 8, B2 + 9]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("index", range(13))
def test_row_lengths(index, dtype):
    V = _row_lengths()[index]
    few = _hip.lm_nll_layout(3, V, dtype)
    if V >= few.last_wave_v:  # B2 itself on the wave mapping, the two above it on the block mapping
        B, T = 1, 3
        assert few.mapping == (2 if V == few.last_wave_v else 3)
    else:
        B, T = _bt(3 * few.rows_per_block + 1)
        assert few.mapping == (1 if V <= few.last_group_v else 2)
    x, t = _inputs(B, T, V, dtype, ig=-100, ignored=0.2 if B * T > 3 else 0.0)
    _check(x.cuda(), t.cuda(), -100)


@pytest.mark.parametrize("V", [64, 300, 1000])
@pytest.mark.parametrize("which", ["one", "wave-1", "wave+1", "3blocks+1", "wrap"])
def test_row_counts(V, which, monkeypatch):
    lay = _hip.lm_nll_layout(1 << 20, V, BF16)
    rows = {"one": 1, "wave-1": lay.rows_per_wave - 1, "wave+1": lay.rows_per_wave + 1,
            "3blocks+1": 3 * lay.rows_per_block + 1, "wrap": 7 * lay.rows_per_block + 1}[which]
    rows = max(rows, 1)  # one row per wave: no smaller count
    if which == "wrap":  # two blocks: every wave takes several row groups
        monkeypatch.setenv("MA_LM_NLL_GRID", "2")
        assert _hip.lm_nll_layout(rows, V, BF16).grid == 2
    x, t = _inputs(*_bt(rows), V, BF16, seed=1)
    _check(x.cuda(), t.cuda(), None)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("V", [77, 1003])
@pytest.mark.parametrize("kind", ["shifted", "offset1", "odd_batch_stride", "transposed_target"])
def test_strided_views(kind, V, dtype):
    B, T = 2, 5
    x, t = _inputs(B, T + 1, V, dtype, seed=2, ig=-100, ignored=0.2)
    if kind == "shifted":
        px, pt = x.cuda()[:, :-1], t.cuda()[:, 1:]
        cx, ct = x[:, :-1], t[:, 1:]
        assert not px.is_contiguous() and not pt.is_contiguous()
    else:
        cx, ct = x[:, :T].contiguous(), t[:, :T].contiguous()
        px, pt = cx.cuda(), ct.cuda()
        if kind == "offset1":  # the base sits one element behind an aligned address
            buf = torch.empty(B * T * V + 1, dtype=dtype, device="cuda")
            px = buf[1:].view(B, T, V).copy_(px)
            assert px.data_ptr() % 16 == px.element_size()
        elif kind == "odd_batch_stride":
            s0 = T * V + (1 if (T * V) % 2 == 0 else 2)
            px = torch.empty(B * s0, dtype=dtype, device="cuda").as_strided((B, T, V), (s0, V, 1)).copy_(px)
            assert px.stride(0) % 2 == 1
        else:
            pt = ct.t().contiguous().cuda().t()
            assert pt.stride() == (1, B)
    _check(px, pt, -100, base=(cx, ct))


def test_offsets_beyond_2_to_the_31():
    V = 1000
    x, t = _inputs(2, 1, V, BF16, seed=3)
    buf = torch.empty(2**31 + 2 * V, dtype=BF16, device="cuda")  # 4.3 GB, two rows of it touched
    view = buf.as_strided((2, 1, V), (2**31 + V, V, 1))
    view.copy_(x)
    _check(view, t.cuda(), None, base=(x, t))


PLANTED = ["nan", "posinf", "all_neginf", "target_neginf", "masked_vocab", "target_200_below"]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("V", [40, 1003, 9001])
@pytest.mark.parametrize("kind", PLANTED)
def test_planted_rows(kind, V, dtype):
    x, t = _inputs(1, 3, V, dtype, seed=4)
    row, tg = x[0, 1], int(t[0, 1])
    if kind == "nan":
        row[(tg + 1) % V] = float("nan")
    elif kind == "posinf":
        row[(tg + 1) % V] = float("inf")
    elif kind == "all_neginf":
        row[:] = float("-inf")
    elif kind == "target_neginf":
        row[tg] = float("-inf")
    elif kind == "masked_vocab":  # whole vectors of -inf next to finite values
        row[: V - 3] = float("-inf")
        t[0, 1] = V - 2
    else:
        row[(tg + 1) % V] = row[tg] + 200
    rows, _ = _oracle(x, t, None)
    kinds = {"nan": math.isnan, "posinf": math.isnan, "all_neginf": math.isnan,
             "target_neginf": lambda v: v == math.inf}
    assert kinds.get(kind, math.isfinite)(float(rows.sum()))
    _check(x.cuda(), t.cuda(), None)


@pytest.mark.parametrize("V", [64, 1003])
@pytest.mark.parametrize("ig", [-100, 5])
@pytest.mark.parametrize("share", ["none", "some", "all"])
def test_ignore_index(share, ig, V):
    x, t = _inputs(3, 7, V, BF16, seed=5, ig=ig, ignored={"none": 0.0, "some": 0.4, "all": 2.0}[share])
    if share == "none":
        t[t == ig] = 6
    x[t == ig] = float("nan")  # an ignored row is never read
    got = _check(x.cuda(), t.cuda(), ig)
    if share == "all":
        assert got.tolist() == [0.0, 0.0]
        m = ma.Perplexity(ignore_index=ig).to("cuda")
        m.update(x.cuda(), t.cuda())
        assert math.isnan(float(m.compute()))


@pytest.mark.parametrize("V", [64, 1003, 9001])
@pytest.mark.parametrize("bad", ["V", "-1"])
def test_target_out_of_range(bad, V):
    x, t = _inputs(1, 3, V, FP32, seed=6)
    good = t.clone()
    t[0, 2] = V if bad == "V" else -1
    got = _check(x.cuda(), t.cuda(), -100)
    assert math.isnan(float(got[0])) and float(got[1]) == 3
    _check(x.cuda(), good.cuda(), -100)  # the device is still in order


def test_same_call_same_bits():
    x, t = (v.cuda() for v in _inputs(5, 13, 1003, BF16, seed=7, ig=-100, ignored=0.3))
    y, u = (v.cuda() for v in _inputs(3, 3, 64, FP32, seed=7))
    first = perplexity_sums(x, t, -100).clone()
    assert torch.equal(perplexity_sums(x, t, -100), first)
    perplexity_sums(y, u, None)
    assert torch.equal(perplexity_sums(x, t, -100), first)


def _ulp(v, dtype):
    return 2.0 ** (math.floor(math.log2(abs(v))) - MANTISSA[dtype]) if v else 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_public_metric_and_functional(dtype):
    """Each update adds the oracle's total, rounded once to the input dtype, in
    fp32: one unit in the last place of that dtype per update, and half a unit
    of fp32 for each of the three additions."""
    m = ma.Perplexity(ignore_index=-100).to("cuda")
    want, slack, kept = 0.0, 0.0, 0
    for seed in range(3):
        x, t = _inputs(2, 10, 1003, dtype, seed=10 + seed, ig=-100, ignored=0.2)
        total = float(_oracle(x[:, :-1], t[:, 1:], -100)[0].sum())
        want += float(torch.tensor(total, dtype=torch.float64).to(dtype))
        slack += _ulp(total, dtype)
        kept += int((t[:, 1:] != -100).sum())
        m.update(x.cuda()[:, :-1], t.cuda()[:, 1:])
    assert float(m.count) == kept
    assert abs(float(m.total_log_probs) - want) <= slack + 1.5 * _ulp(want, FP32)
    assert float(m.compute()) == pytest.approx(math.exp(float(m.total_log_probs) / kept), rel=1e-5)
    x, t = _inputs(2, 9, 1003, dtype, seed=20)
    total = float(_oracle(x, t, None)[0].sum())
    near = torch.tensor(total, dtype=torch.float64).to(dtype).cuda()
    step = torch.tensor(_ulp(total, dtype), dtype=dtype, device="cuda")
    allowed = [float(torch.exp(c / 18)) for c in (near - step, near, near + step)]
    assert float(perplexity(x.cuda(), t.cuda())) in allowed


def test_no_host_sync_in_update():
    m = ma.Perplexity(ignore_index=-100).to("cuda")
    batches = [tuple(v.cuda() for v in _inputs(2, 9, 1003, BF16, seed=30 + i, ig=-100, ignored=0.2)) for i in range(4)]
    m.update(*batches[0])  # allocates the slab
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x, t in batches[1:]:
            m.update(x, t)
        with pytest.raises(RuntimeError):  # the control: the mode does catch a wait
            m.total_log_probs.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(m.count) == sum(int((t != -100).sum()) for _, t in batches)


@pytest.mark.parametrize("how", ["requires_grad", "fp64", "int32_target", "switch_off"])
def test_dispatch_to_the_torch_chain(how, monkeypatch):
    calls = []
    real = _hip.lm_nll_into
    monkeypatch.setattr(_hip, "lm_nll_into", lambda *a, **k: calls.append(real(*a, **k)) or calls[-1])
    x, t = (v.cuda() for v in _inputs(2, 5, 300, FP32, seed=40))
    want = float(perplexity_sums(x, t, None)[0])
    assert calls == [True]
    if how == "requires_grad":
        x.requires_grad_(True)
    elif how == "fp64":
        x = x.double()
    elif how == "int32_target":
        t = t.int()
    else:
        monkeypatch.setenv(_hip.PERPLEXITY_KERNEL_ENV, "0")
    del calls[:]
    m = ma.Perplexity().to("cuda")
    m(x, t)  # forward: the update runs with grad enabled
    value = perplexity(x, t)
    assert calls and not any(calls)
    assert float(m.total_log_probs) == pytest.approx(want, rel=1e-6)
    assert float(value) == pytest.approx(math.exp(want / 10), rel=1e-5)
    if how == "requires_grad":
        value.backward()
        assert x.grad is not None and bool(x.grad.abs().sum() > 0)
        del calls[:]
        with torch.no_grad():
            perplexity(x, t)
        assert calls == [True]
