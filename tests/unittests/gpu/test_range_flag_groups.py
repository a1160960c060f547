"""The "some element lies outside [0,1]" bit, now taken from a group's minimum
and maximum instead of from every element.

Probabilities in [0,1] (``torch.rand``) with EXACTLY ONE element of one row
just outside: the batch must be softmaxed. The element is placed at each
position 0..7 of a group, in the first and in the second 16-byte vector of a
lane, in lane 0, a middle lane and the last valid lane; every placement is one
update of the same collection, and the final curve state must equal the CPU
collection's exactly.

Why exact equality holds across the GPU's and the CPU's softmax: the thresholds
are (0.1, 0.5, 0.9), and the softmax of a row of values in [-0.5, 1.5] stays
below e^2 / C <= 0.055 for C >= 136 — every softmaxed element is below every
threshold by a factor of two, so no rounding moves a bucket. Raw ``torch.rand``
values fill all four buckets, so a batch that skipped the softmax (or took it
when it should not) changes the counts, and counts only ever add up.

The second test pins what must NOT flip the decision: -0.0, 0.0, 1.0 and NaN.
NaN bins below every threshold, exactly like 0.0, which is what the CPU
collection is fed in its place (its own range test would take NaN as "outside").
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

_THR = [0.1, 0.5, 0.9]
_B = 3
_DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _make(C):
    kw = dict(num_classes=C, validate_args=False, ignore_index=None)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=_THR, **kw),
    })


def _places(C, dtype):
    """Element indices: position 0..7 from the start of a vector, first and
    second vector of lane 0, a middle lane and the last valid lane."""
    epv = 8 if dtype == torch.bfloat16 else 4
    nvec = C // epv
    out = []
    for k in (0, 1):
        n = min(64, nvec - 64 * k)  # lanes that hold a vector k
        if n <= 0:
            continue
        for lane in sorted({0, n // 2, n - 1}):
            for pos in range(8):
                i = (lane + 64 * k) * epv + pos
                if i < C:
                    out.append(i)
    return out


def _batches(C, dtype, value, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n, i in enumerate([None] + _places(C, dtype)):  # the first update is not fused: no outlier
        p = torch.rand(_B, C, generator=gen).to(dtype)
        if i is not None:
            p[n % _B, i] = value
        out.append((p, torch.randint(0, C, (_B,), generator=gen)))
    return out


def _curve(coll):
    for m in coll.values(copy_state=False):
        m._maybe_flush_lazy()
    return coll.auroc.confmat.cpu()


def _gpu_curve(monkeypatch, C, batches):
    monkeypatch.setenv(_hip.ONEPASS_ENV, "2")
    coll = _make(C).to("cuda")
    for p, t in batches:
        coll.update(p.cuda(), t.cuda())
    assert coll._fused_plan.onepass_steps == len(batches) - 1
    return _curve(coll)


def _cpu_curve(C, batches):
    coll = _make(C)
    for p, t in batches:
        coll.update(p.float(), t)
    return _curve(coll)


def _outliers(name):
    dtype = _DTYPES[name]
    one_ulp = 1.0 + torch.finfo(dtype).eps  # the next value above 1
    vals = {"one_plus_ulp": one_ulp, "minus_half": -0.5, "one_and_half": 1.5}
    if dtype == torch.float32:
        vals["neg_denormal"] = -1e-45
    return vals


_OUT_CASES = [(C, n, v) for C in (136, 520, 1000, 1024) for n in _DTYPES for v in _outliers(n)]


@pytest.mark.parametrize("C,name,which", _OUT_CASES, ids=[f"C{c}-{n}-{v}" for c, n, v in _OUT_CASES])
def test_one_element_outside_takes_softmax(monkeypatch, C, name, which):
    dtype = _DTYPES[name]
    value = _outliers(name)[which]
    batches = _batches(C, dtype, value, seed=500 + C)
    for p, _ in batches[1:]:  # exactly one element outside, and it survived the cast
        pf = p.float()
        assert int(((pf < 0) | (pf > 1)).sum()) == 1
    got = _gpu_curve(monkeypatch, C, batches)
    want = _cpu_curve(C, batches)
    assert torch.equal(got, want)
    # the decision shows: softmaxed batches put nothing at or above a threshold
    raw = _cpu_curve(C, [(p.float().clamp(0, 1), t) for p, t in batches])
    assert not torch.equal(want, raw)


_IN_CASES = [(C, n) for C in (136, 520, 1000, 1024) for n in _DTYPES]


@pytest.mark.parametrize("C,name", _IN_CASES, ids=[f"C{c}-{n}" for c, n in _IN_CASES])
def test_edge_values_inside_do_not_flip(monkeypatch, C, name):
    dtype = _DTYPES[name]
    batches, cpu_batches = [], []
    for k, value in enumerate((-0.0, 0.0, 1.0, float("nan"))):
        for p, t in _batches(C, dtype, value, seed=900 + C + k)[1 if k else 0:]:
            batches.append((p, t))
            pf = p.float()
            cpu_batches.append((torch.where(torch.isnan(pf), torch.zeros_like(pf), pf), t))
    got = _gpu_curve(monkeypatch, C, batches)
    want = _cpu_curve(C, cpu_batches)
    assert torch.equal(got, want)
    assert int(want[..., 1, 1].sum()) > 0  # raw probabilities reach the thresholds: no softmax was taken
