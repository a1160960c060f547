"""The top-k slot of the fused multiclass step on the GPU.

A collection with a top-1 and a top-k stat-scores group runs its updates from
the second one on through the fused plan, which counts the top-k group in the
same pass over the logits (``plan.topk``, ``plan.topk_steps``).

Oracle A (random logits): the accumulated top-k states equal the summed deltas
of the per-row rule (``_topk_rule``), and the whole run equals, bit for bit and
for every member, the same run with ``METRICS_AMD_FUSE_TOPK=0``, where the
top-k leader updates on its own through the stand-alone kernel.

Oracle B (edge rows, from the second update on): the rule alone, together with
the protocol: step counters, no host sync in steady state, ``reset()``, and a
``compute()`` between updates that must not return a cached value.

The first update of a collection runs every metric by itself and forms the
groups by state equality, so the first batch is plain random logits plus one
constructed row whose target ranks second: top-1 and top-k states differ.
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip
from tests.unittests._topk_rule import stat_rule_deltas

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
INF, NAN = float("inf"), float("nan")

# (C, dtype, B, k): the smallest shapes at which the register mapping of the
# one-pass kernel or a load path of the streaming kernel changes
SHAPES = [
    (136, BF16, 3, 2),        # NV=1, most lanes idle
    (520, BF16, 5, 5),        # 65 vectors: one lane holds two
    (1000, BF16, 257, 5),     # ragged second vector
    (1024, BF16, 1, 65),      # exact fit
    (4096, BF16, 5, 4096),    # NV=8, 64-bit pending mask; k = C: every valid row a tp
    (520, FP32, 257, 65),     # NV=4
    (1001, BF16, 3, 5),       # one-pass declines, streaming scalar path
    (130, BF16, 5, 130),      # no 16- or 8-byte vector path
    (128, BF16, 257, 2),      # thread-per-row kernel: the top-k leader stays unhandled
]
KINDS = ["onepass", "twokernel", "plain"]


def _id(v):
    return {BF16: "bf16", FP32: "fp32"}.get(v, str(v))


def _make(kind, C, k, ig):
    kw = dict(num_classes=C, validate_args=False, ignore_index=ig)
    m = {
        "acc1": ma.MulticlassAccuracy(average="micro", **kw),
        "acck": ma.MulticlassAccuracy(top_k=k, average="macro", **kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
    }
    if kind != "plain":
        m["f1k"] = ma.MulticlassF1Score(top_k=k, average="macro", **kw)
        m["exact"] = ma.MulticlassExactMatch(**kw)
        m["auroc"] = ma.MulticlassAUROC(average="macro", thresholds=5, **kw)
        m["ap"] = ma.MulticlassAveragePrecision(average="macro", thresholds=5, **kw)
    return ma.MetricCollection(m).to("cuda")


def _random_batch(C, B, dtype, gen):
    p = (torch.randn(B, C, generator=gen) * 3.0).to(dtype)
    return p, torch.randint(0, C, (B,), generator=gen)


def _first_batch(C, B, dtype, gen):
    """Random rows; row 0 has its target at rank 1 (argmax 5, target 9)."""
    p, t = _random_batch(C, B, dtype, gen)
    p[0] = torch.randn(C, generator=gen).to(dtype)
    p[0, 5], p[0, 9], t[0] = 32.0, 31.0, 9
    return p, t


def _edge_batch(C, k, dtype, ig, gen):
    """Rows at the edges of the rule; every value is exact in bf16."""
    rows, tgt = [], []

    def add(x, t):
        rows.append(x)
        tgt.append(t)

    def base(v=-2.0):
        return torch.full((C,), v)

    def rnd():
        return torch.randn(C, generator=gen).to(dtype).float()

    # a constant row is in the top k iff t < k
    add(base(1.0), k - 1)
    add(base(1.0), k)
    # the target tied with the argmax, at the lower and at the higher index
    for t in (10, 20):
        x = base()
        x[10] = x[20] = 4.0
        add(x, t)
    # exactly k-1 and exactly k elements above the target
    for above in (k - 1, k):
        x = base()
        x[30:30 + above] = 5.0
        x[100] = 3.0
        add(x, 100)
    # k-1 above, one tie: at a lower index it pushes the target out, at a higher it does not
    for tie in (99, 101):
        x = base()
        x[30:30 + k - 1] = 5.0
        x[100] = x[tie] = 3.0
        add(x, 100)
    # +inf and -inf elements
    x = base()
    x[7], x[50] = INF, 1.0
    add(x, 50)
    x = base()
    x[7] = INF
    add(x, 7)
    x = base()
    x[0:6] = -INF
    add(x, 2)
    # a row of -inf: rank = t
    add(base(-INF), 1)
    add(base(-INF), k)
    # NaN beside the target, NaN first, NaN at the target, nothing but NaN
    x = rnd()
    x[11] = x[12] = NAN
    add(x, 40)
    x = rnd()
    x[0] = NAN
    add(x, 0 + 1)
    x = rnd()
    x[41] = NAN
    add(x, 41)
    add(base(NAN), 5)
    # +0.0 against -0.0: they tie, the index decides
    x = base(-1.0)
    x[10], x[20] = -0.0, 0.0
    add(x, 10)
    add(x.clone(), 20)
    x = base(-1.0)
    x[10], x[20] = 0.0, -0.0
    add(x, 20)
    # targets outside [0, C), ignored rows
    add(rnd(), -1)
    add(rnd(), C)
    if ig is not None:
        add(rnd(), ig)
        x = base()
        x[ig if ig >= 0 else 0] = 4.0
        add(x, ig)
    # random rows in the input dtype: bf16 ties often at C = 1000
    for _ in range(24):
        add(rnd(), int(torch.randint(0, C, (1,), generator=gen)))
    return torch.stack(rows).to(dtype), torch.tensor(tgt, dtype=torch.long)


def _rule_sum(batches, k, ig):
    total = None
    for p, t in batches:
        d = stat_rule_deltas(p, t, k, ig)
        total = d if total is None else tuple(a + b for a, b in zip(total, d))
    return total


def _states(coll):
    for m in coll.values(copy_state=False):
        m._maybe_flush_lazy()
    torch.cuda.synchronize()
    out = {}
    for name, m in coll.items(keep_base=True, copy_state=False):
        for s in m._defaults:
            out[f"{name}.{s}"] = getattr(m, s).clone()
    return out


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _assert_stat(states, name, want, what):
    for s, w in zip(("tp", "fp", "tn", "fn"), want):
        assert torch.equal(states[f"{name}.{s}"].cpu(), w), (what, name, s)


def _onepass_covers(C, dtype):
    epv = 8 if dtype == BF16 else 4
    return C > 128 and C % epv == 0 and C // epv <= 8 * 64


def _run(monkeypatch, kind, C, k, ig, batches, fuse):
    monkeypatch.setenv(_hip.ONEPASS_ENV, "2" if kind == "onepass" else "0")
    monkeypatch.setenv(_hip.FUSE_TOPK_ENV, fuse)
    coll = _make(kind, C, k, ig)
    for p, t in batches:
        coll.update(p.cuda(), t.cuda())
    values = {n: v.clone() for n, v in coll.compute().items()}
    return coll, _states(coll), values


@pytest.mark.parametrize("ig", [None, 3], ids=["noignore", "ignore3"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,dtype,B,k", SHAPES, ids=lambda v: _id(v))
def test_random_logits_match_rule_and_unfused_run(monkeypatch, C, dtype, B, k, kind, ig):
    gen = torch.Generator().manual_seed(1000 * C + B)
    batches = [_first_batch(C, B, dtype, gen)] + [_random_batch(C, B, dtype, gen) for _ in range(3)]
    steps = len(batches) - 1

    coll, got, values = _run(monkeypatch, kind, C, k, ig, batches, "1")
    plan = coll._fused_plan
    assert plan.topk is coll._modules["acck"]
    # C = 128 takes the thread-per-row kernel, which has no slot: unhandled, still right
    assert plan.topk_steps == (steps if C > 128 else 0)
    if kind == "onepass":
        assert plan.onepass_steps == (steps if _onepass_covers(C, dtype) else 0)
    _assert_stat(got, "acck", _rule_sum(batches, k, ig), "rule")
    _assert_stat(got, "acc1", _rule_sum(batches, None, ig), "rule")

    old_coll, old, old_values = _run(monkeypatch, kind, C, k, ig, batches, "0")
    assert old_coll._fused_plan.topk is None and old_coll._fused_plan.topk_steps == 0
    assert got.keys() == old.keys() and values.keys() == old_values.keys()
    for name, v in old.items():
        assert torch.equal(got[name], v), name
    for name, v in old_values.items():
        assert _same(values[name], v), name


# (C, dtype, k, kind, ignore_index)
EDGE_CASES = [
    (136, BF16, 5, "onepass", 3),
    (1000, BF16, 5, "onepass", 3),
    (1000, BF16, 2, "onepass", None),
    (520, FP32, 5, "onepass", -1),
    (4096, BF16, 65, "onepass", 3),
    (1000, BF16, 5, "twokernel", 3),
    (1001, BF16, 5, "twokernel", -1),
    (136, BF16, 2, "plain", 3),
    (1000, BF16, 65, "plain", None),
    (520, FP32, 5, "plain", 3),
    (1001, BF16, 5, "plain", 3),
    (130, BF16, 2, "plain", -1),
]


def _expected_value(C, k, ig, sums):
    """What ``acck`` computes from the rule's states, on the CPU path."""
    ref = ma.MulticlassAccuracy(top_k=k, average="macro", num_classes=C, ignore_index=ig, validate_args=False)
    ref.tp, ref.fp, ref.tn, ref.fn = sums
    ref._update_count = 1
    return ref.compute()


@pytest.mark.parametrize("C,dtype,k,kind,ig", EDGE_CASES, ids=lambda v: _id(v))
def test_edge_rows_and_protocol(monkeypatch, C, dtype, k, kind, ig):
    monkeypatch.setenv(_hip.ONEPASS_ENV, "2" if kind == "onepass" else "0")
    monkeypatch.setenv(_hip.FUSE_TOPK_ENV, "1")
    gen = torch.Generator().manual_seed(7 * C + k)
    b = [_first_batch(C, 5, dtype, gen)] + [_edge_batch(C, k, dtype, ig, gen) for _ in range(3)]
    b.append(_random_batch(C, 1, dtype, gen))
    # the third batch also misses 40 classes outright (target ranked last), so
    # the macro value after it is far from the one before
    miss = torch.zeros(40, C)
    miss[torch.arange(40), torch.arange(60, 100)] = -50.0
    b[2] = (torch.cat([b[2][0], miss.to(dtype)]), torch.cat([b[2][1], torch.arange(60, 100)]))
    # a macro mean of C ratios in [0, 1], summed in fp32 in any order, is off by
    # at most C * 2^-24 from the exact mean; both sides may be
    tol = 2 * C * 2.0 ** -24

    coll = _make(kind, C, k, ig)
    coll.update(b[0][0].cuda(), b[0][1].cuda())
    coll.update(b[1][0].cuda(), b[1][1].cuda())
    plan = coll._fused_plan
    assert plan.topk is coll._modules["acck"]
    want1 = _expected_value(C, k, ig, _rule_sum(b[:2], k, ig))
    v1 = coll.compute()["acck"].cpu()
    assert abs(float(v1) - float(want1)) <= tol

    # steady state: nothing may wait for the device
    p2, t2 = b[2][0].cuda(), b[2][1].cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        coll.update(p2, t2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # compute() between updates returns the value of the fresh states
    want2 = _expected_value(C, k, ig, _rule_sum(b[:3], k, ig))
    assert abs(float(want2) - float(want1)) > 10 * tol  # a stale value would show
    v2 = coll.compute()["acck"].cpu()
    assert abs(float(v2) - float(want2)) <= tol

    got = _states(coll)
    _assert_stat(got, "acck", _rule_sum(b[:3], k, ig), "edge rows")
    _assert_stat(got, "acc1", _rule_sum(b[:3], None, ig), "edge rows")
    assert plan.topk_steps == 2
    if kind == "onepass":
        assert plan.onepass_steps == 2

    # reset() replaces the states: the plan follows, the scratch is zero again
    coll.reset()
    coll.update(b[3][0].cuda(), b[3][1].cuda())
    coll.update(b[4][0].cuda(), b[4][1].cuda())
    got = _states(coll)
    _assert_stat(got, "acck", _rule_sum(b[3:], k, ig), "after reset")
    _assert_stat(got, "acc1", _rule_sum(b[3:], None, ig), "after reset")
    assert plan.topk_steps == 4
    if kind != "plain":
        _assert_stat(got, "f1k", _rule_sum(b[3:], k, ig), "group member")
