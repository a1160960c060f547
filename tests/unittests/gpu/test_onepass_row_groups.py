"""Row groups of the one-pass step (csrc/mc_onepass.hip, template parameter
LPR): a wave holds 64 / LPR rows at once, LPR lanes each.

Every state is an integer count and the row statistics keep the summation
order of the one-row-per-wave kernel (virtual lanes, row_fold.h), so every
comparison is exact: the forced one-pass step under every supported
``MA_ONEPASS_LPR``, with the row prefetch (``MA_ONEPASS_PREFETCH``) off and on,

* against the kernel sequence it replaces (``METRICS_AMD_ONEPASS=0``): stat
  states, confusion matrix, exact-match counts, flushed curve confmat;
* against LPR = 64: the same states plus the bits of rowmax / rowinv after every
  update.

Shapes are the smallest at which the group mapping can break. bf16 C = 136 is 17
vectors (one lane of a 16-lane group holds a second), 256 and 1024 fit a group
width exactly, 1000 is the bench shape with a ragged tail, 1032 the first NV = 4
shape (LPR >= 32 only); fp32 C = 132 / 500 / 512 / 516 are the same edges for 4
elements per vector. B = 1, 3, 4, 5, 67: fewer rows than groups, a full wave
task, a partial last wave, a block tail. Thresholds: 5 and 200 uniform, and a
non-uniform list.

The rows put different fates into one wave (``_fate_rows``); with B rows per
update the list is walked in as many updates as it takes.
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip
from tests.unittests.gpu.test_onepass_tail import _IGNORE, _make, _states

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
INF, NAN = float("inf"), float("nan")
_SHAPES = [(BF16, 136), (BF16, 256), (BF16, 1000), (BF16, 1024), (BF16, 1032),
           (FP32, 132), (FP32, 500), (FP32, 512), (FP32, 516)]
_SHAPE_IDS = [("bf16" if d is BF16 else "fp32") + f"-C{c}" for d, c in _SHAPES]
_BATCHES = (1, 3, 4, 5, 67)
_THRESHOLDS = {"T5": 5, "T200": 200, "list": [0.05, 0.2, 0.35, 0.6, 0.95]}


def _fate_rows(C, dtype, gen):
    """(row, target) pairs, every value exact in bf16. EPV elements make a
    16-byte vector; lane l of a 16-lane group holds vectors l, l + 16, ..."""
    epv = 8 if dtype is BF16 else 4
    nvec = C // epv
    out = []

    def logits():
        return (torch.randn(C, generator=gen) * 3.0).to(dtype).float()

    def probs():
        return torch.softmax(torch.randn(C, generator=gen) * 3.0, dim=0).to(dtype).float()

    def tgt():
        t = int(torch.randint(0, C, (1,), generator=gen))
        return t if t != _IGNORE else t + 1

    out.append((logits(), tgt()))
    out.append((probs(), tgt()))           # deferred, between logit rows
    out.append((logits(), _IGNORE))        # ignored
    out.append((logits(), -1))             # targets out of range
    out.append((logits(), C))
    out.append((torch.full((C,), NAN), 5))   # all NaN: deferred, rejected by count_row
    out.append((torch.full((C,), -INF), 7))  # all -inf
    x = logits()
    x[C // 2] = INF
    out.append((x, C // 2))
    # the argmax tied between two lanes of a group: vectors 5 and 6
    x = logits()
    x[5 * epv + 1] = x[6 * epv] = 40.0
    out.append((x, 6 * epv))
    # tied between virtual lanes of one lane: vectors 0 and 16 (lane 0 of a
    # 16-lane group), and vector 32 where the row has one (a 32-lane group)
    x = logits()
    x[3] = x[16 * epv] = 40.0
    if nvec > 32:
        x[32 * epv + 1] = 40.0
    out.append((x, 16 * epv))
    # the lower index in the higher virtual lane of another lane
    x = logits()
    x[16 * epv + 2] = x[(nvec - 1) * epv + epv - 1] = 40.0
    out.append((x, (nvec - 1) * epv + epv - 1))
    # a NaN next to an element outside [0,1] in an otherwise in-range row:
    # binned from registers with rinv = NaN (the done-mark case)
    x = probs()
    x[9], x[10] = NAN, 2.0
    out.append((x, 10))
    out.append((logits(), tgt()))
    return out


def _updates(C, B, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    fates = _fate_rows(C, dtype, gen)
    n_updates = -(-len(fates) // B)
    batches = []
    for u in range(n_updates):
        rows = [fates[(u * B + i) % len(fates)] for i in range(B)]
        p = torch.stack([r for r, _ in rows]).to(dtype).cuda()
        t = torch.tensor([t for _, t in rows], dtype=torch.long).cuda()
        batches.append((p, t))
    # the first update runs every metric on its own; the fused plan serves the rest
    return [batches[0]] + batches


def _lprs(monkeypatch, dtype, C, T):
    """The LPR values the shape supports, found by asking for each."""
    lib = _hip._lib()
    dt = 1 if dtype is BF16 else 0
    got = []
    with monkeypatch.context() as m:
        for want in (64, 32, 16):
            m.setenv("MA_ONEPASS_LPR", str(want))
            eff = lib.ma_mc_onepass_lpr(dt, C, T)
            assert eff >= want and eff in (16, 32, 64)
            if eff not in got:
                got.append(eff)
    nv = lib.ma_mc_onepass_nv(dt, C, T)
    assert got == {1: [64, 32, 16], 2: [64, 32, 16], 4: [64, 32], 8: [64]}[nv]
    return got


def _run(monkeypatch, mode, lpr, make, thresholds, batches, rowstats=True, prefetch=None):
    with monkeypatch.context() as m:
        m.setenv(_hip.ONEPASS_ENV, mode)
        if lpr is not None:
            m.setenv("MA_ONEPASS_LPR", str(lpr))
        if prefetch is not None:
            m.setenv("MA_ONEPASS_PREFETCH", prefetch)
        coll = make().to("cuda")
        rows = []
        for n, (p, t) in enumerate(batches):
            coll.update(p, t)
            if n > 0 and mode != "0" and rowstats:
                buf = coll._fused_plan.curve.__dict__["_hip_rowstats_buf"]
                rows.append(buf[:, : p.shape[0]].clone().view(torch.int32))
        return coll, rows


def _assert_states(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_every_lpr_matches_two_kernel_and_lpr64(monkeypatch, shape):
    dtype, C = shape
    for thr_name, thresholds in _THRESHOLDS.items():
        T = thresholds if isinstance(thresholds, int) else len(thresholds)
        lprs = _lprs(monkeypatch, dtype, C, T)
        for B in _BATCHES:
            batches = _updates(C, B, dtype, seed=C * 100 + B)
            make = lambda: _make(C, thresholds, _IGNORE)  # noqa: E731
            coll, _ = _run(monkeypatch, "0", None, make, thresholds, batches)
            assert coll._fused_plan.onepass_steps == 0
            two_kernel = _states(coll)
            base_states, base_rows = None, None
            # 64 without the prefetch first; the prefetch variant exists for
            # slices of up to 4 vectors per lane, elsewhere "1" runs the plain kernel
            for lpr, pf in [(v, pf) for v in lprs for pf in ("0", "1")]:
                coll, rows = _run(monkeypatch, "2", lpr, make, thresholds, batches, prefetch=pf)
                assert coll._fused_plan.onepass_steps == len(batches) - 1
                states = _states(coll)
                _assert_states(states, two_kernel, (thr_name, B, lpr, pf, "two-kernel"))
                if base_states is None:
                    base_states, base_rows = states, rows
                    continue
                _assert_states(states, base_states, (thr_name, B, lpr, pf, "lpr64"))
                for u, (got, want) in enumerate(zip(rows, base_rows)):
                    assert torch.equal(got, want), (thr_name, B, lpr, pf, "rowstats of update", u + 1)


@pytest.mark.parametrize("shape", [(BF16, 1000), (FP32, 132)], ids=["bf16-C1000", "fp32-C132"])
def test_two_updates_then_flush(monkeypatch, shape):
    """Pending-b0 identity: two one-pass updates leave the histogram pending,
    the flush pays bucket b0; the flushed curve equals the two-kernel one."""
    dtype, C = shape
    batches = _updates(C, 67, dtype, seed=5)
    batches = batches + batches[-1:]  # stand-alone update, then two fused ones
    make = lambda: _make(C, 200, _IGNORE)  # noqa: E731
    coll, _ = _run(monkeypatch, "0", None, make, 200, batches)
    want = _states(coll)
    for lpr, pf in [(v, pf) for v in _lprs(monkeypatch, dtype, C, 200) for pf in ("0", "1")]:
        coll, _ = _run(monkeypatch, "2", lpr, make, 200, batches, prefetch=pf)
        assert coll._fused_plan.onepass_steps == 2
        assert bool(coll.auroc.__dict__.get("_hip_b0_pending"))
        got = _states(coll)  # flushes
        assert not bool(coll.auroc.__dict__.get("_hip_b0_pending"))
        _assert_states(got, want, (lpr, pf))


def _make_topk(C, k):
    kw = dict(num_classes=C, validate_args=False, ignore_index=_IGNORE)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),
        "acck": ma.MulticlassAccuracy(top_k=k, average="macro", **kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=5, **kw),
    })


@pytest.mark.parametrize("shape", [(BF16, 136), (BF16, 1000), (FP32, 516)],
                         ids=["bf16-C136", "bf16-C1000", "fp32-C516"])
def test_topk_collection(monkeypatch, shape):
    """The top-k slot: x[t] comes from another lane of the group, the rank is a
    group sum; rows with and without a rank to count share a wave."""
    dtype, C = shape
    k = 3
    batches = _updates(C, 67, dtype, seed=9)
    # targets near the top: ranks on both sides of k among the plain rows
    p, t = batches[-1]
    order = p.float().nan_to_num(nan=-INF).argsort(dim=1, descending=True)
    for i in range(0, 67, 13):
        t[i] = order[i, (i // 13) % 5]
    make = lambda: _make_topk(C, k)  # noqa: E731

    def states(coll):
        s = _states(coll)
        a = coll.acck
        s.update({"tpk": a.tp.clone(), "fpk": a.fp.clone(), "tnk": a.tn.clone(), "fnk": a.fn.clone()})
        return s

    coll, _ = _run(monkeypatch, "0", None, make, 5, batches)
    want = states(coll)
    assert int(want["tpk"].sum()) > int(want["tp"].sum())  # the slot counted something top-1 did not
    for lpr, pf in [(v, pf) for v in _lprs(monkeypatch, dtype, C, 5) for pf in ("0", "1")]:
        coll, _ = _run(monkeypatch, "2", lpr, make, 5, batches, prefetch=pf)
        assert coll._fused_plan.onepass_steps == len(batches) - 1
        _assert_states(states(coll), want, (lpr, pf))
