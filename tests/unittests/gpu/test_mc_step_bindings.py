"""The count and apply bindings of the multiclass step, called directly.

``mc_step_count`` + ``mc_step_apply`` over one step record (``_hip.mc_step``)
for every group of participants a caller builds: stat, stat + exact, stat +
top-k, stat + exact + top-k, exact only, confmat only; each with and without
``close_epoch``, at C = 7 (thread-per-row kernel, which has no top-k slot) and
C = 130 (the smallest range of the streaming kernel, which has it), B = 33
rows (not a multiple of the four waves of a block), fp32 logits, bf16 logits
and label predictions, ``ignore_index`` None and 3. One row of the logits is
all-equal (argmax tie: the lowest index wins), one target equals 3. Two steps
run into the same count blocks.

Expected values are exact integers from torch on the CPU: argmax, the per-row
rule of ``_topk_rule`` and bincount; everything is compared with
``torch.equal``. After each step the count block and the top-k block are all
zero again and ``E[1]`` has advanced exactly when ``close_epoch`` asked.

Where the slot is asked for but not there (C = 7, label predictions) the count
binding raises (-103), launches nothing and leaves every buffer as it was.
The confmat-only record has nothing for an apply pass to consume: its count
block is the sink that is never zeroed, so there it must hold the running
counts, and apply only closes the epoch.
"""
import functools

import pytest
import torch

from metrics_amd.ops import _hip
from tests.unittests._topk_rule import stat_rule_deltas

pytestmark = pytest.mark.gpu

B, K, IGNORE, STEPS, INIT = 33, 3, 3, 2, 5
GROUPS = {
    "stat": ("stat",),
    "stat+exact": ("stat", "exact"),
    "stat+topk": ("stat", "topk"),
    "stat+exact+topk": ("stat", "exact", "topk"),
    "exact": ("exact",),
    "confmat": ("confmat",),
}


@functools.lru_cache(maxsize=None)
def _batches(C, kind):
    """STEPS (preds, target) CPU batches, made once per shape and kind."""
    g = torch.Generator().manual_seed(1000 * C + len(kind))
    out = []
    for _ in range(STEPS):
        target = torch.randint(0, C, (B,), generator=g)
        target[2] = IGNORE
        if kind == "labels":
            preds = torch.randint(0, C, (B,), generator=g)
            preds[2] = IGNORE  # a hit on the row that ignore_index drops
        else:
            preds = torch.randn(B, C, generator=g).to(torch.bfloat16 if kind == "bf16" else torch.float32)
            preds[5] = 0.25  # all-equal row: argmax 0
            preds[2, IGNORE] = 9.0
        out.append((preds, target))
    return out


@functools.lru_cache(maxsize=None)
def _expected(C, kind, ignore_index):
    """Per step: (top-1 deltas, top-k deltas | None, confmat delta, valid)."""
    out = []
    for preds, target in _batches(C, kind):
        if kind == "labels":
            x = torch.nn.functional.one_hot(preds, C).float()
            topk = None
        else:
            x = preds.float()
            assert int(x[5].argmax()) == 0
            topk = stat_rule_deltas(x, target, k=K, ignore_index=ignore_index)
        top1 = stat_rule_deltas(x, target, ignore_index=ignore_index)
        valid = torch.ones(B, dtype=torch.bool) if ignore_index is None else target != ignore_index
        a = x.argmax(1)
        cm = torch.bincount(target[valid] * C + a[valid], minlength=C * C).reshape(C, C)
        # the rule and plain argmax + bincount agree on the top-1 slot
        assert torch.equal(top1[0], cm.diagonal()) and torch.equal(top1[1], cm.sum(0) - cm.diagonal())
        out.append((top1, topk, cm, int(valid.sum())))
    return out


def _state(n, dev):
    return torch.full((n,), INIT, dtype=torch.long, device=dev)


@pytest.mark.parametrize("close_epoch", [False, True], ids=["keep", "close"])
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("ignore_index", [None, IGNORE], ids=["noignore", "ignore3"])
@pytest.mark.parametrize("kind", ["fp32", "bf16", "labels"])
@pytest.mark.parametrize("C", [7, 130])
def test_count_and_apply(C, kind, ignore_index, group, close_epoch):
    dev = torch.device("cuda")
    parts = GROUPS[group]
    named = {"counts": torch.zeros(3 * C + 1, dtype=torch.long, device=dev)}
    if "stat" in parts:
        named.update({n: _state(C, dev) for n in ("tp", "fp", "tn", "fn")})
    if "exact" in parts:
        named.update(correct=_state(1, dev), total=_state(1, dev))
    if "confmat" in parts:
        named["confmat"] = _state(C * C, dev).reshape(C, C)
    if "topk" in parts:
        named["topk_counts"] = torch.zeros(3 * C, dtype=torch.long, device=dev)
        named.update({n: _state(C, dev) for n in ("tp_k", "fp_k", "tn_k", "fn_k")})
    # the epoch buffer is always there: an apply that was not asked must leave it
    named["epoch_buf"] = torch.zeros(2, dtype=torch.int32, device=dev)
    if kind != "labels":
        named["rowstats"] = torch.empty(2, B, dtype=torch.float32, device=dev)
    t = _hip.McStepTensors(**named)
    rec = _hip.mc_step(C, ignore_index, t, k=K if "topk" in parts else 0)
    batches = [(p.to(dev), y.to(dev)) for p, y in _batches(C, kind)]

    if "topk" in parts and (kind == "labels" or not _hip.mc_stat_topk_covers(C)):
        before = [x.clone() for x in t if x is not None and x is not t.rowstats]
        with pytest.raises(RuntimeError, match="-103"):
            _hip.mc_step_count(rec, *batches[0])
        torch.cuda.synchronize()
        after = [x for x in t if x is not None and x is not t.rowstats]
        assert all(torch.equal(a, b) for a, b in zip(after, before))
        return

    want = {n: torch.full_like(x, INIT).cpu() for n, x in zip(t._fields, t)
            if x is not None and n not in ("counts", "topk_counts", "rowstats", "epoch_buf")}
    sink = torch.zeros(3 * C + 1, dtype=torch.long)
    for step, (batch, (top1, topk, cm, valid)) in enumerate(zip(batches, _expected(C, kind, ignore_index)), 1):
        assert _hip.mc_step_count(rec, *batch) == B
        _hip.mc_step_apply(rec, B, close_epoch)
        if "stat" in parts:
            for n, d in zip(("tp", "fp", "tn", "fn"), top1):
                want[n] += d
        if "topk" in parts:
            for n, d in zip(("tp_k", "fp_k", "tn_k", "fn_k"), topk):
                want[n] += d
        if "exact" in parts:
            want["correct"] += int(top1[0].sum()) + (B - valid)
            want["total"] += B
        if "confmat" in parts:
            want["confmat"] += cm
            sink += torch.cat([top1[0], top1[1], top1[3], torch.tensor([valid])])
        for n, w in want.items():
            assert torch.equal(getattr(t, n).cpu(), w), (n, step)
        assert torch.equal(t.counts.cpu(), sink), step
        if "topk" in parts:
            assert not bool(t.topk_counts.any()), step
        assert int(t.epoch_buf[1]) == (step if close_epoch else 0)
