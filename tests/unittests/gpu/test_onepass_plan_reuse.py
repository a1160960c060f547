"""The native step plan of the one-pass update across everything that replaces
or keeps the tensors it points at: update, ``reset()``, update, ``.to()`` of the
collection to the same device, update, and a changed batch size (a larger batch
reallocates the row-stats buffer).

The states must equal (``torch.equal``) those of a fresh collection fed the
batches since the reset, and those of the same sequence on the two-kernel path
(METRICS_AMD_ONEPASS=0), which has no plan at all. ``onepass_steps`` must count
every fused step.
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu


def _make(C):
    kw = dict(num_classes=C, validate_args=False, ignore_index=None)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=20, **kw),
    })


def _states(coll):
    for m in coll.values(copy_state=False):
        m._maybe_flush_lazy()
    torch.cuda.synchronize()
    return {
        "tp": coll.acc.tp.clone(), "fp": coll.acc.fp.clone(), "tn": coll.acc.tn.clone(),
        "fn": coll.acc.fn.clone(), "confmat": coll.confmat.confmat.clone(),
        "correct": coll.exact.correct.clone(), "total": coll.exact.total.clone(),
        "curve": coll.auroc.confmat.clone(),
    }


def _sequence(coll, b):
    coll.update(*b[0])   # every metric on its own; forms the compute groups
    coll.update(*b[1])   # builds the plan
    coll.reset()         # fresh state tensors: the plan must follow them
    coll.update(*b[2])
    coll.update(*b[3])   # reuses it
    coll = coll.to("cuda")
    coll.update(*b[4])
    coll.update(*b[5])   # larger batch
    coll.update(*b[6])   # smaller batch, same buffers
    return _states(coll), coll._fused_plan.onepass_steps


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [136, 1000])
def test_plan_follows_reset_move_and_batch_size(monkeypatch, C, dtype):
    gen = torch.Generator(device="cuda").manual_seed(11 + C)
    sizes = [5, 5, 5, 5, 5, 64, 3]
    b = []
    for n, B in enumerate(sizes):
        p = torch.randn(B, C, generator=gen, device="cuda") * 3.0
        if n == 3:
            p = torch.softmax(p, dim=1)  # one all-deferred batch on the way
        b.append((p.to(dtype), torch.randint(0, C, (B,), generator=gen, device="cuda")))

    monkeypatch.setenv(_hip.ONEPASS_ENV, "2")
    got, steps = _sequence(_make(C).to("cuda"), b)
    assert steps == 6  # every update but the first

    fresh = _make(C).to("cuda")
    for p, t in b[2:]:
        fresh.update(p, t)
    want = _states(fresh)
    assert fresh._fused_plan.onepass_steps == 4
    for k, v in want.items():
        assert torch.equal(got[k], v), k

    monkeypatch.setenv(_hip.ONEPASS_ENV, "0")
    old, steps_old = _sequence(_make(C).to("cuda"), b)
    assert steps_old == 0
    for k, v in old.items():
        assert torch.equal(got[k], v), k
