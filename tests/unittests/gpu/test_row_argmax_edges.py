"""Row argmax of the fused multiclass step on crafted rows, against plain torch.

The one-pass kernel finds the row maximum by value and looks the index up
afterwards; the two-kernel path carries (value, index) through the fold. Both
must give: the LOWEST index among the non-NaN elements equal to the maximum
over the non-NaN elements; a row with no non-NaN element is not counted. From
that prediction the oracle below builds tp / fp / tn / fn, the confusion matrix
and correct / total, compared with ``torch.equal`` for METRICS_AMD_ONEPASS=2
and =0.

Every crafted value is a small integer, a half, a zero, an infinity or NaN, so
bf16 holds it exactly. A lane of the one-pass kernel holds vectors ``l`` and
``l + 64`` of the row (8 bf16 or 4 fp32 elements each): element ``i`` of them
has index ``epv*l + i`` and ``epv*(l + 64) + i``.
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

_IGNORE = 3
_NAN, _INF = float("nan"), float("inf")


def _make(C):
    kw = dict(num_classes=C, validate_args=False, ignore_index=_IGNORE)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=5, **kw),
    })


def _rows(C, dtype):
    """Crafted rows as a (B, C) float32 CPU tensor (exact in bf16)."""
    epv = 8 if dtype == torch.bfloat16 else 4
    nvec = C // epv
    base = -(1.0 + (torch.arange(C) % 7).float())  # -1 ... -7
    rows = []

    def tie(*idx, fill=base, value=3.0):
        r = fill.clone()
        for i in idx:
            assert 0 <= i < C
            r[i] = value
        rows.append(r)

    tie(epv * 5 + 1, epv * 5 + epv - 1)                 # inside one 16-byte vector
    if nvec > 64:                                       # the two vectors of one lane
        lane = min(2, nvec - 65)
        tie(epv * (lane + 64) + 1, epv * lane + 1)
    tie(epv * 3 + 2, epv * 4 + 2)                       # neighbouring lanes
    hi = min(37, nvec - 1)                              # lane in the upper wave half, if there is one
    tie(epv * 5, epv * hi)
    tie(epv * 9 + 3, epv * (nvec - 1) + 3, C - 1)       # three-way, the last vector among them
    tie(0)                                              # maximum at index 0
    tie(0, C - 1)
    tie(C - 1)                                          # maximum at index C-1: the ragged last vector
    tie(C - 2, C - 1)
    r = base.clone(); r[10] = -0.0; r[20] = 0.0; rows.append(r)     # +0.0 ties -0.0
    r = base.clone(); r[10] = 0.0; r[20] = -0.0; rows.append(r)
    r = base.clone(); r[C - 1] = 0.0; r[epv * 4] = -0.0; rows.append(r)
    rows.append(torch.full((C,), -_INF))                            # all -inf -> index 0
    r = torch.full((C,), -_INF); r[:3] = _NAN; rows.append(r)       # -inf with NaN in front -> 3
    r = torch.full((C,), -_INF); r[: epv * 2 + 1] = _NAN; rows.append(r)
    r = torch.full((C,), _NAN); r[77] = -5.0; rows.append(r)        # NaN with one finite element
    r = torch.full((C,), _NAN); r[C - 1] = -_INF; rows.append(r)
    rows.append(torch.full((C,), _NAN))                             # all NaN: not counted
    r = base.clone(); r[4] = _NAN; r[5] = 3.0; r[6] = _NAN; r[epv * min(20, nvec - 1)] = 3.0; rows.append(r)
    r = base.clone(); r[40] = _INF; r[41] = _INF; rows.append(r)    # +inf tie
    if dtype == torch.float32:
        lowest = torch.finfo(torch.float32).min                     # below the softmax fold's start value
        r = torch.full((C,), -_INF); r[50] = lowest; r[90] = lowest; rows.append(r)
        rows.append(torch.full((C,), lowest))
        r = torch.full((C,), lowest); r[:2] = _NAN; rows.append(r)
    return torch.stack(rows)


def _predict(x):
    """(prediction, row has a non-NaN element) by the rule in the module docstring."""
    x = x.float()
    nan = torch.isnan(x)
    xm = torch.where(nan, torch.full_like(x, -_INF), x)
    mx = xm.max(dim=1, keepdim=True).values
    hit = (xm == mx) & ~nan
    return hit.float().argmax(dim=1), (~nan).any(dim=1)


def _expected(batches, C):
    tp, fp, fn = (torch.zeros(C, dtype=torch.long) for _ in range(3))
    tn = torch.zeros(C, dtype=torch.long)
    cm = torch.zeros(C, C, dtype=torch.long)
    correct = total = 0
    for preds, target in batches:
        pred, has = _predict(preds.cpu())
        t = target.cpu()
        valid = has & (t != _IGNORE) & (t >= 0) & (t < C)
        pv, tv = pred[valid], t[valid]
        same = pv == tv
        tp += torch.bincount(tv[same], minlength=C)
        fp += torch.bincount(pv[~same], minlength=C)
        fn += torch.bincount(tv[~same], minlength=C)
        cm += torch.bincount(tv * C + pv, minlength=C * C).view(C, C)
        nvalid = int(valid.sum())
        # exact match: a row that is not counted cannot be a mismatch
        correct += int(same.sum()) + (len(t) - nvalid)
        total += len(t)
    n = int(cm.sum())
    tn = n - tp - fp - fn
    return {"tp": tp, "fp": fp, "tn": tn, "fn": fn, "confmat": cm,
            "correct": torch.tensor(correct), "total": torch.tensor(total)}


@pytest.fixture(scope="module", params=[(C, dt) for C in (136, 520, 1000, 1024)
                                        for dt in (torch.bfloat16, torch.float32)],
                ids=lambda p: f"C{p[0]}-{'bf16' if p[1] == torch.bfloat16 else 'fp32'}")
def case(request):
    """Batches and the oracle's states, computed once and shared by both modes."""
    C, dtype = request.param
    gen = torch.Generator().manual_seed(77 + C)
    # the first update runs every metric on its own (no fused kernel): plain logits
    plain = (torch.randn(8, C, generator=gen) * 3.0).to(dtype)
    plain_t = torch.randint(0, C, (8,), generator=gen)
    plain_t[plain_t == _IGNORE] = _IGNORE + 1
    edge = _rows(C, dtype).to(dtype)
    assert edge.shape[0] <= 64
    pred, _ = _predict(edge)
    t = torch.randint(0, C, (edge.shape[0],), generator=gen)
    t[::2] = pred[::2]          # every other row is a hit where it counts
    t[1] = _IGNORE              # an ignored row ...
    t[3] = C                    # ... and two out-of-range targets
    t[5] = -1
    batches = [(plain, plain_t), (edge, t), (edge.flip(0), t.flip(0))]
    return C, batches, _expected(batches, C)


@pytest.mark.parametrize("mode", ["2", "0"])
def test_argmax_edge_rows(monkeypatch, case, mode):
    C, batches, want = case
    monkeypatch.setenv(_hip.ONEPASS_ENV, mode)
    coll = _make(C).to("cuda")
    for p, t in batches:
        coll.update(p.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert coll._fused_plan.onepass_steps == (2 if mode == "2" else 0)
    got = {"tp": coll.acc.tp, "fp": coll.acc.fp, "tn": coll.acc.tn, "fn": coll.acc.fn,
           "confmat": coll.confmat.confmat, "correct": coll.exact.correct, "total": coll.exact.total}
    for k, v in want.items():
        assert torch.equal(got[k].cpu().reshape(v.shape), v), (k, got[k], v)
