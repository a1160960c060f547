"""The one-pass step against results recorded from the commit before the
row-fold rewrite (range test per group, value-first argmax, branch-free
merges, native step plan).

The path-against-path tests (test_onepass_update.py) cannot pin "bit-identical
to the parent": both paths share the changed fold. This fixture can. It was
recorded ONCE, on an MI355X, from commit 6aa92f0 with this file copied into
that tree:

    python tests/unittests/gpu/test_onepass_parent_golden.py tests/golden/onepass_parent.pt

i.e. ``_record()`` below: for C in (1000, 136) and bf16 / fp32 it draws 5 rows
(seeded, on the CPU): four rows of logits and one probability row (row 2, a
softmax, every element in [0,1] — the row the tail kernel bins), runs
``_run_case`` and stores the inputs with what it returned. The test feeds the
stored inputs to ``_run_case`` again and asserts equality:

- the bits of rowmax / rowinv after the last step,
- tp / fp / tn / fn and correct / total,
- SHA-256 of the bytes of the confusion matrix and of the flushed curve state,

after one ungrouped update and two fused ones.
"""
import hashlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_FIXTURE = os.path.join(os.path.dirname(__file__), "..", "..", "golden", "onepass_parent.pt")
_CASES = [(C, dt) for C in (1000, 136) for dt in ("bf16", "fp32")]
_DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
_T = 50
_B = 5


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _run_case(preds, target, C):
    """Three updates of the same batch (the first forms the compute groups, two
    go through the fused plan) with METRICS_AMD_ONEPASS=2 in the environment."""
    import metrics_amd as ma

    kw = dict(num_classes=C, validate_args=False, ignore_index=None)
    coll = ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(average="micro", **kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(average="macro", thresholds=_T, **kw),
    }).to("cuda")
    p, t = preds.cuda(), target.cuda()
    for _ in range(3):
        coll.update(p, t)
    assert coll._fused_plan.onepass_steps == 2
    for m in coll.values(copy_state=False):
        m._maybe_flush_lazy()
    torch.cuda.synchronize()
    rows = coll._fused_plan.curve.__dict__["_hip_rowstats_buf"][:, :_B]
    acc, ex = coll.acc, coll.exact
    return {
        "rowmax_bits": rows[0].contiguous().view(torch.int32).cpu(),
        "rowinv_bits": rows[1].contiguous().view(torch.int32).cpu(),
        "tp": acc.tp.cpu(), "fp": acc.fp.cpu(), "tn": acc.tn.cpu(), "fn": acc.fn.cpu(),
        "correct": ex.correct.cpu(), "total": ex.total.cpu(),
        "confmat_sha256": _sha(coll.confmat.confmat),
        "curve_sha256": _sha(coll.auroc.confmat),
    }


def _record(path):
    os.environ["METRICS_AMD_ONEPASS"] = "2"
    out = {}
    for C, dt in _CASES:
        gen = torch.Generator().manual_seed(9000 + C + (1 if dt == "bf16" else 0))
        logits = torch.randn(_B, C, generator=gen) * 3.0
        preds = logits.to(_DTYPES[dt])
        preds[2] = torch.softmax(logits[2], dim=0).to(_DTYPES[dt])
        target = torch.randint(0, C, (_B,), generator=gen)
        want = _run_case(preds, target, C)
        for k in ("tp", "fp", "tn", "fn"):  # counts <= 15: int16 keeps the file small
            assert int(want[k].max()) < 2 ** 15 and int(want[k].min()) >= 0
            want[k] = want[k].to(torch.int16)
        out[f"{C}-{dt}"] = {"preds": preds, "target": target, "want": want}
    torch.save(out, path)


@pytest.fixture(scope="module")
def golden():
    return torch.load(_FIXTURE, map_location="cpu")


@pytest.mark.parametrize("case", [f"{C}-{dt}" for C, dt in _CASES])
def test_bit_identical_to_parent(monkeypatch, golden, case):
    from metrics_amd.ops import _hip

    g = golden[case]
    monkeypatch.setenv(_hip.ONEPASS_ENV, "2")
    got = _run_case(g["preds"], g["target"], int(case.split("-")[0]))
    assert got.keys() == g["want"].keys()
    for k, want in g["want"].items():
        if isinstance(want, str):
            assert got[k] == want, k
        else:
            assert torch.equal(got[k], want.to(got[k].dtype)), (k, got[k], want)


if __name__ == "__main__":
    sys.path.insert(0, os.getcwd())
    _record(sys.argv[1])
