"""The "pending b0" histogram format of the one-pass step (csrc/mc_onepass.hip)
against the kernel sequence it replaces (METRICS_AMD_ONEPASS=0).

Between two flushes the curve leader's histogram lacks the elements of the
bucket of 0.0 of the rows k_mc_onepass binned from registers; P and R in the
curve scratch say how many, and every flush pays them (k_curve_resolve_pending).
All of it is integer counting, so raw states after ``_maybe_flush_lazy`` and
the ``compute()`` output must be ``torch.equal`` to the two-kernel path, for
every row kind, across every switch between the two writers of the histogram
and through every reader that can meet a pending histogram.

Shapes: bf16 C=136 and fp32 C=132 with T=5 non-uniform thresholds (b0 = 0),
bf16 C=1000 with T=200 linspace (thresholds[0] = 0.0, so b0 = 1); B = 5 (two
blocks) and 257 (a partial 256-row tile behind a full one in the tail).
"""
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip
from tests.unittests.gpu.test_onepass_tail import (
    _IGNORE, _assert_same, _compute, _preds, _run, _target,
)

pytestmark = pytest.mark.gpu

_T5 = [0.05, 0.2, 0.35, 0.6, 0.95]
_SHAPES = [(torch.bfloat16, 136, _T5), (torch.float32, 132, _T5), (torch.bfloat16, 1000, 200)]
_SHAPE_IDS = ["bf16-C136-T5", "fp32-C132-T5", "bf16-C1000-T200"]
_BATCHES = (5, 257)
# (preds kind, target kind); "nanrow": logits with one row of NaN and an in-range
# target: binned (P counts it) though count_row rejects it. "nanmixed":
# probabilities with one logit row that also holds a NaN: that row is binned
# from registers with a NaN row sum (its done mark must still read as done),
# every other row is deferred.
_KINDS = [("logits", "plain"), ("probs", "plain"), ("onelogit", "plain"), ("logits", "bad"),
          ("onelogit", "allignore"), ("onelogit", "someignore"), ("probs", "someignore"),
          ("nanrow", "plain"), ("nanmixed", "plain")]


def _batch(kind, B, C, dtype, gen):
    pk, tk = kind
    if pk == "nanrow":
        p = _preds("logits", B, C, dtype, gen)
        t = _target(tk, B, C, gen)
        p[B // 2] = float("nan")
        t[B // 2] = 5  # in range and not the ignore index
        return p, t
    if pk == "nanmixed":
        p = _preds("onelogit", B, C, dtype, gen)
        t = _target(tk, B, C, gen)
        p[B // 2, 1] = float("nan")
        t[B // 2] = 5
        return p, t
    return _preds(pk, B, C, dtype, gen), _target(tk, B, C, gen)


def _batches(kinds, B, C, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [_batch(k, B, C, dtype, gen) for k in kinds]


def _both(monkeypatch, C, thresholds, batches, script, fused_steps):
    """Run ``script`` under the one-pass step and under the kernel sequence;
    everything it snapshots, what it returns and the final compute() agree."""
    new, steps_new, extra_new = _run(monkeypatch, "2", C, thresholds, _IGNORE, batches, script)
    old, steps_old, extra_old = _run(monkeypatch, "0", C, thresholds, _IGNORE, batches, script)
    assert steps_old == 0 and steps_new == fused_steps
    _assert_same(new, old)
    if extra_new is not None:
        _assert_same(extra_new, extra_old)


def _is_pending(coll):
    return bool(coll.auroc.__dict__.get("_hip_b0_pending"))


@pytest.mark.parametrize("B", _BATCHES)
@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_forty_steps_between_flushes(monkeypatch, shape, B):
    dtype, C, thresholds = shape
    four = _batches([("logits", "plain"), ("logits", "someignore"), ("onelogit", "plain"),
                     ("logits", "bad")], B, C, dtype, seed=100 + C + B)

    def script(coll, batches, snap):
        coll.update(*batches[0])  # forms the compute groups, flushes
        snap()
        for i in range(40):
            coll.update(*batches[i % 4])
        assert _is_pending(coll) == (coll._fused_plan.onepass_steps > 0)
        snap()
        assert not _is_pending(coll)

    _both(monkeypatch, C, thresholds, four, script, 40)


@pytest.mark.parametrize("B", _BATCHES)
@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_row_kinds_alone_and_mixed(monkeypatch, shape, B):
    dtype, C, thresholds = shape
    first = _batches([("logits", "plain")], B, C, dtype, seed=7)

    def script(coll, batches, snap):
        for p, t in batches:  # no flush before the last update
            coll.update(p, t)
        snap()

    for n, kind in enumerate(_KINDS):
        batches = first + _batches([kind], B, C, dtype, seed=200 + n + C + B)
        _both(monkeypatch, C, thresholds, batches, script, 1)
    mixed = first + _batches(_KINDS, B, C, dtype, seed=300 + C + B)
    _both(monkeypatch, C, thresholds, mixed, script, len(_KINDS))


def _misaligned(p):
    """The same values in a contiguous tensor whose storage starts one element
    past a 16-byte boundary: the one-pass gate refuses it."""
    base = torch.empty(p.numel() + 1, dtype=p.dtype, device=p.device)
    view = base[1:].view(p.shape)
    view.copy_(p)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("B", _BATCHES)
@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_writer_switches(monkeypatch, shape, B):
    """Stand-alone first update (dirty, not pending) -> one-pass (flushes first,
    arms pending) -> a step the gate refuses (the two-kernel path: flushes the
    pending histogram first) -> one-pass again."""
    dtype, C, thresholds = shape
    batches = _batches([("logits", "plain"), ("logits", "plain"), ("onelogit", "someignore"),
                        ("logits", "someignore"), ("logits", "plain"), ("probs", "plain")],
                       B, C, dtype, seed=400 + C + B)
    seen = []

    def script(coll, batches, snap):
        plan = lambda: coll._fused_plan.onepass_steps if coll._fused_plan else 0  # noqa: E731
        coll.update(*batches[0])
        coll.update(*batches[1])
        coll.update(*batches[2])
        before = plan()
        coll.update(_misaligned(batches[3][0]), batches[3][1])
        seen.append((before, plan(), _is_pending(coll)))
        coll.update(*batches[4])
        coll.update(*batches[5])
        snap()

    _both(monkeypatch, C, thresholds, batches, script, 4)
    # under the one-pass mode the refused step took the other path, and left
    # the histogram in the other writer's format
    assert seen[0] == (2, 2, False) and seen[1] == (0, 0, False)


def _reader_compute_plan(coll, monkeypatch):
    return [_compute(coll)]


def _reader_compute_no_plan(coll, monkeypatch):
    with monkeypatch.context() as m:
        m.setenv(_hip.COMPUTE_PLAN_ENV, "0")
        return [_compute(coll)]


def _reader_state_dict(coll, monkeypatch):
    for m in coll.values(copy_state=False):
        m.persistent(True)
    return [{k: v.clone() for k, v in coll.state_dict().items()}]


def _reader_merge_state(coll, monkeypatch):
    # the pending leader is the incoming side: merge_state flushes it
    other = ma.MulticlassAUROC(num_classes=coll.auroc.num_classes, average="macro",
                               thresholds=coll.auroc.thresholds.clone(), validate_args=False,
                               ignore_index=_IGNORE).to("cuda")
    other.merge_state(coll.auroc)
    return [{"merged": other.confmat.clone()}]


def _reader_to_cpu(coll, monkeypatch):
    coll.to("cpu")
    out = [{"cpu": coll.auroc.confmat.clone().cuda()}]
    coll.to("cuda")
    return out


_READERS = {
    "compute_plan": _reader_compute_plan, "compute_no_plan": _reader_compute_no_plan,
    "state_dict": _reader_state_dict, "merge_state": _reader_merge_state, "to_cpu": _reader_to_cpu,
}


@pytest.mark.parametrize("reader", list(_READERS))
@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_every_reader_while_pending(monkeypatch, shape, reader):
    dtype, C, thresholds = shape
    B = 257
    batches = _batches([("logits", "plain"), ("logits", "someignore"), ("onelogit", "plain"),
                        ("logits", "plain")], B, C, dtype, seed=500 + C)

    def script(coll, batches, snap):
        coll.update(*batches[0])
        coll.update(*batches[1])
        coll.update(*batches[2])
        assert _is_pending(coll) == (coll._fused_plan.onepass_steps > 0)
        seen = _READERS[reader](coll, monkeypatch)
        assert not _is_pending(coll)
        coll.update(*batches[3])  # one more update, then the final compute()
        return seen

    # after a move to the CPU and back the states are new tensors; the fused
    # plan serves them all the same
    _both(monkeypatch, C, thresholds, batches, script, 3)


@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_forward_while_pending(monkeypatch, shape):
    """forward() flushes, updates every metric on its own and returns the batch
    values; the accumulated states must not lose what was pending."""
    dtype, C, thresholds = shape
    batches = _batches([("logits", "plain"), ("logits", "someignore"), ("logits", "plain"),
                        ("onelogit", "plain")], 257, C, dtype, seed=600 + C)

    def script(coll, batches, snap):
        coll.update(*batches[0])
        coll.update(*batches[1])
        seen = [{k: v.clone() for k, v in coll(*batches[2]).items()}]
        coll.update(*batches[3])
        snap()
        return seen

    new, _, seen_new = _run(monkeypatch, "2", C, thresholds, _IGNORE, batches, script)
    old, _, seen_old = _run(monkeypatch, "0", C, thresholds, _IGNORE, batches, script)
    _assert_same(new, old)
    _assert_same(seen_new, seen_old)


@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_reset_while_pending(monkeypatch, shape):
    dtype, C, thresholds = shape
    batches = _batches([("logits", "plain"), ("logits", "someignore"), ("onelogit", "plain")],
                       257, C, dtype, seed=700 + C)

    def script(coll, batches, snap):
        coll.update(*batches[0])
        coll.update(*batches[1])
        assert _is_pending(coll) == (coll._fused_plan.onepass_steps > 0)
        coll.reset()
        assert not _is_pending(coll)
        scratch = coll.auroc.__dict__.get("_hip_onepass_scratch")
        assert scratch is None or int(scratch[: 2 * C].abs().sum()) == 0
        coll.update(*batches[2])
        snap()

    _both(monkeypatch, C, thresholds, batches, script, 2)


@pytest.mark.parametrize("shape", _SHAPES, ids=_SHAPE_IDS)
def test_load_state_dict_while_pending(monkeypatch, shape):
    """The loaded states replace everything accumulated, pending rows included."""
    dtype, C, thresholds = shape
    batches = _batches([("logits", "plain"), ("logits", "someignore"), ("onelogit", "plain"),
                        ("logits", "plain")], 257, C, dtype, seed=800 + C)

    def script(coll, batches, snap):
        for m in coll.values(copy_state=False):
            m.persistent(True)
        coll.update(*batches[0])
        coll.update(*batches[1])
        saved = {k: v.clone() for k, v in coll.state_dict().items()}
        coll.update(*batches[2])
        assert _is_pending(coll) == (coll._fused_plan.onepass_steps > 0)
        coll.load_state_dict(saved)
        assert not _is_pending(coll)
        snap()
        coll.update(*batches[3])
        snap()

    new, steps_new, _ = _run(monkeypatch, "2", C, thresholds, _IGNORE, batches, script)
    old, steps_old, _ = _run(monkeypatch, "0", C, thresholds, _IGNORE, batches, script)
    assert steps_new > 0 and steps_old == 0
    _assert_same(new, old)


def test_graphed_after_pending_is_armed(monkeypatch):
    """A one-pass step arms pending, then GraphedUpdate captures the fused step
    and replays it three times; the flush after the replays pays what the
    captured steps left out."""
    dtype, C, B = torch.bfloat16, 1000, 257
    batches = _batches([("logits", "plain"), ("logits", "plain"), ("onelogit", "someignore"),
                        ("logits", "someignore"), ("probs", "someignore")], B, C, dtype, seed=31)

    def script(coll, batches, snap):
        coll.update(*batches[0])  # forms the compute groups
        coll.update(*batches[1])
        armed = _is_pending(coll)
        # parallel=False: the capture goes through MetricCollection.update
        graphed = ma.graphs.GraphedUpdate(coll, *batches[0], parallel=False)
        assert not _is_pending(coll)  # the construction resets the states in place
        for p, t in batches[2:]:
            graphed.update(p, t)
        assert _is_pending(coll) == armed
        snap()
        assert not _is_pending(coll)
        return [{"armed": torch.tensor(armed)}]

    new, _, armed_new = _run(monkeypatch, "2", C, 200, _IGNORE, batches, script)
    old, _, armed_old = _run(monkeypatch, "0", C, 200, _IGNORE, batches, script)
    assert bool(armed_new[0]["armed"]) and not bool(armed_old[0]["armed"])
    _assert_same(new, old)
