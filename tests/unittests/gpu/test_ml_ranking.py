"""The multilabel ranking kernel (``csrc/ml_rank.hip``) on the GPU:
``MultilabelCoverageError``, ``MultilabelRankingAveragePrecision`` and
``MultilabelRankingLoss``, their functionals and the collection plan.

Oracle: ``_ranking_oracle`` (numpy fp64) on the normalised scores, which the
test takes from the same torch call on the same device as the dispatch does, so
both see the same ties. Second oracle, on inputs without a tie between a
relevant and an irrelevant label: the torch path (``METRICS_AMD_RANKING_KERNEL
=0``).

Inputs are exact in bf16: logits ``(randint(-12, 12) + 0.5) * 0.5`` extended
with 20, 25 and 30, where the sigmoid saturates into ties, and probabilities
``k/16 + 1/32``.

Bounds over K accumulated updates: every total and the coverage measure are
integers below 2^24, exact. The LRAP and loss measures: the kernel forms every
batch sum in fp64 and rounds the state once per update, so K roundings of a
growing non-negative sum, each at most 2^-24 of the final value; the bound is
twice that, ``K * 2^-23 * max(1, expected)``.
"""
import pytest
import torch

import metrics_amd as ma
import metrics_amd.functional as F
from metrics_amd.ops import _hip
from metrics_amd.utilities.compute import normalize_logits_if_needed
from tests.unittests._ranking_oracle import MEASURES, has_mixed_tie, ranking_sums

pytestmark = pytest.mark.gpu

BF16, FP32, FP16 = torch.bfloat16, torch.float32, torch.float16
K = 3
CLASSES = {
    "coverage": ma.MultilabelCoverageError,
    "lrap": ma.MultilabelRankingAveragePrecision,
    "loss": ma.MultilabelRankingLoss,
}
FUNCTIONALS = {
    "coverage": F.multilabel_coverage_error,
    "lrap": F.multilabel_ranking_average_precision,
    "loss": F.multilabel_ranking_loss,
}
LOGIT_VALUES = torch.cat([(torch.arange(-12, 12) + 0.5) * 0.5, torch.tensor([20.0, 25.0, 30.0])])


def _layout(N, L):
    return _hip.ml_rank_layout(N, L)


def _constants():
    lay = _layout(1, 1)
    return lay[1], lay[4], lay[5], lay[6]  # rows per block (wave per row), slab entries, wave L, max L


def _shapes():
    rows, grid_max, wave_l, max_l = _constants()
    assert max_l == _hip.ML_RANK_MAX_L
    return [
        (1, 1), (1, 2), (3, 7), (5, 64), (5, 65), (4, 128), (4, 129),
        # the last L of the wave-per-row mapping, and the first of the block-per-row one
        (3, wave_l), (3, wave_l + 1),
        # the largest row the kernel stages, and the torch path above it
        (2, max_l), (2, max_l + 1),
        # one row more than a block holds, and one more
        (rows + 1, 9), (rows + 2, 9),
        # a second block of partials
        (2 * rows + 1, 12),
        # more row groups than the grid has blocks: the blocks stride
        (rows * grid_max + 5, 3),
    ]


def _id(v):
    return {BF16: "bf16", FP32: "fp32", FP16: "fp16"}.get(v, str(v))


def _target(N, L, ig, gen):
    t = torch.randint(0, 2, (N, L), generator=gen)
    if ig is not None:
        t[torch.rand(N, L, generator=gen) < 0.1] = ig
    return t


def _logits(N, L, dtype, ig, gen):
    p = LOGIT_VALUES[torch.randint(0, len(LOGIT_VALUES), (N, L), generator=gen)]
    return p.to(dtype), _target(N, L, ig, gen)


def _probs(N, L, dtype, ig, gen):
    p = torch.randint(0, 16, (N, L), generator=gen) / 16.0 + 1.0 / 32.0
    return p.to(dtype), _target(N, L, ig, gen)


def _no_mixed_ties(N, L, dtype, ig, gen):
    """Probabilities whose relevant labels take even grid steps and the others
    odd ones: ties only inside a class (ignored elements are irrelevant)."""
    t = torch.randint(0, 2, (N, L), generator=gen)
    p = (torch.randint(0, 8, (N, L), generator=gen) * 2 + (1 - t)) / 16.0 + 1.0 / 32.0
    if ig is not None:
        t[torch.rand(N, L, generator=gen) < 0.1] = ig
    return p.to(dtype), t


def _batches(N, L, dtype, ig, seed):
    gen = torch.Generator().manual_seed(seed)
    return [_logits(N, L, dtype, ig, gen), _probs(N, L, dtype, ig, gen), _logits(N, L, dtype, ig, gen)]


def _expected(batches, L, ig):
    """The oracle's (measure, total) per metric after all batches, in fp64, and
    what every batch alone gives. The scores come from the device."""
    acc = {name: [0.0, 0.0] for name in MEASURES}
    each = []
    for p, t in batches:
        s = normalize_logits_if_needed(p.cuda(), "sigmoid")
        if s.ndim > 2:
            s, t = s.movedim(1, -1).reshape(-1, L), t.movedim(1, -1).reshape(-1, L)
        sums = ranking_sums(s.double().cpu().numpy(), t.numpy(), ig)
        each.append(sums)
        for name, (m, n) in sums.items():
            acc[name][0] += m
            acc[name][1] += n
    return acc, each


def _assert_states(metrics, want, k, what=""):
    for name, m in metrics.items():
        measure, total = float(m.measure), float(m.total)
        em, et = want[name]
        assert total == et, (what, name, "total", total, et)
        bound = 0.0 if name == "coverage" else k * 2.0 ** -23 * max(1.0, em)
        print(f"{what} {name}: measure {measure!r} expected {em!r} bound {bound!r}")
        assert abs(measure - em) <= bound, (what, name, measure, em, bound)


def _torch_path_bound(N, L, k):
    """fp32 error of a measure the torch path accumulated over k updates of N
    rows: a row is a mean of at most L rounded quotients (L + 2 roundings of a
    value of at most 1), and each of the k * N additions rounds a sum of at
    most k * N."""
    return k * N * (L + 2 + k * N) * 2.0 ** -24


def _run(batches, L, ig):
    metrics = {name: cls(num_labels=L, ignore_index=ig, validate_args=False).to("cuda") for name, cls in CLASSES.items()}
    for p, t in batches:
        for m in metrics.values():
            m.update(p.cuda(), t.cuda())
    torch.cuda.synchronize()
    return metrics


N_SHAPES = 15  # the shapes depend on the library's layout, so they are built on the GPU machine


@pytest.fixture(scope="module")
def shapes():
    out = _shapes()
    assert len(out) == N_SHAPES
    return out


@pytest.mark.parametrize("ig", [None, -1], ids=_id)
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("index", range(N_SHAPES))
def test_against_the_oracle(index, dtype, ig, shapes):
    N, L = shapes[index]
    batches = _batches(N, L, dtype, ig, seed=index * 4 + (dtype == BF16) * 2 + (ig is not None))
    want, each = _expected(batches, L, ig)
    covered = _layout(N, L) is not None
    assert covered == (L <= _hip.ML_RANK_MAX_L)

    metrics = _run(batches, L, ig)
    if covered:
        _assert_states(metrics, want, K, f"({N}, {L})")
        # the same updates from reset: identical bits
        first = {name: (m.measure.clone(), m.total.clone()) for name, m in metrics.items()}
        for m in metrics.values():
            m.reset()
            for p, t in batches:
                m.update(p.cuda(), t.cuda())
        for name, m in metrics.items():
            assert torch.equal(m.measure, first[name][0]) and torch.equal(m.total, first[name][1]), name
    else:
        # above the gate the torch path runs, as before: totals and coverage
        # exact, LRAP within its fp32 sums; its loss is open on these mixed ties
        for name in ("coverage", "lrap"):
            m = metrics[name]
            assert float(m.total) == want[name][1], name
            bound = 0.0 if name == "coverage" else _torch_path_bound(N, L, K)
            assert abs(float(m.measure) - want[name][0]) <= bound, (name, float(m.measure), want[name][0])
        assert float(metrics["loss"].total) == want["loss"][1]

    # functionals, first batch, against the same oracle
    if covered:
        p, t = batches[0]
        for name, fn in FUNCTIONALS.items():
            got = float(fn(p.cuda(), t.cuda(), num_labels=L, ignore_index=ig, validate_args=False))
            m, n = each[0][name]
            # the sums are exact in fp32 after one rounding each; so is the quotient
            assert abs(got - m / n) <= 3 * 2.0 ** -24 * max(1.0, m / n), (name, got, m / n)


def test_fp16_is_normalised_in_fp16_and_widened():
    N, L, ig = 7, 33, -1
    batches = _batches(N, L, FP16, ig, seed=77)
    want, _ = _expected(batches, L, ig)
    _assert_states(_run(batches, L, ig), want, K, "fp16")


def test_more_than_two_dimensions():
    gen = torch.Generator().manual_seed(3)
    L, ig = 5, -1
    batches = []
    for _ in range(K):
        p = LOGIT_VALUES[torch.randint(0, len(LOGIT_VALUES), (2, L, 3), generator=gen)]
        t = torch.randint(0, 2, (2, L, 3), generator=gen)
        t[torch.rand(2, L, 3, generator=gen) < 0.1] = ig
        batches.append((p, t))
    want, each = _expected(batches, L, ig)
    _assert_states(_run(batches, L, ig), want, K, "(2, 5, 3)")
    p, t = batches[0]
    for name, fn in FUNCTIONALS.items():
        got = float(fn(p.cuda(), t.cuda(), num_labels=L, ignore_index=ig, validate_args=False))
        m, n = each[0][name]
        assert abs(got - m / n) <= 3 * 2.0 ** -24 * max(1.0, m / n), name


def _planted(dtype, ig):
    """Ten rows of eight labels, one edge each. -1 marks an ignored element
    (kept as 0 when the case runs without ignore_index)."""
    g = lambda *ks: [k / 16.0 + 1.0 / 32.0 for k in ks]  # noqa: E731
    rows = [
        (g(1, 5, 3, 7, 2, 9, 4, 6), [1, 1, 1, 1, 1, 1, 1, 1]),       # all relevant
        (g(1, 5, 3, 7, 2, 9, 4, 6), [0, 0, 0, 0, 0, 0, 0, 0]),       # none relevant
        (g(1, 5, 3, 7, 2, 9, 4, 6), [-1, -1, -1, -1, -1, -1, -1, -1]),  # all ignored
        (g(1, 5, 3, 7, 2, 9, 4, 6), [1, 0, -1, 0, 1, 0, 0, 1]),      # one ignored
        (g(4, 4, 4, 4, 4, 4, 4, 4), [1, 0, 0, 1, 0, 1, 0, 0]),       # all scores equal
        (g(5, 1, 5, 2, 5, 3, 4, 6), [1, 0, 1, 0, 1, 0, 0, 0]),       # ties among relevant labels only
        (g(5, 1, 1, 2, 1, 3, 3, 6), [1, 0, 0, 1, 0, 0, 0, 1]),       # ties among irrelevant labels only
        (g(5, 5, 1, 5, 2, 2, 3, 5), [0, 1, 0, 1, 1, 0, 0, 0]),       # mixed ties, irrelevant in front
        (g(5, 5, 1, 5, 2, 2, 3, 5), [1, 0, 0, 0, 0, 1, 0, 1]),       # mixed ties, relevant in front
        (g(0, 15, 0, 15, 0, 15, 0, 15), [1, 0, 0, 1, 0, 0, 1, 1]),   # the ends of the grid
    ]
    p = torch.tensor([r[0] for r in rows]).to(dtype)
    t = torch.tensor([r[1] for r in rows])
    if ig is None:
        t[t == -1] = 0
    return p, t


@pytest.mark.parametrize("ig", [None, -1], ids=_id)
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
def test_planted_rows(dtype, ig):
    p, t = _planted(dtype, ig)
    batches = [(p, t)] * K
    want, _ = _expected(batches, 8, ig)
    _assert_states(_run(batches, 8, ig), want, K, "planted")
    # every row alone, so that no row hides behind another
    for r in range(p.shape[0]):
        one = [(p[r:r + 1], t[r:r + 1])]
        want, _ = _expected(one, 8, ig)
        _assert_states(_run(one, 8, ig), want, 1, f"planted row {r}")


@pytest.mark.parametrize("ig", [None, -1], ids=_id)
def test_a_batch_without_a_valid_row(ig):
    """All-relevant and none-relevant rows only: the loss adds 1 to its total
    and nothing to the measure, decided on the device; a later batch with a
    valid row adds its N."""
    p = torch.tensor([[0.25, 0.75, 0.5], [0.5, 0.5, 0.125], [0.5, 0.25, 0.75]])
    t0 = torch.tensor([[1, 1, 1], [0, 0, 0], [1, 1, 1]])
    t1 = torch.tensor([[1, 1, 1], [0, 1, 0], [0, 0, 0]])
    batches = [(p, t0), (p, t1), (p, t0)]
    want, each = _expected(batches, 3, ig)
    assert each[0]["loss"] == (0.0, 1.0) and each[1]["loss"][1] == 3.0 and want["loss"][1] == 5.0
    _assert_states(_run(batches, 3, ig), want, K, "no valid row")
    got = F.multilabel_ranking_loss(p.cuda(), t0.cuda(), num_labels=3, ignore_index=ig, validate_args=False)
    assert float(got) == 0.0


@pytest.mark.parametrize("ig", [None, -1], ids=_id)
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("N, L", [(3, 7), (5, 65), (6, 130), (2, 1030)])
def test_kernel_and_torch_path_agree_without_mixed_ties(N, L, dtype, ig, monkeypatch):
    gen = torch.Generator().manual_seed(N * 1000 + L)
    batches = [_no_mixed_ties(N, L, dtype, ig, gen) for _ in range(K)]
    for p, t in batches:
        assert not has_mixed_tie(p.double().numpy(), t.numpy(), ig)
    kernel = _run(batches, L, ig)
    monkeypatch.setenv(_hip.RANKING_KERNEL_ENV, "0")
    torch_path = _run(batches, L, ig)
    for name in MEASURES:
        a, b = kernel[name], torch_path[name]
        assert float(a.total) == float(b.total), name
        em = float(b.measure)
        bound = 0.0 if name == "coverage" else K * 2.0 ** -23 * max(1.0, em)
        print(f"({N}, {L}) {name}: kernel {float(a.measure)!r} torch path {em!r} bound {bound!r}")
        assert abs(float(a.measure) - em) <= bound, (name, float(a.measure), em)


def test_nan_scores_do_not_fault():
    gen = torch.Generator().manual_seed(11)
    for N, L in ((4, 9), (2, 1030)):
        p, t = _probs(N, L, FP32, -1, gen)
        p.view(-1)[::5] = float("nan")
        m = _run([(p, t)], L, -1)
        assert float(m["coverage"].total) == N and float(m["lrap"].total) == N


def _make(L, ig, extra=False):
    kw = dict(num_labels=L, ignore_index=ig, validate_args=False)
    members = {name: cls(**kw) for name, cls in CLASSES.items()}
    if extra:
        members["f1"] = ma.MultilabelF1Score(average="macro", **kw)
        members["auroc"] = ma.MultilabelAUROC(thresholds=50, **kw)
    return ma.MetricCollection(members).to("cuda")


def test_no_host_sync_in_update():
    L, ig = 40, -1
    gen = torch.Generator().manual_seed(21)
    dev = [(p.cuda(), t.cuda()) for p, t in (_logits(64, L, BF16, ig, gen) for _ in range(4))]
    alone = {name: cls(num_labels=L, ignore_index=ig, validate_args=False).to("cuda") for name, cls in CLASSES.items()}
    coll = _make(L, ig)
    for p, t in dev[:2]:  # the second update builds the plan and the buffers
        coll.update(p, t)
        for m in alone.values():
            m.update(p, t)
    assert coll._fused_rank_plan is not None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, t in dev[2:]:
            coll.update(p, t)
            for m in alone.values():
                m.update(p, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert coll._fused_rank_plan.steps == 3


def test_the_torch_path_waits_for_the_device(monkeypatch):
    """The negative control of the check above: the row loop and the mask index
    of the torch path are host syncs."""
    monkeypatch.setenv(_hip.RANKING_KERNEL_ENV, "0")
    gen = torch.Generator().manual_seed(22)
    p, t = _logits(8, 6, FP32, None, gen)
    p, t = p.cuda(), t.cuda()
    for name in ("lrap", "loss"):
        m = CLASSES[name](num_labels=6, validate_args=False).to("cuda")
        m.update(p, t)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                m.update(p, t)
        finally:
            torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("ig", [None, -1], ids=_id)
def test_collection_plan_equals_the_stand_alone_metrics(ig):
    N, L, updates = 37, 130, 4
    gen = torch.Generator().manual_seed(31)
    batches = [_logits(N, L, BF16, ig, gen) for _ in range(updates)]
    coll = _make(L, ig)
    for p, t in batches:
        coll.update(p.cuda(), t.cuda())
    plan = coll._fused_rank_plan
    assert plan is not None and plan.steps == updates - 1
    alone = _run(batches, L, ig)
    for name, m in coll.items(keep_base=True, copy_state=False):
        assert torch.equal(m.measure, alone[name].measure), name
        assert torch.equal(m.total, alone[name].total), name
    res = coll.compute()
    for name in MEASURES:
        assert torch.equal(res[name], alone[name].compute()), name


def test_ranking_plan_runs_next_to_the_multilabel_step():
    N, L, ig, updates = 33, 20, -1, 3
    gen = torch.Generator().manual_seed(41)
    batches = [_logits(N, L, BF16, ig, gen) for _ in range(updates)]
    coll = _make(L, ig, extra=True)
    for p, t in batches:
        coll.update(p.cuda(), t.cuda())
    assert coll._fused_ml_plan is not None and coll._fused_ml_plan.steps == updates - 1
    assert coll._fused_rank_plan is not None and coll._fused_rank_plan.steps == updates - 1
    alone = _run(batches, L, ig)
    for name in MEASURES:
        m = coll[name]
        assert torch.equal(m.measure, alone[name].measure) and torch.equal(m.total, alone[name].total), name
        assert m._update_count == updates


def test_env_switch_builds_no_plan(monkeypatch):
    monkeypatch.setenv(_hip.RANKING_KERNEL_ENV, "0")
    assert not _hip.ranking_kernel_enabled()
    gen = torch.Generator().manual_seed(51)
    coll = _make(6, None)
    for _ in range(2):
        p, t = _no_mixed_ties(4, 6, FP32, None, gen)
        coll.update(p.cuda(), t.cuda())
    assert coll._fused_rank_plan is None


def test_a_single_ranking_member_builds_no_plan():
    coll = ma.MetricCollection({
        "lrap": ma.MultilabelRankingAveragePrecision(num_labels=6, validate_args=False),
        "f1": ma.MultilabelF1Score(num_labels=6, validate_args=False),
    }).to("cuda")
    gen = torch.Generator().manual_seed(61)
    for _ in range(2):
        p, t = _probs(4, 6, FP32, None, gen)
        coll.update(p.cuda(), t.cuda())
    assert coll._fused_rank_plan is None
