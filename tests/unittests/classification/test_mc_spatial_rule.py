"""``_mc_spatial_rule`` (the rule the fused spatial step is tested against on
the GPU) held against the CPU metrics on NaN-free inputs."""
import pytest
import torch

import metrics_amd as ma
from tests.unittests._mc_spatial_rule import mc_spatial_argmax, mc_spatial_rule, mc_spatial_rule_sum

INF, NAN = float("inf"), float("nan")


def _batch(shape, C, ig, gen, out_of_range=False):
    N, spatial = shape[0], shape[1:]
    p = (torch.randint(-12, 12, (N, C, *spatial), generator=gen) + 0.5) * 0.5
    t = torch.randint(0, C, (N, *spatial), generator=gen)
    if ig is not None:
        t[torch.rand(t.shape, generator=gen) < 0.1] = ig
    if out_of_range:
        t.view(-1)[1] = C + 3
    return p, t


@pytest.mark.parametrize("ig", [None, -1, 255])
@pytest.mark.parametrize("shape,C", [((3, 7), 2), ((2, 5, 6), 19), ((2, 2, 3, 4), 5), ((1, 1), 3)])
def test_rule_equals_the_cpu_metrics(shape, C, ig):
    gen = torch.Generator().manual_seed(sum(shape) + C)
    batches = [_batch(shape, C, ig, gen) for _ in range(3)]
    tp, fp, tn, fn, confmat, correct, total = mc_spatial_rule_sum(batches, C, ig)
    kw = dict(num_classes=C, ignore_index=ig, validate_args=False)
    stat = ma.MulticlassStatScores(average=None, **kw)
    cm = ma.MulticlassConfusionMatrix(**kw)
    em = ma.MulticlassExactMatch(**kw)
    for p, t in batches:
        stat.update(p, t)
        cm.update(p, t)
        em.update(p, t)
    for name, want in (("tp", tp), ("fp", fp), ("tn", tn), ("fn", fn)):
        assert torch.equal(getattr(stat, name), want), name
    assert torch.equal(cm.confmat, confmat)
    assert torch.equal(em.correct.reshape(1), correct) and torch.equal(em.total.reshape(1), total)


def test_out_of_range_target_is_a_mismatch_and_is_not_counted():
    gen = torch.Generator().manual_seed(5)
    p, t = _batch((3, 4, 4), 4, -1, gen, out_of_range=True)
    tp, fp, tn, fn, confmat, correct, total = mc_spatial_rule(p, t, 4, -1)
    em = ma.MulticlassExactMatch(num_classes=4, ignore_index=-1, validate_args=False)
    em.update(p, t)
    assert torch.equal(em.correct.reshape(1), correct) and int(total) == 3
    counted = ((t != -1) & (t >= 0) & (t < 4)).sum()
    assert int(confmat.sum()) == int(counted) == int((tp + fn).sum())
    # the sample holding it cannot be correct
    q = torch.zeros(1, 4, 2)
    q[0, 2] = 1.0
    assert int(mc_spatial_rule(q, torch.tensor([[2, 9]]), 4, None)[5]) == 0
    assert int(mc_spatial_rule(q, torch.tensor([[2, 9]]), 4, 9)[5]) == 1


def test_argmax_rule_on_planted_columns():
    cols = [
        ([1.0, NAN, 3.0, 2.0], 2),    # NaN is skipped
        ([NAN, NAN, NAN, NAN], 0),    # all NaN
        ([NAN, -INF, -INF, NAN], 0),  # nothing exceeds -inf
        ([0.0, -0.0, -1.0, -0.0], 0),  # +0.0 and -0.0 tie, lowest index
        ([-0.0, 0.0, -1.0, 0.0], 0),
        ([2.0, INF, INF, 1.0], 1),
        ([-INF, -5.0, NAN, -5.0], 1),
    ]
    x = torch.tensor([c for c, _ in cols]).T.reshape(1, 4, len(cols))
    assert mc_spatial_argmax(x).tolist() == [[w for _, w in cols]]
    assert mc_spatial_argmax(x.bfloat16()).tolist() == [[w for _, w in cols]]


def test_all_ignored_sample_is_correct_and_empty_batch():
    p = torch.zeros(2, 3, 4)
    t = torch.full((2, 4), -1)
    t[1, 0] = 1
    out = mc_spatial_rule(p, t, 3, -1)
    assert int(out[5]) == 1 and int(out[6]) == 2 and int(out[4].sum()) == 1
    out = mc_spatial_rule(torch.zeros(0, 3, 4), torch.zeros(0, 4, dtype=torch.long), 3, -1)
    assert int(out[5]) == 0 and int(out[6]) == 0 and int(out[4].sum()) == 0
