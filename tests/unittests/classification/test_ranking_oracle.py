"""The numpy oracle of the ranking measures (``_ranking_oracle``) against the
project's CPU functionals, and its two counting forms against each other.

The CPU functionals are the torch path of ``functional/classification/
ranking.py``. The ranking loss there sorts with an unstable ``argsort``, so the
comparison stays on inputs without a tie between a relevant and an irrelevant
label (``_no_mixed_ties``); everything else may tie freely.

Bound. Coverage and every total are integers below 2^24: exact. An LRAP row is
the fp32 mean of n <= L rounded quotients, each at most 1: at most L + 2
roundings of 2^-24; a loss row is one rounded quotient of exact integers. The
batch sum adds N such rows (each add rounds a sum of at most N by 2^-24 of it)
and the final division by N brings that back to N * 2^-24 in the mean, plus one
rounding: (N + L + 3) * 2^-24 in all, taken as (N + L + 2) * 2^-23 relative to
max(1, expected).
"""
import numpy as np
import pytest
import torch

import metrics_amd.functional as F
from metrics_amd.utilities.compute import normalize_logits_if_needed
from tests.unittests._ranking_oracle import has_mixed_tie, ranking_rows, ranking_sums

BF16, FP32 = torch.bfloat16, torch.float32


def _no_mixed_ties(N, L, dtype, logits, ig, gen):
    """Scores exact in bf16 whose relevant labels take even grid steps and the
    others odd ones: ties only inside a class."""
    t = torch.randint(0, 2, (N, L), generator=gen)
    k = torch.randint(0, 8, (N, L), generator=gen) * 2 + (1 - t)
    if logits:
        p = ((k - 8) + 0.5) * 0.5  # |x| <= 3.75: distinct after the sigmoid in bf16 too
    else:
        p = k / 16.0 + 1.0 / 32.0
    if ig is not None:
        t[torch.rand(N, L, generator=gen) < 0.15] = ig
    # planted rows: all relevant, none relevant
    if N >= 3:
        t[1] = 1
        t[2] = 0
    return p.to(dtype), t


CASES = [(N, L, dtype, logits, ig)
         for N, L in ((1, 1), (1, 2), (4, 5), (9, 16), (6, 40))
         for dtype in (FP32, BF16) for logits in (False, True) for ig in (None, -1)]


@pytest.mark.parametrize("N, L, dtype, logits, ig", CASES)
def test_oracle_equals_the_cpu_functionals(N, L, dtype, logits, ig):
    gen = torch.Generator().manual_seed(N * 131 + L * 7 + int(logits))
    p, t = _no_mixed_ties(N, L, dtype, logits, ig, gen)
    scores = normalize_logits_if_needed(p, "sigmoid").double().numpy()
    assert not has_mixed_tie(scores, t.numpy(), ig)
    want = ranking_sums(scores, t.numpy(), ig)
    kw = dict(num_labels=L, ignore_index=ig, validate_args=False)  # validation rejects L = 1
    got = {
        "coverage": F.multilabel_coverage_error(p, t, **kw),
        "lrap": F.multilabel_ranking_average_precision(p, t, **kw),
        "loss": F.multilabel_ranking_loss(p, t, **kw),
    }
    for name, v in got.items():
        measure, total = want[name]
        expect = measure / total
        # coverage: exact integers, one rounding of their fp32 quotient
        bound = 2.0 ** -24 * expect if name == "coverage" else (N + L + 2) * 2.0 ** -23 * max(1.0, expect)
        assert abs(float(v) - expect) <= bound, (name, float(v), expect)


def test_no_valid_row_adds_one_to_the_total():
    p = torch.tensor([[0.25, 0.75, 0.5], [0.5, 0.5, 0.125]])
    t = torch.tensor([[1, 1, 1], [0, 0, 0]])
    want = ranking_sums(p.numpy(), t.numpy())
    assert want["loss"] == (0.0, 1.0) and want["lrap"] == (2.0, 2.0) and want["coverage"] == (3.0, 2.0)
    assert float(F.multilabel_ranking_loss(p, t, num_labels=3)) == 0.0
    assert float(F.multilabel_ranking_average_precision(p, t, num_labels=3)) == 1.0
    assert float(F.multilabel_coverage_error(p, t, num_labels=3)) == 1.5


def test_a_row_with_an_ignored_element_covers_every_label():
    p = torch.tensor([[0.75, 0.25, 0.5, 0.125]])
    t = torch.tensor([[1, 0, -1, 0]])
    rows = ranking_rows(p.numpy(), t.numpy(), -1)
    assert rows["coverage"].tolist() == [4.0]
    assert float(F.multilabel_coverage_error(p, t, num_labels=4, ignore_index=-1)) == 4.0
    # without the ignored element the top relevant label covers itself alone
    assert ranking_rows(p.numpy(), torch.tensor([[1, 0, 0, 0]]).numpy(), -1)["coverage"].tolist() == [1.0]


def test_the_stable_rule_on_a_mixed_tie():
    """Relevant label 2 ties with labels 0 and 3: under the stable ascending
    sort it sits behind label 0 and in front of label 3."""
    s = np.array([[0.5, 0.25, 0.5, 0.5]])
    t = np.array([[0, 0, 1, 0]])
    assert has_mixed_tie(s, t)
    rows = ranking_rows(s, t)
    # inv_2 = #{s_k < 0.5} + #{k < 2 : s_k == 0.5} = 1 + 1; (4 - 2 - 1) / (1 * 3)
    assert rows["loss"].tolist() == [1.0 / 3.0]
    # LRAP counts ties as "at least as high": 1 relevant of 3 labels
    assert rows["lrap"].tolist() == [1.0 / 3.0]
    assert rows["coverage"].tolist() == [3.0]


@pytest.mark.parametrize("ig", [None, -1])
def test_the_two_counting_forms_agree(ig):
    gen = torch.Generator().manual_seed(5)
    for N, L in ((1, 1), (3, 2), (7, 9), (5, 33)):
        s = (torch.randint(0, 6, (N, L), generator=gen) / 8.0).numpy()  # heavy ties of every kind
        t = torch.randint(0, 2, (N, L), generator=gen)
        if ig is not None:
            t[torch.rand(N, L, generator=gen) < 0.2] = ig
        a = ranking_rows(s, t.numpy(), ig, form="direct")
        b = ranking_rows(s, t.numpy(), ig, form="sorted")
        for name in a:
            assert np.array_equal(a[name], b[name]), (name, N, L)
