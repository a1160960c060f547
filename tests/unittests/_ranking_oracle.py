"""numpy fp64 oracle of the multilabel ranking measures (coverage error, label
ranking average precision, ranking loss), written from the per-row formulas of
``csrc/ml_rank.hip`` and independent of both the kernel and the torch path.

It works on the NORMALISED scores (what ``normalize_logits_if_needed`` returned
for the batch) and applies ``ignore_index`` itself: an ignored element is not
relevant and takes the score -inf. Per row, R = relevant labels, n = |R|:

* coverage: L if the row holds an ignored element (the quirk of the torch path,
  docs/PARITY.md), else ``#{k : s_k >= min_R s}`` if n > 0, else 0;
* LRAP: ``(1/n) sum_{j in R} #{k in R : s_k >= s_j} / #{k : s_k >= s_j}`` if
  0 < n < L, else 1;
* loss: rows with 0 < n < L are valid, ``inv_j = #{k : s_k < s_j} +
  #{k < j : s_k == s_j}`` (the position under a stable ascending sort), value
  ``(sum_{j in R} (L - inv_j) - n(n+1)/2) / (n (L - n))``; a batch without a
  valid row adds 1 to ``total`` and nothing to the measure.

NaN scores are outside the oracle. Two forms of the per-label counts: ``direct``
spells the set sizes out with an (N, L, L) compare, ``sorted`` gets them from
one stable sort per row and serves the large shapes; ``test_ranking_oracle``
holds the two against each other.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

MEASURES = ("coverage", "lrap", "loss")


def _prepare(scores, target, ignore_index: Optional[int]):
    s = np.array(scores, dtype=np.float64)
    t = np.asarray(target)
    assert s.ndim == 2 and s.shape == t.shape
    ign = (t == ignore_index) if ignore_index is not None else np.zeros(t.shape, dtype=bool)
    s[ign] = -np.inf
    rel = (t == 1) & ~ign
    return s, rel, ign


def _counts_direct(s: np.ndarray, rel: np.ndarray):
    """(ge_all, ge_rel, inv), each (N, L), by the set definitions."""
    L = s.shape[1]
    ge = s[:, None, :] >= s[:, :, None]  # [i, j, k] = s_k >= s_j
    ge_all = ge.sum(axis=2)
    ge_rel = (ge & rel[:, None, :]).sum(axis=2)
    lt = (s[:, None, :] < s[:, :, None]).sum(axis=2)
    before = np.arange(L)[None, None, :] < np.arange(L)[None, :, None]  # k < j
    eqb = ((s[:, None, :] == s[:, :, None]) & before).sum(axis=2)
    return ge_all, ge_rel, lt + eqb


def _counts_sorted(s: np.ndarray, rel: np.ndarray):
    """The same three counts from one stable ascending sort per row."""
    N, L = s.shape
    order = np.argsort(s, axis=1, kind="stable")
    inv = np.empty_like(order)
    np.put_along_axis(inv, order, np.broadcast_to(np.arange(L), (N, L)), axis=1)
    ss = np.take_along_axis(s, order, axis=1)
    # first sorted position of every tie run = number of strictly smaller scores
    new_run = np.ones((N, L), dtype=bool)
    new_run[:, 1:] = ss[:, 1:] != ss[:, :-1]
    run_start = np.maximum.accumulate(np.where(new_run, np.arange(L)[None, :], 0), axis=1)
    rel_sorted = np.take_along_axis(rel, order, axis=1).astype(np.int64)
    rel_before = np.cumsum(rel_sorted, axis=1) - rel_sorted  # relevant at smaller sorted positions
    start_of = np.take_along_axis(run_start, inv, axis=1)  # per label: start of its run
    lt_all = start_of
    lt_rel = np.take_along_axis(rel_before, start_of, axis=1)
    n = rel.sum(axis=1, keepdims=True)
    return L - lt_all, n - lt_rel, inv


def ranking_rows(scores, target, ignore_index: Optional[int] = None, form: str = "auto") -> Dict[str, np.ndarray]:
    """Per-row values: ``coverage``, ``lrap``, ``loss`` (0 where the row is not
    valid) and ``valid``, each (N,) fp64 / bool."""
    s, rel, ign = _prepare(scores, target, ignore_index)
    N, L = s.shape
    if form == "auto":
        form = "direct" if N * L * L <= 1 << 22 else "sorted"
    ge_all, ge_rel, inv = (_counts_direct if form == "direct" else _counts_sorted)(s, rel)
    n = rel.sum(axis=1)

    rel_min = np.where(rel, s, np.inf).min(axis=1)
    covered = (s >= rel_min[:, None]).sum(axis=1)
    coverage = np.where(ign.any(axis=1), L, np.where(n > 0, covered, 0)).astype(np.float64)

    valid = (n > 0) & (n < L)
    safe_n = np.maximum(n, 1).astype(np.float64)
    ratio = np.where(rel, ge_rel / np.maximum(ge_all, 1), 0.0)
    lrap = np.where(valid, ratio.sum(axis=1) / safe_n, 1.0)

    ranks = np.where(rel, L - inv, 0).sum(axis=1).astype(np.float64)
    denom = np.where(valid, safe_n * (L - n), 1.0)
    loss = np.where(valid, (ranks - 0.5 * n * (n + 1)) / denom, 0.0)
    return {"coverage": coverage, "lrap": lrap, "loss": loss, "valid": valid}


def ranking_sums(scores, target, ignore_index: Optional[int] = None, form: str = "auto") -> Dict[str, Tuple[float, float]]:
    """What one batch adds to ``(measure, total)`` of each of the three metrics."""
    rows = ranking_rows(scores, target, ignore_index, form)
    N = float(len(rows["valid"]))
    out = {
        "coverage": (float(rows["coverage"].sum()), N),
        "lrap": (float(rows["lrap"].sum()), N),
    }
    out["loss"] = (float(rows["loss"].sum()), N) if rows["valid"].any() else (0.0, 1.0)
    return out


def has_mixed_tie(scores, target, ignore_index: Optional[int] = None) -> bool:
    """True if some row holds a relevant and an irrelevant label with the same
    score: there the unstable argsort of the torch path leaves the ranking loss
    open (docs/PARITY.md) and only the stable rule above is defined."""
    s, rel, _ = _prepare(scores, target, ignore_index)
    for row, r in zip(s, rel):
        if np.intersect1d(row[r], row[~r]).size:
            return True
    return False
