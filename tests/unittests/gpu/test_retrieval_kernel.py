"""The segmented retrieval scoring pass (csrc/retrieval_score.hip) against a plain numpy fp64 oracle.

Bounds: integer record fields and cum_rel are exact; a per-query score and the
aggregated scalar are formed in fp64 and rounded once, so they lie within one
fp32 ulp of the oracle's value rounded to fp32; the PR curve, whose divisions
and mean torch does, is held to the atol 1e-6 of the existing GPU retrieval tests.
"""
import numpy as np
import pytest
import torch

import metrics_amd as ma
from metrics_amd.ops import _hip
from metrics_amd.retrieval import metrics as rmetrics

gpu = pytest.mark.gpu
T = _hip.RETRIEVAL_BLOCK_MIN
INT_FIELDS = ("count", "npos", "nneg", "hits_k", "neg_hits_k", "first_pos", "hits_r", "u")
MODULES = {
    "map": ma.RetrievalMAP, "mrr": ma.RetrievalMRR, "precision": ma.RetrievalPrecision,
    "recall": ma.RetrievalRecall, "hit_rate": ma.RetrievalHitRate, "fall_out": ma.RetrievalFallOut,
    "ndcg": ma.RetrievalNormalizedDCG, "r_precision": ma.RetrievalRPrecision, "auroc": ma.RetrievalAUROC,
}


def oracle(idx, preds, target, top_k=None, max_k=None):
    """Per query, in (index asc, score desc) stable order: the record fields, the scores, cum_rel."""
    order = np.lexsort((-preds.astype(np.float64), idx))
    idx, s_all, t_all = idx[order], preds[order].astype(np.float64), target[order].astype(np.float64)
    bounds = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1], True])
    rec = {f: [] for f in INT_FIELDS + ("tsum", "ap", "dcg", "idcg")}
    sc = {m: [] for m in MODULES}
    cum_rel = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        s, t = s_all[a:b], t_all[a:b]
        n = b - a
        k = n if top_k is None else min(top_k, n)
        pos, neg = t > 0, t == 0
        npos, nneg = int(pos.sum()), int(neg.sum())
        hits, nh = int(pos[:k].sum()), int(neg[:k].sum())
        first = int(np.argmax(pos)) if npos else -1
        ranks = np.arange(1, n + 1, dtype=np.float64)
        cum = np.cumsum(pos)
        ap = float((cum[:k] / ranks[:k])[pos[:k]].sum())
        disc = np.log2(ranks[:k] + 1.0)
        dcg, idcg = float((t[:k] / disc).sum()), float((np.sort(t)[::-1][:k] / disc).sum())
        sp, sn = s[:k][pos[:k]], s[:k][neg[:k]]
        u = int(2 * (sp[:, None] > sn[None, :]).sum() + (sp[:, None] == sn[None, :]).sum())
        auroc = 0.0
        if hits and nh:  # trapezoid over the distinct scores
            last = np.r_[s[1:k] != s[:k - 1], True]
            tpr = np.r_[0.0, np.cumsum(pos[:k])[last] / hits]
            fpr = np.r_[0.0, np.cumsum(neg[:k])[last] / nh]
            auroc = float(((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2).sum())
        hits_r = int(pos[:npos].sum())
        for f, v in zip(rec, (n, npos, nneg, hits, nh, first, hits_r, u, float(t.sum()), ap, dcg, idcg)):
            rec[f].append(v)
        sc["map"].append(ap / hits if hits else 0.0)
        sc["mrr"].append(1.0 / (first + 1) if 0 <= first < k else 0.0)
        sc["precision"].append(hits / (n if top_k is None else top_k))
        sc["recall"].append(hits / max(npos, 1))
        sc["hit_rate"].append(float(hits > 0))
        sc["fall_out"].append(nh / max(nneg, 1))
        sc["ndcg"].append(dcg / idcg if idcg > 0 else 0.0)
        sc["r_precision"].append(hits_r / max(npos, 1))
        sc["auroc"].append(auroc)
        if max_k:
            cum_rel.append(np.r_[cum, np.full(max(max_k - n, 0), cum[-1])][:max_k])
    rec = {f: np.array(v) for f, v in rec.items()}
    return rec, {m: np.array(v) for m, v in sc.items()}, np.array(cum_rel)


def make(lengths, seed, ties=False, graded=False, planted=()):
    """Shuffled (indexes, preds, target) with queries of the given lengths under gapped index
    values, then the planted (preds, target) queries; `ties` draws the scores from 4 values."""
    rng = np.random.default_rng(seed)
    nq = len(lengths) + len(planted)
    ids = np.sort(np.r_[[0, 5, 1000, 2**31 - 1], 1000 + np.cumsum(rng.integers(1, 10**6, nq))][:nq])
    idx, preds, target = [], [], []
    for q, n in enumerate(lengths):
        idx.append(np.full(n, ids[q]))
        preds.append(rng.integers(0, 4, n) / 4.0 if ties else rng.permutation(n) / n + rng.integers(0, 3))
        hi = 4 if graded else 2
        target.append(rng.integers(0, hi, n) * (rng.random() > 0.15))  # some all-zero queries
    for q, (p, t) in enumerate(planted, len(lengths)):
        idx.append(np.full(len(p), ids[q]))
        preds.append(np.asarray(p, dtype=np.float64))
        target.append(np.asarray(t))
    idx, preds, target = np.concatenate(idx), np.concatenate(preds).astype(np.float32), np.concatenate(target)
    perm = rng.permutation(len(idx))
    return idx[perm].astype(np.int64), preds[perm], target[perm].astype(np.int64)


def _w_set(w, reps):
    return [1, w - 1, w, w + 1] * reps


PLANTED = [
    (np.linspace(1, 0, 70), np.ones(70)),                       # all positive
    (np.linspace(1, 0, 70), np.zeros(70)),                      # all negative
    ([0.3], [1]),                                               # a single element
    (np.linspace(1, 0, 130), np.r_[np.zeros(129), 1]),          # first positive at the last rank
    (np.r_[np.linspace(2, 1, 60), np.full(10, 0.5), np.linspace(0.4, 0, 20)], np.arange(90) % 2),  # tie over a chunk edge
    (np.r_[0.9, np.full(5, 0.5), 0.1], [0, 1, 0, 1, 1, 0, 1]),  # tie over the k_eff = 3 cut
    (np.full(100, 0.25), np.arange(100) % 3 == 0),              # every score equal
]
ZEROS = ([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], [1, 0, 0, 1, 0, 1])  # +0.0 and -0.0 tie: AUROC only (order-free)
DATASETS = {
    "w8_wraps": lambda: make(_w_set(8, 300), 1),
    "w16": lambda: make(_w_set(16, 6), 2, ties=True),
    "w32": lambda: make(_w_set(32, 4), 3),
    "w64": lambda: make(_w_set(64, 3) + [63, 64, 65, 129], 4, planted=PLANTED),
    "block": lambda: make([T - 1, T, T + 1, 3 * T + 77, 1, 65], 5, ties=True),
    "mixed_w8": lambda: make([2] * 700 + [129, T + 1], 6),
    "one_query": lambda: make([65], 7),
    "graded": lambda: make(_w_set(16, 4) + [129, T + 1], 8, graded=True),
}
_CACHE = {}


def data(name):
    if name not in _CACHE:
        _CACHE[name] = DATASETS[name]()
    return _CACHE[name]


def dev(arrs, float_target=False):
    i, p, t = (torch.from_numpy(a).cuda() for a in arrs)
    return i, p, t.float() if float_target else t


def assert_ulp(got, ref, what):
    ref32 = np.asarray(ref, dtype=np.float64).astype(np.float32)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref32.astype(np.float64))
    bad = err > np.spacing(np.abs(ref32)).astype(np.float64)
    print(what, "max err", err.max(initial=0.0))
    assert not bad.any(), (what, np.flatnonzero(bad)[:5], err.max())


def test_oracle_matches_cpu_modules():
    """The oracle against the CPU modular metrics: few ties for the order-dependent measures, heavy for AUROC."""
    for name, cls in MODULES.items():
        arrs = make([1, 7, 8, 9, 40, 70], 11, ties=name == "auroc", graded=name == "ndcg")
        for top_k in (None, 3):
            kw = {} if name == "r_precision" else {"top_k": top_k}
            m = cls(aggregation=lambda v, dim=None: v, empty_target_action="pos" if name == "fall_out" else "neg", **kw)
            i, p, t = (torch.from_numpy(a) for a in arrs)
            m.update(p, t, indexes=i)
            _, sc, _ = oracle(*arrs, top_k=None if name == "r_precision" else top_k)
            ref = sc[name].copy()
            empty = oracle(*arrs)[0]["nneg" if name == "fall_out" else "tsum"] == 0
            ref[empty] = 1.0 if name == "fall_out" else 0.0
            np.testing.assert_allclose(m.compute().numpy(), ref, atol=1e-6, err_msg=f"{name} top_k={top_k}")


@gpu
@pytest.mark.parametrize("top_k", [None, 1, 3, 5000])
@pytest.mark.parametrize("name", list(DATASETS))
def test_records_and_scores(name, top_k):
    arrs = data(name)
    rec, sc, _ = oracle(*arrs, top_k=top_k)
    G = len(rec["count"])
    for metric in MODULES:
        if (metric == "ndcg") != (name == "graded"):
            continue  # graded targets are NDCG's alone
        res = _hip.retrieval_scores(*dev(arrs, float_target=metric == "ndcg" and top_k == 3), metric, top_k=top_k,
                                    action="error", aggregation=None)
        assert int(res.header[0]) == G
        got = {f: v.cpu().numpy() for f, v in _hip.retrieval_records(res, G).items()}
        wanted = {"map": ("ap",), "ndcg": ("dcg", "idcg"), "auroc": ("u",), "r_precision": ("hits_r",)}.get(metric, ())
        for f in INT_FIELDS:
            if f in ("u", "hits_r") and f not in wanted:
                continue
            np.testing.assert_array_equal(got[f], rec[f], err_msg=f"{metric} {f}")
        # an fp64 sum of n terms in another order than numpy's: n rounding errors of 2^-52 at the most
        rtol = (rec["count"].max() + 8) * np.finfo(np.float64).eps
        for f in ("tsum",) + tuple(w for w in wanted if w not in INT_FIELDS):
            np.testing.assert_allclose(got[f], rec[f], rtol=rtol, atol=0, err_msg=f"{metric} {f}")
        assert_ulp(res.scores[:G].cpu().numpy(), sc[metric], f"{name} {metric} top_k={top_k}")


@gpu
def test_signed_zero_scores_tie():
    arrs = make([9], 12, planted=[ZEROS])
    rec, sc, _ = oracle(*arrs)
    res = _hip.retrieval_scores(*dev(arrs), "auroc", action="error", aggregation=None)
    assert _hip.retrieval_records(res, 2)["u"].tolist() == rec["u"].tolist()
    assert_ulp(res.scores[:2].cpu().numpy(), sc["auroc"], "signed zeros")


@gpu
@pytest.mark.parametrize("max_k", [1, 7, 5000])
@pytest.mark.parametrize("name", ["w8_wraps", "w64", "block"])
def test_cum_rel(name, max_k):
    arrs = data(name)
    rec, _, cum = oracle(*arrs, max_k=max_k)
    G = len(cum)
    args = dev(arrs)
    res = _hip.retrieval_scores(*args, "curve", aggregation=None, phases=1)
    assert res.header[:3].tolist() == [G, rec["count"].max(), rec["count"].min()]
    out = torch.full((G, max_k), -1, dtype=torch.int32, device="cuda")
    res = _hip.retrieval_scores(*args, "curve", aggregation=None, phases=2, max_k=max_k, cum_rel=out)
    np.testing.assert_array_equal(out.cpu().numpy(), cum)
    np.testing.assert_array_equal(res.scores[:G].cpu().numpy(), rec["npos"])


@gpu
@pytest.mark.parametrize("adaptive_k", [False, True])
@pytest.mark.parametrize("max_k", [None, 1, 7, 5000])
@pytest.mark.parametrize("action", ["neg", "pos", "skip"])
def test_pr_curve_matches_cpu_module(action, max_k, adaptive_k):
    arrs = make(_w_set(16, 3) + [129, 7], 13)
    outcome = []
    for device in ("cpu", "cuda"):
        kw = dict(max_k=max_k, adaptive_k=adaptive_k, empty_target_action=action)
        for m in (ma.RetrievalPrecisionRecallCurve(**kw), ma.RetrievalRecallAtFixedPrecision(min_precision=0.4, **kw)):
            i, p, t = (torch.from_numpy(a).to(device) for a in arrs)
            m.update(p, t, indexes=i)
            try:
                outcome.append([x.cpu() for x in m.compute()])
            except RuntimeError as err:  # the functional's adaptive_k curves of unequal length do not stack
                outcome.append(type(err))
    for ref, got in zip(outcome[:2], outcome[2:]):
        if isinstance(ref, type):
            assert got is ref
            continue
        for r, g in zip(ref, got):
            torch.testing.assert_close(g.float(), r.float(), atol=1e-6, rtol=0)


@gpu
@pytest.mark.parametrize("aggregation", ["mean", "median", "min", "max", "callable"])
@pytest.mark.parametrize("action", ["neg", "pos", "skip"])
@pytest.mark.parametrize("metric", ["map", "fall_out"])
def test_actions_and_aggregations(metric, action, aggregation):
    arrs = data("w64")
    rec, sc, _ = oracle(*arrs, top_k=3)
    empty = rec["nneg" if metric == "fall_out" else "tsum"] == 0
    assert empty.any() and not empty.all()
    ref = sc[metric].copy()
    ref[empty] = 1.0 if action == "pos" else 0.0
    ref = ref[~empty] if action == "skip" else ref
    fn = {"mean": np.mean, "min": np.min, "max": np.max,
          "median": lambda v: np.sort(v.astype(np.float32))[(len(v) - 1) // 2], "callable": np.max}[aggregation]
    agg = (lambda v, dim=None: v.max()) if aggregation == "callable" else aggregation
    m = MODULES[metric](top_k=3, empty_target_action=action, aggregation=agg).cuda()
    i, p, t = dev(arrs)
    m.update(p, t, indexes=i)
    assert_ulp(m.compute().cpu().numpy(), fn(ref), f"{metric} {action} {aggregation}")


@gpu
def test_every_query_empty_and_error():
    arrs = make([5, 9], 14)
    i, p, t = dev(arrs)
    m = ma.RetrievalMAP(empty_target_action="skip").cuda()
    m.update(p, torch.zeros_like(t), indexes=i)
    assert float(m.compute()) == 0.0
    m = ma.RetrievalMAP(empty_target_action="error").cuda()
    m.update(p, torch.zeros_like(t), indexes=i)
    with pytest.raises(ValueError, match="no positive target"):
        m.compute()


@gpu
def test_two_calls_are_bit_identical():
    args = dev(data("block"))
    runs = []
    for _ in range(2):
        res = _hip.retrieval_scores(*args, "auroc", top_k=None, aggregation="mean")
        G = int(res.header[0])
        raw = res.scratch[res.records_offset:res.records_offset + 72 * G]
        runs.append((res.value.clone(), res.scores[:G].clone(), raw.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    args = dev(data("graded"), float_target=True)
    vals = [_hip.retrieval_scores(*args, "ndcg", top_k=3, aggregation="mean").value.clone() for _ in range(2)]
    assert torch.equal(vals[0].view(torch.int32), vals[1].view(torch.int32))


@gpu
@pytest.mark.parametrize("kernel", ["1", "0"])
def test_dispatch(monkeypatch, kernel):
    """Kernel on: neither the per-query `_metric` nor the functional curve runs. Switched off: they do."""
    def boom(*a, **k):
        raise AssertionError("per-query path")

    monkeypatch.setenv(_hip.RETRIEVAL_KERNEL_ENV, kernel)
    monkeypatch.setattr(ma.RetrievalAUROC, "_metric", boom)
    monkeypatch.setattr(rmetrics, "retrieval_precision_recall_curve", boom)
    i, p, t = dev(make([5, 9, 70], 15, ties=True))
    t[:3] = 1  # some query has a positive
    for m in (ma.RetrievalAUROC().cuda(), ma.RetrievalPrecisionRecallCurve(max_k=4).cuda()):
        m.update(p, t, indexes=i)
        if kernel == "1":
            m.compute()
        else:
            with pytest.raises(AssertionError, match="per-query path"):
                m.compute()
