#!/usr/bin/env python3
"""compute() time of the retrieval metrics, segmented HIP pass against the path before it.

One update, then compute() only. Per shape (N elements, Q queries of random
membership) and metric (MAP, NDCG top_k=10, AUROC, PR curve max_k=10) two
windows alternate in one process (kernel, off, kernel, off, ...), ``--repeats``
of each, every window closed by one synchronize: the kernel's is ``--steps``
computes long, the one with ``METRICS_AMD_RETRIEVAL_KERNEL=0`` ``--steps-off``
(default 1: the per-query loops take seconds to minutes; ``--max-loop-queries``
skips the switched-off side of a loop metric above that many queries and says
so). The JSON line carries the median window of each side with min and max.

``floor_ms`` is what the bytes the pass must move take at ``--copy-tbs`` TB/s:
per element 8 B index + 4 B score + 8 B target read, 12 B key and fp32 target
written, 8 radix passes over the 8-bit digits of the 64-bit key each reading and
writing those 12 B, 8 B key + 4 B target read by the scoring kernel (for NDCG
one more key-only sort and 8 B read), and 72 B record + 5 B score and flag per
query. The target rides the sort as its value, so there is no gather through a
permutation; had there been one, each 4 B target would cost a 32 B sector. That
the radix sort moves exactly 8 passes is an assumption, not a measurement.

    python tools/bench_retrieval.py [--steps 20] [--steps-off 1] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import metrics_amd as ma  # noqa: E402
from metrics_amd.ops import _hip  # noqa: E402

SHAPES = [(1_000_000, 100_000), (1_000_000, 1_000), (10_000_000, 1_000_000), (1_000_000, 1)]
METRICS = {
    "map": lambda: ma.RetrievalMAP(),
    "ndcg@10": lambda: ma.RetrievalNormalizedDCG(top_k=10),
    "auroc": lambda: ma.RetrievalAUROC(),
    "pr_curve@10": lambda: ma.RetrievalPrecisionRecallCurve(max_k=10),
}
LOOP_METRICS = ("auroc", "pr_curve@10")  # a Python loop over the queries when switched off
ENV = _hip.RETRIEVAL_KERNEL_ENV


def floor_bytes(n: int, q: int, name: str) -> int:
    sorts = 2 if name.startswith("ndcg") else 1
    per_element = 20 + 12 + 8 * 2 * 12 + 12
    if sorts == 2:
        per_element += 8 + 8 * 2 * 8 + 8
    return n * per_element + q * 77


def _window(metric, steps: int, env: str) -> float:
    os.environ[ENV] = env  # read at every compute
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        metric._computed = None  # compute() again, not the cached value
        out = metric.compute()
    torch.cuda.synchronize()
    del out
    return 1000.0 * (time.perf_counter() - t0) / steps


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--steps-off", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-loop-queries", type=int, default=100_000)
    ap.add_argument("--copy-tbs", type=float, default=6.29, help="what a copy kernel reaches on the chip, TB/s")
    ap.add_argument("--shapes", default="", help="N:Q,N:Q,... instead of the default shapes")
    ap.add_argument("--metrics", default="", help="comma-separated subset of " + ",".join(METRICS))
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_retrieval.py needs a GPU"
    device = torch.device("cuda", 0)
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")] if args.shapes else SHAPES
    names = args.metrics.split(",") if args.metrics else list(METRICS)
    for n, q in shapes:
        torch.manual_seed(1234)
        indexes = torch.randint(0, q, (n,), device=device)
        preds = torch.rand(n, device=device)
        target = (torch.rand(n, device=device) < 0.2).long()
        for name in names:
            metric = METRICS[name]().to(device)
            metric.update(preds, target, indexes=indexes)
            skip_off = name in LOOP_METRICS and q > args.max_loop_queries
            ms_on, ms_off = [], []
            _window(metric, 2, "1")  # warm-up: scratch allocation, kernel load
            if not skip_off:
                _window(metric, 1, "0")
            for _ in range(args.repeats):
                ms_on.append(_window(metric, args.steps, "1"))
                if not skip_off:
                    ms_off.append(_window(metric, args.steps_off, "0"))
            os.environ[ENV] = "1"
            s_on = _summary(ms_on)
            s_off = _summary(ms_off) if ms_off else None
            print(json.dumps({
                "shape": [n, q], "metric": name,
                "kernel_ms": s_on, "off_ms": s_off,
                "off_skipped": "per-query loop above --max-loop-queries" if skip_off else None,
                "ratio": s_off["median"] / s_on["median"] if s_off else None,
                "steps": args.steps, "steps_off": args.steps_off, "repeats": args.repeats,
                "floor_ms": floor_bytes(n, q, name) / (args.copy_tbs * 1e9),
                "megabytes": floor_bytes(n, q, name) / 1e6,
            }), flush=True)


if __name__ == "__main__":
    main()
