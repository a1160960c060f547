#!/usr/bin/env python3
"""Guard figures for the collection compute() (profiles/README.md, "Collection
compute plan"): the bench collection runs `update(); compute()` pairs; per
compute() it reports the host wall time up to the return of the call
(`enqueue`) and the time with a synchronise after it (`synced`), as the median
over the pairs of each repetition. The stream is drained before every
compute(), so neither figure contains the update.

    python tools/compute_guard.py
    METRICS_AMD_COMPUTE_PLAN=0 python tools/compute_guard.py

Under a kernel trace (in a run of its own) the launches and the kernel time
per compute follow from the counts this prints: every kernel that is not one
of the two update kernels belongs to a compute, and `computes_total` says how
many there were, warm-up included.

Prints one JSON line. Run from the repository root of the tree to measure.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.getcwd())
from bench import build_collection  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--thresholds", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", default="")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    B, C = args.batch, args.classes
    preds = [torch.randn(B, C, device=dev, dtype=torch.bfloat16) for _ in range(4)]
    target = [torch.randint(0, C, (B,), device=dev) for _ in range(4)]
    coll = build_collection(C, dev, args.thresholds)
    warm = 8
    for i in range(warm):
        coll.update(preds[i % 4], target[i % 4])
        coll.compute()
    coll.reset()
    torch.cuda.synchronize()
    enq, syn = [], []
    for _ in range(args.reps):
        e, s = [], []
        for i in range(args.pairs):
            coll.update(preds[i % 4], target[i % 4])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            coll.compute()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            e.append(1e6 * (t1 - t0))
            s.append(1e6 * (t2 - t0))
        enq.append(round(statistics.median(e), 2))
        syn.append(round(statistics.median(s), 2))
    print(json.dumps({
        "tree": args.tree, "compute_plan_env": os.environ.get("METRICS_AMD_COMPUTE_PLAN"),
        "C": C, "B": B, "T": args.thresholds, "pairs": args.pairs,
        "enqueue_us": enq, "synced_us": syn,
        "enqueue_us_median": statistics.median(enq), "synced_us_median": statistics.median(syn),
        "computes_total": warm + args.reps * args.pairs,
        "updates_total": warm + args.reps * args.pairs,
        "plan_steps": getattr(getattr(coll, "_compute_plan", None), "steps", None),
    }))


if __name__ == "__main__":
    main()
