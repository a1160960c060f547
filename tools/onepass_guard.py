#!/usr/bin/env python3
"""Guard table for the one-pass update (profiles/README.md, "One-pass update"):
update loop of the bench collection, us/step before (`enqueue`) and after
(`synced`) the final synchronise, for one input kind and class count.

    METRICS_AMD_ONEPASS=2 python tools/onepass_guard.py --kind softmax --classes 1000

Prints one JSON line. Run from the repository root of the tree to measure.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.getcwd())
from bench import build_collection  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["randn", "softmax", "rand"], default="randn")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--thresholds", type=int, default=200)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", default="")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    B, C = args.batch, args.classes
    preds = []
    for _ in range(4):
        if args.kind == "rand":
            p = torch.rand(B, C, device=dev)
        else:
            p = torch.randn(B, C, device=dev)
            if args.kind == "softmax":
                p = torch.softmax(p, dim=1)
        preds.append(p.to(torch.bfloat16))
    target = [torch.randint(0, C, (B,), device=dev) for _ in range(4)]
    coll = build_collection(C, dev, args.thresholds)
    for i in range(33):
        coll.update(preds[i % 4], target[i % 4])
    coll.compute()
    coll.reset()
    torch.cuda.synchronize()
    enq, syn = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for i in range(args.steps):
            coll.update(preds[i % 4], target[i % 4])
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        enq.append(round(1e6 * (t1 - t0) / args.steps, 2))
        syn.append(round(1e6 * (t2 - t0) / args.steps, 2))
    plan = getattr(coll, "_fused_plan", None)
    print(json.dumps({
        "tree": args.tree, "onepass_env": os.environ.get("METRICS_AMD_ONEPASS"),
        "tail_grid_env": os.environ.get("MA_ONEPASS_TAIL_GRID"),
        "kind": args.kind, "C": C, "B": B, "T": args.thresholds,
        "enqueue_us": enq, "synced_us": syn,
        "onepass_steps": getattr(plan, "onepass_steps", None),
    }))


if __name__ == "__main__":
    main()
