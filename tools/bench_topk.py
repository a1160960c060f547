#!/usr/bin/env python3
"""Step time of collections with a top-5 member, by the discipline of bench.py.

Two collections at the bench shape (B=8192, C=1000, bf16 logits, T=200):

  bench16_top5   the 16 bench metrics plus MulticlassAccuracy(top_k=5, micro)
  top1_top5      top-1 and top-5 accuracy alone

Seeded pre-generated batches, a warm-up that includes one compute(), one
synchronize at the end of the timed window. Only the public API is used, so
the script runs on any commit; set METRICS_AMD_FUSE_TOPK=0 for the A/B run.
One JSON line per collection.

    python tools/bench_topk.py [--steps 400] [--warmup 16] [--which both]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import metrics_amd as ma  # noqa: E402
from bench import build_collection  # noqa: E402


def _collections(C, T, device):
    kw = dict(num_classes=C, validate_args=False)

    def bench16_top5():
        base = build_collection(C, device, T)
        metrics = {name: m for name, m in base.items(keep_base=True, copy_state=False)}
        metrics["acc_top5"] = ma.MulticlassAccuracy(top_k=5, average="micro", **kw)
        return ma.MetricCollection(metrics).to(device)

    def top1_top5():
        return ma.MetricCollection({
            "acc_top1": ma.MulticlassAccuracy(average="micro", **kw),
            "acc_top5": ma.MulticlassAccuracy(top_k=5, average="micro", **kw),
        }).to(device)

    return {"bench16_top5": bench16_top5, "top1_top5": top1_top5}


def _time(coll, preds, target, steps, warmup, compute_every):
    n = len(preds)

    def one_step(i):
        coll.update(preds[i % n], target[i % n])
        if compute_every and (i + 1) % compute_every == 0:
            coll.compute()

    for i in range(warmup):
        one_step(i)
    coll.compute()
    coll.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one_step(i)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--curve-thresholds", type=int, default=200)
    ap.add_argument("--compute-every", type=int, default=32)
    ap.add_argument("--which", choices=["both", "bench16_top5", "top1_top5"], default="both")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_topk.py needs a GPU"
    device = torch.device("cuda", 0)
    torch.manual_seed(1234)
    preds = [torch.randn(args.batch, args.classes, device=device, dtype=torch.bfloat16) for _ in range(4)]
    target = [torch.randint(0, args.classes, (args.batch,), device=device) for _ in range(4)]

    makers = _collections(args.classes, args.curve_thresholds, device)
    for name, make in makers.items():
        if args.which not in ("both", name):
            continue
        coll = make()
        elapsed = _time(coll, preds, target, args.steps, args.warmup, args.compute_every)
        plan = getattr(coll, "_fused_plan", None)
        print(json.dumps({
            "collection": name,
            "ms_per_step": 1000.0 * elapsed / args.steps,
            "steps": args.steps,
            "fuse_topk_env": os.environ.get("METRICS_AMD_FUSE_TOPK", "1"),
            "topk_steps": getattr(plan, "topk_steps", None),
            "acc_top5": float(coll.compute()["acc_top5"]),
        }), flush=True)


if __name__ == "__main__":
    main()
