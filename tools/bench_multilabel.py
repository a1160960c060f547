#!/usr/bin/env python3
"""Steady-state step time of a multilabel collection, by the discipline of bench.py.

The collection is {F1 (macro), Accuracy (micro), HammingDistance,
ConfusionMatrix, ExactMatch, AUROC, AveragePrecision}, validate_args=False,
T=200 curve thresholds, bf16 inputs, at the shapes (8192, 1000), (8192, 80)
and (65536, 14). Seeded pre-generated batches, a warm-up that includes one
compute() and a reset(), then ``--repeats`` timed windows of ``--steps``
updates, each closed by one synchronize; the JSON line per shape carries the
median window and the spread (min, max) over the windows.

Only the public API is used, so the script runs on any commit: where a commit
has no fused multilabel plan it measures the per-leader path. Set
METRICS_AMD_FUSE_MULTILABEL=0 for the A/B run on a commit that has it.

    python tools/bench_multilabel.py [--steps 200] [--warmup 16] [--repeats 5] [--inputs logits]
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

SHAPES = [(8192, 1000), (8192, 80), (65536, 14)]
# what one fused step has to move per element: 2 B of bf16 prediction, 8 B of int64 target
BYTES_PER_ELEMENT = 10


def build_collection(L, T, device):
    kw = dict(num_labels=L, validate_args=False)
    return ma.MetricCollection({
        "f1": ma.MultilabelF1Score(average="macro", **kw),
        "acc": ma.MultilabelAccuracy(average="micro", **kw),
        "hamming": ma.MultilabelHammingDistance(**kw),
        "confmat": ma.MultilabelConfusionMatrix(**kw),
        "exact": ma.MultilabelExactMatch(**kw),
        "auroc": ma.MultilabelAUROC(thresholds=T, **kw),
        "ap": ma.MultilabelAveragePrecision(thresholds=T, **kw),
    }).to(device)


def _window(coll, preds, target, steps):
    n = len(preds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        coll.update(preds[i % n], target[i % n])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--curve-thresholds", type=int, default=200)
    ap.add_argument("--inputs", choices=["logits", "probs"], default="logits")
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_multilabel.py needs a GPU"
    device = torch.device("cuda", 0)
    for N, L in SHAPES:
        torch.manual_seed(1234)
        preds = [torch.randn(N, L, device=device) * 3.0 for _ in range(4)]
        if args.inputs == "probs":
            preds = [p.sigmoid() for p in preds]
        preds = [p.to(torch.bfloat16) for p in preds]
        target = [torch.randint(0, 2, (N, L), device=device) for _ in range(4)]
        coll = build_collection(L, args.curve_thresholds, device)
        for i in range(args.warmup):
            coll.update(preds[i % 4], target[i % 4])
        coll.compute()
        coll.reset()
        windows = [_window(coll, preds, target, args.steps) for _ in range(args.repeats)]
        ms = sorted(1000.0 * w / args.steps for w in windows)
        plan = getattr(coll, "_fused_ml_plan", None)
        values = coll.compute()
        print(json.dumps({
            "label": args.label,
            "shape": [N, L],
            "inputs": args.inputs,
            "ms_per_step": statistics.median(ms),
            "ms_min": ms[0],
            "ms_max": ms[-1],
            "steps": args.steps,
            "repeats": args.repeats,
            "fuse_multilabel_env": os.environ.get("METRICS_AMD_FUSE_MULTILABEL", "1"),
            "fused_steps": getattr(plan, "steps", None),
            "step_megabytes": N * L * BYTES_PER_ELEMENT / 1e6,
            "f1": float(values["f1"]),
            "exact": float(values["exact"]),
            "auroc": float(values["auroc"]),
        }), flush=True)


if __name__ == "__main__":
    main()
