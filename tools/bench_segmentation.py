#!/usr/bin/env python3
"""Steady-state step time of a multiclass collection fed per-pixel predictions,
by the discipline of bench.py.

The collection is {Accuracy, F1, JaccardIndex, ConfusionMatrix, ExactMatch,
AUROC, AveragePrecision}, validate_args=False, T=200 curve thresholds, bf16
(N, C, H, W) inputs with an (N, H, W) target, updates only, at the shapes
(16, 19, 512, 1024), (32, 21, 256, 256) and (8, 96, 512, 512), as logits and as
probabilities (their softmax). Seeded pre-generated batches, a warm-up that
includes one compute() and a reset(), then ``--repeats`` timed windows of
``--steps`` updates, each closed by one synchronize; the JSON line per shape,
input kind and variant carries the median window and the spread (min, max).

``--variants fused,off`` measures the fused spatial step and the same
collection built under METRICS_AMD_FUSE_SPATIAL=0 in ONE process, their windows
alternating, so that both see the same clocks and the same neighbours. Only the
public API is used, so the script also runs on a commit without the step
(``--variants off``, which is all such a commit has).

    python tools/bench_segmentation.py [--steps 20] [--warmup 6] [--repeats 5] [--variants fused,off]
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

SHAPES = [(16, 19, 512, 1024), (32, 21, 256, 256), (8, 96, 512, 512)]
FUSE_ENV = "METRICS_AMD_FUSE_SPATIAL"
HBM_TBPS = 6.29  # the peak the project quotes for an MI355X


def build_collection(C, T, device, ignore_index=None):
    kw = dict(num_classes=C, validate_args=False, ignore_index=ignore_index)
    return ma.MetricCollection({
        "acc": ma.MulticlassAccuracy(**kw),
        "f1": ma.MulticlassF1Score(**kw),
        "jaccard": ma.MulticlassJaccardIndex(**kw),
        "confmat": ma.MulticlassConfusionMatrix(**kw),
        "exact": ma.MulticlassExactMatch(**kw),
        "auroc": ma.MulticlassAUROC(thresholds=T, **kw),
        "ap": ma.MulticlassAveragePrecision(thresholds=T, **kw),
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--curve-thresholds", type=int, default=200)
    ap.add_argument("--inputs", default="logits,probs")
    ap.add_argument("--variants", default="fused,off")
    ap.add_argument("--shapes", default="0,1,2", help="indices into the shape list")
    ap.add_argument("--ignore-index", type=int, default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_segmentation.py needs a GPU"
    device = torch.device("cuda", 0)
    variants = args.variants.split(",")
    for shape in [SHAPES[int(i)] for i in args.shapes.split(",")]:
        N, C, H, W = shape
        for kind in args.inputs.split(","):
            torch.manual_seed(1234)
            preds = [torch.randn(*shape, device=device) * 3.0 for _ in range(2)]
            if kind == "probs":
                preds = [p.softmax(1) for p in preds]
            preds = [p.to(torch.bfloat16) for p in preds]
            target = [torch.randint(0, C, (N, H, W), device=device) for _ in range(2)]
            colls = {}
            for v in variants:
                # the switch is read when the collection builds its plan, at the second update
                os.environ[FUSE_ENV] = "0" if v == "off" else "1"
                coll = colls[v] = build_collection(C, args.curve_thresholds, device, args.ignore_index)
                for i in range(args.warmup):
                    coll.update(preds[i % 2], target[i % 2])
                coll.compute()
                coll.reset()
            windows = {v: [] for v in variants}
            for _ in range(args.repeats):
                for v in variants:
                    windows[v].append(_window(colls[v], preds, target, args.steps))
            pixels = N * H * W
            # what one fused step has to read per pixel: C bf16 predictions and one int64 target
            step_bytes = pixels * (2 * C + 8)
            for v in variants:
                ms = sorted(1000.0 * w / args.steps for w in windows[v])
                plan = getattr(colls[v], "_fused_sp_plan", None)
                values = colls[v].compute()
                print(json.dumps({
                    "label": args.label,
                    "variant": v,
                    "shape": list(shape),
                    "inputs": kind,
                    "ms_per_step": statistics.median(ms),
                    "ms_min": ms[0],
                    "ms_max": ms[-1],
                    "steps": args.steps,
                    "repeats": args.repeats,
                    "fused_steps": getattr(plan, "steps", None),
                    "curve_steps": getattr(plan, "curve_steps", None),
                    "step_megabytes": step_bytes / 1e6,
                    "read_floor_ms": step_bytes / (HBM_TBPS * 1e12) * 1e3,
                    "acc": float(values["acc"]),
                    "jaccard": float(values["jaccard"]),
                    "auroc": float(values["auroc"]),
                }), flush=True)
            del colls, preds, target
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
