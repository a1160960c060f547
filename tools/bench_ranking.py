#!/usr/bin/env python3
"""Steady-state step time of a multilabel ranking collection, kernel against torch path.

The collection is {CoverageError, RankingAveragePrecision, RankingLoss},
validate_args=False, bf16 logits, 30 % relevant labels, at the shapes
(8192, 1000), (8192, 80) and (65536, 14). Seeded pre-generated batches. Two
collections per shape: one runs with the ranking kernel (``csrc/ml_rank.hip``,
one native call per step through the collection plan), one with
``METRICS_AMD_RANKING_KERNEL=0``, the torch path every commit before the kernel
ran. Their timed windows alternate in one session (on, off, on, off, ...), each
closed by one synchronize; the JSON line per shape carries the median window of
each side and the spread (min, max) over the windows.

The torch path loops over the rows on the host and syncs in every row, so a
step of it takes seconds at these shapes: its windows are ``--steps-off``
updates long (default 1), the kernel's ``--steps`` (default 100).

``native_ms`` is the native call alone (both launches, all three measures, on
scores that are normalised already), timed with device events around
``--steps`` calls; ``floor_ms`` is what reading the step's 10 B per element (2 B
of bf16 score, 8 B of int64 target) takes at ``--copy-tbs`` TB/s.

    python tools/bench_ranking.py [--steps 100] [--steps-off 1] [--repeats 5]
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
from metrics_amd.ops import _hip, multilabel_ranking_sums  # noqa: E402

SHAPES = [(8192, 1000), (8192, 80), (65536, 14)]
BYTES_PER_ELEMENT = 10
ENV = _hip.RANKING_KERNEL_ENV


def build_collection(L, device):
    kw = dict(num_labels=L, validate_args=False)
    return ma.MetricCollection({
        "coverage": ma.MultilabelCoverageError(**kw),
        "lrap": ma.MultilabelRankingAveragePrecision(**kw),
        "loss": ma.MultilabelRankingLoss(**kw),
    }).to(device)


def _window(coll, preds, target, steps, env):
    os.environ[ENV] = env  # read at every update
    n = len(preds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        coll.update(preds[i % n], target[i % n])
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps


def _native_ms(preds, target, steps):
    scores = [p.sigmoid() for p in preds]
    multilabel_ranking_sums(scores[0], target[0], None)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(steps):
        multilabel_ranking_sums(scores[i % len(scores)], target[i % len(scores)], None)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--steps-off", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--copy-tbs", type=float, default=6.29, help="what a copy kernel reaches on the chip, TB/s")
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_ranking.py needs a GPU"
    device = torch.device("cuda", 0)
    for N, L in SHAPES:
        torch.manual_seed(1234)
        preds = [(torch.randn(N, L, device=device) * 3.0).to(torch.bfloat16) for _ in range(4)]
        target = [(torch.rand(N, L, device=device) < 0.3).long() for _ in range(4)]
        os.environ[ENV] = "1"
        on = build_collection(L, device)
        for i in range(args.warmup):
            on.update(preds[i % 4], target[i % 4])
        on.compute()
        on.reset()
        os.environ[ENV] = "0"
        off = build_collection(L, device)
        for i in range(2):  # the second update is the first one on the group leaders
            off.update(preds[i % 4], target[i % 4])
        off.compute()
        off.reset()
        ms_on, ms_off = [], []
        for _ in range(args.repeats):
            ms_on.append(_window(on, preds, target, args.steps, "1"))
            ms_off.append(_window(off, preds, target, args.steps_off, "0"))
        os.environ[ENV] = "1"
        native = _native_ms(preds, target, args.steps)
        plan = getattr(on, "_fused_rank_plan", None)
        v_on, v_off = on.compute(), off.compute()
        s_on, s_off = _summary(ms_on), _summary(ms_off)
        print(json.dumps({
            "label": args.label,
            "shape": [N, L],
            "kernel_ms_per_step": s_on,
            "torch_path_ms_per_step": s_off,
            "ratio": s_off["median"] / s_on["median"],
            "steps": args.steps,
            "steps_off": args.steps_off,
            "repeats": args.repeats,
            "plan_steps": getattr(plan, "steps", None),
            "off_plan": getattr(off, "_fused_rank_plan", None) is not None,
            "native_ms": native,
            "floor_ms": N * L * BYTES_PER_ELEMENT / (args.copy_tbs * 1e9),
            "step_megabytes": N * L * BYTES_PER_ELEMENT / 1e6,
            "values_kernel": {k: float(v) for k, v in v_on.items()},
            "values_torch_path": {k: float(v) for k, v in v_off.items()},
        }), flush=True)


if __name__ == "__main__":
    main()
