#!/usr/bin/env python3
"""Steady-state update time of ``Perplexity``, NLL kernel against the torch chain.

Updates only, on one seeded pre-generated batch per shape, at the shapes a
language-model evaluation runs (``SHAPES`` below): contiguous logits, the
shifted views ``logits[:, :-1]`` / ``labels[:, 1:]`` of a (B, T + 1, V) buffer,
and a batch with a third of its rows ignored. Two metrics per shape: one runs
the kernel (``csrc/lm_nll.hip``, one native call of two launches per update),
one runs with ``METRICS_AMD_PERPLEXITY_KERNEL=0``, the torch chain every commit
before the kernel ran. Their timed windows alternate in one process (kernel,
off, kernel, off, ...), each closed by one synchronize; the JSON line per shape
carries the median window of each side and the spread (min, max) over
``--repeats`` windows. ``--depths 4 8`` times the kernel once per value of the
``MA_LM_NLL_DEPTH`` knob (16-byte loads in flight per lane).

A step of the torch chain moves the logits many times over, so its windows are
``--steps-off`` updates long (default 10), the kernel's ``--steps`` (default 200).

``floor_ms`` is what one read of the kept rows takes at ``--copy-tbs`` TB/s:
kept rows x V x element size.

    python tools/bench_perplexity.py [--steps 200] [--steps-off 10] [--repeats 5]
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

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
# (B, T, V, dtype, variant)
SHAPES = [
    (8, 2048, 32000, BF16, "contiguous"),
    (4, 4096, 128256, BF16, "contiguous"),
    (4, 4096, 128256, BF16, "shifted"),
    (4, 4096, 128256, BF16, "third_ignored"),
    (64, 512, 50304, FP16, "contiguous"),
    (1, 512, 262144, FP32, "contiguous"),
    (4096, 256, 256, FP32, "contiguous"),
]
ENV = _hip.PERPLEXITY_KERNEL_ENV
IGNORE = -100


def make_batch(B, T, V, dtype, variant, device):
    torch.manual_seed(1234)
    rows_t = T + 1 if variant == "shifted" else T
    logits = torch.randn(B, rows_t, V, device=device, dtype=dtype)
    labels = torch.randint(0, V, (B, rows_t), device=device)
    if variant == "third_ignored":
        labels[torch.rand(B, rows_t, device=device) < 1 / 3] = IGNORE
    if variant == "shifted":
        return logits[:, :-1], labels[:, 1:]
    return logits, labels


def _window(metric, preds, target, steps, env, depth=None):
    os.environ[ENV] = env  # read at every update
    if depth is not None:
        os.environ["MA_LM_NLL_DEPTH"] = str(depth)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        metric.update(preds, target)
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--steps-off", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--depths", type=int, nargs="*", default=[], help="MA_LM_NLL_DEPTH values to time (default: the built-in)")
    ap.add_argument("--copy-tbs", type=float, default=6.29, help="what a copy kernel reaches on the chip, TB/s")
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench_perplexity.py needs a GPU"
    device = torch.device("cuda", 0)
    depths = args.depths or [None]
    for B, T, V, dtype, variant in SHAPES:
        preds, target = make_batch(B, T, V, dtype, variant, device)
        kept = int((target != IGNORE).sum())
        lay = _hip.lm_nll_layout(B * T, V, dtype)
        on = {d: ma.Perplexity(ignore_index=IGNORE).to(device) for d in depths}
        off = ma.Perplexity(ignore_index=IGNORE).to(device)
        for d in depths:
            _window(on[d], preds, target, args.warmup, "1", d)
            on[d].reset()
        _window(off, preds, target, 1, "0")
        off.reset()
        ms_on, ms_off = {d: [] for d in depths}, []
        for _ in range(args.repeats):
            for d in depths:
                ms_on[d].append(_window(on[d], preds, target, args.steps, "1", d))
            ms_off.append(_window(off, preds, target, args.steps_off, "0"))
        os.environ[ENV] = "1"
        s_off = _summary(ms_off)
        for d in depths:
            s_on = _summary(ms_on[d])
            print(json.dumps({
                "label": args.label,
                "shape": [B, T, V],
                "dtype": str(dtype).replace("torch.", ""),
                "variant": variant,
                "depth": d,
                "mapping": lay.mapping if lay is not None else None,
                "kernel_ms_per_step": s_on,
                "torch_chain_ms_per_step": s_off,
                "ratio": s_off["median"] / s_on["median"],
                "steps": args.steps,
                "steps_off": args.steps_off,
                "repeats": args.repeats,
                "kept_rows": kept,
                "floor_ms": kept * V * preds.element_size() / (args.copy_tbs * 1e9),
                "value_kernel": float(on[d].compute()),
                "value_torch_chain": float(off.compute()),
            }), flush=True)
        del preds, target, on, off
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
