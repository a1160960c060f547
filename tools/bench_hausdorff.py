#!/usr/bin/env python3
"""Call time of ``hausdorff_distance``, kernel against the switched-off torch path.

Masks are blob-like, not noise: per-class low-resolution random fields,
upsampled bilinearly, argmax over the classes. A segmentation model's output
has boundaries of about this length; noise would make nearly every pixel an
edge pixel. Seeded.

Shapes the switched-off path can still run (its dense distance matrix fits):
index inputs with 3 classes at (8, 64, 64) and (8, 128, 128). There the kernel
(``csrc/hausdorff.hip``) and ``METRICS_AMD_HAUSDORFF_KERNEL=0`` alternate in one
process (on, off, on, off, ...); a kernel window is ``--steps`` calls, a
switched-off window ONE call, because it takes seconds. Kernel-only shapes:
(16, 512, 1024) index with 19 classes and (8, 3, 512, 512) one-hot (bool).
Every call ends in the readback of its own result, so a window is closed.

One JSON line per shape: median, min and max of the windows in ms per call,
the edge pixels per listed plane, and for the first group the largest
difference between the two paths' values (square planes: they agree exactly).

    python tools/bench_hausdorff.py [--steps 100] [--repeats 5]
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

from metrics_amd.functional.segmentation import hausdorff_distance  # noqa: E402
from metrics_amd.ops import _hip  # noqa: E402

ENV = _hip.HAUSDORFF_KERNEL_ENV
# (N, C, H, W), input format, whether the switched-off path runs too
SHAPES = [
    ((8, 3, 64, 64), "index", True),
    ((8, 3, 128, 128), "index", True),
    ((16, 19, 512, 1024), "index", False),
    ((8, 3, 512, 512), "one-hot", False),
]


def blob_labels(N, C, H, W, device, gen):
    low = torch.rand(N, C, max(H // 16, 4), max(W // 16, 4), generator=gen).to(device)
    return torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False).argmax(1)


def edge_counts(labels, C):
    """Edge pixels per (n, c) plane of a label map, by the four-neighbour rule."""
    p = torch.nn.functional.pad(labels, (1, 1, 1, 1), value=-1)
    mid = p[:, 1:-1, 1:-1]
    edge = (p[:, :-2, 1:-1] != mid) | (p[:, 2:, 1:-1] != mid) | (p[:, 1:-1, :-2] != mid) | (p[:, 1:-1, 2:] != mid)
    n = torch.arange(labels.shape[0], device=labels.device)[:, None, None].expand_as(labels)
    return torch.bincount((n * C + labels)[edge], minlength=labels.shape[0] * C).view(-1, C)


def _window(args, steps, env):
    os.environ[ENV] = env  # read at every call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = hausdorff_distance(*args)
        out.cpu()
    return 1000.0 * (time.perf_counter() - t0) / steps, out


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "bench_hausdorff.py needs a GPU"
    device = torch.device("cuda", 0)
    for (N, C, H, W), fmt, with_off in SHAPES:
        gen = torch.Generator().manual_seed(1234)
        lp, lt = blob_labels(N, C, H, W, device, gen), blob_labels(N, C, H, W, device, gen)
        counts = torch.stack([edge_counts(lp, C), edge_counts(lt, C)])[:, :, 1:].float()
        if fmt == "one-hot":
            lp, lt = (torch.nn.functional.one_hot(x, C).movedim(-1, 1).bool().contiguous() for x in (lp, lt))
        args = (lp, lt, C, False, "euclidean", None, False, fmt)
        calls = _hip.hausdorff_kernel_calls()
        _window(args, a.warmup, "1")
        assert _hip.hausdorff_kernel_calls() == calls + a.warmup, "the kernel did not take the call"
        if with_off:
            _window(args, 1, "0")
        ms_on, ms_off, v_on, v_off = [], [], None, None
        for _ in range(a.repeats):
            ms, v_on = _window(args, a.steps, "1")
            ms_on.append(ms)
            if with_off:
                ms, v_off = _window(args, 1, "0")
                ms_off.append(ms)
        os.environ[ENV] = "1"
        line = {
            "label": a.label, "shape": [N, C, H, W], "input_format": fmt,
            "kernel_ms_per_call": _summary(ms_on), "steps": a.steps, "repeats": a.repeats,
            "edge_pixels_per_plane": {"mean": counts.mean().item(), "min": counts.min().item(), "max": counts.max().item()},
            "finite_mean": v_on[torch.isfinite(v_on)].mean().item(), "inf_planes": int(torch.isinf(v_on).sum()),
        }
        if with_off:
            s_off = _summary(ms_off)
            line.update({"switched_off_ms_per_call": s_off, "ratio": s_off["median"] / line["kernel_ms_per_call"]["median"],
                         "max_abs_diff": (v_on - v_off).abs().nan_to_num(0.0, 0.0, 0.0).max().item()})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
