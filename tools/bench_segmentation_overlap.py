#!/usr/bin/env python3
"""Call time of ``mean_iou``, overlap kernel against the switched-off torch chain.

Masks are blob-like, not noise (per-class low-resolution random fields,
upsampled, argmax over the classes), except the row that says "random": labels
drawn per pixel, the wave merge's worst case. Seeded.

For every row the kernel (``csrc/seg_overlap.hip``) and
``METRICS_AMD_SEG_OVERLAP_KERNEL=0`` (the one-hot torch chain) alternate in one
process (on, off, on, off, ...): a kernel window is ``--steps`` calls, a
switched-off window ``--off-steps`` calls, because each of those moves
gigabytes. Every window ends in a device synchronize.

One JSON line per row: median, min and max of the windows in ms per call for
both paths, their ratio, the read floor (the bytes of both inputs at the
6.29 TB/s a copy kernel reaches on an MI355X) and the kernel's ratio to it, the
mapping the layout chose, and whether the two paths returned the same bits.

    python tools/bench_segmentation_overlap.py [--steps 100] [--off-steps 5] [--repeats 5]
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

from metrics_amd.functional.segmentation import mean_iou  # noqa: E402
from metrics_amd.ops import _hip  # noqa: E402

ENV = _hip.SEG_OVERLAP_KERNEL_ENV
COPY_BYTES_PER_S = 6.29e12
MAPPINGS = ("chunk", "wave", "planes")
# name, label shape (N, *spatial), C, label dtype, pattern, input format
ROWS = [
    ("int64 (16,512,1024)", (16, 512, 1024), 19, torch.int64, "blobs", "index"),
    ("int64 (32,256,256)", (32, 256, 256), 21, torch.int64, "blobs", "index"),
    ("uint8 (16,512,1024)", (16, 512, 1024), 19, torch.uint8, "blobs", "index"),
    ("small planes, wave mapping", (4096, 64, 64), 5, torch.int64, "blobs", "index"),
    ("small planes, chunk mapping", (4096, 64, 65), 5, torch.int64, "blobs", "index"),
    ("volume (2,128,128,128)", (2, 128, 128, 128), 14, torch.int64, "blobs", "index"),
    ("random int64 (16,512,1024)", (16, 512, 1024), 19, torch.int64, "random", "index"),
    ("bool planes (8,3,512,512)", (8, 512, 512), 3, torch.int64, "blobs", "one-hot"),
    ("mixed: int64 labels, bool planes", (8, 512, 512), 3, torch.int64, "blobs", "mixed"),
]


def labels(shape, C, pattern, device, gen):
    if pattern == "random":
        return torch.randint(0, C, shape, generator=gen).to(device)
    N, spatial = shape[0], shape[1:]
    low = torch.rand(N, C, *(max(s // 16, 4) for s in spatial), generator=gen).to(device)
    mode = {2: "bilinear", 3: "trilinear"}[len(spatial)]
    out = torch.empty(shape, dtype=torch.int64, device=device)
    for i in range(0, N, 256):  # in slices: the upsampled fields are C times the labels
        out[i:i + 256] = torch.nn.functional.interpolate(low[i:i + 256], size=spatial, mode=mode).argmax(1)
    return out


def _window(args, kwargs, steps, env):
    os.environ[ENV] = env  # read at every call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = mean_iou(*args, **kwargs)
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps, out


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--off-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "bench_segmentation_overlap.py needs a GPU"
    device = torch.device("cuda", 0)
    for name, shape, C, dtype, pattern, fmt in ROWS:
        gen = torch.Generator().manual_seed(1234)
        p, t = (labels(shape, C, pattern, device, gen).to(dtype) for _ in range(2))
        planes = [fmt == "one-hot", fmt != "index"]
        if planes[0]:
            p = torch.nn.functional.one_hot(p, C).movedim(-1, 1).bool().contiguous()
        if planes[1]:
            t = torch.nn.functional.one_hot(t, C).movedim(-1, 1).bool().contiguous()
        args, kwargs = (p, t), {"num_classes": C, "per_class": True, "input_format": fmt}
        calls = _hip.seg_overlap_kernel_calls()
        _window(args, kwargs, a.warmup, "1")
        assert _hip.seg_overlap_kernel_calls() == calls + a.warmup, "the kernel did not take the call"
        _window(args, kwargs, 1, "0")
        ms_on, ms_off = [], []
        for _ in range(a.repeats):
            ms, v_on = _window(args, kwargs, a.steps, "1")
            ms_on.append(ms)
            ms, v_off = _window(args, kwargs, a.off_steps, "0")
            ms_off.append(ms)
        os.environ[ENV] = "1"
        s_on, s_off = _summary(ms_on), _summary(ms_off)
        floor_ms = 1000.0 * (p.numel() * p.element_size() + t.numel() * t.element_size()) / COPY_BYTES_PER_S
        lay = _hip.seg_overlap_layout(shape[0], C, p[0, 0].numel() if planes[0] else p[0].numel(), *planes)
        print(json.dumps({
            "label": a.label, "row": name, "shape": list(shape), "C": C, "dtype": str(dtype).split(".")[1],
            "input_format": fmt, "mapping": MAPPINGS[lay[6]], "kernel_ms_per_call": s_on,
            "switched_off_ms_per_call": s_off, "steps": a.steps, "off_steps": a.off_steps, "repeats": a.repeats,
            "ratio_to_switched_off": s_off["median"] / s_on["median"], "read_floor_ms": floor_ms,
            "ratio_to_floor": s_on["median"] / floor_ms, "same_bits": bool(torch.equal(v_on, v_off)),
        }), flush=True)
        del p, t, v_on, v_off
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
