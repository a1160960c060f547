#!/usr/bin/env python3
"""Call time of ``pairwise_manhattan_distance`` / ``pairwise_minkowski_distance``,
the tiled kernel against the switched-off torch chain.

For every row and exponent the kernel (``csrc/pairwise_lp.hip``) and
``METRICS_AMD_PAIRWISE_KERNEL=0`` (the torch chain with its (N, M, D)
temporaries) alternate in one process (on, off, on, off, ...), ``--repeats``
windows each, every window closed by a device synchronize. A window holds as
many whole public calls as fill ``--window-s`` seconds (from one timed call after
the warm-up), at least ``--min-steps``; the row reports the steps it used, so a
window shorter than asked is visible. Inputs are seeded randn.

The row marked "kernel only" is not run switched off: the chain's temporaries
do not fit the card. Its line carries the bytes ONE such temporary would take.

Floors, from shapes:
  vector  N * M * D times the instructions of the exponent class (2 for p = 1
          and p = 2, 3 for p = 3) over the fp32 vector rate: 256 CUs x 128
          lanes x 2.4 GHz = 78.6e12 lane-instructions/s (the 157.3 TFLOP/s
          fp32 peak counts an FMA as 2);
  bytes   both inputs read once and the output written once at the 6.29 TB/s a
          copy kernel reaches on an MI355X.
The larger one binds and is named in the line.

One JSON line per row and exponent: median, min and max of the windows in ms per
call for both paths, their ratio, the floors, the layout, and the largest
relative difference between the two paths' results.

    python tools/bench_pairwise.py [--window-s 0.25] [--repeats 5] [--only SUBSTRING]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from metrics_amd.functional.pairwise import pairwise_manhattan_distance, pairwise_minkowski_distance  # noqa: E402
from metrics_amd.ops import _hip  # noqa: E402

ENV = _hip.PAIRWISE_KERNEL_ENV
COPY_BYTES_PER_S = 6.29e12
VECTOR_LANE_INSTR_PER_S = 256 * 128 * 2.4e9
INSTR = {1: 2, 2: 2, 3: 3}
# name, (N, M, D), dtype, reduction, run the chain too
ROWS = [
    ("(2048, 2048, 128)", (2048, 2048, 128), torch.float32, None, True),
    ("(2048, 2048, 128) mean", (2048, 2048, 128), torch.float32, "mean", True),
    ("(2048, 2048, 128) bf16", (2048, 2048, 128), torch.bfloat16, None, True),
    ("(4096, 4096, 64)", (4096, 4096, 64), torch.float32, None, True),
    ("(512, 512, 2048)", (512, 512, 2048), torch.float32, None, True),
    ("(65536, 64, 16)", (65536, 64, 16), torch.float32, None, True),
    ("(20, 15, 7) toy: launch cost", (20, 15, 7), torch.float32, None, True),
    ("(8192, 8192, 512) kernel only", (8192, 8192, 512), torch.float32, None, False),
]


def _call(x, y, p, reduction):
    if p == 1:
        return pairwise_manhattan_distance(x, y, reduction=reduction)
    return pairwise_minkowski_distance(x, y, exponent=p, reduction=reduction)


def _window(x, y, p, reduction, steps, env):
    os.environ[ENV] = env  # read at every call
    out = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = _call(x, y, p, reduction)
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps, out


def _steps(x, y, p, reduction, env, a):
    _window(x, y, p, reduction, a.warmup, env)
    ms, _ = _window(x, y, p, reduction, 1, env)
    return max(a.min_steps, min(a.max_steps, math.ceil(1000.0 * a.window_s / ms)))


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--min-steps", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", help="rows whose name contains this")
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "bench_pairwise.py needs a GPU"
    for name, (N, M, D), dtype, reduction, with_chain in ROWS:
        if a.only not in name:
            continue
        gen = torch.Generator().manual_seed(1234)
        x = torch.randn(N, D, generator=gen).to("cuda", dtype)
        y = torch.randn(M, D, generator=gen).to("cuda", dtype)
        size = x.element_size()
        for p in (1, 2, 3):
            calls = _hip.pairwise_kernel_calls()
            steps_on = _steps(x, y, p, reduction, "1", a)
            assert _hip.pairwise_kernel_calls() == calls + a.warmup + 1, "the kernel did not take the call"
            steps_off = _steps(x, y, p, reduction, "0", a) if with_chain else 0
            ms_on, ms_off, v_off = [], [], None
            for _ in range(a.repeats):
                ms, v_on = _window(x, y, p, reduction, steps_on, "1")
                ms_on.append(ms)
                if with_chain:
                    ms, v_off = _window(x, y, p, reduction, steps_off, "0")
                    ms_off.append(ms)
            os.environ[ENV] = "1"
            s_on = _summary(ms_on)
            vector_ms = 1000.0 * N * M * D * INSTR[p] / VECTOR_LANE_INSTR_PER_S
            bytes_ms = 1000.0 * size * ((N + M) * D + (N if reduction else N * M)) / COPY_BYTES_PER_S
            line = {
                "label": a.label, "row": name, "shape": [N, M, D], "dtype": str(dtype).split(".")[1], "exponent": p,
                "reduction": reduction, "kernel_ms_per_call": s_on, "steps": steps_on, "repeats": a.repeats,
                "vector_floor_ms": vector_ms, "bytes_floor_ms": bytes_ms,
                "binding_floor": "vector" if vector_ms >= bytes_ms else "bytes",
                "ratio_to_floor": s_on["median"] / max(vector_ms, bytes_ms),
                "layout": _hip.pairwise_lp_layout(N, M, D),
            }
            if with_chain:
                s_off = _summary(ms_off)
                diff = ((v_on.double() - v_off.double()).abs() / v_off.double().abs().clamp_min(1e-30)).max().item()
                line.update({"switched_off_ms_per_call": s_off, "off_steps": steps_off,
                             "ratio_to_switched_off": s_off["median"] / s_on["median"], "max_rel_diff": diff})
            else:
                line.update({"switched_off_ms_per_call": "does not run",
                             "chain_bytes_per_temporary": N * M * D * size})
            print(json.dumps(line), flush=True)
            del v_on, v_off
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
