#!/usr/bin/env python3
"""Call time of ``kendall_rank_corrcoef``, kernel against the switched-off numpy path.

Whole functional calls (tau-b, no t-test) on fp32 inputs, seeded. The kernel
(``csrc/kendall.hip``) and ``METRICS_AMD_KENDALL_KERNEL=0`` alternate in one
process (on, off, on, off, ...), ``--repeats`` windows each. A window is as many
calls as fit ``--window-ms`` by the warm-up's estimate (at least one, at most
``--steps``); every call ends in the readback of its own result, so a window is
closed. Shapes: n = 1e3 ... 1e7 at D = 1, 1e5 at D = 8, and 1e6 heavily tied
(x in 7 values, y in 300).

One JSON line per shape: median, min and max of the windows in ms per call for
both paths, their ratio, and the largest difference between the two paths' tau.

    python tools/bench_kendall.py [--repeats 5] [--max-n 10000000]
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

from metrics_amd.functional.regression.kendall import kendall_rank_corrcoef  # noqa: E402
from metrics_amd.ops import _hip  # noqa: E402

ENV = _hip.KENDALL_KERNEL_ENV
# (n, D, tied)
SHAPES = [(10**3, 1, False), (10**4, 1, False), (10**5, 1, False), (10**6, 1, False), (10**7, 1, False),
          (10**5, 8, False), (10**6, 1, True)]


def _window(x, y, steps, env):
    os.environ[ENV] = env  # read at every call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = kendall_rank_corrcoef(x, y).cpu()
    return 1000.0 * (time.perf_counter() - t0) / steps, out


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=10**7)
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "bench_kendall.py needs a GPU"
    device = torch.device("cuda", 0)
    for n, D, tied in SHAPES:
        if n > a.max_n:
            continue
        gen = torch.Generator().manual_seed(1234)
        shape = (n,) if D == 1 else (n, D)
        if tied:
            x, y = (torch.randint(0, k, shape, generator=gen).float().to(device) for k in (7, 300))
        else:
            x, y = (torch.randn(shape, generator=gen).to(device) for _ in range(2))
        calls = _hip.kendall_kernel_calls()
        _window(x, y, 2, "1")
        assert _hip.kendall_kernel_calls() == calls + 2, "the kernel did not take the call"
        _window(x, y, 1, "0")
        steps = {env: max(1, min(a.steps, int(a.window_ms / _window(x, y, 1, env)[0]))) for env in ("1", "0")}
        ms = {"1": [], "0": []}
        tau = {}
        for _ in range(a.repeats):
            for env in ("1", "0"):
                t, tau[env] = _window(x, y, steps[env], env)
                ms[env].append(t)
        os.environ[ENV] = "1"
        on, off = _summary(ms["1"]), _summary(ms["0"])
        print(json.dumps({
            "label": a.label, "n": n, "D": D, "tied": tied, "repeats": a.repeats,
            "kernel_ms_per_call": on, "kernel_calls_per_window": steps["1"],
            "switched_off_ms_per_call": off, "switched_off_calls_per_window": steps["0"],
            "ratio": off["median"] / on["median"],
            "max_abs_tau_diff": (tau["1"] - tau["0"]).abs().max().item(),
        }), flush=True)


if __name__ == "__main__":
    main()
