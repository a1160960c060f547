#!/usr/bin/env python3
"""Call time of ``spearman_corrcoef``, kernel against the switched-off torch chain.

Whole functional calls on seeded inputs. The kernel (``csrc/spearman.hip``) and
``METRICS_AMD_SPEARMAN_KERNEL=0`` alternate in one process (on, off, on, off,
...), ``--repeats`` windows each. A window is as many calls as fit
``--window-ms`` by the warm-up's estimate (at least one, at most ``--steps``);
every call ends in the readback of its own result, so a window is closed. The
switched-off chain loops over the repeated values on the host, so the row with
1e4 levels gets one call per switched-off window whatever the estimate says.
At 1e7 continuous fp32 values the chain meets so many repeated values that one
call does not end within minutes: that row times the kernel alone
(``--off-at-1e7`` runs the chain there too).

One JSON line per shape: median, min and max of the windows in ms per call for
both paths, their ratio, the largest difference between the two paths' rho, and
the byte floor of the kernel path at ``COPY_TBPS``: per element the inputs read
and the 12-byte pair written, per sort one 8-byte histogram read plus
``ceil(end_bit / 8)`` passes that read and write the pair (that the sort makes
exactly these passes is an assumption), the pair read and written by the first
rank pass and read by the second.

    python tools/bench_spearman.py [--repeats 5] [--max-elems 10000000]
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

from metrics_amd.functional.regression.spearman import spearman_corrcoef  # noqa: E402
from metrics_amd.ops import _hip  # noqa: E402

ENV = _hip.SPEARMAN_KERNEL_ENV
COPY_TBPS = 6.29
# (n, D, kind, dtype); kind: cont, tied (x in 7 values, y in 300), q1e4 (both quantised to 1e4 levels)
SHAPES = [(10**3, 1, "cont", "float32"), (10**5, 1, "cont", "float32"), (10**6, 1, "cont", "float32"),
          (10**7, 1, "cont", "float32"), (10**5, 8, "cont", "float32"), (128, 4096, "cont", "float32"),
          (10**6, 1, "tied", "float32"), (10**6, 1, "q1e4", "float32"), (10**6, 1, "cont", "bfloat16")]


def floor_ms(n: int, D: int, esize: int) -> float:
    end_bit = 32 + (D - 1).bit_length()
    sort = 8 + -(-end_bit // 8) * 24
    return 1000.0 * n * D * (2 * esize + 12 + 2 * sort + 24 + 12) / (COPY_TBPS * 1e12)


def _window(x, y, steps, env):
    os.environ[ENV] = env  # read at every call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = spearman_corrcoef(x, y).float().cpu()
    return 1000.0 * (time.perf_counter() - t0) / steps, out


def _summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-elems", type=int, default=10**7)
    ap.add_argument("--off-at-1e7", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "bench_spearman.py needs a GPU"
    device = torch.device("cuda", 0)
    for n, D, kind, dtype in SHAPES:
        if n * D > a.max_elems:
            continue
        gen = torch.Generator().manual_seed(1234)
        shape = (n,) if D == 1 else (n, D)
        if kind == "tied":
            x, y = (torch.randint(0, k, shape, generator=gen).float() for k in (7, 300))
        else:
            x, y = (torch.randn(shape, generator=gen) for _ in range(2))
            if kind == "q1e4":
                x, y = ((t.clamp(-4, 4) * 1250).round() / 1250 for t in (x, y))
        x, y = (t.to(getattr(torch, dtype)).to(device) for t in (x, y))
        envs = ("1", "0") if n < 10**7 or a.off_at_1e7 else ("1",)
        calls = _hip.spearman_kernel_calls()
        print(f"# {n} x {D} {kind} {dtype}: kernel warm-up", file=sys.stderr, flush=True)
        _window(x, y, 2, "1")
        print("# kernel warm-up done", file=sys.stderr, flush=True)
        assert _hip.spearman_kernel_calls() == calls + 2, "the kernel did not take the call"
        steps = {env: max(1, min(a.steps, int(a.window_ms / min(_window(x, y, 1, env)[0] for _ in range(2)))))
                 for env in envs}
        if kind == "q1e4":
            steps["0"] = 1
        ms = {"1": [], "0": []}
        rho = {}
        for _ in range(a.repeats):
            for env in envs:
                t, rho[env] = _window(x, y, steps[env], env)
                ms[env].append(t)
        os.environ[ENV] = "1"
        on, off = _summary(ms["1"]), (_summary(ms["0"]) if ms["0"] else None)
        print(json.dumps({
            "label": a.label, "n": n, "D": D, "kind": kind, "dtype": dtype, "repeats": a.repeats,
            "kernel_ms_per_call": on, "kernel_calls_per_window": steps["1"],
            "switched_off_ms_per_call": off,
            "switched_off_calls_per_window": steps.get("0"),
            "ratio": off and off["median"] / on["median"], "floor_ms": floor_ms(n, D, x.element_size()),
            "max_abs_rho_diff": off and (rho["1"] - rho["0"]).abs().max().item(),
        }), flush=True)


if __name__ == "__main__":
    main()
