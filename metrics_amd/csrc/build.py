"""Build the in-tree HIP kernel library for gfx950.

The library is a plain HIP shared object (no torch C++ ABI linkage): Python
binds it with ctypes and passes raw device pointers + the current torch HIP
stream. That keeps the build a single fast hipcc invocation that
cross-compiles on CPU-only boxes, and the resulting .so lives in-tree
(metrics_amd/_lib/) so it travels with the repo snapshot to GPU machines.

Usage: python -m metrics_amd.csrc.build
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

CSRC = Path(__file__).resolve().parent
LIBDIR = CSRC.parent / "_lib"
LIBNAME = "libmetrics_hip.so"
ARCH = os.environ.get("METRICS_AMD_ARCH", "gfx950")
# Sources compiled with flags of their own. lm_nll.hip is built without the
# packed fp32 instructions (v_pk_add/mul/fma_f32): its folds are scalar per
# lane, and nothing in it may be paired up by the compiler; retrieval_score.hip
# likewise keeps its per-lane fp64 sums scalar, and hausdorff.hip the fp32
# distances of the points a lane holds (rounded one by one like the torch chain);
# kendall.hip has integer counts and fp64 sums only and is built the same way,
# and so is spearman.hip (integer rank sums, an fp64 tail). mc_compute.hip: its
# two-role kernel is integer work around the per-lane fp32 terms of the AUC sums.
# seg_overlap.hip is integer counting only and is built the same way.
# pairwise_lp.hip keeps one fp32 accumulator per output element, each term
# rounded on its own, and is built the same way.
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
OWN_FLAGS = {"lm_nll.hip": NO_PACKED_FP32, "retrieval_score.hip": NO_PACKED_FP32, "hausdorff.hip": NO_PACKED_FP32,
             "kendall.hip": NO_PACKED_FP32, "spearman.hip": NO_PACKED_FP32, "mc_compute.hip": NO_PACKED_FP32,
             "seg_overlap.hip": NO_PACKED_FP32, "pairwise_lp.hip": NO_PACKED_FP32}


def build(verbose: bool = True) -> Path:
    """Compile csrc/*.hip (gfx950) and csrc/*.cpp (host) into metrics_amd/_lib/."""
    LIBDIR.mkdir(exist_ok=True)
    out = LIBDIR / LIBNAME
    base = ["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC"]
    srcs = []
    for p in sorted(CSRC.glob("*.hip")):
        if p.name not in OWN_FLAGS:
            srcs.append(str(p))
            continue
        # a file with flags of its own becomes an object first (under _lib/, untracked)
        obj = LIBDIR / (p.stem + ".o")
        cmd = [*base, *OWN_FLAGS[p.name], "-c", str(p), "-o", str(obj)]
        if verbose:
            print("+", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        srcs.append(f"-Wl,{obj}")  # straight to the linker: hipcc reads every bare input as HIP source
    cmd = [
        *base,
        "-shared",
        *srcs,
        "-o",
        str(out),
    ]
    if verbose:
        print("+", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)

    # host-side native components (COCO matcher): plain g++, no GPU linkage
    cpp_srcs = sorted(str(p) for p in CSRC.glob("*.cpp"))
    if cpp_srcs:
        cpu_out = LIBDIR / "libmetrics_cpu.so"
        cmd = ["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-fopenmp", *cpp_srcs, "-o", str(cpu_out)]
        if verbose:
            print("+", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    return out


def cpu_lib_path() -> Path:
    return LIBDIR / "libmetrics_cpu.so"


def lib_path() -> Path:
    return LIBDIR / LIBNAME


def is_built() -> bool:
    return lib_path().exists()


if __name__ == "__main__":
    build()
