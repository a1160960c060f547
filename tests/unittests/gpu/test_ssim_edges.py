"""Fused SSIM kernel (csrc/ssim.hip) at its edges, against the fp64 oracle.

Every case goes through the public functional, so the gate in ``_try_ssim_hip``
is covered too, and a wrapper around ``_hip.ssim2d_fused`` counts which path ran.
The cases, the oracle results and the per-case tolerance
``max(4 * |CPU fp32 path - oracle|, 8 * 2^-24 * max(1, |oracle|))`` come from
tests/unittests/_standalone_cases.py; tests/unittests/test_standalone_oracles.py
proves the oracle against the CPU path and the reference without a GPU. Each
test prints ``case |cpu - oracle| |gpu - oracle|`` (run with ``-s``): the source of
the table in docs/PARITY.md.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from metrics_amd import ops
from metrics_amd.functional.image import (
    multiscale_structural_similarity_index_measure as ms_ssim,
    structural_similarity_index_measure as ssim,
)
from metrics_amd.ops import _hip
from tests.unittests import _standalone_cases as cases
from tests.unittests import _standalone_oracles as oracle


@pytest.fixture(autouse=True)
def _require_hip():
    assert torch.cuda.is_available()
    assert ops.hip_available(), "HIP kernel library must be built and loadable on a GPU box"


@pytest.fixture
def fused(monkeypatch):
    """Counts entries into the fused kernel's wrapper and launches that went through."""
    calls = {"entered": 0, "ran": 0}
    real = _hip.ssim2d_fused

    def counted(*args, **kwargs):
        calls["entered"] += 1
        out = real(*args, **kwargs)
        calls["ran"] += 1
        return out

    monkeypatch.setattr(_hip, "ssim2d_fused", counted)
    return calls


def _check(cid, got, want, cpu, dtype=torch.float32):
    got = cases.ssim_functional_outputs(got)
    assert len(got) == len(want)
    for name, g, w, c in zip(("sim", "cs"), got, want, cpu):
        assert g.dtype == dtype and g.is_cuda
        cpu_err = float(np.abs(oracle.as_f64(c) - w).max())
        gpu_err = float(np.abs(oracle.as_f64(g).reshape(w.shape) - w).max())
        print(f"\nSSIM-ERR {cid} {str(dtype)[6:]} {name} cpu={cpu_err:.3e} gpu={gpu_err:.3e}")
        cases.assert_ssim_close(g, w, c, (cid, name), dtype)


@pytest.mark.parametrize("cid", list(cases.SSIM_CASES))
def test_ssim_case_meets_oracle(cid, fused):
    p, t, kw, want, cpu = cases.ssim_expected(cid)
    got = ssim(p.cuda(), t.cuda(), **kw)
    # which path ran: the kernel, or (radius 14: 67200 B of LDS) the torch formulation
    assert fused["entered"] == 1
    assert fused["ran"] == (1 if cases.SSIM_CASES[cid]["path"] == "kernel" else 0)
    _check(cid, got, want, cpu)
    if cid.partition("family-")[2] in cases.SSIM_EXACT_ONE:
        assert torch.all(cases.ssim_functional_outputs(got)[0] == 1.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64], ids=["bf16", "fp16", "fp64"])
@pytest.mark.parametrize("cid", cases.SSIM_DTYPE_CASES)
def test_ssim_dtypes(cid, dtype, fused):
    """The oracle and the CPU path (in fp32) see the rounded inputs. fp64 is cast to
    fp32 by the wrapper: fp32 tolerance, fp64 result."""
    p, t, kw, want, cpu = cases.ssim_expected(cid, dtype)
    assert p.dtype == dtype
    got = ssim(p.cuda(), t.cuda(), **kw)
    assert fused == {"entered": 1, "ran": 1}
    _check(cid, got, want, cpu, dtype)


def test_ssim_mixed_dtype_target_follows_preds(fused):
    p, t, kw, want, cpu = cases.ssim_expected("shape-33x31")
    got = ssim(p.cuda(), t.cuda().double(), **kw)
    assert fused["ran"] == 1
    _check("shape-33x31/target-fp64", got, want, cpu)


def test_ssim_non_contiguous_inputs(fused):
    p, t, kw, want, cpu = cases.ssim_expected("batch-3x2")
    B, C, H, W = p.shape
    wide_p, wide_t = torch.full((B, 2 * C, H, W), 9.0).cuda(), torch.full((B, 2 * C, H, W), -9.0).cuda()
    wide_p[:, ::2], wide_t[:, ::2] = p.cuda(), t.cuda()
    sl_p, sl_t = wide_p[:, ::2], wide_t[:, ::2]
    assert not sl_p.is_contiguous()
    _check("batch-3x2/channel-slice", ssim(sl_p, sl_t, **kw), want, cpu)
    cl_p = p.cuda().contiguous(memory_format=torch.channels_last)
    cl_t = t.cuda().contiguous(memory_format=torch.channels_last)
    assert not cl_p.is_contiguous()
    _check("batch-3x2/channels-last", ssim(cl_p, cl_t, **kw), want, cpu)
    assert fused == {"entered": 2, "ran": 2}


@pytest.mark.parametrize("cid", list(cases.MS_SSIM_CASES))
def test_ms_ssim_meets_oracle(cid, fused):
    p, t, kw, want, cpu = cases.ms_ssim_expected(cid)
    got = ms_ssim(p.cuda(), t.cuda(), **kw)
    scales = len(kw.get("betas", (0,) * 5))
    assert fused == {"entered": scales, "ran": scales}  # 176 -> 11: every scale fits the kernel
    cpu_err = float(np.abs(oracle.as_f64(cpu) - want).max())
    gpu_err = float(np.abs(oracle.as_f64(got).reshape(want.shape) - want).max())
    print(f"\nSSIM-ERR {cid} float32 ms cpu={cpu_err:.3e} gpu={gpu_err:.3e}")
    cases.assert_ssim_close(got, want, cpu, cid)


@pytest.mark.parametrize("B,C", cases.SSIM_PLANE_COUNTS, ids=lambda v: str(v))
def test_ssim_plane_count_around_grid_limit(B, C, fused):
    """B*C = 65535 planes is the most grid.z holds and runs the kernel; 65540 takes
    the torch formulation instead of failing the launch."""
    from metrics_amd.functional.image.ssim import structural_similarity_index_measure as ssim_fn

    p, t = cases.ssim_plane_images(B, C)
    kw = {"sigma": 0.5, "data_range": 1.0, "reduction": "none"}
    want, _, _ = oracle.ssim_oracle(p, t, sigma=0.5, data_range=1.0)
    cpu = ssim_fn(p, t, **kw)
    # the torch formulation as a native depthwise convolution: the convolution library's
    # search for a batch of 327700 10x10 images takes 20 s and is not what this test is about
    with torch.backends.cudnn.flags(enabled=B * C <= 65535):
        got = ssim(p.cuda(), t.cuda(), **kw)
    assert fused["entered"] == 1 and fused["ran"] == (1 if B * C <= 65535 else 0)
    assert got.shape == (B,)
    assert float(np.ptp(want)) > 0.1  # every image has its own value: a wrong plane mapping shows
    _check(f"planes-{B * C}", got, [want], [cpu])
