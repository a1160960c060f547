"""ctypes bindings for the in-tree gfx950 HIP kernel library.

Every wrapper takes torch CUDA (= HIP on ROCm) tensors, validates layout,
and launches on the *current* torch stream — so kernels order correctly with
surrounding torch ops without any global synchronization.

If the library is missing on a GPU machine, these raise loudly: metric
updates must never silently fall back to stock torch kernels on MI355X.
"""
from __future__ import annotations

import ctypes
import math
import operator
import os
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from metrics_amd.csrc.build import lib_path

_LIB: Optional[ctypes.CDLL] = None
_LOAD_ERR: Optional[str] = None


def _load() -> Optional[ctypes.CDLL]:
    global _LIB, _LOAD_ERR
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not p.exists():
        _LOAD_ERR = f"HIP kernel library not built at {p}. Run `python -m metrics_amd.csrc.build`."
        return None
    try:
        lib = ctypes.CDLL(str(p))
    except OSError as err:
        _LOAD_ERR = f"Failed to load {p}: {err}"
        return None
    _declare_argtypes(lib)  # raises on a record mismatch: such a library is never published
    _LIB = lib
    return _LIB


_U64 = ctypes.c_uint64
_LL = ctypes.c_longlong
_I = ctypes.c_int
_F = ctypes.c_float
_D = ctypes.c_double


class McStepTensors(NamedTuple):
    """The tensor objects one multiclass step works on, by name. Every optional
    group is None when absent."""

    counts: Tensor  # [tp|fp|fn|valid], (3*C+1,) int64: the count pass fills it, the apply pass zeroes it
    confmat: Optional[Tensor] = None  # (C, C) state, counted into directly
    tp: Optional[Tensor] = None  # the four stat states, (C,) each
    fp: Optional[Tensor] = None
    tn: Optional[Tensor] = None
    fn: Optional[Tensor] = None
    correct: Optional[Tensor] = None  # the exact-match states
    total: Optional[Tensor] = None
    rowstats: Optional[Tensor] = None  # (2, >=B) float32 [rowmax; rowinv], with epoch_buf
    epoch_buf: Optional[Tensor] = None  # the curve leader's device epoch E
    topk_counts: Optional[Tensor] = None  # [tp_k|fp_k|fn_k], (3*C,) int64, with the four states below
    tp_k: Optional[Tensor] = None
    fp_k: Optional[Tensor] = None
    tn_k: Optional[Tensor] = None
    fn_k: Optional[Tensor] = None


class McStep(ctypes.Structure):
    """Mirror of ``McStep`` in csrc/mc_step.h, field for field: the fixed part
    of one multiclass step as the native count / apply / plan entries read it.
    ``_load`` holds field names, order and size against the header,
    tests/unittests/test_mc_step_record.py every field's offset as well."""

    _fields_ = [
        ("C", _LL), ("ignore_index", _LL), ("has_ignore", _LL),
        ("counts", _U64), ("confmat", _U64),
        ("tp", _U64), ("fp", _U64), ("tn", _U64), ("fn", _U64),
        ("correct", _U64), ("total", _U64),
        ("rowmax", _U64), ("rowinv", _U64), ("epoch_buf", _U64),
        ("k", _LL), ("topk_counts", _U64),
        ("tp_k", _U64), ("fp_k", _U64), ("tn_k", _U64), ("fn_k", _U64),
    ]


_STEP_P = ctypes.POINTER(McStep)


def mc_step(num_classes: int, ignore_index: Optional[int], t: McStepTensors, k: int = 0) -> McStep:
    """The record of one step over ``num_classes`` classes and the tensors
    ``t`` (``k`` > 0 turns the top-k slot on). It holds bare addresses: whoever
    keeps the record keeps ``t`` next to it."""
    rec = McStep(C=num_classes, ignore_index=ignore_index if ignore_index is not None else 0,
                 has_ignore=ignore_index is not None, k=k)
    for name, x in zip(t._fields, t):
        if x is not None and name != "rowstats":
            setattr(rec, name, x.data_ptr())
    if t.rowstats is not None:
        rec.rowmax = t.rowstats.data_ptr()
        rec.rowinv = rec.rowmax + 4 * t.rowstats.shape[1]
    return rec


class MlStepTensors(NamedTuple):
    """The tensor objects one fused multilabel step works on, by name. Every
    optional group is None when absent."""

    counts: Tensor  # (6*L,) int64 count scratch: the step fills it, the tail zeroes it
    records: Tensor  # one uint8 per block of the step kernel
    tp: Optional[Tensor] = None  # the four stat states, (L,) each
    fp: Optional[Tensor] = None
    tn: Optional[Tensor] = None
    fn: Optional[Tensor] = None
    confmat: Optional[Tensor] = None  # (L, 2, 2) state
    correct: Optional[Tensor] = None  # the exact-match states, with rowbad
    total: Optional[Tensor] = None
    rowbad: Optional[Tensor] = None  # (>=N,) int32 mismatch words, zero between steps
    thresholds: Optional[Tensor] = None  # the curve group: float32 thresholds,
    hist: Optional[Tensor] = None  # the lazy (L, T+1, 2) histogram,
    epoch_buf: Optional[Tensor] = None  # the device epoch E
    region_flags: Optional[Tensor] = None  # and one uint8 per region, zero between steps


class MlStep(ctypes.Structure):
    """Mirror of ``MlStep`` in csrc/ml_step.h, field for field. ``_load`` holds
    field names, order and size against the header."""

    _fields_ = [
        ("L", _LL), ("ignore_index", _LL), ("has_ignore", _LL), ("thr", _D),
        ("counts", _U64), ("records", _U64),
        ("tp", _U64), ("fp", _U64), ("tn", _U64), ("fn", _U64), ("confmat", _U64),
        ("correct", _U64), ("total", _U64), ("rowbad", _U64),
        ("T", _LL), ("thresholds", _U64), ("uniform", _LL), ("t0", _D), ("inv_step", _D),
        ("hist", _U64), ("epoch_buf", _U64), ("region_flags", _U64), ("region_cap", _LL),
    ]


_ML_STEP_P = ctypes.POINTER(MlStep)


def ml_step(num_labels: int, ignore_index: Optional[int], threshold: float, t: MlStepTensors,
            uniform: tuple = (0, 0.0, 1.0)) -> MlStep:
    """The record of one multilabel step over ``num_labels`` labels and the
    tensors ``t``, filled by name. The curve group is on iff ``t.thresholds`` is
    given; ``uniform`` = its :func:`_uniform_params`. It holds bare addresses:
    whoever keeps the record keeps ``t`` next to it."""
    rec = MlStep(L=num_labels, ignore_index=ignore_index if ignore_index is not None else 0,
                 has_ignore=ignore_index is not None, thr=float(threshold))
    for name, x in zip(t._fields, t):
        if x is not None:
            setattr(rec, name, x.data_ptr())
    if t.thresholds is not None:
        rec.T = t.thresholds.shape[0]
        rec.uniform, rec.t0, rec.inv_step = uniform
        rec.region_cap = t.region_flags.shape[0]
    return rec


class BinStepTensors(NamedTuple):
    """The tensor objects one fused binary step works on, by name. Every
    optional group is None when absent."""

    counts: Tensor  # (6,) int64 count scratch: the step fills it, the tail zeroes it
    records: Tensor  # one uint8 per block of the step kernel
    tp: Optional[Tensor] = None  # the four stat states, one element each
    fp: Optional[Tensor] = None
    tn: Optional[Tensor] = None
    fn: Optional[Tensor] = None
    confmat: Optional[Tensor] = None  # (2, 2) state
    thresholds: Optional[Tensor] = None  # the curve group: float32 thresholds,
    hist: Optional[Tensor] = None  # the lazy (1, T+1, 2) histogram,
    curve_scratch: Optional[Tensor] = None  # the per-step (2, T+1, 2) scratch, zero between steps,
    epoch_buf: Optional[Tensor] = None  # and the device epoch E


class BinStep(ctypes.Structure):
    """Mirror of ``BinStep`` in csrc/bin_step.h, field for field. ``_load`` holds
    field names, order and size against the header."""

    _fields_ = [
        ("ignore_index", _LL), ("has_ignore", _LL), ("thr", _D),
        ("counts", _U64), ("records", _U64),
        ("tp", _U64), ("fp", _U64), ("tn", _U64), ("fn", _U64), ("confmat", _U64),
        ("T", _LL), ("thresholds", _U64), ("uniform", _LL), ("t0", _D), ("inv_step", _D),
        ("hist", _U64), ("curve_scratch", _U64), ("epoch_buf", _U64),
    ]


_BIN_STEP_P = ctypes.POINTER(BinStep)


def bin_step(ignore_index: Optional[int], threshold: float, t: BinStepTensors,
             uniform: tuple = (0, 0.0, 1.0)) -> BinStep:
    """The record of one binary step over the tensors ``t``, filled by name. The
    curve group is on iff ``t.thresholds`` is given; ``uniform`` = its
    :func:`_uniform_params`. It holds bare addresses: whoever keeps the record
    keeps ``t`` next to it."""
    rec = BinStep(ignore_index=ignore_index if ignore_index is not None else 0,
                  has_ignore=ignore_index is not None, thr=float(threshold))
    for name, x in zip(t._fields, t):
        if x is not None:
            setattr(rec, name, x.data_ptr())
    if t.thresholds is not None:
        rec.T = t.thresholds.shape[0]
        rec.uniform, rec.t0, rec.inv_step = uniform
    return rec


class McSpatialStepTensors(NamedTuple):
    """The tensor objects one fused spatial multiclass step works on, by name.
    Every optional group is None when absent."""

    counts: Tensor  # [tp|fp|fn], (3*C,) int64 count scratch: the step fills it, the tail zeroes it
    records: Tensor  # three int32 per block of the step kernel
    tp: Optional[Tensor] = None  # the four stat states, (C,) each
    fp: Optional[Tensor] = None
    tn: Optional[Tensor] = None
    fn: Optional[Tensor] = None
    confmat: Optional[Tensor] = None  # (C, C) state, counted into directly
    correct: Optional[Tensor] = None  # the exact-match states, with rowbad
    total: Optional[Tensor] = None
    rowbad: Optional[Tensor] = None  # (>=N,) int32 mismatch words, zero between steps
    thresholds: Optional[Tensor] = None  # the curve group: float32 thresholds,
    hist: Optional[Tensor] = None  # the lazy (C, T+1, 2) histogram,
    epoch_buf: Optional[Tensor] = None  # the device epoch E,
    rowstats: Optional[Tensor] = None  # (2, >=N*S) float32 [rowmax; rowinv] in row order (n, s)
    tile_flags: Optional[Tensor] = None  # and one uint8 per wave tile, zero between steps


class McSpatialStep(ctypes.Structure):
    """Mirror of ``McSpatialStep`` in csrc/mc_spatial.h, field for field.
    ``_load`` holds field names, order and size against the header."""

    _fields_ = [
        ("C", _LL), ("ignore_index", _LL), ("has_ignore", _LL),
        ("counts", _U64), ("records", _U64),
        ("tp", _U64), ("fp", _U64), ("tn", _U64), ("fn", _U64), ("confmat", _U64),
        ("correct", _U64), ("total", _U64), ("rowbad", _U64), ("sample_cap", _LL),
        ("T", _LL), ("thresholds", _U64), ("uniform", _LL), ("t0", _D), ("inv_step", _D),
        ("hist", _U64), ("epoch_buf", _U64), ("rowmax", _U64), ("rowinv", _U64), ("row_cap", _LL),
        ("tile_flags", _U64), ("tile_cap", _LL),
    ]


_MC_SPATIAL_STEP_P = ctypes.POINTER(McSpatialStep)


def mc_spatial_step(num_classes: int, ignore_index: Optional[int], t: McSpatialStepTensors,
                    uniform: tuple = (0, 0.0, 1.0)) -> McSpatialStep:
    """The record of one spatial step over ``num_classes`` classes and the
    tensors ``t``, filled by name. The curve group is on iff ``t.thresholds`` is
    given; ``uniform`` = its :func:`_uniform_params`. It holds bare addresses:
    whoever keeps the record keeps ``t`` next to it."""
    rec = McSpatialStep(C=num_classes, ignore_index=ignore_index if ignore_index is not None else 0,
                        has_ignore=ignore_index is not None)
    for name, x in zip(t._fields, t):
        if x is not None and name != "rowstats":
            setattr(rec, name, x.data_ptr())
    if t.rowbad is not None:
        rec.sample_cap = t.rowbad.shape[0]
    if t.thresholds is not None:
        rec.T = t.thresholds.shape[0]
        rec.uniform, rec.t0, rec.inv_step = uniform
        rec.row_cap = t.rowstats.shape[1]
        rec.rowmax = t.rowstats.data_ptr()
        rec.rowinv = rec.rowmax + 4 * rec.row_cap
        rec.tile_cap = t.tile_flags.shape[0]
    return rec


_SIGNATURES = {
    "ma_mc_spatial_step": [_U64, _MC_SPATIAL_STEP_P, _U64, _I, _U64, _LL, _LL],
    "ma_mc_spatial_layout": [_LL, _LL, _LL, _I, _I, ctypes.POINTER(_LL)],
    "ma_mc_spatial_step_sizeof": [],
    "ma_mc_spatial_max_classes": [],
    "ma_mc_spatial_lds_bytes": [],
    "ma_mc_spatial_lds_static": [],
    "ma_bin_step": [_U64, _BIN_STEP_P, _U64, _I, _U64, _LL],
    "ma_bin_step_layout": [_LL, _I, _I, ctypes.POINTER(_LL)],
    "ma_bin_step_sizeof": [],
    "ma_ml_step": [_U64, _ML_STEP_P, _U64, _I, _U64, _LL],
    "ma_ml_step_layout": [_LL, _LL, _I, ctypes.POINTER(_LL)],
    "ma_ml_step_sizeof": [],
    "ma_ml_rank": [_U64, _U64, _I, _U64, _LL, _LL, _LL, _I, _I, _U64, _U64, _U64, _U64, _U64, _U64, _U64],
    "ma_ml_rank_layout": [_LL, _LL, ctypes.POINTER(_LL)],
    "ma_mc_stat_logits": [_U64, _STEP_P, _U64, _I, _U64, _LL, _U64],
    "ma_mc_stat_topk_covers": [_LL],
    "ma_mc_stat_labels": [_U64, _STEP_P, _U64, _U64, _LL],
    "ma_mc_stat_apply": [_U64, _STEP_P, _LL, _I],
    "ma_mc_step_dump": [_STEP_P, ctypes.POINTER(_U64)],
    "ma_mc_step_sizeof": [],
    "ma_bincount": [_U64, _U64, _LL, _LL, _U64],
    "ma_binary_stat": [_U64, _U64, _I, _U64, _LL, _F, _LL, _I, _U64, _U64],
    "ma_multilabel_stat": [_U64, _U64, _I, _U64, _LL, _LL, _F, _LL, _I, _U64, _U64],
    "ma_binary_curve_hist": [_U64, _U64, _I, _U64, _LL, _U64, _I, _LL, _I, _I, _F, _F, _I, _U64, _U64],
    "ma_multiclass_curve_hist": [_U64, _U64, _I, _U64, _LL, _LL, _U64, _I, _LL, _I, _I, _I, _F, _F, _I, _U64, _U64, _U64, _I, _I, _I, _U64],
    "ma_curve_suffix": [_U64, _U64, _LL, _I, _I, _I, _U64, _U64, _U64, _U64],
    "ma_curve_resolve_pending": [_U64, _U64, _LL, _I, _U64, _U64],
    "ma_curve_epoch_bump": [_U64, _U64],
    "ma_confmat_scalars": [_U64, _U64, _LL, _U64, ctypes.c_float, _U64],
    "ma_confmat_moments": [_U64, _U64, _LL, _U64],
    "ma_compute_plan_create": [_LL, _I, _U64, _U64, _U64, _U64, _U64, _U64, _U64, _U64, _U64, _U64, _U64, _U64, _I, _F, _LL, ctypes.POINTER(ctypes.c_ulonglong)],
    "ma_compute_plan_step": [_U64, _U64, _I, _U64, _U64, _U64, _U64],
    "ma_linear_stat_multi": [_U64, _U64, _U64, _U64, _U64, _LL, _I, _U64, _U64],
    "ma_mc_onepass_nv": [_I, _LL, _I],
    "ma_mc_onepass_lpr": [_I, _LL, _I],
    "ma_mc_onepass_scratch_words": [_LL],
    "ma_onepass_plan_create": [_STEP_P, _I, _U64, _I, _I, _F, _F, _U64, _U64, ctypes.POINTER(ctypes.c_ulonglong)],
    "ma_onepass_plan_step": [_U64, _U64, _U64, _U64, _LL],
    "ma_curve_auc_from_confmat": [_U64, _U64, _I, _LL, _I, _U64, _U64],
    "ma_err_reduce": [_U64, _U64, _U64, _I, _LL, _I, _D, _U64, _I, _I, _U64],
    "ma_box_iou": [_U64, _U64, _LL, _U64, _LL, _I, _U64],
    "ma_clf_curve_scratch_bytes": [_LL, _I, ctypes.POINTER(ctypes.c_ulonglong)],
    "ma_binary_clf_curve": [_U64, _U64, _U64, _U64, _LL, _LL, _U64, ctypes.c_ulonglong, _U64, _U64, _U64, _U64],
    "ma_ssim2d_fused": [_U64, _U64, _U64, _I, _LL, _LL, _LL, _LL, _U64, _I, _U64, _I, _F, _F, _U64, _F, _F, _I, _I, _I, _U64, _U64],
    "ma_binary_erosion2d": [_U64, _U64, _LL, _LL, _LL, _LL, _U64, _I, _I, _I, _I, _I, _U64],
    "ma_calib_bins": [_U64, _U64, _U64, _LL, _U64, _I, _I, _F, _F, _U64],
    "ma_mc_clf_curve_scratch_bytes": [_LL, _LL, ctypes.POINTER(ctypes.c_ulonglong)],
    "ma_mc_clf_curve": [_U64, _U64, _U64, _LL, _LL, _I, _U64, ctypes.c_ulonglong, _U64, _U64, _U64, _U64],
    "ma_retrieval_sort_scratch_bytes": [_LL, ctypes.POINTER(ctypes.c_ulonglong)],
    "ma_retrieval_sort": [_U64, _U64, _U64, _LL, _U64, ctypes.c_ulonglong, _U64, _U64],
    "ma_mc_topk_stat": [_U64, _U64, _I, _U64, _LL, _LL, _I, _LL, _I, _U64, _U64, _U64, _U64],
}


def _declare_argtypes(lib: ctypes.CDLL) -> None:
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    lib.ma_onepass_plan_destroy.argtypes = [_U64]
    lib.ma_onepass_plan_destroy.restype = None
    lib.ma_compute_plan_destroy.argtypes = [_U64]
    lib.ma_compute_plan_destroy.restype = None
    lib.ma_mc_step_field_names.argtypes = []
    lib.ma_mc_step_field_names.restype = ctypes.c_char_p
    mirror = [name for name, _ in McStep._fields_]
    if mc_step_native_fields(lib) != mirror or lib.ma_mc_step_sizeof() != ctypes.sizeof(McStep):
        raise RuntimeError(
            f"McStep: the Python mirror {mirror} and csrc/mc_step.h {mc_step_native_fields(lib)} differ in"
            " field names, order or size; rebuild the library"
        )
    lib.ma_ml_step_field_names.argtypes = []
    lib.ma_ml_step_field_names.restype = ctypes.c_char_p
    mirror = [name for name, _ in MlStep._fields_]
    if ml_step_native_fields(lib) != mirror or lib.ma_ml_step_sizeof() != ctypes.sizeof(MlStep):
        raise RuntimeError(
            f"MlStep: the Python mirror {mirror} and csrc/ml_step.h {ml_step_native_fields(lib)} differ in"
            " field names, order or size; rebuild the library"
        )
    lib.ma_bin_step_field_names.argtypes = []
    lib.ma_bin_step_field_names.restype = ctypes.c_char_p
    mirror = [name for name, _ in BinStep._fields_]
    if bin_step_native_fields(lib) != mirror or lib.ma_bin_step_sizeof() != ctypes.sizeof(BinStep):
        raise RuntimeError(
            f"BinStep: the Python mirror {mirror} and csrc/bin_step.h {bin_step_native_fields(lib)} differ in"
            " field names, order or size; rebuild the library"
        )
    lib.ma_mc_spatial_step_field_names.argtypes = []
    lib.ma_mc_spatial_step_field_names.restype = ctypes.c_char_p
    mirror = [name for name, _ in McSpatialStep._fields_]
    if mc_spatial_step_native_fields(lib) != mirror or lib.ma_mc_spatial_step_sizeof() != ctypes.sizeof(McSpatialStep):
        raise RuntimeError(
            f"McSpatialStep: the Python mirror {mirror} and csrc/mc_spatial.h {mc_spatial_step_native_fields(lib)}"
            " differ in field names, order or size; rebuild the library"
        )
    native = (lib.ma_mc_spatial_max_classes(), lib.ma_mc_spatial_lds_bytes(), lib.ma_mc_spatial_lds_static())
    if native != (MC_SPATIAL_MAX_C, MC_SPATIAL_LDS_BYTES, MC_SPATIAL_LDS_STATIC):
        raise RuntimeError(
            f"csrc/mc_spatial.hip: class cap and LDS gate {native} differ from the Python constants; rebuild the library"
        )


def mc_spatial_step_native_fields(lib: ctypes.CDLL) -> list:
    """The field names of the native ``McSpatialStep`` in declaration order."""
    return lib.ma_mc_spatial_step_field_names().decode().rstrip(",").split(",")


def bin_step_native_fields(lib: ctypes.CDLL) -> list:
    """The field names of the native ``BinStep`` in declaration order."""
    return lib.ma_bin_step_field_names().decode().rstrip(",").split(",")


def mc_step_native_fields(lib: ctypes.CDLL) -> list:
    """The field names of the native ``McStep`` in declaration order."""
    return lib.ma_mc_step_field_names().decode().rstrip(",").split(",")


def ml_step_native_fields(lib: ctypes.CDLL) -> list:
    """The field names of the native ``MlStep`` in declaration order."""
    return lib.ma_ml_step_field_names().decode().rstrip(",").split(",")


def hip_available() -> bool:
    """True if the kernel library is built and loadable."""
    return _load() is not None


def _lib() -> ctypes.CDLL:
    lib = _load()
    if lib is None:
        raise RuntimeError(
            f"metrics_amd HIP extension required for GPU tensors but unavailable: {_LOAD_ERR}"
        )
    return lib


try:
    # raw-stream fast path (same API torch.compile generated code uses):
    # torch.cuda.current_stream() builds a Stream object + device-index
    # lookups per call (~9us measured) — pure dispatch overhead at our call
    # rates (every kernel launch goes through _stream()).
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover - older torch
    _raw_stream = None


def _stream() -> int:
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _check(rc: int, name: str) -> None:
    if rc != 0:
        raise RuntimeError(f"HIP kernel {name} failed with error code {rc}")


def _dtype_code(t: Tensor) -> int:
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise TypeError(f"HIP metric kernels support float32/bfloat16 inputs, got {t.dtype}")


def _to_supported(t: Tensor) -> Tensor:
    """Kernels read fp32/bf16; cast anything else (fp16 under AMP, fp64) to fp32."""
    if t.is_floating_point() and t.dtype not in (torch.float32, torch.bfloat16):
        return t.float()
    return t


def mc_step_count(rec: McStep, preds: Tensor, target: Tensor, argmax: Optional[Tensor] = None) -> int:
    """The count launch every multiclass update shares: ``ma_mc_stat_logits``
    for (B, C) float ``preds`` (fused row-argmax, plus row statistics and the
    top-k slot where ``rec`` has them), ``ma_mc_stat_labels`` for integer label
    ``preds``. Counts land in the count block(s) of ``rec``, whose owner keeps
    them alive. Returns B, the number of samples."""
    lib = _lib()
    if preds.ndim == 2 and preds.is_floating_point():
        preds = _to_supported(preds).contiguous()
        target = target.contiguous().long()
        B = preds.shape[0]
        assert preds.shape[1] == rec.C, "preds must be (B, num_classes)"
        rc = lib.ma_mc_stat_logits(
            _stream(), rec, preds.data_ptr(), _dtype_code(preds), target.data_ptr(), B,
            argmax.data_ptr() if argmax is not None else 0,
        )
        _check(rc, "ma_mc_stat_logits")
    else:
        preds = preds.contiguous().long().flatten()
        target = target.contiguous().long().flatten()
        B = preds.numel()
        rc = lib.ma_mc_stat_labels(_stream(), rec, preds.data_ptr(), target.data_ptr(), B)
        _check(rc, "ma_mc_stat_labels")
    return B


def mc_step_apply(rec: McStep, B: int, close_epoch: bool = False) -> None:
    """The apply launch (``ma_mc_stat_apply``, one block): the count block(s)
    of ``rec`` are added to its stat states and zeroed, the exact-match states
    get their share of the ``B`` rows, and ``close_epoch`` closes the curve
    leader's device epoch in the same launch."""
    rc = _lib().ma_mc_stat_apply(_stream(), rec, B, 1 if close_epoch else 0)
    _check(rc, "ma_mc_stat_apply")


def _fresh_mc_stat(preds, target, C, ignore_index, want_confmat, argmax: Optional[Tensor] = None):
    """:func:`mc_step_count` into one freshly zeroed count block; tp, fp, fn
    and valid are views of it."""
    dev = preds.device
    t = McStepTensors(
        counts=torch.zeros(3 * C + 1, dtype=torch.long, device=dev),
        confmat=torch.zeros(C, C, dtype=torch.long, device=dev) if want_confmat else None,
    )
    mc_step_count(mc_step(C, ignore_index, t), preds, target, argmax)
    tp, fp, fn, valid = t.counts.split((C, C, C, 1))
    return tp, fp, fn, valid, t.confmat


def mc_stat_logits(
    preds: Tensor, target: Tensor, ignore_index: Optional[int], want_confmat: bool,
    want_argmax: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor], Optional[Tensor]]:
    """Fused row-argmax + per-class tp/fp/fn (+confmat) over (B, C) logits.

    Returns (tp, fp, fn, valid_count, confmat|None, argmax|None), all int64 on device.
    """
    assert preds.ndim == 2 and target.ndim == 1 and preds.shape[0] == target.shape[0]
    assert preds.is_floating_point(), "integer preds are labels: use mc_stat_labels"
    B, C = preds.shape
    argmax = torch.empty(B, dtype=torch.long, device=preds.device) if want_argmax else None
    return (*_fresh_mc_stat(preds, target, C, ignore_index, want_confmat, argmax), argmax)


def mc_stat_labels(
    preds: Tensor, target: Tensor, num_classes: int, ignore_index: Optional[int], want_confmat: bool
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor]]:
    """Per-class tp/fp/fn (+confmat) from integer label predictions."""
    return _fresh_mc_stat(preds.long().flatten(), target, num_classes, ignore_index, want_confmat)


def bincount(x: Tensor, minlength: int) -> Tensor:
    """Deterministic LDS-privatized histogram of a non-negative int64 tensor."""
    lib = _lib()
    x = x.contiguous().long().flatten()
    out = torch.zeros(minlength, dtype=torch.long, device=x.device)
    rc = lib.ma_bincount(
        _stream(),
        x.data_ptr(),
        x.numel(),
        minlength,
        out.data_ptr(),
    )
    _check(rc, "ma_bincount")
    return out


def binary_stat(
    preds: Tensor, target: Tensor, threshold: float, ignore_index: Optional[int]
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Fused binary tp/fp/tn/fn in one pass; picks raw vs sigmoid thresholding on-device."""
    lib = _lib()
    preds = _to_supported(preds).contiguous()
    target = target.contiguous().long()
    N = preds.numel()
    dev = preds.device
    out = torch.zeros(2, 4, dtype=torch.long, device=dev)  # {raw,sig} x {tp,fp,tn,fn}
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    # no clamp: at thr=0/1 the kernel's logit(thr) is -inf/+inf, which makes the
    # sigmoid branch always/never positive — exactly the reference comparison
    thr = float(threshold)
    rc = lib.ma_binary_stat(
        _stream(),
        preds.data_ptr(),
        _dtype_code(preds),
        target.data_ptr(),
        N,
        thr,
        ignore_index if ignore_index is not None else 0,
        1 if ignore_index is not None else 0,
        out.data_ptr(),
        flag.data_ptr(),
    )
    _check(rc, "ma_binary_stat")
    sel = flag.long().squeeze(0)  # 0 -> raw counts, 1 -> sigmoid counts (no host sync)
    counts = out[0] * (1 - sel) + out[1] * sel
    return counts[0], counts[1], counts[2], counts[3]


def multilabel_stat(
    preds: Tensor, target: Tensor, threshold: float, ignore_index: Optional[int]
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Fused per-label tp/fp/tn/fn over (N, L)."""
    lib = _lib()
    assert preds.ndim == 2
    preds = _to_supported(preds).contiguous()
    target = target.contiguous().long()
    N, L = preds.shape
    dev = preds.device
    out = torch.zeros(2, L, 4, dtype=torch.long, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    thr = float(threshold)
    rc = lib.ma_multilabel_stat(
        _stream(),
        preds.data_ptr(),
        _dtype_code(preds),
        target.data_ptr(),
        N,
        L,
        thr,
        ignore_index if ignore_index is not None else 0,
        1 if ignore_index is not None else 0,
        out.data_ptr(),
        flag.data_ptr(),
    )
    _check(rc, "ma_multilabel_stat")
    sel = flag.long().squeeze(0)
    counts = out[0] * (1 - sel) + out[1] * sel  # (L, 4)
    return counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3]


_UNIFORM_CACHE: dict = {}

# Per-device DEVICE-side epoch buffer E (2 x uint32): E[1] counts completed
# curve updates (bumped by the suffix kernel), E[0] records the epoch whose
# inputs were out-of-range. "Normalize this update" <=> E[0] == E[1]+1. All
# state lives on device, so the whole protocol is hipGraph-capturable.
# Stream-safety: launches go to the caller's current stream; each
# (detect -> histogram -> suffix) triple is issued back-to-back on one stream.
_FLAG_BUFS: dict = {}
_HIST_POOL: dict = {}
_ROWSTATS_POOL: dict = {}
# -1 auto, 0 wave-aggregated global atomics, 1 LDS-privatized (A/B probe knob)
_CURVE_VARIANT = int(os.environ.get("METRICS_AMD_CURVE_VARIANT", "-1"))
_CURVE_CCHUNK = int(os.environ.get("METRICS_AMD_CURVE_CCHUNK", "0"))

# Largest threshold count the curve kernels serve. The binding limit is
# k_curve_suffix (the only suffix kernel left once the tiled one no longer
# fits): (T+1)*2 u64 of dynamic LDS plus its two static u64 totals against the
# 160 KiB of a gfx950 workgroup, i.e. 16*(T+1) + 16 <= 163840. The histogram
# kernels reach further (binary: 12*T + 8 bytes, T <= 13652; multiclass: 4*T
# bytes), so the suffix bound decides. Callers route larger T to the torch path.
CURVE_MAX_T = (160 * 1024 - 16) // 16 - 1  # 10238


def curve_kernels_cover(num_thresholds: int) -> bool:
    """True if the threshold-curve kernels can hold ``num_thresholds`` in LDS."""
    return int(num_thresholds) <= CURVE_MAX_T


def owner_buffer(owner, key: str, shape: tuple, dtype, device, zero: bool = True, grow: bool = False) -> Tensor:
    """This owner's buffer under ``owner.__dict__[key]`` (one dtype per key):
    allocated on first use (zeroed unless ``zero`` is False) and again when
    device or shape no longer fit. ``grow``: a buffer at least ``shape`` in
    every dimension fits (the row-statistics buffer only grows with the batch)."""
    buf = owner.__dict__.get(key)
    if buf is not None and buf.device == device:
        have = buf.shape
        if have == shape or (grow and len(have) == len(shape) and all(map(operator.ge, have, shape))):
            return buf
    buf = owner.__dict__[key] = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
    return buf


def mc_count_block(owner, num_classes: int, device, key: str = "_hip_scratch", valid: bool = True) -> Tensor:
    """The owner's zeroed count block [tp|fp|fn|valid] (without the valid slot:
    the top-k block) that the apply pass leaves zeroed again."""
    return owner_buffer(owner, key, (3 * num_classes + (1 if valid else 0),), torch.long, device)


def rows_by_class(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    """(N, C, ...) float predictions as (rows, C) and everything else flat,
    with the flat target: the layout the multiclass count kernels read."""
    if preds.ndim == target.ndim + 1 and preds.is_floating_point():
        C = preds.shape[1]
        preds = preds.reshape(preds.shape[0], C, -1).movedim(1, -1).reshape(-1, C)
    else:
        preds = preds.reshape(-1)
    return preds, target.reshape(-1)


def _rowstats_buf(owner, B: int, device) -> Tensor:
    """The owner's (2, >=B) float32 [rowmax; rowinv] buffer."""
    return owner_buffer(owner, "_hip_rowstats_buf", (2, B), torch.float32, device, zero=False, grow=True)


def _epoch_buf(device, owner=None) -> Tensor:
    """Device-epoch buffer E (2 x uint32). Owned per-METRIC when ``owner`` is
    given so independent metrics can update on parallel streams without racing
    on the protocol state; falls back to a per-device buffer otherwise."""
    if owner is not None:
        return owner_buffer(owner, "_hip_epoch_buf", (2,), torch.int32, device)
    key = device.index
    buf = _FLAG_BUFS.get(key)
    if buf is None:
        buf = torch.zeros(2, dtype=torch.int32, device=device)
        _FLAG_BUFS[key] = buf
    return buf


def _pooled_hist(outer: int, T: int, device, owner=None) -> Tensor:
    """Persistent histogram scratch, zeroed once; the suffix kernel re-zeroes
    it in-flight after consuming it (zero_hist=1), so reuse needs no fill.
    Owned per-METRIC when ``owner`` is given (parallel-stream safety)."""
    if owner is not None:
        return owner_buffer(owner, "_hip_hist_buf", (outer, T + 1, 2), torch.long, device)
    key = (outer, T, device.index)
    buf = _HIST_POOL.get(key)
    if buf is None:
        buf = torch.zeros(outer, T + 1, 2, dtype=torch.long, device=device)
        if len(_HIST_POOL) > 64:
            _HIST_POOL.clear()
        _HIST_POOL[key] = buf
    return buf


def _uniform_params(thr: Tensor):
    """Detect uniform threshold spacing for the O(1) bucket guess.

    The kernel's +-1 fixup keeps results exact even if the guess is off.
    Result is cached per (data_ptr, numel): thresholds are fixed per metric,
    and the detection needs device->host syncs we don't want per update.
    """
    key = (thr.data_ptr(), thr.numel(), thr.device.index)
    hit = _UNIFORM_CACHE.get(key)
    if hit is not None:
        return hit
    T = thr.numel()
    if T < 2:
        out = (0, 0.0, 1.0)
    else:
        tc = thr.detach().float().cpu()
        t0, t_last = float(tc[0]), float(tc[-1])
        if t_last <= t0:
            out = (0, 0.0, 1.0)
        else:
            step = (t_last - t0) / (T - 1)
            diffs = tc[1:] - tc[:-1]
            # strictly uniform within small tolerance -> O(1) guess stays O(1)
            uniform = bool(((diffs - step).abs() <= 1e-3 * step + 1e-9).all())
            out = (1 if uniform else 0, t0, (T - 1) / (t_last - t0))
    if len(_UNIFORM_CACHE) > 256:
        _UNIFORM_CACHE.clear()
    _UNIFORM_CACHE[key] = out
    return out


def binary_curve_confmat(
    preds: Tensor, target: Tensor, thresholds: Tensor, ignore_index: Optional[int]
) -> Tensor:
    """(T,2,2) threshold confmat via bucketized histogram + on-device suffix-sum.

    ``preds`` must already be probabilities in [0,1].
    """
    lib = _lib()
    preds = _to_supported(preds).contiguous()
    target = target.contiguous().long()
    thr = thresholds.contiguous().float()
    T = thr.numel()
    dev = preds.device
    uni, t0, inv_step = _uniform_params(thr)
    hist = torch.zeros(T + 1, 2, dtype=torch.long, device=dev)
    rc = lib.ma_binary_curve_hist(
        _stream(),
        preds.data_ptr(),
        _dtype_code(preds),
        target.data_ptr(),
        preds.numel(),
        thr.data_ptr(),
        T,
        ignore_index if ignore_index is not None else 0,
        1 if ignore_index is not None else 0,
        uni,
        t0,
        inv_step,
        0,
        0,
        hist.data_ptr(),
    )
    _check(rc, "ma_binary_curve_hist")
    confmat = torch.zeros(T, 2, 2, dtype=torch.long, device=dev)
    rc = lib.ma_curve_suffix(
        _stream(),
        hist.data_ptr(),
        1,
        T,
        0,
        0,
        0,
        confmat.data_ptr(),
        0,
        0,
    )
    _check(rc, "ma_curve_suffix")
    return confmat


def multiclass_curve_confmat(
    probs: Tensor, target: Tensor, thresholds: Tensor, ignore_index: Optional[int], mode: int = 0
) -> Tensor:
    """(T,C,2,2) threshold confmats. mode 0: multiclass one-vs-rest (target (B,));
    mode 1: multilabel (target (B,C)). ``probs`` already normalized (B,C)."""
    lib = _lib()
    probs = _to_supported(probs).contiguous()
    target = target.contiguous().long()
    thr = thresholds.contiguous().float()
    B, C = probs.shape
    T = thr.numel()
    dev = probs.device
    uni, t0, inv_step = _uniform_params(thr)
    hist = torch.zeros(C, T + 1, 2, dtype=torch.long, device=dev)
    rc = lib.ma_multiclass_curve_hist(
        _stream(),
        probs.data_ptr(),
        _dtype_code(probs),
        target.data_ptr(),
        B,
        C,
        thr.data_ptr(),
        T,
        ignore_index if ignore_index is not None else 0,
        1 if ignore_index is not None else 0,
        mode,
        uni,
        t0,
        inv_step,
        0,
        0,
        0,
        0,
        _CURVE_VARIANT,
        _CURVE_CCHUNK,
        0,
        hist.data_ptr(),
    )
    _check(rc, "ma_multiclass_curve_hist")
    # write the (T, C, 2, 2) state layout directly (transposed suffix kernel)
    confmat = torch.zeros(T, C, 2, 2, dtype=torch.long, device=dev)
    rc = lib.ma_curve_suffix(
        _stream(),
        hist.data_ptr(),
        C,
        T,
        1,
        0,
        0,
        confmat.data_ptr(),
        0,
        0,
    )
    _check(rc, "ma_curve_suffix")
    return confmat


_CLF_SCRATCH_CACHE: dict = {}


def binary_clf_curve(
    preds: Tensor, target: Tensor, weights: Optional[Tensor] = None, pos_label: int = 1
) -> Tuple[Tensor, Tensor, Tensor]:
    """Exact (fps, tps, thresholds) at distinct descending scores.

    rocPRIM radix sort (stable, fp32 keys) + fp64 device scans + fused
    gather/flag and compaction kernels — the K2 path for thresholds=None
    ROC/PR/AUROC. One D2H sync for the data-dependent output length (the
    reference's torch path syncs there too).
    """
    lib = _lib()
    preds = _to_supported(preds)
    if preds.dtype != torch.float32:
        preds = preds.float()
    preds = preds.contiguous().flatten()
    target = target.contiguous().long().flatten()
    w = weights.contiguous().float().flatten() if weights is not None else None
    N = preds.numel()
    dev = preds.device
    key = (N, w is not None)
    nbytes = _CLF_SCRATCH_CACHE.get(key)
    if nbytes is None:
        out_b = ctypes.c_ulonglong(0)
        rc = lib.ma_clf_curve_scratch_bytes(N, 1 if w is not None else 0, ctypes.byref(out_b))
        _check(rc, "ma_clf_curve_scratch_bytes")
        nbytes = out_b.value
        if len(_CLF_SCRATCH_CACHE) > 256:
            _CLF_SCRATCH_CACHE.clear()
        _CLF_SCRATCH_CACHE[key] = nbytes
    scratch = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    out_fps = torch.empty(N, dtype=torch.float32, device=dev)
    out_tps = torch.empty(N, dtype=torch.float32, device=dev)
    out_thr = torch.empty(N, dtype=torch.float32, device=dev)
    out_cnt = torch.zeros(1, dtype=torch.long, device=dev)
    rc = lib.ma_binary_clf_curve(
        _stream(),
        preds.data_ptr(),
        target.data_ptr(),
        w.data_ptr() if w is not None else 0,
        N,
        pos_label,
        scratch.data_ptr(),
        nbytes,
        out_fps.data_ptr(),
        out_tps.data_ptr(),
        out_thr.data_ptr(),
        out_cnt.data_ptr(),
    )
    _check(rc, "ma_binary_clf_curve")
    k = int(out_cnt.item())
    return out_fps[:k], out_tps[:k], out_thr[:k]


_MC_CURVE_SCRATCH_CACHE: dict = {}


def mc_clf_curve(probs: Tensor, target: Tensor, multilabel: bool = False):
    """Per-class exact curves for ALL classes in one composite-key sort.

    ``probs`` (B, C); ``target`` (B,) class ids (multiclass) or (B, C) 0/1
    (multilabel). Returns a list of C ``(fps, tps, thresholds)`` tuples —
    one device sort + ONE host count transfer instead of C sorts + C syncs.
    """
    lib = _lib()
    probs = _to_supported(probs)
    if probs.dtype != torch.float32:
        probs = probs.float()
    probs = probs.contiguous()
    target = target.contiguous().long()
    B, C = probs.shape
    n = B * C
    dev = probs.device
    nbytes = _MC_CURVE_SCRATCH_CACHE.get((B, C))
    if nbytes is None:
        out_b = ctypes.c_ulonglong(0)
        rc = lib.ma_mc_clf_curve_scratch_bytes(B, C, ctypes.byref(out_b))
        _check(rc, "ma_mc_clf_curve_scratch_bytes")
        nbytes = out_b.value
        if len(_MC_CURVE_SCRATCH_CACHE) > 256:
            _MC_CURVE_SCRATCH_CACHE.clear()
        _MC_CURVE_SCRATCH_CACHE[(B, C)] = nbytes
    scratch = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    out_fps = torch.empty(n, dtype=torch.float32, device=dev)
    out_tps = torch.empty(n, dtype=torch.float32, device=dev)
    out_thr = torch.empty(n, dtype=torch.float32, device=dev)
    out_counts = torch.zeros(C, dtype=torch.long, device=dev)
    rc = lib.ma_mc_clf_curve(
        _stream(),
        probs.data_ptr(),
        target.data_ptr(),
        B,
        C,
        1 if multilabel else 0,
        scratch.data_ptr(),
        nbytes,
        out_fps.data_ptr(),
        out_tps.data_ptr(),
        out_thr.data_ptr(),
        out_counts.data_ptr(),
    )
    _check(rc, "ma_mc_clf_curve")
    # per-class positive counts ride the same single host transfer: the
    # callers' "no positive / no negative samples" branches then need no
    # further syncs (neg_c = B - pos_c)
    if multilabel:
        pos = target.sum(0)
    else:
        pos = torch.bincount(target.clamp(min=0), minlength=C)[:C]
    packed = torch.cat([out_counts, pos]).cpu()
    counts = packed[:C].tolist()
    pos_counts = packed[C:].tolist()
    res = []
    off = 0
    for c in range(C):
        k = counts[c]
        res.append(
            (out_fps[off : off + k], out_tps[off : off + k], out_thr[off : off + k],
             int(pos_counts[c]), B - int(pos_counts[c]))
        )
        off += k
    return res


_RETR_SCRATCH_CACHE: dict = {}


def retrieval_sort(indexes: Tensor, preds: Tensor) -> Tuple[Tensor, Tensor]:
    """(order, by_index) permutations for retrieval grouping in ONE radix pass.

    ``order`` sorts by (query index asc, pred desc); ``by_index`` by index
    only with original order preserved for ties. Composite 64-bit keys
    replace the torch double-argsort lexsort. Requires indexes < 2^31.
    """
    lib = _lib()
    indexes = indexes.contiguous().long()
    preds = _to_supported(preds).float().contiguous()
    n = preds.numel()
    dev = preds.device
    nbytes = _RETR_SCRATCH_CACHE.get(n)
    if nbytes is None:
        out_b = ctypes.c_ulonglong(0)
        rc = lib.ma_retrieval_sort_scratch_bytes(n, ctypes.byref(out_b))
        _check(rc, "ma_retrieval_sort_scratch_bytes")
        nbytes = out_b.value
        if len(_RETR_SCRATCH_CACHE) > 256:
            _RETR_SCRATCH_CACHE.clear()
        _RETR_SCRATCH_CACHE[n] = nbytes
    scratch = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    by_index = torch.empty(n, dtype=torch.int32, device=dev)
    rc = lib.ma_retrieval_sort(
        _stream(),
        indexes.data_ptr(),
        preds.data_ptr(),
        n,
        scratch.data_ptr(),
        nbytes,
        order.data_ptr(),
        by_index.data_ptr(),
    )
    _check(rc, "ma_retrieval_sort")
    return order.long(), by_index.long()


_ERR_OPS = {"sq_err": (0, 1), "abs_err": (1, 1), "ape": (2, 1), "sq_log_err": (3, 1), "moments": (4, 6), "logcosh": (5, 1)}


def err_reduce(x: Tensor, y: Tensor, op: str, eps: float = 1.17e-6) -> Tensor:
    """Deterministic fused elementwise-error reduction; returns fp64 sums (n_out,)."""
    lib = _lib()
    op_id, n_out = _ERR_OPS[op]
    if y.dtype != x.dtype or y.numel() != x.numel():  # the kernel reads both as x's type and length
        raise TypeError(f"err_reduce needs x and y of one dtype and size, got {x.dtype}[{x.numel()}] and {y.dtype}[{y.numel()}]")
    x = x.contiguous()
    y = y.contiguous()
    N = x.numel()
    num_blocks = min(max((N + 255) // 256, 1), 2048)
    dev = x.device
    partials = torch.zeros(num_blocks, n_out, dtype=torch.float64, device=dev)
    out = torch.zeros(n_out, dtype=torch.float64, device=dev)
    rc = lib.ma_err_reduce(
        _stream(),
        x.data_ptr(),
        y.data_ptr(),
        _dtype_code(x),
        N,
        op_id,
        eps,
        partials.data_ptr(),
        num_blocks,
        n_out,
        out.data_ptr(),
    )
    _check(rc, "ma_err_reduce")
    return out


_CALIB_SCALE = 8589934592.0  # 2^33, matches csrc/kernels2.hip


class CalibLdsOverflow(RuntimeError):
    """More bins than the LDS histogram holds (2048); caller falls back."""


def calib_bins(conf: Tensor, acc: Tensor, bounds: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Fused bucketize + per-bin (count, Σconf, Σacc) — K5 kernel.

    Integer fixed-point accumulation => deterministic. Returns fp32
    (acc_bin_sum, conf_bin_sum, count_bin) of length ``len(bounds)-1``.
    """
    lib = _lib()
    conf = _to_supported(conf).float().contiguous().flatten()
    acc = acc.float().contiguous().flatten()
    bounds = bounds.float().contiguous()
    n_bins = bounds.numel() - 1
    uni, b0, inv_step = _uniform_params(bounds)
    out = torch.zeros(3, n_bins, dtype=torch.long, device=conf.device)
    rc = lib.ma_calib_bins(
        _stream(),
        conf.data_ptr(),
        acc.data_ptr(),
        conf.numel(),
        bounds.data_ptr(),
        n_bins,
        uni,
        b0,
        inv_step,
        out.data_ptr(),
    )
    if rc == 9001:
        raise CalibLdsOverflow("calibration bin count exceeds the LDS budget")
    _check(rc, "ma_calib_bins")
    count = out[0].float()
    conf_sum = out[1].double().div_(_CALIB_SCALE).float()
    acc_sum = out[2].double().div_(_CALIB_SCALE).float()
    return acc_sum, conf_sum, count


def mc_topk_stat(
    preds: Tensor, target: Tensor, num_classes: int, k: int, ignore_index: Optional[int]
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Per-class (tp, fp, tn, fn) for top-k multiclass stat scores — K3 kernel.

    torchmetrics semantics: the effective prediction is the target when it
    ranks in the top-k, else the argmax (_refine_preds_oh).
    """
    lib = _lib()
    assert preds.ndim == 2 and preds.is_floating_point()
    preds = _to_supported(preds).contiguous()
    target = target.contiguous().long()
    B, C = preds.shape
    dev = preds.device
    tp = torch.zeros(C, dtype=torch.long, device=dev)
    fp = torch.zeros(C, dtype=torch.long, device=dev)
    fn = torch.zeros(C, dtype=torch.long, device=dev)
    valid = torch.zeros(1, dtype=torch.long, device=dev)
    rc = lib.ma_mc_topk_stat(
        _stream(),
        preds.data_ptr(),
        _dtype_code(preds),
        target.data_ptr(),
        B,
        C,
        k,
        ignore_index if ignore_index is not None else 0,
        1 if ignore_index is not None else 0,
        tp.data_ptr(),
        fp.data_ptr(),
        fn.data_ptr(),
        valid.data_ptr(),
    )
    _check(rc, "ma_mc_topk_stat")
    tn = valid - (tp + fp + fn)
    return tp, fp, tn, fn


class SsimLdsOverflow(RuntimeError):
    """Window too large for the one-kernel LDS tiling, or more than 65535
    planes (the grid's z limit); caller falls back."""


def ssim2d_fused(
    preds: Tensor,
    target: Tensor,
    wh: Tensor,
    ww: Tensor,
    c1: float,
    c2: float,
    dr: Optional[Tensor],
    k1: float,
    k2: float,
    want_cs: bool,
    crop_h: int,
    crop_w: int,
) -> Tuple[Tensor, Optional[Tensor]]:
    """Fused 2D SSIM: per-image Σssim (and optional cropped Σcs) in ONE kernel.

    ``wh``/``ww`` are the separable window weight vectors (odd length);
    ``dr`` an optional 0-dim float32 device tensor holding data_range (c1/c2
    then computed in-kernel — no host sync for the data_range=None path).
    """
    lib = _lib()
    preds = _to_supported(preds).contiguous()
    target = target.to(preds.dtype).contiguous()
    B, C, H, W = preds.shape
    rh = (wh.numel() - 1) // 2
    rw = (ww.numel() - 1) // 2
    dev = preds.device
    wh = wh.contiguous().float()
    ww = ww.contiguous().float()
    sum_sim = torch.zeros(B, dtype=torch.float64, device=dev)
    sum_cs = torch.zeros(B, dtype=torch.float64, device=dev) if want_cs else None
    rc = lib.ma_ssim2d_fused(
        _stream(),
        preds.data_ptr(),
        target.data_ptr(),
        _dtype_code(preds),
        B, C, H, W,
        wh.data_ptr(), rh,
        ww.data_ptr(), rw,
        c1, c2,
        dr.data_ptr() if dr is not None else 0,
        k1, k2,
        1 if want_cs else 0,
        crop_h, crop_w,
        sum_sim.data_ptr(),
        sum_cs.data_ptr() if sum_cs is not None else 0,
    )
    if rc == 9001:
        raise SsimLdsOverflow(
            f"window radius ({rh},{rw}) exceeds the LDS tile budget, or {B * C} planes exceed the grid")
    _check(rc, "ma_ssim2d_fused")
    return sum_sim, sum_cs


def binary_erosion2d(img: Tensor, strel: Tensor, origin: Tuple[int, int], border_value: int) -> Tensor:
    """Windowed erosion of a (N,C,H,W) binary uint8 image; returns uint8."""
    lib = _lib()
    img = img.contiguous()
    assert img.dtype == torch.uint8 and img.ndim == 4
    N, C, H, W = img.shape
    strel = strel.contiguous().int()
    kh, kw = strel.shape
    out = torch.empty_like(img)
    rc = lib.ma_binary_erosion2d(
        _stream(),
        img.data_ptr(),
        N, C, H, W,
        strel.data_ptr(),
        kh, kw,
        origin[0], origin[1],
        int(border_value),
        out.data_ptr(),
    )
    _check(rc, "ma_binary_erosion2d")
    return out


def box_iou(boxes1: Tensor, boxes2: Tensor, variant: str = "iou") -> Tensor:
    """All-pairs (N,M) box IoU / GIoU / DIoU / CIoU on xyxy boxes."""
    lib = _lib()
    v = {"iou": 0, "giou": 1, "diou": 2, "ciou": 3}[variant]
    boxes1 = boxes1.contiguous().float()
    boxes2 = boxes2.contiguous().float()
    N, M = boxes1.shape[0], boxes2.shape[0]
    out = torch.empty(N, M, dtype=torch.float32, device=boxes1.device)
    if N == 0 or M == 0:
        return out
    rc = lib.ma_box_iou(
        _stream(),
        boxes1.data_ptr(),
        N,
        boxes2.data_ptr(),
        M,
        v,
        out.data_ptr(),
    )
    _check(rc, "ma_box_iou")
    return out


def curve_hist_into_confmat(
    probs: Tensor, target: Tensor, thresholds: Tensor, ignore_index: Optional[int],
    confmat_state: Tensor, mode: int, norm: Optional[str] = None, owner=None,
    stats_ready: bool = False, lazy: Optional[bool] = None,
    skip_epoch_bump: bool = False,
) -> None:
    """Bucketized histogram + transposed suffix-sum accumulated DIRECTLY into the
    metric's confmat state ((T,2,2) binary / (T,C,2,2) multiclass|multilabel) —
    no intermediate confmat materialization or host-side add.

    ``norm`` ("softmax" / "sigmoid" / None) moves the reference's
    normalize-iff-outside-[0,1] semantics INTO the kernels: a fused row-stats
    (or range-detect) pass sets a per-device epoch flag and the histogram
    kernel normalizes inline — replacing the 4-kernel torch chain
    (compare / any-reduce / softmax / where) and its 3 extra full-tensor
    round-trips through HBM. The histogram scratch is pooled and re-zeroed by
    the suffix kernel in-flight, so steady-state updates launch no fills.
    """
    lib = _lib()
    if owner is not None:
        flush_if_b0_pending(owner)  # the one-pass step wrote last: complete its histogram first
    thr = thresholds.contiguous().float()
    T = thr.numel()
    uni, t0, inv_step = _uniform_params(thr)
    dev = probs.device
    if confmat_state.ndim == 3:  # binary (T,2,2)
        preds = _to_supported(probs).contiguous().flatten()
        tgt = target.contiguous().long().flatten()
        hist = _pooled_hist(1, T, dev, owner)
        if norm == "sigmoid":
            norm_i, flag_ptr = 1, _epoch_buf(dev, owner).data_ptr()
        else:
            norm_i, flag_ptr = 0, 0
        rc = lib.ma_binary_curve_hist(
            _stream(),
            preds.data_ptr(),
            _dtype_code(preds),
            tgt.data_ptr(),
            preds.numel(),
            thr.data_ptr(),
            T,
            ignore_index if ignore_index is not None else 0,
            1 if ignore_index is not None else 0,
            uni,
            t0,
            inv_step,
            norm_i,
            flag_ptr,
            hist.data_ptr(),
        )
        _check(rc, "ma_binary_curve_hist")
        outer, transposed = 1, 0
    else:
        probs = _to_supported(probs).contiguous()
        tgt = target.contiguous().long()
        B, C = probs.shape
        hist = _pooled_hist(C, T, dev, owner)
        if norm == "softmax":
            if owner is not None:
                rbuf = _rowstats_buf(owner, B, dev)
            else:
                rkey = (B, dev.index)
                rbuf = _ROWSTATS_POOL.get(rkey)
                if rbuf is None:
                    rbuf = torch.empty(2, B, dtype=torch.float32, device=dev)
                    if len(_ROWSTATS_POOL) > 64:
                        _ROWSTATS_POOL.clear()
                    _ROWSTATS_POOL[rkey] = rbuf
            norm_i, flag_ptr = 1, _epoch_buf(dev, owner).data_ptr()
            rm_ptr, ri_ptr = rbuf[0].data_ptr(), rbuf[1].data_ptr()
        elif norm == "sigmoid":
            norm_i, flag_ptr, rm_ptr, ri_ptr = 2, _epoch_buf(dev, owner).data_ptr(), 0, 0
        else:
            norm_i, flag_ptr, rm_ptr, ri_ptr = 0, 0, 0, 0
        rc = lib.ma_multiclass_curve_hist(
            _stream(),
            probs.data_ptr(),
            _dtype_code(probs),
            tgt.data_ptr(),
            B,
            C,
            thr.data_ptr(),
            T,
            ignore_index if ignore_index is not None else 0,
            1 if ignore_index is not None else 0,
            mode,
            uni,
            t0,
            inv_step,
            norm_i,
            flag_ptr,
            rm_ptr,
            ri_ptr,
            _CURVE_VARIANT,
            _CURVE_CCHUNK,
            1 if stats_ready else 0,
            hist.data_ptr(),
        )
        _check(rc, "ma_multiclass_curve_hist")
        outer, transposed = C, 1
    assert confmat_state.is_contiguous()
    # Lazy mode (default for metric-owned updates): histograms accumulate
    # additively across updates in the per-owner buffer; the O(T*outer)
    # suffix/confmat materialization is DEFERRED to the first state read
    # (compute/sync/state_dict/forward — Metric._maybe_flush_lazy). The
    # per-update device epoch is closed by a 1-thread bump kernel instead of
    # the suffix kernel. Cuts a ~22us/step kernel at the bench shape.
    if lazy is None:
        lazy = owner is not None
    if lazy and owner is not None:
        if norm is not None and not skip_epoch_bump:
            rc = lib.ma_curve_epoch_bump(_stream(), _epoch_buf(dev, owner).data_ptr())
            _check(rc, "ma_curve_epoch_bump")
        owner.__dict__["_hip_lazy_meta"] = (outer, T, transposed)
        owner.__dict__["_lazy_dirty"] = True
        return
    rc = lib.ma_curve_suffix(
        _stream(),
        hist.data_ptr(),
        outer,
        T,
        transposed,
        1,  # re-zero the pooled hist in-flight
        _epoch_buf(dev, owner).data_ptr() if norm is not None else 0,
        confmat_state.data_ptr(),
        0,
        0,
    )
    _check(rc, "ma_curve_suffix")


import weakref as _weakref

# Tensors cannot key a WeakKeyDictionary (their __eq__ is elementwise), so
# these caches key on id(tensor) and evict via a weakref finalizer; entries
# double-check identity through the stored weakref to survive id reuse.
_CONFMAT_MUTATIONS: dict = {}
_CONFMAT_SCALARS_CACHE: dict = {}
_CONFMAT_SCRATCH: dict = {}


def _tensor_cache_get(cache: dict, t: Tensor):
    ent = cache.get(id(t))
    if ent is not None and ent[0]() is t:
        return ent[1]
    return None


def _tensor_cache_put(cache: dict, t: Tensor, value) -> None:
    key = id(t)

    def _evict(_ref, _key=key, _cache=cache):
        _cache.pop(_key, None)

    cache[key] = (_weakref.ref(t, _evict), value)


def _mark_kernel_mutated(t: Tensor) -> None:
    """Raw-pointer kernel writes bypass torch's _version counter; note them so
    version-keyed caches (confmat_scalars) invalidate correctly. Steady-state
    cost is one dict hit + in-place increment (this runs every update)."""
    ent = _CONFMAT_MUTATIONS.get(id(t))
    if ent is not None and ent[0]() is t:
        ent[1][0] += 1
        return
    _tensor_cache_put(_CONFMAT_MUTATIONS, t, [1])


def confmat_scalars(confmat: Tensor, zero_division: float = 0.0) -> Tensor:
    """Fused (C,C) confusion-matrix scalars: (mcc, unweighted kappa, macro
    jaccard) in two launches, cached per (tensor, version) so the metrics of a
    compute group (which alias one confmat state) pay for it once."""
    muts = _tensor_cache_get(_CONFMAT_MUTATIONS, confmat)
    ver = (confmat._version, muts[0] if muts is not None else 0)
    hit = _tensor_cache_get(_CONFMAT_SCALARS_CACHE, confmat)
    if hit is not None and hit[0] == ver and hit[2] == zero_division:
        return hit[1]
    lib = _lib()
    C = confmat.shape[0]
    dev = confmat.device
    key = (C, dev.index)
    scratch = _CONFMAT_SCRATCH.get(key)
    if scratch is None:
        scratch = torch.zeros(3 * C, dtype=torch.long, device=dev)
        if len(_CONFMAT_SCRATCH) > 16:
            _CONFMAT_SCRATCH.clear()
        _CONFMAT_SCRATCH[key] = scratch
    out = torch.empty(3, dtype=torch.float32, device=dev)
    cm = confmat if confmat.is_contiguous() else confmat.contiguous()
    rc = lib.ma_confmat_scalars(_stream(), cm.data_ptr(), C, scratch.data_ptr(),
                                float(zero_division), out.data_ptr())
    _check(rc, "ma_confmat_scalars")
    _tensor_cache_put(_CONFMAT_SCALARS_CACHE, confmat, (ver, out, zero_division))
    return out


def flush_curve_hist(owner) -> None:
    """Materialize an owner's lazily-accumulated curve histogram into its
    ``confmat`` state (suffix-sum; re-zeroes the histogram in-flight)."""
    meta = owner.__dict__.get("_hip_lazy_meta")
    buf = owner.__dict__.get("_hip_hist_buf")
    if meta is None or buf is None:
        return
    outer, T, transposed = meta
    confmat = owner.confmat
    assert confmat.is_contiguous() and confmat.device == buf.device
    pending = take_b0_pending(owner)
    rc = _lib().ma_curve_suffix(
        _stream(), buf.data_ptr(), outer, T, transposed, 1, 0, confmat.data_ptr(),
        pending[0].data_ptr() if pending else 0, pending[1].data_ptr() if pending else 0,
    )
    _check(rc, "ma_curve_suffix")


# "Pending b0" protocol of the one-pass step (csrc/mc_onepass.hip). Between two
# flushes the owner's lazy histogram may lack the elements of the bucket of 0.0;
# the head of ``_hip_onepass_scratch`` ([P: C][R: C]) says how many. The owner's
# ``_hip_b0_pending`` is True exactly while P or R may be nonzero, and then
# ``_lazy_dirty`` is True as well. Rules, all decided on the host outside any
# captured region:
#   - every flush passes the scratch to the native flush, which pays what is
#     owed in front of the suffix kernel and zeroes P and R (take_b0_pending);
#   - a one-pass step on an owner that is dirty but not pending flushes first;
#   - any other writer of the owner's histogram flushes first when the owner is
#     pending (flush_if_b0_pending);
#   - whatever zeroes the histogram zeroes the scratch and clears the flag
#     (Metric._discard_lazy, GraphedUpdate._reset_states_inplace);
#   - whatever replaces the scratch or the histogram flushes first.
def take_b0_pending(owner) -> Optional[tuple]:
    """(curve scratch, float32 thresholds) for the native flush if ``owner``'s
    histogram is in pending format, else None. Clears the flag: the caller
    flushes now, in the same native call that consumes the histogram."""
    own = owner.__dict__
    if not own.get("_hip_b0_pending"):
        return None
    own["_hip_b0_pending"] = False
    plan = own.get("_hip_onepass_plan")  # None in a copy of the owner
    src = owner.thresholds
    thr = plan.thr if plan is not None and plan.thr_src is src else src.contiguous().float()
    return own["_hip_onepass_scratch"], thr


def flush_if_b0_pending(owner) -> None:
    """Called by every writer of ``owner``'s histogram other than the one-pass
    step: a pending histogram is flushed before they add to it."""
    if owner.__dict__.get("_hip_b0_pending"):
        owner._maybe_flush_lazy()


def curve_resolve_pending(hist: Tensor, thresholds: Tensor, pending: Optional[Tensor]) -> None:
    """The resolve kernel alone: complete the (C, T+1, 2) int64 ``hist`` in
    place from ``pending`` = [P: C][R: C] (int64, zeroed by the kernel), for
    float32 ``thresholds``. ``pending`` None: nothing is launched."""
    C, T = hist.shape[0], hist.shape[1] - 1
    assert hist.is_contiguous() and hist.dtype == torch.long and thresholds.dtype == torch.float32
    assert thresholds.is_contiguous() and thresholds.numel() == T
    assert pending is None or (pending.is_contiguous() and pending.dtype == torch.long and pending.numel() >= 2 * C)
    rc = _lib().ma_curve_resolve_pending(
        _stream(), hist.data_ptr(), C, T, thresholds.data_ptr(), pending.data_ptr() if pending is not None else 0
    )
    _check(rc, "ma_curve_resolve_pending")


def onepass_scratch_layout(num_classes: int) -> dict:
    """Offsets in u64 words of the one-pass curve scratch, as the Python side
    reads it: ``P`` and ``R`` (``num_classes`` words each) lead, the per-block
    records (2 words for each of 1024 blocks) and flag bytes (1024) follow.
    ``words`` must equal ``ma_mc_onepass_scratch_words(num_classes)``."""
    C = int(num_classes)
    rec = 2 * C
    flags = rec + 2 * 1024
    return {"P": 0, "R": C, "records": rec, "flags": flags, "words": flags + 1024 // 8}


def mc_stat_into(
    preds: Tensor, target: Tensor, num_classes: int, ignore_index: Optional[int],
    scratch: Tensor, tp: Tensor, fp: Tensor, tn: Tensor, fn: Tensor,
) -> None:
    """Fused stat-scores update accumulated DIRECTLY into the metric states.

    ``scratch`` is the metric's count block (:func:`mc_count_block`); 2 launches
    total (count + single-block apply): the apply kernel consumes AND zeroes
    the whole block in one pass, so no fill kernel runs in steady state and
    no host-side epoch is needed (hipGraph-capturable).
    """
    rec = mc_step(num_classes, ignore_index, McStepTensors(counts=scratch, tp=tp, fp=fp, tn=tn, fn=fn))
    mc_step_apply(rec, mc_step_count(rec, preds, target))
    _mark_kernel_mutated(tp)


def mc_confmat_into(
    preds: Tensor, target: Tensor, num_classes: int, ignore_index: Optional[int],
    confmat_state: Tensor, dummy: Tensor,
) -> None:
    """Confusion-matrix update atomically accumulated DIRECTLY into the (C,C)
    state — no per-batch confmat materialization, fill, or host-side add.

    ``dummy`` is a per-metric (3*C+1,) int64 sink for the per-class counters
    the kernel also produces (never read, never zeroed: garbage accumulates
    harmlessly in int64).
    """
    assert confmat_state.is_contiguous()
    rec = mc_step(num_classes, ignore_index, McStepTensors(counts=dummy, confmat=confmat_state))
    mc_step_count(rec, preds, target)
    _mark_kernel_mutated(confmat_state)


def mc_exact_into(
    preds: Tensor, target: Tensor, num_classes: int, ignore_index: Optional[int],
    scratch: Tensor, correct: Tensor, total: Tensor,
) -> None:
    """Exact-match (== row argmax equals target) accumulated into correct/total.

    Reuses the fused stat kernel's per-class tp counts: correct = sum(tp),
    total = valid rows. Same self-zeroing count block protocol as
    :func:`mc_stat_into`; 2 launches, zero fills in steady state.
    """
    rec = mc_step(num_classes, ignore_index, McStepTensors(counts=scratch, correct=correct, total=total))
    mc_step_apply(rec, mc_step_count(rec, preds, target))


# Batched linear-stat plans: the stat metrics of a compute group share one
# (tp,fp,tn,fn) state; each generation the FIRST caller batch-evaluates every
# formula seen so far in ONE kernel and later callers hit the cache. Keyed by
# id(tp) with weakref eviction; generation = (tp._version, kernel mutations).
_LINEAR_PLANS: dict = {}


def linear_stat_compute(tp: Tensor, fp: Tensor, tn: Tensor, fn: Tensor, formula, average: str) -> Tensor:
    """One-launch linear-ratio stat reduction (precision/recall/accuracy/...).

    ``formula`` is the metric's :class:`~metrics_amd.utilities.compute.LinearFormula`:
    score_c = post(safe_div(num . stats_c, den . stats_c)), then micro / macro /
    weighted averaging exactly like ``_adjust_weights_safe_divide``. Returns a
    0-dim float32 tensor.
    Formulas over the same state tensor are batched per compute generation:
    one grid launch evaluates all of them (see ``k_linear_stat_multi``).
    """
    lib = _lib()
    C = tp.numel()
    key = formula.params(average)
    muts = _tensor_cache_get(_CONFMAT_MUTATIONS, tp)
    gen = (tp._version, muts[0] if muts is not None else 0)
    plan = _tensor_cache_get(_LINEAR_PLANS, tp)
    if plan is None:
        # formulas: key -> slot; params_dev rebuilt when the set grows
        plan = {"formulas": {}, "params_dev": None, "gen": None, "outs": None}
        _tensor_cache_put(_LINEAR_PLANS, tp, plan)
    slot = plan["formulas"].get(key)
    if slot is None:
        slot = len(plan["formulas"])
        plan["formulas"][key] = slot
        plan["params_dev"] = None  # set changed: re-upload next batch eval
        plan["gen"] = None
    if plan["gen"] == gen and plan["outs"] is not None:
        return plan["outs"][slot].reshape(())
    n = len(plan["formulas"])
    if plan["params_dev"] is None:
        flat = [0.0] * (13 * n)
        for k2, s2 in plan["formulas"].items():
            flat[13 * s2 : 13 * s2 + 13] = list(k2)
        plan["params_dev"] = torch.tensor(flat, dtype=torch.float32, device=tp.device)
    # fresh outs per generation: returned views must never be recycled
    outs = torch.empty(n, dtype=torch.float32, device=tp.device)
    rc = lib.ma_linear_stat_multi(
        _stream(), tp.data_ptr(), fp.data_ptr(), tn.data_ptr(), fn.data_ptr(),
        C, n, plan["params_dev"].data_ptr(), outs.data_ptr(),
    )
    _check(rc, "ma_linear_stat_multi")
    plan["gen"] = gen
    plan["outs"] = outs
    return outs[slot].reshape(())


def curve_auc_from_confmat(confmat_state: Tensor, mode: int) -> Tuple[Tensor, Tensor]:
    """Per-class AUROC (mode 0) / AveragePrecision (mode 1) + support weights
    straight from the (T, C, 2, 2) thresholded confmat state — one launch."""
    lib = _lib()
    assert confmat_state.ndim == 4 and confmat_state.is_contiguous()
    T, C = confmat_state.shape[0], confmat_state.shape[1]
    out = torch.empty(C, dtype=torch.float32, device=confmat_state.device)
    weights = torch.empty(C, dtype=torch.float32, device=confmat_state.device)
    rc = lib.ma_curve_auc_from_confmat(
        _stream(), confmat_state.data_ptr(), T, C, mode, out.data_ptr(), weights.data_ptr()
    )
    _check(rc, "ma_curve_auc_from_confmat")
    return out, weights


# Top-k slot of the fused collection step. METRICS_AMD_FUSE_TOPK=0 keeps every
# top-k stat leader out of the fused plan: it then updates on its own through
# mc_topk_stat, exactly as before (A/B lever and escape hatch). Read when a
# collection builds its fused plan.
FUSE_TOPK_ENV = "METRICS_AMD_FUSE_TOPK"
_TOPK_COVERS_CACHE: dict = {}


def fuse_topk_enabled() -> bool:
    return os.environ.get(FUSE_TOPK_ENV, "1") != "0"


def mc_stat_topk_covers(num_classes: int) -> bool:
    """Whether the streaming stat kernel has the top-k slot at this class count
    (the thread-per-row kernel for small C has none)."""
    hit = _TOPK_COVERS_CACHE.get(num_classes)
    if hit is None:
        hit = _TOPK_COVERS_CACHE[num_classes] = bool(_lib().ma_mc_stat_topk_covers(num_classes))
    return hit


def mc_step_mark_mutated(t: McStepTensors) -> None:
    """Note the raw-pointer writes of one step for the version-keyed caches."""
    if t.confmat is not None:
        _mark_kernel_mutated(t.confmat)
    if t.tp is not None:
        _mark_kernel_mutated(t.tp)  # generation key for the batched linear-stat plan
    if t.tp_k is not None:
        _mark_kernel_mutated(t.tp_k)  # the top-k group's own linear-stat plan


# One-pass fused-collection step (csrc/mc_onepass.hip). METRICS_AMD_ONEPASS:
#   0  off: the stat + curve-hist + apply kernel sequence, exactly as before
#      (A/B lever and escape hatch)
#   1  (default) on where the guard table in profiles/README.md shows a gain:
#      C >= 5*T. The saving rests on most softmax outputs falling below the
#      first positive threshold (~1/T on a linspace grid) while a row's mean
#      probability is 1/C; measured at T=200: C=1000 and 4096 win, C<=512 lose.
#   2  on for every shape the kernel covers (tests, sweeps)
# It is read when a collection builds its fused plan.
ONEPASS_ENV = "METRICS_AMD_ONEPASS"
_ONEPASS_C_PER_T = 5
_ONEPASS_NV_CACHE: dict = {}


def onepass_mode() -> int:
    v = os.environ.get(ONEPASS_ENV, "1")
    return int(v) if v in ("0", "1", "2") else 1


class _NativePlan:
    """A native plan handle with the tensor objects whose addresses the plan
    holds: kept next to it, so none of the addresses can be freed or reused
    under the plan, and ``is`` on each of them decides whether the plan still
    fits. Destroyed with this object; a copy or pickle of the owner gets None
    and builds its own."""

    __slots__ = ("handle", "tensors", "_destroy")

    def _adopt(self, handle: int, tensors: tuple, destroy) -> None:
        self.handle, self.tensors, self._destroy = handle, tensors, destroy

    def fits(self, tensors) -> bool:
        return all(map(operator.is_, self.tensors, tensors))

    def __del__(self):
        handle = getattr(self, "handle", 0)  # unset when the create call raised
        if handle:
            self._destroy(handle)
            self.handle = 0

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())


class _OnepassPlan(_NativePlan):
    """Native step plan of the one-pass update (``ma_onepass_plan_*``).
    ``tensors`` = (*step tensors, hist, curve scratch, the leader's thresholds),
    ``scalars`` = (dtype code, C, T, ignore_index, k), ``thr`` the float32
    thresholds the plan reads."""

    __slots__ = ("scalars", "thr_src", "thr")

    def __init__(self, lib, step: McStepTensors, hist: Tensor, cs: Tensor, thr_src: Tensor, scalars, thr: Tensor):
        dt, C, T, ignore_index, k = scalars
        uni, t0, inv_step = _uniform_params(thr)
        handle = ctypes.c_ulonglong(0)
        rc = lib.ma_onepass_plan_create(
            mc_step(C, ignore_index, step, k), dt,
            thr.data_ptr(), T, uni, t0, inv_step, hist.data_ptr(), cs.data_ptr(), ctypes.byref(handle),
        )
        _check(rc, "ma_onepass_plan_create")
        self._adopt(handle.value, (*step, hist, cs, thr_src), lib.ma_onepass_plan_destroy)
        self.scalars = scalars
        self.thr_src = thr_src
        self.thr = thr


def mc_onepass_update(
    preds: Tensor, target: Tensor, num_classes: int, ignore_index: Optional[int],
    step: McStepTensors, k: int, curve, force: bool = False,
) -> bool:
    """The whole fused-collection step (stat scores, confusion matrix, exact
    match, threshold-curve histogram) in ONE native call that reads the logits
    once: one-pass kernel + tail kernel (epilogue and deferred rows), two
    launches on the current stream. No allocation in steady state and no host sync, so it
    is hipGraph-capturable.

    Returns False without launching anything when the shape is not covered
    (C <= 128, C not a multiple of the vector width, row too long for the
    register layout, unaligned storage) or, unless ``force``, lies below the
    C >= 5*T gate: the caller keeps the two-kernel path.
    ``step`` holds the participants (stat states, row statistics and epoch
    buffer are required), ``k`` > 0 turns its top-k slot on (every shape the
    kernel covers has it), ``curve`` is the curve leader (owns the histogram
    and the curve scratch).
    """
    lib = _lib()
    C = num_classes
    plan = curve.__dict__.get("_hip_onepass_plan")
    thr_src = curve.thresholds
    if plan is not None and plan.thr_src is thr_src:
        thr = plan.thr
    else:
        thr = thr_src.contiguous().float()
    T = thr.numel()
    if not force and C < _ONEPASS_C_PER_T * T:
        return False
    preds = _to_supported(preds).contiguous()
    dt = _dtype_code(preds)
    key = (dt, C, T)
    hit = _ONEPASS_NV_CACHE.get(key)
    if hit is None:
        hit = _ONEPASS_NV_CACHE[key] = (lib.ma_mc_onepass_nv(dt, C, T), lib.ma_mc_onepass_scratch_words(C))
    nv, cs_words = hit
    if nv == 0 or preds.data_ptr() % 16:
        return False
    target = target.contiguous().long()
    dev = preds.device
    # The native plan holds the addresses of everything that stays the same
    # from step to step (_NativePlan); dtype, C, T, ignore_index and k decide
    # with them whether it still fits. reset() and a move to another device
    # replace the state tensors: the next step rebuilds the plan. Until then
    # one stale set of states stays alive.
    own = curve.__dict__
    if not own.get("_hip_b0_pending") and own.get("_lazy_dirty"):
        # another writer filled the histogram since the last flush: its rows are
        # not in P and R, so they are flushed before this step arms the format
        curve._maybe_flush_lazy()
    tensors = (*step, own.get("_hip_hist_buf"), own.get("_hip_onepass_scratch"), thr_src)
    scalars = (dt, C, T, ignore_index, k)
    if plan is None or plan.scalars != scalars or not plan.fits(tensors):
        # histogram or scratch may be replaced below: nothing may be owed then
        flush_if_b0_pending(curve)
        # [P | R | per-block records | per-block flags]; P and R are zeroed by
        # the flush, records and flags are overwritten every step
        cs = owner_buffer(curve, "_hip_onepass_scratch", (cs_words,), torch.long, dev)
        hist = _pooled_hist(C, T, dev, curve)
        assert curve.confmat.is_contiguous()
        plan = own["_hip_onepass_plan"] = _OnepassPlan(lib, step, hist, cs, thr_src, scalars, thr)
    rc = lib.ma_onepass_plan_step(plan.handle, _stream(), preds.data_ptr(), target.data_ptr(), preds.shape[0])
    _check(rc, "ma_onepass_plan_step")
    mc_step_mark_mutated(step)
    # same lazy protocol as curve_hist_into_confmat: the histogram accumulates,
    # the suffix/confmat materialization waits for the first state read
    own["_hip_lazy_meta"] = (C, T, 1)
    own["_lazy_dirty"] = True
    own["_hip_b0_pending"] = True  # the histogram now lacks bucket b0 of the rows binned from registers
    return True


# Fused multilabel step (csrc/ml_step.hip). METRICS_AMD_FUSE_MULTILABEL=0 keeps
# every leader of a multilabel collection on its own update path, exactly as
# before (A/B lever, escape hatch and the oracle of the tests). Read when a
# collection builds its plan.
FUSE_MULTILABEL_ENV = "METRICS_AMD_FUSE_MULTILABEL"

# Largest threshold count with which the curve leader rides the fused step: the
# step kernel keeps a private histogram of one label chunk in LDS,
# [CW][T+1][2] u32 plus the T float thresholds, next to 2048 bytes of static
# LDS (block counters), against the 160 KiB of a gfx950 workgroup. The
# narrowest chunk is CW = 16 labels: 16*(T+1)*8 + 4*T + 2048 <= 163840, i.e.
# 132*T <= 161664 (ML_LDS_BYTES / ML_LDS_STATIC in csrc/ml_step.hip). Above it
# the curve leader updates on its own and the other leaders still fuse.
ML_STEP_MAX_T = (160 * 1024 - 2048 - 128) // 132  # 1224

_ML_LAYOUT_CACHE: dict = {}


class _MlStepRecord:
    """A step record with the tensor objects whose addresses it holds, kept in
    the ``__dict__`` of a leader. A copy or pickle of the leader gets None and
    builds its own, as with :class:`_NativePlan`."""

    __slots__ = ("tensors", "scalars", "rec")

    def __init__(self, tensors, scalars, rec):
        self.tensors, self.scalars, self.rec = tensors, scalars, rec

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())


def fuse_multilabel_enabled() -> bool:
    return os.environ.get(FUSE_MULTILABEL_ENV, "1") != "0"


def ml_step_layout(num_labels: int, rows: int, num_thresholds: int) -> Optional[tuple]:
    """(region flag bytes, record bytes, chunk width, rows per region, step
    blocks, tail blocks) of a fused multilabel step, None where the kernels do
    not cover the shape. ``num_thresholds`` 0: no curve leader. Host only."""
    key = (num_labels, rows, num_thresholds)
    if key not in _ML_LAYOUT_CACHE:
        out = (_LL * 6)()
        rc = _lib().ma_ml_step_layout(num_labels, rows, num_thresholds, out)
        if len(_ML_LAYOUT_CACHE) > 256:
            _ML_LAYOUT_CACHE.clear()
        _ML_LAYOUT_CACHE[key] = tuple(out) if rc == 0 else None
    return _ML_LAYOUT_CACHE[key]


def ml_step_update(
    preds: Tensor, target: Tensor, num_labels: int, ignore_index: Optional[int], threshold: float,
    stat=None, confmat=None, exact=None, curve=None,
) -> bool:
    """The whole step of a fused multilabel collection in ONE native call of two
    launches that reads the (N, L) fp32 / bf16 ``preds`` and the int64
    ``target`` once: per-label stat counts into the ``stat`` leader's
    tp/fp/tn/fn, [[tn, fp], [fn, tp]] into the ``confmat`` leader's state, the
    exact-match counts into the ``exact`` leader's correct/total, and the
    threshold-curve histogram into the ``curve`` leader's lazy buffer (absent
    leaders are None). Every buffer lives in the ``__dict__`` of the leader it
    serves (:func:`owner_buffer`); no allocation, fill or host sync in steady
    state. Both inputs must be contiguous.

    Returns False without launching anything where the kernels do not cover
    the shape: the caller lets every leader update on its own.
    """
    lib = _lib()
    dt = _dtype_code(preds)
    N, L = preds.shape
    dev = preds.device
    base = stat if stat is not None else confmat if confmat is not None else exact if exact is not None else curve
    thr, T = None, 0
    if curve is not None:
        src = curve.thresholds
        hit = curve.__dict__.get("_hip_ml_thr")
        if hit is not None and hit[0] is src:
            thr = hit[1]
        else:
            thr = src.contiguous().float()
            curve.__dict__["_hip_ml_thr"] = (src, thr)
        T = thr.numel()
    lay = ml_step_layout(L, N, T)
    if lay is None:
        return False
    tensors = MlStepTensors(
        counts=owner_buffer(base, "_hip_ml_counts", (6 * L,), torch.long, dev),
        records=owner_buffer(base, "_hip_ml_records", (lay[1],), torch.uint8, dev),
        tp=stat.tp if stat is not None else None,
        fp=stat.fp if stat is not None else None,
        tn=stat.tn if stat is not None else None,
        fn=stat.fn if stat is not None else None,
        confmat=confmat.confmat if confmat is not None else None,
        correct=exact.correct if exact is not None else None,
        total=exact.total if exact is not None else None,
        rowbad=owner_buffer(exact, "_hip_ml_rowbad", (max(N, 1),), torch.int32, dev, grow=True)
        if exact is not None else None,
    )
    if curve is not None:
        tensors = tensors._replace(
            thresholds=thr,
            hist=_pooled_hist(L, T, dev, curve),
            epoch_buf=_epoch_buf(dev, curve),
            region_flags=owner_buffer(curve, "_hip_ml_region_flags", (max(lay[0], 1),), torch.uint8, dev, grow=True),
        )
    # the record holds the addresses of everything that stays the same from
    # step to step; reset() and a move to another device replace state tensors
    # and the next step rebuilds it (the identity rule of _NativePlan.fits)
    scalars = (L, ignore_index, float(threshold), T)
    kept = base.__dict__.get("_hip_ml_rec")
    if kept is not None and kept.scalars == scalars and all(map(operator.is_, kept.tensors, tensors)):
        rec = kept.rec
    else:
        for name in ("tp", "fp", "tn", "fn", "confmat", "correct", "total"):
            x = getattr(tensors, name)
            if x is not None and not (x.is_contiguous() and x.dtype == torch.long and x.device == dev):
                return False
        rec = ml_step(L, ignore_index, threshold, tensors, _uniform_params(thr) if curve is not None else (0, 0.0, 1.0))
        base.__dict__["_hip_ml_rec"] = _MlStepRecord(tensors, scalars, rec)
    rc = lib.ma_ml_step(_stream(), rec, preds.data_ptr(), dt, target.data_ptr(), N)
    if rc == -103:
        return False  # nothing was launched
    _check(rc, "ma_ml_step")
    for name in ("tp", "fp", "tn", "fn", "confmat", "correct", "total"):
        x = getattr(tensors, name)
        if x is not None:
            _mark_kernel_mutated(x)
    if curve is not None:
        # same lazy protocol as curve_hist_into_confmat: the histogram
        # accumulates, the suffix/confmat materialization waits for a state read
        curve.__dict__["_hip_lazy_meta"] = (L, T, 1)
        curve.__dict__["_lazy_dirty"] = True
    return True


# Fused binary step (csrc/bin_step.hip). METRICS_AMD_FUSE_BINARY=0 keeps every
# leader of a binary collection on its own update path, exactly as before (A/B
# lever, escape hatch and the oracle of the tests). Read when a collection
# builds its plan.
FUSE_BINARY_ENV = "METRICS_AMD_FUSE_BINARY"

# Largest threshold count with which the curve leader rides the fused step: the
# step kernel keeps the histogram twice in LDS (raw and sigmoid),
# [2][T+1][2] u32 plus the T float thresholds, next to 256 bytes of static LDS
# (block counters), against the 160 KiB of a gfx950 workgroup:
# 16*(T+1) + 4*T + 256 <= 163840, i.e. 20*T <= 163568 (BIN_LDS_BYTES /
# BIN_LDS_STATIC in csrc/bin_step.hip). Above it the curve leader updates on
# its own and the other leaders still fuse.
BIN_STEP_MAX_T = (160 * 1024 - 256 - 16) // 20  # 8178

_BIN_LAYOUT_CACHE: dict = {}


def fuse_binary_enabled() -> bool:
    return os.environ.get(FUSE_BINARY_ENV, "1") != "0"


def bin_step_layout(numel: int, dtype_code: int, num_thresholds: int) -> Optional[tuple]:
    """(record bytes, elements per unit, elements per vector, step blocks, tail
    blocks, dynamic LDS bytes, histogram copies per block) of a fused binary
    step over ``numel`` elements of fp32 (``dtype_code`` 0) or bf16 (1) at a
    16-byte aligned address, None where the kernels do not cover the shape.
    ``num_thresholds`` 0: no curve leader. Host only."""
    key = (numel, dtype_code, num_thresholds)
    if key not in _BIN_LAYOUT_CACHE:
        out = (_LL * 7)()
        rc = _lib().ma_bin_step_layout(numel, dtype_code, num_thresholds, out)
        if len(_BIN_LAYOUT_CACHE) > 256:
            _BIN_LAYOUT_CACHE.clear()
        _BIN_LAYOUT_CACHE[key] = tuple(out) if rc == 0 else None
    return _BIN_LAYOUT_CACHE[key]


def bin_step_update(
    preds: Tensor, target: Tensor, ignore_index: Optional[int], threshold: float,
    stat=None, confmat=None, curve=None,
) -> bool:
    """The whole step of a fused binary collection in ONE native call of two
    launches that reads the fp32 / bf16 ``preds`` (any shape, read as a flat
    stream) and the int64 ``target`` once: the stat counts into the ``stat``
    leader's tp/fp/tn/fn, [[tn, fp], [fn, tp]] into the ``confmat`` leader's
    state, and the threshold-curve histogram into the ``curve`` leader's lazy
    buffer (absent leaders are None). Every buffer lives in the ``__dict__`` of
    the leader it serves (:func:`owner_buffer`); no allocation, fill or host
    sync in steady state. Both inputs must be contiguous.

    Returns False without launching anything where the kernels do not cover
    the shape: the caller lets every leader update on its own.
    """
    lib = _lib()
    dt = _dtype_code(preds)
    N = preds.numel()
    dev = preds.device
    base = stat if stat is not None else confmat if confmat is not None else curve
    thr, T = None, 0
    if curve is not None:
        src = curve.thresholds
        hit = curve.__dict__.get("_hip_bin_thr")
        if hit is not None and hit[0] is src:
            thr = hit[1]
        else:
            thr = src.contiguous().float()
            curve.__dict__["_hip_bin_thr"] = (src, thr)
        T = thr.numel()
    lay = bin_step_layout(N, dt, T)
    if lay is None:
        return False
    if curve is not None:
        flush_if_b0_pending(curve)  # never pending for a binary leader; the rule of every histogram writer
    tensors = BinStepTensors(
        counts=owner_buffer(base, "_hip_bin_counts", (6,), torch.long, dev),
        records=owner_buffer(base, "_hip_bin_records", (lay[0],), torch.uint8, dev),
        tp=stat.tp if stat is not None else None,
        fp=stat.fp if stat is not None else None,
        tn=stat.tn if stat is not None else None,
        fn=stat.fn if stat is not None else None,
        confmat=confmat.confmat if confmat is not None else None,
    )
    if curve is not None:
        tensors = tensors._replace(
            thresholds=thr,
            hist=_pooled_hist(1, T, dev, curve),
            curve_scratch=owner_buffer(curve, "_hip_bin_curve_scratch", (2, T + 1, 2), torch.long, dev),
            epoch_buf=_epoch_buf(dev, curve),
        )
    # the record holds the addresses of everything that stays the same from
    # step to step; reset() and a move to another device replace state tensors
    # and the next step rebuilds it (the identity rule of _NativePlan.fits)
    scalars = (ignore_index, float(threshold), T)
    kept = base.__dict__.get("_hip_bin_rec")
    if kept is not None and kept.scalars == scalars and all(map(operator.is_, kept.tensors, tensors)):
        rec = kept.rec
    else:
        for name in ("tp", "fp", "tn", "fn", "confmat"):
            x = getattr(tensors, name)
            if x is not None and not (x.is_contiguous() and x.dtype == torch.long and x.device == dev):
                return False
        rec = bin_step(ignore_index, threshold, tensors, _uniform_params(thr) if curve is not None else (0, 0.0, 1.0))
        base.__dict__["_hip_bin_rec"] = _MlStepRecord(tensors, scalars, rec)
    rc = lib.ma_bin_step(_stream(), rec, preds.data_ptr(), dt, target.data_ptr(), N)
    if rc == -103:
        return False  # nothing was launched
    _check(rc, "ma_bin_step")
    for name in ("tp", "fp", "tn", "fn", "confmat"):
        x = getattr(tensors, name)
        if x is not None:
            _mark_kernel_mutated(x)
    if curve is not None:
        # same lazy protocol as curve_hist_into_confmat for a binary owner: the
        # histogram accumulates, the suffix/confmat materialization waits for a
        # state read
        curve.__dict__["_hip_lazy_meta"] = (1, T, 0)
        curve.__dict__["_lazy_dirty"] = True
    return True


# Fused spatial multiclass step (csrc/mc_spatial.hip): (N, C, *spatial) float
# predictions with an (N, *spatial) target. METRICS_AMD_FUSE_SPATIAL=0 keeps
# every leader on its own update path, exactly as before (A/B lever, escape
# hatch and the oracle of the tests). Read when a collection builds its plan.
FUSE_SPATIAL_ENV = "METRICS_AMD_FUSE_SPATIAL"

# Class cap: the step kernel counts tp/fp/fn in an LDS block [3][C] u32.
MC_SPATIAL_MAX_C = 256
# Curve gate: the curve leader rides the step while the block's private
# histogram [C][T+1][2] u32, the count block and the static part (block record
# and reduction words, rounded up) fit the 160 KiB of a gfx950 workgroup:
# 8*C*(T+1) + 12*C + 128 <= 163840 (SP_LDS_BYTES / SP_LDS_STATIC in
# csrc/mc_spatial.hip), C <= 101 at T = 200. The T float thresholds join them
# in LDS while 4*T more bytes fit and are read from global memory otherwise;
# the (C, C) matrix joins while it still fits behind all of that. Above the
# gate the curve leader updates on its own and the other leaders still fuse.
MC_SPATIAL_LDS_BYTES = 160 * 1024
MC_SPATIAL_LDS_STATIC = 128

_MC_SPATIAL_LAYOUT_CACHE: dict = {}


def fuse_spatial_enabled() -> bool:
    return os.environ.get(FUSE_SPATIAL_ENV, "1") != "0"


def mc_spatial_curve_rides(num_classes: int, num_thresholds: int) -> bool:
    """The curve gate of the fused spatial step."""
    C, T = int(num_classes), int(num_thresholds)
    return 8 * C * (T + 1) + 12 * C + MC_SPATIAL_LDS_STATIC <= MC_SPATIAL_LDS_BYTES


def mc_spatial_max_curve_classes(num_thresholds: int) -> int:
    """The largest class count with which the curve leader rides at this
    threshold count (the class cap aside)."""
    return (MC_SPATIAL_LDS_BYTES - MC_SPATIAL_LDS_STATIC) // (8 * (int(num_thresholds) + 1) + 12)


def mc_spatial_layout(N: int, C: int, S: int, dtype_code: int, num_thresholds: int) -> Optional[tuple]:
    """(pixels per lane of the vector path, 1 if the shape takes it, pixels per
    wave tile, threads per block, step blocks, tail blocks, dynamic LDS bytes,
    1 if the (C, C) matrix is kept in LDS, 1 if the thresholds are, wave tiles,
    tile flag bytes to provide, record words to provide) of a fused spatial
    step over (N, C, S) predictions of fp32 (``dtype_code`` 0) or bf16 (1) at a
    16-byte aligned address, None where the kernels do not cover the shape.
    ``num_thresholds`` 0: no curve leader. Host only."""
    key = (N, C, S, dtype_code, num_thresholds)
    if key not in _MC_SPATIAL_LAYOUT_CACHE:
        out = (_LL * 12)()
        rc = _lib().ma_mc_spatial_layout(N, C, S, dtype_code, num_thresholds, out)
        if len(_MC_SPATIAL_LAYOUT_CACHE) > 256:
            _MC_SPATIAL_LAYOUT_CACHE.clear()
        _MC_SPATIAL_LAYOUT_CACHE[key] = tuple(out) if rc == 0 else None
    return _MC_SPATIAL_LAYOUT_CACHE[key]


def mc_spatial_step_update(
    preds: Tensor, target: Tensor, num_classes: int, ignore_index: Optional[int],
    stat=None, confmat=None, exact=None, curve=None,
) -> bool:
    """The whole step of a multiclass collection fed (N, C, *spatial) fp32 /
    bf16 ``preds`` and an int64 ``target`` (N, *spatial), in ONE native call of
    two launches that reads both once and transposes nothing: per-class stat
    counts into the ``stat`` leader's tp/fp/tn/fn, the (C, C) counts into the
    ``confmat`` leader's state, the exact-match counts into the ``exact``
    leader's correct/total, and the threshold-curve histogram into the
    ``curve`` leader's lazy buffer (absent leaders are None). Every buffer
    lives in the ``__dict__`` of the leader it serves (:func:`owner_buffer`);
    no allocation, fill or host sync in steady state. Both inputs must be
    contiguous.

    Returns False without launching anything where the kernels do not cover
    the shape: the caller lets every leader update on its own.
    """
    lib = _lib()
    dt = _dtype_code(preds)
    N, C = preds.shape[0], num_classes
    S = preds.numel() // (N * C) if N else math.prod(preds.shape[2:])
    dev = preds.device
    base = stat if stat is not None else confmat if confmat is not None else exact if exact is not None else curve
    thr, T = None, 0
    if curve is not None:
        src = curve.thresholds
        hit = curve.__dict__.get("_hip_sp_thr")
        if hit is not None and hit[0] is src:
            thr = hit[1]
        else:
            thr = src.contiguous().float()
            curve.__dict__["_hip_sp_thr"] = (src, thr)
        T = thr.numel()
    lay = mc_spatial_layout(N, C, S, dt, T)
    if lay is None:
        return False
    if curve is not None:
        flush_if_b0_pending(curve)  # a one-pass step over 2-D batches wrote last: complete its histogram first
    tensors = McSpatialStepTensors(
        counts=owner_buffer(base, "_hip_sp_counts", (3 * C,), torch.long, dev),
        records=owner_buffer(base, "_hip_sp_records", (lay[11],), torch.int32, dev),
        tp=stat.tp if stat is not None else None,
        fp=stat.fp if stat is not None else None,
        tn=stat.tn if stat is not None else None,
        fn=stat.fn if stat is not None else None,
        confmat=confmat.confmat if confmat is not None else None,
        correct=exact.correct if exact is not None else None,
        total=exact.total if exact is not None else None,
        rowbad=owner_buffer(exact, "_hip_sp_rowbad", (max(N, 1),), torch.int32, dev, grow=True)
        if exact is not None else None,
    )
    if curve is not None:
        tensors = tensors._replace(
            thresholds=thr,
            hist=_pooled_hist(C, T, dev, curve),
            epoch_buf=_epoch_buf(dev, curve),
            rowstats=_rowstats_buf(curve, max(N * S, 1), dev),
            tile_flags=owner_buffer(curve, "_hip_sp_tile_flags", (max(lay[10], 1),), torch.uint8, dev, grow=True),
        )
    # the record holds the addresses of everything that stays the same from
    # step to step; reset() and a move to another device replace state tensors
    # and the next step rebuilds it (the identity rule of _NativePlan.fits)
    scalars = (C, ignore_index, T)
    kept = base.__dict__.get("_hip_sp_rec")
    if kept is not None and kept.scalars == scalars and all(map(operator.is_, kept.tensors, tensors)):
        rec = kept.rec
    else:
        for name, shape in (("tp", (C,)), ("fp", (C,)), ("tn", (C,)), ("fn", (C,)), ("confmat", (C, C)),
                            ("correct", (1,)), ("total", (1,))):
            x = getattr(tensors, name)
            if x is not None and not (
                x.is_contiguous() and x.dtype == torch.long and x.device == dev and tuple(x.shape) == shape
            ):
                return False
        rec = mc_spatial_step(C, ignore_index, tensors, _uniform_params(thr) if curve is not None else (0, 0.0, 1.0))
        base.__dict__["_hip_sp_rec"] = _MlStepRecord(tensors, scalars, rec)
    rc = lib.ma_mc_spatial_step(_stream(), rec, preds.data_ptr(), dt, target.data_ptr(), N, S)
    if rc == -103:
        return False  # nothing was launched
    _check(rc, "ma_mc_spatial_step")
    # the raw-pointer writes of the step, for the version-keyed caches (the
    # same states mc_step_mark_mutated notes)
    if tensors.confmat is not None:
        _mark_kernel_mutated(tensors.confmat)
    if tensors.tp is not None:
        _mark_kernel_mutated(tensors.tp)
    if curve is not None:
        # same lazy protocol as curve_hist_into_confmat: the histogram
        # accumulates, the suffix/confmat materialization waits for a state read
        curve.__dict__["_hip_lazy_meta"] = (C, T, 1)
        curve.__dict__["_lazy_dirty"] = True
    return True


# Multilabel ranking measures (csrc/ml_rank.hip). METRICS_AMD_RANKING_KERNEL=0
# keeps the torch path of functional/classification/ranking.py everywhere,
# exactly as before (A/B lever, escape hatch and an oracle of the tests). Read
# at every call, and when a collection builds its plan.
RANKING_KERNEL_ENV = "METRICS_AMD_RANKING_KERNEL"

# Largest label count the kernel covers: a block stages one row in LDS as fp32
# scores plus the u16 indices of the relevant labels, 6 bytes per label (the row
# padded to a multiple of 4), behind 256 bytes of block scratch, against the
# 160 KiB of a gfx950 workgroup: 6*L + 256 <= 163840 (RANK_LDS_BYTES /
# RANK_LDS_STATIC / RANK_LABEL_BYTES in csrc/ml_rank.hip). Above it the torch
# path runs.
ML_RANK_MAX_L = (160 * 1024 - 256) // 6 // 4 * 4  # 27264

RANK_WANT_COVERAGE, RANK_WANT_LRAP, RANK_WANT_LOSS = 1, 2, 4

_RANK_LAYOUT_CACHE: dict = {}
_RANK_FUNCTIONAL_OWNERS: dict = {}


class _RankOwner:
    """Holds the scratch of the functional form, one per device."""


def ranking_kernel_enabled() -> bool:
    return os.environ.get(RANKING_KERNEL_ENV, "1") != "0"


def ml_rank_layout(rows: int, num_labels: int) -> Optional[tuple]:
    """(waves per row, rows per block and pass, blocks, dynamic LDS bytes, slab
    entries, last L of the wave-per-row mapping, largest L covered) of a
    ranking call, None where the kernel does not cover the shape. Host only."""
    key = (rows, num_labels)
    if key not in _RANK_LAYOUT_CACHE:
        out = (_LL * 7)()
        rc = _lib().ma_ml_rank_layout(rows, num_labels, out)
        if len(_RANK_LAYOUT_CACHE) > 256:
            _RANK_LAYOUT_CACHE.clear()
        _RANK_LAYOUT_CACHE[key] = tuple(out) if rc == 0 else None
    return _RANK_LAYOUT_CACHE[key]


def _rank_state_ok(pair, dev) -> bool:
    return all(
        isinstance(x, Tensor) and x.dtype == torch.float32 and x.numel() == 1 and x.device == dev and x.is_contiguous()
        for x in pair
    )


def ml_ranking_into(
    preds: Tensor, target: Tensor, ignore_index: Optional[int],
    coverage: Optional[Tuple[Tensor, Tensor]] = None,
    lrap: Optional[Tuple[Tensor, Tensor]] = None,
    loss: Optional[Tuple[Tensor, Tensor]] = None,
    owner=None,
) -> bool:
    """The ranking sums of one batch in ONE native call of two launches, added
    in place into the ``(measure, total)`` pairs given (one-element fp32
    tensors; an absent measure is None). ``preds`` holds the already normalised
    (N, L) fp32 / bf16 scores, ``target`` the int64 targets, both contiguous;
    ``ignore_index`` is applied in the kernel. The fp64 slab lives in the
    ``__dict__`` of ``owner`` (:func:`owner_buffer`); no allocation, fill or
    host sync in steady state.

    Returns False without launching anything where the kernel does not cover
    the shape or a state: the caller runs the torch path.
    """
    lib = _lib()
    dt = _dtype_code(preds)
    N, L = preds.shape
    dev = preds.device
    pairs = (coverage, lrap, loss)
    want = sum(bit for bit, pair in zip((RANK_WANT_COVERAGE, RANK_WANT_LRAP, RANK_WANT_LOSS), pairs) if pair is not None)
    if want == 0 or N == 0:
        return False
    lay = ml_rank_layout(N, L)
    if lay is None or not all(_rank_state_ok(pair, dev) for pair in pairs if pair is not None):
        return False
    if owner is None:
        owner = _RANK_FUNCTIONAL_OWNERS.get(dev)
        if owner is None:
            owner = _RANK_FUNCTIONAL_OWNERS[dev] = _RankOwner()
    slab = owner_buffer(owner, "_hip_rank_slab", (lay[4] * 4,), torch.float64, dev, zero=False)
    ptrs = [x.data_ptr() if pair is not None else 0 for pair in pairs for x in (pair or (None, None))]
    rc = lib.ma_ml_rank(
        _stream(), preds.data_ptr(), dt, target.data_ptr(), N, L,
        ignore_index if ignore_index is not None else 0, int(ignore_index is not None), want,
        slab.data_ptr(), *ptrs,
    )
    if rc == -103:
        return False  # nothing was launched
    _check(rc, "ma_ml_rank")
    return True


def ml_ranking_sums(preds: Tensor, target: Tensor, ignore_index: Optional[int], want: int) -> Optional[Tensor]:
    """Functional form: the sums of one batch as a fresh (3, 2) fp32 tensor,
    rows coverage / LRAP / loss, columns (measure, total); rows ``want`` does
    not name stay zero. None where the kernel does not cover the shape."""
    out = torch.zeros(3, 2, dtype=torch.float32, device=preds.device)
    pairs = [(out[i, 0], out[i, 1]) if want & bit else None
             for i, bit in enumerate((RANK_WANT_COVERAGE, RANK_WANT_LRAP, RANK_WANT_LOSS))]
    if not ml_ranking_into(preds, target, ignore_index, *pairs):
        return None
    return out


# Collection compute plan (csrc/mc_compute.hip). METRICS_AMD_COMPUTE_PLAN=0
# turns it off: every member then computes through its own path, exactly as
# before (A/B lever and the oracle of the tests). Read at every compute.
COMPUTE_PLAN_ENV = "METRICS_AMD_COMPUTE_PLAN"
COMPUTE_FLUSH = 1  # step flag: the curve histogram holds updates to flush


def compute_plan_enabled() -> bool:
    return os.environ.get(COMPUTE_PLAN_ENV, "1") != "0"


class ComputeStates(NamedTuple):
    """The state tensors a compute plan reads, None where a group is absent:
    the stat states, the (C, C) confusion matrix, the exact-match states, the
    (T, C, 2, 2) curve state and the curve leader's histogram."""

    tp: Optional[Tensor] = None
    fp: Optional[Tensor] = None
    tn: Optional[Tensor] = None
    fn: Optional[Tensor] = None
    confmat: Optional[Tensor] = None
    correct: Optional[Tensor] = None
    total: Optional[Tensor] = None
    curve_state: Optional[Tensor] = None
    hist: Optional[Tensor] = None


class _ComputePlan(_NativePlan):
    """Native compute plan (``ma_compute_plan_*``): ``tensors`` are the
    :class:`ComputeStates` it was built for, ``owned`` the plan's own buffers."""

    __slots__ = ("owned", "auc_views", "n_formulas", "auc_stride", "device")

    def __init__(self, dev, C: int, T: int, states: ComputeStates, params, zero_division: float):
        """params = the 13 floats of every linear formula, flattened."""
        lib = _lib()
        self.device = dev
        n = len(params) // 13
        has_curve = states.curve_state is not None
        params_dev = torch.tensor(params, dtype=torch.float32, device=dev) if n else None
        cm_scratch = torch.zeros(3 * C, dtype=torch.long, device=dev) if states.confmat is not None else None
        # each per-class vector starts 256-byte aligned, as a fresh tensor does
        self.auc_stride = (C + 63) // 64 * 64
        auc = torch.empty(4, self.auc_stride, dtype=torch.float32, device=dev) if has_curve else None
        self.auc_views = tuple(auc[i, :C] for i in range(4)) if has_curve else None
        ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        handle = ctypes.c_ulonglong(0)
        rc = lib.ma_compute_plan_create(
            C, T, ptr(states.tp), ptr(states.fp), ptr(states.tn), ptr(states.fn),
            ptr(states.confmat), ptr(cm_scratch), ptr(states.correct), ptr(states.total),
            ptr(states.hist) if has_curve else 0, ptr(states.curve_state),
            0,  # the lazy flush does not close an epoch: every update closed its own
            ptr(params_dev), n, float(zero_division), self.auc_stride, ctypes.byref(handle),
        )
        _check(rc, "ma_compute_plan_create")
        self._adopt(handle.value, states, lib.ma_compute_plan_destroy)
        self.owned = (params_dev, cm_scratch, auc)
        self.n_formulas = n

    def step(self, flush: bool, pending: Optional[tuple] = None):
        """One native call, at most three launches, one more in front of them
        for ``pending`` = (curve scratch, float32 thresholds) of a histogram in
        pending-b0 format (:func:`take_b0_pending`; with ``flush`` only). Returns (out, auc): a fresh
        ``[linear 0..n-1 | mcc, kappa, jaccard | exact]`` float32 buffer and the
        (C,) views ``(auroc, auroc weights, ap, ap weights)`` of the plan's own
        per-class buffer (None without a curve group; overwritten by the next
        step, so only reductions of them go to a caller)."""
        _, _, auc = self.owned
        # fresh per compute: views of it go to the caller and are never recycled
        out = torch.empty(self.n_formulas + 4, dtype=torch.float32, device=self.device)
        rc = _lib().ma_compute_plan_step(
            self.handle, _stream(), COMPUTE_FLUSH if flush else 0, out.data_ptr(),
            auc.data_ptr() if auc is not None else 0,
            pending[0].data_ptr() if pending else 0, pending[1].data_ptr() if pending else 0,
        )
        _check(rc, "ma_compute_plan_step")
        return out, self.auc_views
