"""The step record of the fused spatial multiclass step: the ``ctypes`` mirror
in ``ops/_hip.py`` against ``McSpatialStep`` in ``csrc/mc_spatial.h``, and the
host-only layout entry with its -103 answers. Needs only the built library, no
GPU."""
import ctypes

import pytest

from metrics_amd.ops import _hip

pytestmark = pytest.mark.skipif(not _hip.hip_available(), reason="kernel library not built")


def test_sizes_are_equal():
    assert _hip._lib().ma_mc_spatial_step_sizeof() == ctypes.sizeof(_hip.McSpatialStep)
    assert ctypes.sizeof(_hip.McSpatialStep) == 8 * len(_hip.McSpatialStep._fields_)  # no padding


def test_field_names_and_order_equal_the_header():
    names = _hip.mc_spatial_step_native_fields(_hip._lib())
    assert len(set(names)) == len(names)
    assert [name for name, _ in _hip.McSpatialStep._fields_] == names


def test_exported_constants_equal_the_library():
    lib = _hip._lib()
    assert lib.ma_mc_spatial_max_classes() == _hip.MC_SPATIAL_MAX_C >= 256
    assert lib.ma_mc_spatial_lds_bytes() == _hip.MC_SPATIAL_LDS_BYTES == 160 * 1024
    assert lib.ma_mc_spatial_lds_static() == _hip.MC_SPATIAL_LDS_STATIC


def test_builder_fills_fields_by_name():
    class Fake:
        def __init__(self, ptr, shape=()):
            self._ptr, self.shape = ptr, shape

        def data_ptr(self):
            return self._ptr

    shapes = {"rowbad": (11,), "thresholds": (200,), "tile_flags": (77,)}
    names = [n for n in _hip.McSpatialStepTensors._fields if n != "rowstats"]
    t = _hip.McSpatialStepTensors(
        rowstats=Fake(4096, (2, 33)), **{n: Fake(1000 + 8 * i, shapes.get(n, ())) for i, n in enumerate(names)}
    )
    rec = _hip.mc_spatial_step(19, 255, t, (1, 0.0, 199.0))
    assert (rec.C, rec.ignore_index, rec.has_ignore) == (19, 255, 1)
    for i, n in enumerate(names):
        assert getattr(rec, n) == 1000 + 8 * i, n
    assert (rec.rowmax, rec.rowinv, rec.row_cap) == (4096, 4096 + 4 * 33, 33)
    assert (rec.T, rec.uniform, rec.t0, rec.inv_step) == (200, 1, 0.0, 199.0)
    assert (rec.sample_cap, rec.tile_cap) == (11, 77)

    rec = _hip.mc_spatial_step(7, None, _hip.McSpatialStepTensors(counts=Fake(64), records=Fake(128)))
    assert (rec.C, rec.has_ignore, rec.counts, rec.records) == (7, 0, 64, 128)
    for n in [n for n, _ in _hip.McSpatialStep._fields_ if n not in ("C", "counts", "records")]:
        assert getattr(rec, n) == 0, n


def test_layout_places_tiles_and_gates():
    V = {0: 4, 1: 8}
    for dt in (0, 1):
        for N, C, S, T in [(1, 2, 1, 0), (3, 19, 120, 100), (2, 21, 63, 200), (2, 96, 160, 200), (5, 7, 64 * V[dt] + 1, 5)]:
            lay = _hip.mc_spatial_layout(N, C, S, dt, T)
            assert lay is not None, (N, C, S, dt, T)
            v, vec, tile_px, threads, grid, tgrid, lds, cm_lds, thr_lds, n_tiles, flag_cap, rec_words = lay
            assert v == V[dt] and vec == (1 if S % v == 0 else 0)
            assert tile_px == (64 * v if vec else 64)
            assert n_tiles == N * -(-S // tile_px) <= flag_cap
            assert 1 <= grid <= rec_words // 3 and grid * (threads // 64) >= min(n_tiles, grid * (threads // 64))
            assert tgrid >= 1 and threads % 64 == 0
            want = 12 * C + (8 * C * (T + 1) if T else 0) + (4 * T if thr_lds else 0) + (4 * C * C if cm_lds else 0)
            assert lds == want and lds + _hip.MC_SPATIAL_LDS_STATIC <= _hip.MC_SPATIAL_LDS_BYTES
    # an empty batch launches the tail alone
    assert _hip.mc_spatial_layout(0, 5, 16, 0, 10)[4] == 0 and _hip.mc_spatial_layout(2, 5, 0, 0, 10)[4] == 0


def test_gate_and_cap_are_the_exported_formula():
    cmax = _hip.mc_spatial_max_curve_classes(200)
    assert cmax == 101
    assert _hip.mc_spatial_curve_rides(cmax, 200) and not _hip.mc_spatial_curve_rides(cmax + 1, 200)
    assert _hip.mc_spatial_layout(2, cmax, 24, 1, 200) is not None
    assert _hip.mc_spatial_layout(2, cmax + 1, 24, 1, 200) is None
    assert _hip.mc_spatial_layout(2, cmax + 1, 24, 1, 0) is not None  # without the curve leader
    cap = _hip.MC_SPATIAL_MAX_C
    assert _hip.mc_spatial_layout(1, cap, 8, 0, 0) is not None
    assert _hip.mc_spatial_layout(1, cap + 1, 8, 0, 0) is None


def test_uncovered_calls_return_minus_103_without_a_device():
    """Every refusal of ``ma_mc_spatial_step`` is decided on the host before
    anything is launched, so the calls below need no GPU and no real buffer."""
    lib = _hip._lib()
    ok = dict(C=5, counts=4096, records=8192)

    def call(rec, preds=1 << 20, dtype=0, target=1 << 21, N=2, S=16):
        return lib.ma_mc_spatial_step(0, rec, preds, dtype, target, N, S)

    S = _hip.McSpatialStep
    assert call(S(**ok), dtype=2) == -103  # fp16 and the like
    assert call(S(C=5, records=8192)) == -103  # no count scratch
    assert call(S(C=5, counts=4096)) == -103  # no records
    assert call(S(**ok), preds=0) == -103 and call(S(**ok), target=0) == -103
    assert call(S(**ok), target=(1 << 21) + 4) == -103  # misaligned target
    assert call(S(**ok), preds=(1 << 20) + 2) == -103  # fp32 at an odd address
    assert call(S(**ok), dtype=1, preds=(1 << 20) + 1) == -103  # bf16 at an odd address
    assert call(S(tp=8, **ok)) == -103  # half a stat group
    assert call(S(correct=8, total=16, **ok)) == -103  # exact group without rowbad
    assert call(S(correct=8, total=16, rowbad=32, sample_cap=1, **ok)) == -103  # rowbad too small
    assert call(S(C=0, counts=4096, records=8192)) == -103
    assert call(S(C=_hip.MC_SPATIAL_MAX_C + 1, counts=4096, records=8192)) == -103  # class cap
    assert call(S(**ok), N=-1) == -103 and call(S(**ok), N=1 << 20, S=1 << 20) == -103
    curve = dict(T=200, thresholds=64, hist=128, epoch_buf=256, rowmax=512, rowinv=1024, tile_flags=2048)
    assert call(S(**dict(curve, hist=0), **ok)) == -103  # curve group incomplete
    assert call(S(row_cap=31, tile_cap=8, **curve, **ok)) == -103  # row statistics too small (N*S = 32)
    assert call(S(row_cap=64, tile_cap=1, **curve, **ok), S=17) == -103  # flags: 2 tiles at S = 17
    assert call(S(C=102, counts=4096, records=8192, row_cap=64, tile_cap=8, **curve)) == -103  # above the curve gate
