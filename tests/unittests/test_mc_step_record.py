"""The step record of the fused multiclass step: the ``ctypes`` mirror in
``ops/_hip.py`` against ``McStep`` in ``csrc/mc_step.h``.

The native count, apply and plan entries read the record's fields by name; a
field out of place on the Python side would hand a kernel the wrong state
tensor without failing. Three native, host-only functions make the layout
checkable: ``ma_mc_step_field_names`` (the header's names in declaration
order), ``ma_mc_step_sizeof`` and ``ma_mc_step_dump`` (every field's value in
declaration order). The names pin which field stands where; with the names
equal, a distinct value per field read back through the dump pins each
field's offset and width. The dump alone would not see two 8-byte fields
swapped in the mirror, which the last test demonstrates. Needs only the built
library, no GPU.
"""
import ctypes

import pytest

from metrics_amd.ops import _hip

pytestmark = pytest.mark.skipif(not _hip.hip_available(), reason="kernel library not built")


def test_sizes_are_equal():
    assert _hip._lib().ma_mc_step_sizeof() == ctypes.sizeof(_hip.McStep)


def test_field_names_equal_the_header():
    assert [name for name, _ in _hip.McStep._fields_] == _hip.mc_step_native_fields(_hip._lib())


def _dump(rec, n):
    out = (ctypes.c_uint64 * (n + 1))(*([0xDEAD] * (n + 1)))
    assert _hip._lib().ma_mc_step_dump(rec, out) == n
    assert out[n] == 0xDEAD  # nothing written past the last field
    return list(out)[:n]


def test_every_field_lands_at_its_native_place():
    """Values are assigned by the NATIVE names, in the native order, so a
    mirror whose field of some name sits elsewhere fails here as well."""
    names = _hip.mc_step_native_fields(_hip._lib())
    assert len(set(names)) == len(names) == len(_hip.McStep._fields_)
    # one distinct value per field, none of them 0, and with the high half set
    # so that a field narrower than 8 bytes on either side would show
    values = [((i + 1) << 40) + 7 * i + 3 for i in range(len(names))]
    rec = _hip.McStep(**dict(zip(names, values)))
    assert _dump(rec, len(names)) == values


def test_a_swapped_mirror_is_caught():
    """The hazard itself: a mirror with two pointer pairs swapped has the right
    size and field count, and both checks above reject it."""
    fields = dict(_hip.McStep._fields_)
    order = [name for name, _ in _hip.McStep._fields_]
    for a, b in (("fp", "fn"), ("tp", "tp_k")):
        i, j = order.index(a), order.index(b)
        order[i], order[j] = order[j], order[i]

    class Swapped(ctypes.Structure):
        _fields_ = [(name, fields[name]) for name in order]

    names = _hip.mc_step_native_fields(_hip._lib())
    assert ctypes.sizeof(Swapped) == _hip._lib().ma_mc_step_sizeof()
    assert [name for name, _ in Swapped._fields_] != names
    values = list(range(1, len(names) + 1))
    rec = Swapped(**dict(zip(names, values)))
    got = _dump(ctypes.cast(ctypes.pointer(rec), ctypes.POINTER(_hip.McStep)).contents, len(names))
    assert got != values and sorted(got) == values


def test_builder_fills_fields_by_name():
    """``mc_step`` on stand-ins that only have ``data_ptr`` and ``shape``: every
    named tensor lands in the field of its name, absent groups stay 0, and the
    row statistics split into rowmax | rowinv."""

    class Fake:
        def __init__(self, ptr, shape=()):
            self._ptr, self.shape = ptr, shape

        def data_ptr(self):
            return self._ptr

    names = [n for n in _hip.McStepTensors._fields if n != "rowstats"]
    t = _hip.McStepTensors(rowstats=Fake(4096, (2, 33)), **{n: Fake(1000 + 8 * i) for i, n in enumerate(names)})
    rec = _hip.mc_step(130, 3, t, k=5)
    assert (rec.C, rec.ignore_index, rec.has_ignore, rec.k) == (130, 3, 1, 5)
    for i, n in enumerate(names):
        assert getattr(rec, n) == 1000 + 8 * i, n
    assert (rec.rowmax, rec.rowinv) == (4096, 4096 + 4 * 33)

    rec = _hip.mc_step(7, None, _hip.McStepTensors(counts=Fake(64)))
    assert (rec.C, rec.ignore_index, rec.has_ignore, rec.k, rec.counts) == (7, 0, 0, 0, 64)
    for n in [n for n, _ in _hip.McStep._fields_ if n not in ("C", "counts")]:
        assert getattr(rec, n) == 0, n
