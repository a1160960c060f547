"""How many kernels one step of the native compute plan launches
(``ma_compute_plan_launches``, csrc/mc_compute.hip). Host only: the plan is a
record of addresses, which the reporter never follows, so made-up non-zero
addresses stand for the state tensors and no GPU is needed.
"""
import ctypes

import pytest

from metrics_amd.ops import _hip

pytestmark = pytest.mark.skipif(not _hip.hip_available(), reason="kernel library not built")

A = 0x1000  # any non-zero address: "this group is present"


def _plan(C=1000, T=200, stat=True, confmat=True, exact=True, curve=True):
    handle = ctypes.c_ulonglong(0)
    s, cm, ex, cu = (A if stat else 0), (A if confmat else 0), (A if exact else 0), (A if curve else 0)
    rc = _hip._lib().ma_compute_plan_create(
        C, T, s, s, s, s, cm, cm, ex, ex, cu, cu, 0, s, 9 if stat else 0, 0.0, (C + 63) // 64 * 64,
        ctypes.byref(handle),
    )
    assert rc == 0
    return handle.value


def _launches(handle, flush, pending):
    try:
        return _hip.compute_plan_launches(handle, flush, pending)
    finally:
        _hip._lib().ma_compute_plan_destroy(handle)


@pytest.mark.parametrize("flush,pending", [(True, True), (True, False), (False, False)])
def test_bench_collection_makes_two(flush, pending):
    assert _launches(_plan(), flush, pending) == 2


def test_one_role_present_still_two_with_scalars():
    assert _launches(_plan(curve=False), False, False) == 2
    assert _launches(_plan(confmat=False), True, True) == 2
    # curve members alone: the passes kernel and nothing for the scalars kernel to do
    assert _launches(_plan(stat=False, confmat=False, exact=False), True, True) == 1


def test_scalars_only_makes_one():
    assert _launches(_plan(confmat=False, curve=False), False, False) == 1


def test_large_t_keeps_the_separate_kernels():
    """T beyond the tiled kernel's LDS: resolve (pending only), suffix (flush
    only), two AUC kernels, then the confusion-matrix pass and the scalars."""
    big = 20000
    assert _launches(_plan(T=big), True, True) == 6
    assert _launches(_plan(T=big), True, False) == 5
    assert _launches(_plan(T=big), False, False) == 4
    assert _launches(_plan(T=big, confmat=False, stat=False, exact=False), True, True) == 4


def test_pending_without_a_flush_is_refused():
    assert _launches(_plan(), False, True) == -103
    assert _launches(_plan(curve=False), True, True) == -103
