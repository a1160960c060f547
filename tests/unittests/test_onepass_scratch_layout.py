"""The curve scratch of the one-pass step: the layout ``ops/_hip.py`` assumes
(``onepass_scratch_layout``: P and R lead, C words each) against the size the
native side reports (``ma_mc_onepass_scratch_words``, csrc/mc_onepass.hip).

The Python side hands the scratch's address to the native flush as the
``[P: C][R: C]`` vector and zeroes the whole buffer on reset, so the two must
agree on where P and R are and on how long the buffer is. Needs only the built
library, no GPU.
"""
import pytest

from metrics_amd.ops import _hip

pytestmark = pytest.mark.skipif(not _hip.hip_available(), reason="kernel library not built")


@pytest.mark.parametrize("C", [1, 129, 136, 1000, 4096])
def test_words_agree(C):
    lay = _hip.onepass_scratch_layout(C)
    assert lay["words"] == _hip._lib().ma_mc_onepass_scratch_words(C)


@pytest.mark.parametrize("C", [136, 1000])
def test_regions_are_ordered_and_aligned(C):
    lay = _hip.onepass_scratch_layout(C)
    assert (lay["P"], lay["R"]) == (0, C)
    assert lay["R"] + C == lay["records"] < lay["flags"] < lay["words"]
    assert (lay["records"] * 8) % 16 == 0  # the records are read as 16-byte vectors
