"""k_curve_resolve_pending (csrc/kernels.hip) alone, through
``_hip.curve_resolve_pending``, on synthetic histograms.

The kernel completes a (C, T+1, 2) histogram in "pending b0" format
(csrc/mc_onepass.hip): with b0 = the bucket of 0.0,

    hist[c][b0][1] += P[c]          - sum_j hist[c][j][1]
    hist[c][b0][0] += (R[c] - P[c]) - sum_j hist[c][j][0]

and zeroes P and R. Everything is an integer, so the result must be
``torch.equal`` to the same formula in torch int64.

Shapes: (C, T) = (3, 1) (one wave of the four of a block has no class; a class
row of four words, fewer than a wave), (136, 5) with b0 = 0, (1000, 200)
linspace with b0 = 1 (thresholds[0] = 0.0 <= 0.0) and a class row longer than
one pass of the wave. The pending vector is the head of a longer buffer, as in
the one-pass scratch; what lies behind 2*C must stay untouched.
"""
import pytest
import torch

from metrics_amd.ops import _hip

pytestmark = pytest.mark.gpu

_CASES = {
    "C3-T1": (3, torch.tensor([0.5])),
    "C136-T5": (136, torch.tensor([0.05, 0.2, 0.35, 0.6, 0.95])),
    "C1000-T200": (1000, torch.linspace(0, 1, 200)),
}
_B0 = {"C3-T1": 0, "C136-T5": 0, "C1000-T200": 1}


def _synthetic(C, T, b0, seed):
    """A complete histogram of R rows per class, and the same with bucket b0
    short of what a one-pass step leaves out, with the P and R that go with it."""
    gen = torch.Generator().manual_seed(seed)
    full = torch.randint(0, 50, (C, T + 1, 2), generator=gen)
    full[:, b0, :] += 1000  # most elements live in b0
    # every class has the same row count R = its element count: top up label 0 of b0
    per_class = full.sum(dim=(1, 2))
    R = int(per_class.max()) + 7
    full[:, b0, 0] += R - per_class
    P = full[:, :, 1].sum(dim=1)
    owed = torch.stack([
        torch.randint(0, 900, (C,), generator=gen),  # label 0: fewer than the 1000 there
        torch.minimum(torch.randint(0, 900, (C,), generator=gen), full[:, b0, 1]),
    ], dim=1)
    pending_hist = full.clone()
    pending_hist[:, b0, :] -= owed
    return full, pending_hist, P, torch.full((C,), R, dtype=torch.long)


@pytest.mark.parametrize("name", list(_CASES))
def test_resolve_matches_int64_formula(name):
    C, thr = _CASES[name]
    T, b0 = thr.numel(), _B0[name]
    assert int(torch.searchsorted(thr, torch.tensor([0.0]), right=True)) == b0
    full, pending_hist, P, R = _synthetic(C, T, b0, seed=C + T)
    # the formula, in torch int64, from the pending histogram itself
    want = pending_hist.clone()
    want[:, b0, 1] += P - pending_hist[:, :, 1].sum(dim=1)
    want[:, b0, 0] += (R - P) - pending_hist[:, :, 0].sum(dim=1)
    assert torch.equal(want, full)  # and it restores the complete histogram

    hist = pending_hist.cuda().contiguous()
    tail = torch.arange(1, 38)  # stands for the records behind P and R
    pending = torch.cat([P, R, tail]).cuda()
    _hip.curve_resolve_pending(hist, thr.cuda().float().contiguous(), pending)
    torch.cuda.synchronize()
    assert torch.equal(hist.cpu(), want)
    assert torch.equal(pending[: 2 * C].cpu(), torch.zeros(2 * C, dtype=torch.long))
    assert torch.equal(pending[2 * C:].cpu(), tail)


def test_nothing_owed_changes_nothing():
    """P and R of a complete histogram: both deficits are zero."""
    C, thr = _CASES["C136-T5"]
    full, _, P, R = _synthetic(C, thr.numel(), 0, seed=5)
    hist = full.cuda().contiguous()
    pending = torch.cat([P, R]).cuda()
    _hip.curve_resolve_pending(hist, thr.cuda(), pending)
    torch.cuda.synchronize()
    assert torch.equal(hist.cpu(), full)
    assert int(pending.abs().sum()) == 0


def test_null_pending_launches_nothing():
    C, thr = _CASES["C136-T5"]
    _, pending_hist, _, _ = _synthetic(C, thr.numel(), 0, seed=6)
    hist = pending_hist.cuda().contiguous()
    _hip.curve_resolve_pending(hist, thr.cuda(), None)
    torch.cuda.synchronize()
    assert torch.equal(hist.cpu(), pending_hist)
