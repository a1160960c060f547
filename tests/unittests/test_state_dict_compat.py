"""State-dict byte-compatibility with the reference (BASELINE requirement).

A checkpoint written by the reference must load into our metric and vice
versa: same keys (prefix + state name), same shapes/dtypes, same semantics
after restore.

The reference side is replayed from the golden tapes under
tests/golden/reference/ (see tests/unittests/_golden.py): its state dicts and
computed values are the recorded ones. What the reference computed from OUR
checkpoint was recorded too, so test_our_checkpoint_loads_into_reference pins
our compute() to that record; that our keys, shapes and dtypes are the ones a
strict load accepts is what test_state_dict_keys_match_reference asserts.
"""
from __future__ import annotations

import io

import torch

import metrics_amd as ma
from tests.unittests._golden import ref_module


def _tm():
    return ref_module("torchmetrics")


def _roundtrip(state_dict):
    buf = io.BytesIO()
    torch.save(state_dict, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _pairs(tm):
    g = torch.Generator().manual_seed(31)
    mc = (torch.randn(64, 5, generator=g).softmax(-1), torch.randint(0, 5, (64,), generator=g))
    reg = (torch.randn(64, generator=g), torch.randn(64, generator=g))
    return [
        (ma.MulticlassAccuracy(num_classes=5), tm.classification.MulticlassAccuracy(num_classes=5), mc),
        (ma.MulticlassConfusionMatrix(num_classes=5), tm.classification.MulticlassConfusionMatrix(num_classes=5), mc),
        (ma.MeanSquaredError(), tm.MeanSquaredError(), reg),
        (ma.PearsonCorrCoef(), tm.PearsonCorrCoef(), reg),
        (ma.MeanMetric(), tm.MeanMetric(), (reg[0],)),
    ]


def test_state_dict_keys_match_reference():
    tm = _tm()
    for ours, ref, args in _pairs(tm):
        ours.persistent(True)
        ref.persistent(True)
        ours.update(*args)
        ref.update(*args)
        k1, k2 = set(ours.state_dict().keys()), set(ref.state_dict().keys())
        assert k1 == k2, (type(ours).__name__, k1, k2)
        for k in k1:
            a, b = ours.state_dict()[k], ref.state_dict()[k]
            if isinstance(a, torch.Tensor):
                assert a.shape == b.shape and a.dtype == b.dtype, (type(ours).__name__, k)


def test_reference_checkpoint_loads_into_ours():
    tm = _tm()
    for ours, ref, args in _pairs(tm):
        ref.persistent(True)
        ref.update(*args)
        expected = ref.compute()
        sd = _roundtrip(ref.state_dict())
        ours.persistent(True)
        ours.load_state_dict(sd)
        ours._update_count = ref._update_count
        got = ours.compute()
        assert torch.allclose(
            torch.as_tensor(got).float(), torch.as_tensor(expected).float(), atol=1e-6
        ), type(ours).__name__


def test_our_checkpoint_loads_into_reference():
    tm = _tm()
    for ours, ref, args in _pairs(tm):
        ours.persistent(True)
        ours.update(*args)
        expected = ours.compute()
        sd = _roundtrip(ours.state_dict())
        ref.persistent(True)
        ref.load_state_dict(sd)
        ref._update_count = ours._update_count
        got = ref.compute()
        assert torch.allclose(
            torch.as_tensor(got).float(), torch.as_tensor(expected).float(), atol=1e-6
        ), type(ours).__name__


def test_collection_checkpoint_cross_load():
    tm = _tm()
    g = torch.Generator().manual_seed(32)
    args = (torch.randn(64, 5, generator=g).softmax(-1), torch.randint(0, 5, (64,), generator=g))

    ours = ma.MetricCollection([ma.MulticlassAccuracy(num_classes=5), ma.MulticlassConfusionMatrix(num_classes=5)])
    ref = tm.MetricCollection(
        [tm.classification.MulticlassAccuracy(num_classes=5), tm.classification.MulticlassConfusionMatrix(num_classes=5)]
    )
    ours.persistent(True)
    ref.persistent(True)
    ours.update(*args)
    ref.update(*args)
    assert set(ours.state_dict().keys()) == set(ref.state_dict().keys())
    ours2 = ma.MetricCollection([ma.MulticlassAccuracy(num_classes=5), ma.MulticlassConfusionMatrix(num_classes=5)])
    ours2.persistent(True)
    ours2.load_state_dict(_roundtrip(ref.state_dict()))
    for m, n in zip(ours2.values(copy_state=False), ours.values(copy_state=False)):
        m._update_count = n._update_count
    got, exp = ours2.compute(), ref.compute()
    for k in exp:
        assert torch.allclose(torch.as_tensor(got[k]).float(), torch.as_tensor(exp[k]).float(), atol=1e-6), k
