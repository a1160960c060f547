"""Golden tapes: the reference implementation's behaviour, recorded once.

The differential tests drive our metrics and the reference's (torchmetrics)
side by side with identical seeded inputs. So that the suite needs nothing
outside the repository, the reference side is a *tape*: every value the
reference returned while a test ran was recorded, in order, into
``tests/golden/reference/<test module>.pt`` and is replayed from there.

The tests are written against ordinary-looking reference objects::

    tm = ref_module("torchmetrics")
    ref = tm.classification.BinaryAccuracy()
    ref.update(preds, target)
    expected = ref.compute()

``tm`` and ``ref`` are proxies. Each attribute access, call or operator on a
proxy is one step of the tape; a step yields plain data (tensors, numbers,
strings and containers of them), another proxy, or the exception the reference
raised. On replay every step is checked against the recorded operation, so a
test whose reference-side call sequence changed fails loudly instead of
reading the wrong value.

Re-recording needs a torchmetrics source tree::

    METRICS_AMD_REFERENCE_SRC=/path/to/torchmetrics/src \\
        python -m pytest tests/unittests -m "not gpu" -k "<tests to re-record>"

Only the tests that ran are rewritten; the other tapes are kept.
"""
from __future__ import annotations

import atexit
import builtins
import copy
import importlib
import operator
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(_HERE, "..", "golden", "reference")
REFERENCE_SRC = os.environ.get("METRICS_AMD_REFERENCE_SRC")
RECORDING = bool(REFERENCE_SRC)

_tapes: dict = {}  # test module stem -> {test name -> [[op, kind, payload], ...]}
_cursor: dict = {}  # (stem, test name) -> next step to replay
_dirty: set = set()


def _current_test():
    cur = os.environ.get("PYTEST_CURRENT_TEST")
    if not cur:
        raise RuntimeError("reference proxies can only be used inside a running test")
    path, _, name = cur.rsplit(" (", 1)[0].partition("::")
    return os.path.splitext(os.path.basename(path))[0], name


def _tape():
    stem, name = _current_test()
    if stem not in _tapes:
        path = os.path.join(GOLDEN_DIR, stem + ".pt")
        _tapes[stem] = torch.load(path, weights_only=True) if os.path.exists(path) else {}
    key = (stem, name)
    if key not in _cursor:
        _cursor[key] = 0
        if RECORDING:
            _tapes[stem][name] = []
            _dirty.add(stem)
    if name not in _tapes[stem]:
        raise AssertionError(f"no golden tape for {stem}::{name}; re-record it (see tests/unittests/_golden.py)")
    return _tapes[stem][name], key


@atexit.register
def _flush():
    for stem in sorted(_dirty):
        os.makedirs(GOLDEN_DIR, exist_ok=True)
        torch.save(_tapes[stem], os.path.join(GOLDEN_DIR, stem + ".pt"))


def _to_data(x):
    """(True, plain copy) if x is data a tape can hold, else (False, None)."""
    if x is None or isinstance(x, (bool, int, float, str)):
        return True, x
    if isinstance(x, torch.Tensor):
        return True, x.detach().cpu().clone()
    if isinstance(x, (list, tuple)):
        items = [_to_data(v) for v in x]
        if all(ok for ok, _ in items):
            return True, (list if isinstance(x, list) else tuple)(v for _, v in items)
        return False, None
    if isinstance(x, dict):
        items = {k: _to_data(v) for k, v in x.items()}
        if all(isinstance(k, (str, int)) for k in items) and all(ok for ok, _ in items.values()):
            return True, {k: v for k, (_, v) in items.items()}
    return False, None


def _unwrap(x):
    if isinstance(x, _Ref):
        return object.__getattribute__(x, "_ref_obj")
    if isinstance(x, (list, tuple)):
        return type(x)(_unwrap(v) for v in x)
    if isinstance(x, dict):
        return {k: _unwrap(v) for k, v in x.items()}
    return x


def _step(op, thunk, must_be_data=False):
    tape, key = _tape()
    if RECORDING:
        try:
            result = thunk()
        except Exception as err:
            tape.append([op, "raise", [type(err).__name__, str(err)]])
            raise
        ok, data = _to_data(result)
        if ok:
            tape.append([op, "data", data])
            return copy.deepcopy(data)
        if must_be_data:
            raise TypeError(f"{op}: {type(result).__name__} cannot be stored on a golden tape")
        tape.append([op, "obj", None])
        return _Ref(result, op)
    i = _cursor[key]
    if i >= len(tape) or tape[i][0] != op:
        recorded = tape[i][0] if i < len(tape) else "end of tape"
        raise AssertionError(
            f"golden tape of {key[0]}::{key[1]} is stale at step {i}: the test asks for {op!r}, "
            f"the tape holds {recorded!r}; re-record it (see tests/unittests/_golden.py)"
        )
    _cursor[key] = i + 1
    _, kind, payload = tape[i]
    if kind == "data":
        return copy.deepcopy(payload)
    if kind == "obj":
        return _Ref(None, op)
    exc = getattr(builtins, payload[0], None)
    if not (isinstance(exc, type) and issubclass(exc, Exception)):
        exc = RuntimeError
    raise exc(payload[1])


def _detached(x):
    """Clones of the tensors in x: a replay cannot repeat a side effect, so the
    reference never gets to touch the test's own inputs."""
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, (list, tuple)):
        return type(x)(_detached(v) for v in x)
    if isinstance(x, dict):
        return {k: _detached(v) for k, v in x.items()}
    return x


class _Ref:
    """Stand-in for a reference-side object (module, class, metric instance)."""

    __slots__ = ("_ref_obj", "_ref_path")

    def __init__(self, obj, path):
        object.__setattr__(self, "_ref_obj", obj)
        object.__setattr__(self, "_ref_path", path)

    def __getattr__(self, name):
        if name.startswith("__") and name != "__all__":
            raise AttributeError(name)
        obj, path = _unwrap(self), object.__getattribute__(self, "_ref_path")
        return _step(f"{path}.{name}", lambda: getattr(obj, name))

    def __setattr__(self, name, value):
        if RECORDING:
            setattr(_unwrap(self), name, _unwrap(value))

    def __call__(self, *args, **kwargs):
        obj, path = _unwrap(self), object.__getattribute__(self, "_ref_path")
        return _step(f"{path}()", lambda: obj(*_detached(_unwrap(args)), **_detached(_unwrap(kwargs))))

    def __dir__(self):
        obj, path = _unwrap(self), object.__getattribute__(self, "_ref_path")
        return _step(f"dir({path})", lambda: sorted(dir(obj)), must_be_data=True)

    __hash__ = object.__hash__


def _operator(name, fn, reflected=False):
    def method(self, *args):
        obj, path = _unwrap(self), object.__getattribute__(self, "_ref_path")
        if reflected:
            return _step(f"{path}.{name}", lambda: fn(_unwrap(args[0]), obj))
        return _step(f"{path}.{name}", lambda: fn(obj, *_unwrap(args)))

    method.__name__ = name
    return method


for _n, _f in (("add", operator.add), ("sub", operator.sub), ("mul", operator.mul), ("truediv", operator.truediv),
               ("floordiv", operator.floordiv), ("mod", operator.mod), ("pow", operator.pow),
               ("matmul", operator.matmul), ("and", operator.and_), ("or", operator.or_), ("xor", operator.xor)):
    setattr(_Ref, f"__{_n}__", _operator(f"__{_n}__", _f))
    setattr(_Ref, f"__r{_n}__", _operator(f"__r{_n}__", _f, reflected=True))
for _n, _f in (("eq", operator.eq), ("ne", operator.ne), ("lt", operator.lt), ("le", operator.le),
               ("gt", operator.gt), ("ge", operator.ge), ("getitem", operator.getitem), ("abs", abs),
               ("neg", operator.neg), ("pos", operator.pos), ("invert", operator.invert)):
    setattr(_Ref, f"__{_n}__", _operator(f"__{_n}__", _f))


def _import_reference(name):
    shim = os.path.abspath(os.path.join(_HERE, "..", "..", "tools", "refbench"))
    for p in (shim, REFERENCE_SRC):
        if p not in sys.path:
            sys.path.insert(0, p)
    return importlib.import_module(name)


def ref_module(name="torchmetrics"):
    """The reference module ``name`` (raises what its import raised when recorded)."""
    return _step(f"import {name}", lambda: _import_reference(name))


def ref_object(label, loader):
    """A reference-side object built by ``loader()``, which runs only while recording."""
    return _step(f"object {label}", lambda: (_import_reference("torchmetrics"), loader())[1])


def ref_value(label, fn):
    """Plain data computed from the reference by ``fn()``, which runs only while recording."""
    return _step(f"value {label}", lambda: (_import_reference("torchmetrics"), fn())[1], must_be_data=True)
