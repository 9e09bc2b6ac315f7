"""Recorded calls into the reference (TEST INFRASTRUCTURE ONLY): what the reference's own functions returned, kept under
``tests/golden/reference_calls/<suite>.npz`` so that the tests that compare against them run wherever the repository is,
with or without the reference tree.

    VGG_RECORD_REFERENCE=1 python -m pytest tests/<module>.py     (needs the reference tree, see ref_harness.py)

runs the reference's functions live through ``ref_harness`` and rewrites the suite's file at exit.  Otherwise every call
returns (or raises) what the reference did for it, after checking that the arguments are the ones it was recorded with:
integer / boolean data exactly, floating-point data to 1e-9 of its magnitude (the inputs are drawn by seeded numpy / torch
code, whose last bits may differ between CPUs).  Calls are matched by test, function and order within the test.

Results are stored as arrays plus a JSON tree (no pickle): tensors, numpy arrays and scalars, tuples, lists, dicts,
named tuples and plain objects (read back as ``types.SimpleNamespace``)."""
import atexit
import builtins
import json
import os
import types

import numpy as np
import torch

from oracle import ref_harness

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_calls")
RECORD = os.environ.get("VGG_RECORD_REFERENCE") == "1"


class _Encoder:
    def __init__(self):
        self.arrays = {}

    def _array(self, a):
        key = f"a{len(self.arrays)}"
        self.arrays[key] = np.array(a, order="C")          # (ascontiguousarray would give 0-d arrays a dimension)
        return key

    def __call__(self, x):
        if x is None or isinstance(x, (bool, int, float, str)):
            return {"v": x}
        if isinstance(x, (torch.device, torch.dtype)):
            return {"v": str(x)}
        if isinstance(x, torch.Tensor):
            return {"t": self._array(x.detach().cpu().numpy())}
        if isinstance(x, (np.ndarray, np.generic)):
            return {"n": self._array(np.asarray(x)), "scalar": isinstance(x, np.generic)}
        if isinstance(x, tuple) and hasattr(x, "_fields"):
            return {"ns": {f: self(getattr(x, f)) for f in x._fields}}
        if isinstance(x, (tuple, list, torch.Size)):
            return {"list" if isinstance(x, list) else "tuple": [self(v) for v in x]}
        if isinstance(x, dict):
            return {"dict": [[self(k), self(v)] for k, v in x.items()]}
        if hasattr(x, "__dict__"):
            return {"ns": {k: self(v) for k, v in vars(x).items() if not k.startswith("_")}}
        raise TypeError(f"cannot record a {type(x).__name__}")


def _decode(node, arrays):
    if "v" in node:
        return node["v"]
    if "t" in node:
        return torch.from_numpy(arrays[node["t"]].copy())
    if "n" in node:
        a = arrays[node["n"]].copy()
        return a[()] if node.get("scalar") else a
    if "tuple" in node:
        return tuple(_decode(v, arrays) for v in node["tuple"])
    if "list" in node:
        return [_decode(v, arrays) for v in node["list"]]
    if "dict" in node:
        return {_decode(k, arrays): _decode(v, arrays) for k, v in node["dict"]}
    if "ns" in node:
        return types.SimpleNamespace(**{k: _decode(v, arrays) for k, v in node["ns"].items()})
    raise ValueError(f"unknown record node {sorted(node)}")


def fingerprint(x):
    """A JSON-able summary of an argument: shapes, dtypes, exact integer / boolean content, floating-point sums."""
    if callable(x) and not isinstance(x, (torch.Tensor, np.ndarray)) and hasattr(x, "__name__"):
        return ["fn", x.__name__]
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, (np.ndarray, np.generic)):
        a = np.asarray(x)
        if a.dtype.kind in "fc":
            a = a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)
            fin = np.isfinite(a)
            w = np.arange(1, a.size + 1, dtype=np.float64).reshape(a.shape) if a.size else a.real
            return ["f", list(a.shape), str(x.dtype), int((~fin).sum()), float(np.abs(a[fin]).sum()),
                    float((np.abs(a) * w)[fin].sum())]
        return ["i", list(a.shape), str(a.dtype), a.astype(np.int64).ravel().tolist() if a.size <= 64 else
                [int(a.astype(np.int64).sum()), int((a.astype(np.int64).ravel() * np.arange(a.size)).sum())]]
    if isinstance(x, float):
        return ["f", [], "float", 0 if np.isfinite(x) else 1, abs(x) if np.isfinite(x) else 0.0, 0.0]
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, dict):
        return ["dict", [[fingerprint(k), fingerprint(v)] for k, v in x.items()]]
    if isinstance(x, (tuple, list, torch.Size)):
        return ["seq", [fingerprint(v) for v in x]]
    if hasattr(x, "__dict__"):
        return ["obj", {k: fingerprint(v) for k, v in sorted(vars(x).items()) if not k.startswith("_")}]
    return ["repr", type(x).__name__]


def _same(a, b):
    if isinstance(a, list) and isinstance(b, list) and a[:1] == ["f"] and b[:1] == ["f"] and len(a) == len(b) == 6:
        return a[:4] == b[:4] and all(abs(x - y) <= 1e-9 * max(abs(x), abs(y), 1e-300) + 1e-300 for x, y in zip(a[4:], b[4:]))
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


def _exception(spec):
    mod, name = spec
    cls = getattr(builtins if mod == "builtins" else _import(mod), name, None)
    if not (isinstance(cls, type) and issubclass(cls, Exception)):
        raise RuntimeError(f"recorded exception {mod}.{name} cannot be raised here")
    return cls


class Calls:
    """The recorded reference calls of one test suite (one file under tests/golden/reference_calls/)."""

    def __init__(self, suite):
        self.suite = suite
        self.path = os.path.join(GOLDEN, f"{suite}.npz")
        self.live = RECORD
        self.counters = {}
        if self.live:
            ref_harness.install()
            self.enc, self.records = _Encoder(), {}
            atexit.register(self.save)
        else:
            if not os.path.isfile(self.path):
                raise FileNotFoundError(f"{self.path}: recorded reference calls missing (see oracle/ref_replay.py)")
            with np.load(self.path, allow_pickle=False) as z:
                self.arrays = {k: z[k] for k in z.files if k != "__tree__"}
                self.records = json.loads(str(z["__tree__"]))

    def _key(self, name):
        test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::", 1)[-1]
        n = self.counters.get((test, name), 0)
        self.counters[(test, name)] = n + 1
        return f"{test}|{name}|{n}"

    def fn(self, name, live=None, key_args=None):
        """A callable standing for the reference function `name` ("package.module:qualname").  live: the callable to run
        when recording (default: `name` imported from the reference); key_args(*args, **kwargs) -> what identifies the
        call's inputs (default: the arguments themselves)."""
        def call(*args, **kwargs):
            key = self._key(name)
            fp = fingerprint(key_args(*args, **kwargs) if key_args else [list(args), kwargs])
            if self.live:
                f = live if live is not None else reference(name)
                try:
                    out = f(*args, **kwargs)
                except Exception as exc:
                    self.records[key] = {"args": fp, "raises": [type(exc).__module__, type(exc).__name__]}
                    raise
                self.records[key] = {"args": fp, "out": self.enc(out)}
                return out
            if key not in self.records:
                raise KeyError(f"{self.path}: no recorded call {key} (re-record with VGG_RECORD_REFERENCE=1)")
            rec = self.records[key]
            if not _same(json.loads(json.dumps(fp)), rec["args"]):
                raise AssertionError(f"{key}: the arguments differ from the ones the reference was recorded with")
            if "raises" in rec:
                raise _exception(rec["raises"])(f"(recorded) the reference raised {rec['raises'][1]}")
            return _decode(rec["out"], self.arrays)
        return call

    def module(self, name):
        """Stands for reference module `name`: its attributes are recorded functions; attributes set on it reach the real
        module while recording (the kornia helpers some tests restate) and are dropped on replay."""
        return _Module(self, name)

    def save(self):
        os.makedirs(GOLDEN, exist_ok=True)
        np.savez_compressed(self.path, __tree__=np.array(json.dumps(self.records)), **self.enc.arrays)


class _Module:
    def __init__(self, owner, name):
        object.__setattr__(self, "_owner", owner)
        object.__setattr__(self, "_name", name)

    def __getattr__(self, attr):
        return self._owner.fn(f"{self._name}:{attr}")

    def __setattr__(self, attr, value):
        if self._owner.live:
            setattr(_import(self._name), attr, value)


def _import(mod):
    import importlib
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return importlib.import_module(mod)


def reference(name):
    """The reference object `name` ("package.module:qualname"), imported live (recording runs only)."""
    mod, qual = name.split(":")
    obj = _import(mod)
    for part in qual.split("."):
        obj = getattr(obj, part)
    return obj


_suites = {}


def calls(suite):
    """The shared ``Calls`` of `suite` (one per process, so that a recording run writes every test's calls)."""
    if suite not in _suites:
        _suites[suite] = Calls(suite)
    return _suites[suite]
