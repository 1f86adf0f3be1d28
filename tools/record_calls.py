"""Record the ordered C-ABI calls of a workload: the A/B instrument of a refactor that may change no launch.

    python tools/record_calls.py WORKLOAD.py --run NAME --out FILE.jsonl        one line per configuration of the workload
    python tools/record_calls.py --summary PARENT_A.jsonl PARENT_B.jsonl HEAD.jsonl >> FILE.jsonl

Inside `with Recorder() as rec:` every `mgf_*` function of `_lib.lib()` is wrapped: the name and every non-pointer argument are logged
(a pointer as null / ptr, a struct by field, a ctypes array by element), with the number of torch ops since the previous call (a
TorchDispatchMode; view ops left out).  `rec.summary()` hashes the ordered list.  WORKLOAD.py defines `configs()` -> [(name, fn)];
`fn(Recorder)` runs what it wants recorded under a Recorder and returns {"recorder": rec, ...its own result fields (hashes, counts)}.
Plain Python, nothing preloaded; code that holds on to the library handle across calls is not seen.
"""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.environ.get("MGF_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphganformer_amd import _lib                                                   # noqa: E402


def _describe(arg):
    if arg is None:
        return "null"
    if isinstance(arg, C.Structure):
        return {name: _describe(getattr(arg, name)) for name, _ in arg._fields_}
    if isinstance(arg, C.Array):
        return [_describe(v) for v in arg]
    if hasattr(arg, "_obj"):                                     # byref(x)
        return _describe(arg._obj)
    if isinstance(arg, C._Pointer):
        return _describe(arg.contents) if arg else "null"
    if isinstance(arg, C._SimpleCData):
        return _describe(arg.value)
    if isinstance(arg, float):
        return repr(arg)
    return arg if isinstance(arg, (int, str)) else repr(arg)


def _pointer_type(typ):
    return typ in (C.c_void_p, C.c_char_p) or (isinstance(typ, type) and issubclass(typ, C._Pointer))


def _describe_arg(arg, typ):
    if isinstance(arg, int) and _pointer_type(typ):
        return "ptr" if arg else "null"
    if isinstance(arg, C.Structure):                             # pointer fields of a struct: by their declared type
        return {name: _describe_arg(getattr(arg, name), t) for name, t in arg._fields_}
    if hasattr(arg, "_obj") and isinstance(arg._obj, C.Structure):
        return _describe_arg(arg._obj, None)
    if isinstance(arg, C.Array) and arg._type_ is C.c_void_p:
        return ["ptr" if v else "null" for v in arg]
    if typ is C.c_float and isinstance(arg, (int, float)):
        return repr(C.c_float(arg).value)
    return _describe(arg)


def _is_view(func):
    return any(r.alias_info is not None and not r.alias_info.is_write for r in func._schema.returns)


class _Proxy:
    def __init__(self, handle, rec):
        self._handle, self._rec = handle, rec

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith("mgf_"):
            return fn
        rec = self._rec

        def call(*args):
            rec.calls.append((len(rec.gap), name, [_describe_arg(a, t) for a, t in zip(args, fn.argtypes or [None] * len(args))]))
            rec.gaps.append(sorted(rec.gap))
            rec.gap = []
            return fn(*args)
        return call


class Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.calls, self.gaps, self.gap = [], [], []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not _is_view(func):
            self.gap.append(str(func))
        return func(*args, **(kwargs or {}))

    def __enter__(self):
        self._handle = _lib.lib()
        _lib._lib = _Proxy(self._handle, self)
        return super().__enter__()

    def __exit__(self, *exc):
        _lib._lib = self._handle
        return super().__exit__(*exc)

    def summary(self):
        sha = lambda o: hashlib.sha256(json.dumps(o, sort_keys=True).encode()).hexdigest()[:16]
        return {"n_mgf_calls": len(self.calls), "n_torch_ops": sum(len(g) for g in self.gaps) + len(self.gap),
                "calls_sha256": sha(self.calls), "torch_ops_sha256": sha(self.gaps + [sorted(self.gap)])}


def _leaves(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _leaves(v, f"{prefix}{k}.")
        else:
            yield prefix + k, v


def summarise(parent_a, parent_b, head):
    """One summary line per configuration: the call list of the head against the parent's, and every result field on which the parent's two
    runs agree against the head's."""
    runs = [{r["config"]: r for r in map(json.loads, open(p))} for p in (parent_a, parent_b, head)]
    # (graph_kernel_nodes, where a workload reports it, counts launches: it belongs to the call list, not to the results)
    call_keys = ("n_mgf_calls", "n_torch_ops", "calls_sha256", "torch_ops_sha256", "graph_kernel_nodes")
    skip = call_keys + ("config", "run", "variant")
    for cfg, a in runs[0].items():
        b, h = runs[1][cfg], runs[2][cfg]
        la, lb, lh = (dict(x for x in _leaves(r) if x[0] not in skip) for r in (a, b, h))
        differs = sorted(k for k in la if la[k] != lb.get(k))
        line = {"config": cfg, "summary": True, "calls_identical": all(a.get(k) == b.get(k) == h.get(k) for k in call_keys),
                "parent_reproducible": not differs,
                "results_bit_identical": set(lh) == set(la) and all(lh[k] == la[k] for k in la if k not in differs)}
        if differs:
            line["parent_differs_in"] = differs
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("workload", nargs="?", help="a Python file that defines configs() -> [(name, fn(Recorder))]")
    ap.add_argument("--run", default="head", help="the run's name in every line (parentA, parentB, head)")
    ap.add_argument("--out", default=None, help="append the lines to this file (default: print them)")
    ap.add_argument("--only", default=None, help="run the configurations whose name contains this")
    ap.add_argument("--summary", nargs=3, metavar=("PARENT_A", "PARENT_B", "HEAD"), help="compare three recorded runs")
    args = ap.parse_args()
    if args.summary:
        return summarise(*args.summary)
    spec = importlib.util.spec_from_file_location("workload", args.workload)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name, fn in mod.configs():
        if args.only and args.only not in name:
            continue
        res = fn(Recorder)
        line = json.dumps({"config": name, **res.pop("recorder").summary(), **res, "variant": args.run.rstrip("AB"), "run": args.run})
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        print(line[:200], flush=True)


if __name__ == "__main__":
    main()
