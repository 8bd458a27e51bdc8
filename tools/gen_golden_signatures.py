"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/context_signatures.json: ``str(inspect.signature(...))`` of every public callable of
``beat_amd.engine.Context`` and of every public function and public method defined in ``beat_amd.summary``,
``beat_amd.covariance``, ``beat_amd.discretization`` and ``beat_amd.ffi`` -- the modules that hand host arrays to the
device.  Run it on the commit whose interface is to be kept; tests/test_signatures_host.py compares the tree with it.

    python tools/gen_golden_signatures.py
"""
import importlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODULES = ("summary", "covariance", "discretization", "ffi")


def _callables(owner):
    return {name: str(inspect.signature(fn)) for name, fn in inspect.getmembers(owner, callable)
            if not name.startswith("_") and (inspect.isfunction(fn) or inspect.ismethod(fn))}


def signatures():
    from beat_amd import engine
    out = {"engine.Context": _callables(engine.Context)}
    for mod in MODULES:
        m = importlib.import_module("beat_amd." + mod)
        own = {name: obj for name, obj in vars(m).items()
               if not name.startswith("_") and getattr(obj, "__module__", None) == m.__name__}
        out[mod] = {name: str(inspect.signature(fn)) for name, fn in own.items() if inspect.isfunction(fn)}
        for name, cls in own.items():
            if inspect.isclass(cls):
                out["%s.%s" % (mod, name)] = _callables(cls)
    return out


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "context_signatures.json")
    with open(path, "w") as fh:
        json.dump(signatures(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s: %s" % (path, {k: len(v) for k, v in signatures().items()}))
