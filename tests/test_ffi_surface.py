"""CPU: the surface of the Python binding and of the planners is what tests/golden/ffi_surface.json recorded before the binding
was rewritten around one signature table: the ctypes prototype of every C symbol, the public names of _ffi and of its classes,
and the signature of every public callable.  (No compute calls: the library is loaded, never run.)"""
import ctypes as C
import inspect
import json
import os

from rrtplanner_amd import _ffi, dubins, rrt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffi_surface.json")
PLANNERS = (rrt.RRT, rrt.RRTStandard, rrt.RRTStar, rrt.RRTStarInformed, dubins.RRTDubins, dubins.RRTStarDubins)


def _public(obj):
    return sorted(k for k in dir(obj) if not k.startswith("_"))


def _signatures(obj):
    """{public name: signature} of the callables of a class or module that have one; "property" for a property"""
    out = {}
    for k in _public(obj):
        v = inspect.getattr_static(obj, k)
        if isinstance(v, property):
            out[k] = "property"
        elif isinstance(v, (staticmethod, classmethod)) or inspect.isfunction(v):
            out[k] = str(inspect.signature(getattr(obj, k)))
    return out


def _ctype(t):
    """repr(t), with pointer and array classes spelled by what they point to and hold: ctypes caches those classes for the whole
    process, and the module their repr names is that of whichever caller asked for them first, so it changes with the import order"""
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return f"POINTER({_ctype(t._type_)})"
    if isinstance(t, type) and issubclass(t, C.Array):
        return f"{_ctype(t._type_)} * {t._length_}"
    return repr(t)


def surface():
    L = _ffi.lib()
    symbols = {s: {"argtypes": [_ctype(t) for t in getattr(L, s).argtypes], "restype": _ctype(getattr(L, s).restype)} for s in sorted(_ffi.SYMBOLS)}
    ffi = {name: {"names": _public(obj), "signatures": _signatures(obj)}
           for name, obj in (("Context", _ffi.Context), ("Batch", _ffi.Batch), ("DeviceTree", _ffi.DeviceTree), ("module", _ffi))}
    return {"symbols": symbols, "ffi": ffi, "planners": {cls.__name__: _signatures(cls) for cls in PLANNERS}}


def test_surface_is_the_recorded_one():
    want = json.load(open(GOLDEN))
    got = surface()
    assert sorted(got) == sorted(want)
    for part in want:
        assert sorted(got[part]) == sorted(want[part]), part
        for name in want[part]:
            assert got[part][name] == want[part][name], (part, name)
