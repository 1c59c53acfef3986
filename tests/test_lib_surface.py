"""CPU: the public surface of julius_amd.lib -- what tests, tools, smoke() and bench.py reach the library through.

tests/golden/lib_surface.txt lists it as recorded before the binding was put on one kit: public module attributes
plus _PKG, every class's public methods (and __init__, and Frontend._pack) with parameter names, kinds and defaults,
and the field names of every struct mirror.  The module must offer at least that, with identical signatures."""
import ctypes as C
import inspect
import types
from pathlib import Path

from julius_amd import lexblob, lib

GOLDEN = Path(__file__).parent / "golden" / "lib_surface.txt"


def _sig(f):
    s = inspect.signature(f)
    return str(s.replace(parameters=[p.replace(annotation=p.empty) for p in s.parameters.values()],
                         return_annotation=s.empty))


def _members(cls):
    own = [k for k in cls.__mro__ if k.__module__ == cls.__module__]
    names = sorted({m for k in own for m in vars(k)})
    for m in names:
        if m.startswith("_") and m != "__init__" and (cls.__name__, m) != ("Frontend", "_pack"):
            continue
        raw = inspect.getattr_static(cls, m)
        if m == "_pack":         # now an alias of pack_chunks(chunks): positional use only, so its arity is what is kept
            yield f"{type(raw).__name__} {m}/{len(inspect.signature(raw.__func__).parameters)}"
        elif isinstance(raw, (staticmethod, classmethod)):
            yield f"{type(raw).__name__} {m}{_sig(raw.__func__)}"
        elif inspect.isfunction(raw):
            yield f"method {m}{_sig(raw)}"
        elif not hasattr(raw, "__get__"):
            yield f"attribute {m}"


def surface_lines():
    out = []
    for name, v in sorted(vars(lib).items()):
        if (name.startswith("_") and name != "_PKG") or isinstance(v, types.ModuleType) or name == "annotations":
            continue
        if (inspect.isclass(v) or inspect.isfunction(v)) and v.__module__ != lib.__name__:
            continue
        if inspect.isfunction(v):
            out.append(f"function {name}{_sig(v)}")
        elif inspect.isclass(v):
            out.append(f"class {name}")
            out += [f"{name}: {line}" for line in _members(v)]
        else:
            out.append(f"attribute {name}")
    for mod in (lib, lexblob):
        for name, v in sorted(vars(mod).items()):
            if inspect.isclass(v) and issubclass(v, C.Structure) and v is not C.Structure:
                out.append(f"struct {mod.__name__}.{name}: " + " ".join(f[0] for f in v._fields_))
    return out


def test_surface_is_kept():
    want = GOLDEN.read_text().splitlines()
    assert len(want) > 150
    have = set(surface_lines())
    missing = [line for line in want if line not in have]
    assert not missing, "julius_amd.lib no longer offers:\n" + "\n".join(missing)


def test_constants_keep_their_values():
    assert (lib.GPRUNE_NONE, lib.GPRUNE_SAFE, lib.GPRUNE_HEU, lib.GPRUNE_BEAM) == (0, 1, 2, 3)
    assert (lib.IWCD_MAX, lib.IWCD_AVG, lib.IWCD_NBEST) == (0, 1, 2)
    assert (lib.SS_OFF, lib.SS_CALC, lib.SS_LOAD) == (0, 1, 2)
    assert (lib.LIVE_CMEAN_SET, lib.LIVE_LOADED, lib.ADIN_DS, lib.ADIN_ZMEAN) == (1, 2, 1, 2)
    assert (lib.FVAD_MODEL_INTS, lib.FVAD_STATE_INTS, lib.LOG_ZERO) == (130, 266, -1000000.0)
    assert lib._PKG == Path(lib.__file__).resolve().parent
