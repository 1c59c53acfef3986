"""CPU: the C-ABI library loads and exports every symbol include/*.h declares;
no compute calls (there is no GPU here).  Also: no fallback -- engine creation
must FAIL loudly without a device."""
import subprocess
import sys

import pytest

from julius_amd import lib


def test_library_loads_and_exports_declared_symbols():
    l = lib.load()
    missing = [s for s in lib.declared_symbols() if not hasattr(l, s)]
    assert not missing, f"declared in include/julius_amd.h but not exported: {missing}"
    assert l.jamd_abi_version() == 4


def test_signature_table_names_every_declared_function():
    """Every function of the header has its restype / argtypes: one called without them would pass pointers as C int."""
    assert sorted(lib.SIGNATURES) == lib.declared_symbols()


def _header_param_counts():
    import re
    hdr = (lib._PKG.parent / "include" / "julius_amd.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    counts = {}
    for name, params in re.findall(r"\b(jamd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        params = params.strip()
        assert name not in counts, f"{name} is declared twice"
        counts[name] = 0 if params in ("", "void") else len(params.split(","))
    return counts


def test_signature_table_has_the_headers_parameter_counts():
    counts = _header_param_counts()
    assert sorted(counts) == lib.declared_symbols()
    wrong = {n: (len(args), counts[n]) for n, (_, args) in lib.SIGNATURES.items() if len(args) != counts[n]}
    assert not wrong, f"argtypes / header parameters: {wrong}"


def _mirrors():
    from julius_amd import lexblob
    return {"jamd_gmm_desc": lib.GmmDesc, "jamd_gmm_ms_desc": lib.GmmStreamsDesc, "jamd_dnn_desc": lib.DnnDesc,
            "jamd_lexicon_desc": lexblob.LexiconDesc, "jamd_trellis_atom": lexblob.TrellisAtom,
            "jamd_pass1_result": lib.Pass1Result, "jamd_frontend_desc": lib.FrontendDesc,
            "jamd_frontend_ss": lib.FrontendSS, "jamd_frontend_live_desc": lib.FrontendLiveDesc,
            "jamd_adin_desc": lib.AdinDesc, "jamd_adin_cut_desc": lib.AdinCutDesc, "jamd_fvad_model": lib.FvadModel,
            "jamd_fvad_desc": lib.FvadDesc, "jamd_adin_cut_fvad": lib.AdinCutFvad}


def test_struct_mirrors_have_the_headers_layout(tmp_path):
    """sizeof and every field's offsetof and size, as gcc lays the header's structs out, against the ctypes mirrors."""
    import ctypes as C
    from julius_amd import lexblob
    mirrors = _mirrors()
    structs = [v for m in (lib, lexblob) for v in vars(m).values()
               if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    assert len(mirrors) == 14 and set(mirrors.values()) == set(structs), "a struct mirror is not checked"
    body, want = [], []
    for ctype, cls in mirrors.items():
        body.append(f'  printf("{ctype} %zu\\n", sizeof({ctype}));')
        want.append(f"{ctype} {C.sizeof(cls)}")
        for f, _ in cls._fields_:
            body.append(f'  printf("{ctype}.{f} %zu %zu\\n", offsetof({ctype}, {f}), sizeof((({ctype} *)0)->{f}));')
            want.append(f"{ctype}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "julius_amd.h"\nint main(void) {\n'
                   + "\n".join(body) + "\n  return 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(lib._PKG.parent / "include"),
                    str(src), "-o", str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]


def test_atom_dtype_is_the_trellis_atom():
    import ctypes as C
    from julius_amd import lexblob
    dt, atom = lexblob.ATOM_DTYPE, lexblob.TrellisAtom
    assert list(dt.names) == [f for f, _ in atom._fields_]
    assert dt.itemsize == C.sizeof(atom)
    for f, ctype in atom._fields_:
        sub, off = dt.fields[f][:2]
        assert (off, sub.itemsize) == (getattr(atom, f).offset, getattr(atom, f).size), f
        assert sub.kind == ("f" if ctype is C.c_float else "i"), f


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "julius_amd.h"\nint main(void){return JAMD_ABI_VERSION-1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(lib._PKG.parent / "include"),
                    str(src), "-o", str(tmp_path / "t")], check=True)


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(lib.JamdError):
        lib.Engine(0)


def test_product_does_not_import_oracle():
    """Nothing under julius_amd/ or include/ may reference oracle/."""
    import re
    from pathlib import Path
    root = lib._PKG
    bad = []
    for p in list(root.rglob("*.py")) + list(root.rglob("*.hip")) + list(root.rglob("*.h")) + list(root.rglob("*.c")):
        txt = p.read_text()
        if re.search(r"(from|import)\s+oracle|liboracle|libjref|jamd_oracle", txt):
            bad.append(str(p))
    assert not bad, bad


def test_standalone_driver_is_plain_c(tmp_path):
    """julius_amd/host/jamd_batch.c compiles as C99 against the public header alone."""
    src = lib._PKG / "host" / "jamd_batch.c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(lib._PKG.parent / "include"),
                    "-c", str(src), "-o", str(tmp_path / "b.o")], check=True)


def test_unknown_lexicon_flags_are_refused():
    """jamd_lexicon_create() refuses lm_type bits it does not know; the check comes before any device call,
    so a placeholder engine handle is enough here."""
    import ctypes as C
    import sys
    sys.path.insert(0, str(lib._PKG.parent / "tests"))
    from beamutil import load_beam_golden
    from julius_amd import lexblob
    lex = load_beam_golden("beam_multipath.npz")["lex"]
    assert lex["lm_type"] == 0x100
    d, keep = lexblob.make_desc(lex)
    fake_engine = C.create_string_buffer(256)
    h = C.c_void_p()
    L = lib.load()
    d.lm_type = 0x200                                                                                # unknown flag bits
    assert L.jamd_lexicon_create(C.cast(fake_engine, C.c_void_p), C.byref(d), C.byref(h)) == -1     # JAMD_EINVAL
    assert not h.value
