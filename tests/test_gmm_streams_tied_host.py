"""CPU: the host layer of jamd_gmm_ms_create_opt() / jamd_gmm_ms_load_binhmm_opt() -- what they refuse and what the
binary HMM reader takes of a tied-mixture multi-stream model -- without a device.  Every refusal comes before the first
device call, so a placeholder engine handle is enough (as tests/test_gmm_streams_host.py); a description that passes
every check fails only where the device is selected (JAMD_ENODEV), or, on a machine that has one, is created."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import streamstied as st  # noqa: E402
from julius_amd import lib  # noqa: E402

EINVAL, ENODEV = -1, -2
Opt = lib.GmmStreamsTied.Opt


def _fake_engine():
    return C.create_string_buffer(256)


def _create(model, opt=(lib.GPRUNE_NONE, 0, 0)):
    L = lib.load()
    d, keep = lib.GmmStreams.make_desc(model)
    eng, h = _fake_engine(), C.c_void_p()
    o = Opt(*opt) if opt is not None else None
    rc = L.jamd_gmm_ms_create_opt(C.cast(eng, C.c_void_p), C.byref(d), C.byref(o) if o is not None else None, C.byref(h))
    msg = L.jamd_last_error().decode()
    if h.value:
        L.jamd_gmm_ms_destroy(h)
    return rc, msg


def _good():
    """5 states over 26 + 13, book 0 (6 members) on stream 0 and book 1 (5 members) on stream 1."""
    return st.load_case("lay_26_13")["model"]


def _with(key, fn):
    m = dict(_good())
    m[key] = fn(np.array(m[key], copy=True), m)
    return m


def _put(a, idx, v):
    a[idx] = v
    return a


def _wrong_length(a, m):
    """member 2 of book 0 (in every pdf of the book, so the lists still agree) is a density of stream 1"""
    other = a[m["pdf_off"][1]]
    for p in np.nonzero(m["pdf_book"] == 0)[0]:
        a[m["pdf_off"][p] + 2] = other
    return a


# id -> (description, options, what the message must say)
REFUSALS = {
    "sparse_book_ids": (lambda: _with("pdf_book", lambda a, m: np.where(a == 1, 3, a)), (0, 0, 0),
                        r"pdf_book: codebook ids are not dense \(no pdf names book 1 of 0 \.\. 3\)"),
    "book_id_beyond_the_pdfs": (lambda: _with("pdf_book", lambda a, m: _put(a, 0, 1000)), (0, 0, 0),
                                r"pdf_book: codebook ids are not dense \(1000 is named"),
    "ent_dens_differs_in_a_book": (lambda: _with("ent_dens", lambda a, m: _put(a, m["pdf_off"][2] + 1, a[m["pdf_off"][2]])),
                                   (0, 0, 0), r"ent_dens: pdfs 0 and 2 of codebook 0 do not list the same densities"),
    "book_spans_two_streams": (lambda: _with("pdf_book", lambda a, m: _put(a, 1, 0)), (0, 0, 0),
                               r"pdf_stream: codebook 0 spans streams 0 \(pdf 0\) and 1 \(pdf 1\)"),
    "member_of_the_wrong_length": (lambda: _with("ent_dens", _wrong_length), (0, 0, 0),
                                   r"density \d+ has length 13, the vsize of stream 0 \(pdf 0\) is 26"),
    "gprune_heu": (_good, (lib.GPRUNE_HEU, 2, 0), r"gprune heu is not served"),
    "gprune_beam": (_good, (lib.GPRUNE_BEAM, 2, 0), r"gprune beam is not served"),
    "gprune_unknown": (_good, (7, 2, 0), r"gprune=7"),
    "gprune_num_0": (_good, (lib.GPRUNE_SAFE, 0, 0), r"gprune safe needs gprune_num >= 1"),
    "gprune_num_65": (_good, (lib.GPRUNE_SAFE, 65, 0), r"gprune_num 65 > 64"),
    "chunk_frames_negative": (_good, (lib.GPRUNE_SAFE, 2, -1), r"chunk_frames=-1"),
    "opt_null": (_good, None, r"opt is NULL"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_create_opt_refuses_before_any_device_call(name):
    make, opt, pattern = REFUSALS[name]
    rc, msg = _create(make(), opt)
    assert rc == EINVAL
    assert msg.startswith("jamd_gmm_ms_create_opt: ") and re.search(pattern, msg), msg


@pytest.mark.parametrize("opt", [(lib.GPRUNE_NONE, 0, 0), (lib.GPRUNE_NONE, 99, 0), (lib.GPRUNE_SAFE, 1, 0),
                                 (lib.GPRUNE_SAFE, 64, 128)])
@pytest.mark.parametrize("name", ["lay_26_13", "branches", "compound", "K130", "one_stream"])
def test_good_tied_description_passes_every_check(name, opt):
    """(gprune_num is ignored under none.)  Fails before this pull request: the symbol does not exist."""
    rc, msg = _create(st.load_case(name)["model"], opt)
    assert rc in (0, ENODEV), msg


def test_old_refusals_keep_their_text_under_the_new_name():
    """What jamd_gmm_ms_create() refuses the new entry refuses too, in the same words."""
    rc, msg = _create(_with("vsize", lambda a, m: _put(a, 1, a[1] + 1)))
    assert rc == EINVAL and msg == "jamd_gmm_ms_create_opt: vsize sums to 40, veclen is 39"


@pytest.mark.parametrize("name", ["lay_26_13", "branches", "compound"])
def test_old_entry_still_refuses_a_tied_pdf(name):
    L = lib.load()
    d, keep = lib.GmmStreams.make_desc(st.load_case(name)["model"])
    eng, h = _fake_engine(), C.c_void_p()
    assert L.jamd_gmm_ms_create(C.cast(eng, C.c_void_p), C.byref(d), C.byref(h)) == EINVAL
    assert re.match(r"jamd_gmm_ms_create: pdf \d+ is a tied-mixture pdf \(pdf_book=\d+\)", L.jamd_last_error().decode())


def _load(path, opt=(lib.GPRUNE_SAFE, 2, 0), old=False):
    L = lib.load()
    eng, h = _fake_engine(), C.c_void_p()
    if old:
        rc = L.jamd_gmm_ms_load_binhmm(C.cast(eng, C.c_void_p), str(path).encode(), C.byref(h))
    else:
        o = Opt(*opt) if opt is not None else None
        rc = L.jamd_gmm_ms_load_binhmm_opt(C.cast(eng, C.c_void_p), str(path).encode(), C.byref(o) if o is not None else None,
                                           C.byref(h))
    msg = L.jamd_last_error().decode()
    if h.value:
        L.jamd_gmm_ms_destroy(h)
    return rc, msg


@pytest.mark.parametrize("name", ["branches", "compound"])
def test_reader_takes_tied_multi_stream_binhmm_and_refuses_damaged_ones(tmp_path, name):
    """The committed mkbinhmm files (codebook section, tmix pdfs, a NULL member, plain pdfs beside tied ones) parse
    and pass every check under both modes; cut short before the HMM section they are refused, never read past; the
    entry without options keeps refusing them by the tied pdf."""
    path = st.load_binhmm(name, tmp_path / "binhmm")
    for opt in ((lib.GPRUNE_NONE, 0, 0), (lib.GPRUNE_SAFE, 2, 0)):
        rc, msg = _load(path, opt)
        assert rc in (0, ENODEV), msg
    raw = path.read_bytes()
    for k in range(1, 7):
        (tmp_path / "cut").write_bytes(raw[:len(raw) * k // 8])
        rc, msg = _load(tmp_path / "cut")
        assert rc == EINVAL, (k, msg)
    assert _load(tmp_path / "absent")[0] == EINVAL
    rc, msg = _load(path, None)
    assert rc == EINVAL and msg == "jamd_gmm_ms_load_binhmm_opt: opt is NULL"
    rc, msg = _load(path, (lib.GPRUNE_BEAM, 2, 0))
    assert rc == EINVAL and "gprune beam" in msg
    rc, msg = _load(path, old=True)
    assert rc == EINVAL and "is a tied-mixture pdf" in msg, msg


def test_option_struct_has_the_headers_layout(tmp_path):
    """sizeof and every field's offsetof and size of jamd_gmm_ms_opt, as gcc lays it out, against the ctypes mirror."""
    t, want, body = "jamd_gmm_ms_opt", [f"jamd_gmm_ms_opt {C.sizeof(Opt)}"], ['  printf("jamd_gmm_ms_opt %zu\\n", sizeof(jamd_gmm_ms_opt));']
    for f, _ in Opt._fields_:
        body.append(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t} *)0)->{f}));')
        want.append(f"{t}.{f} {getattr(Opt, f).offset} {getattr(Opt, f).size}")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "julius_amd.h"\nint main(void) {\n'
                   + "\n".join(body) + "\n  return 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(lib._PKG.parent / "include"),
                    str(src), "-o", str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == want
