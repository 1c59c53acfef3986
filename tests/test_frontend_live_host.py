"""The host half of the live-input front end against the compiled reference (oracle/_ref/libjref.so), without a device:
the frame count of a segment (jamd_frontend_live_frames() against the reference's own cyclic buffers driven by
tests/frontendliveref.py), and the -cmnload / -cmnsave file (csrc/cmn_file.h against CMN_load_from_file() /
CMN_save_to_file()), whose reader is also built as a stand-alone program under the host sanitizers."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import frontendliveref as L
from frontendref import RefFrontend, same
from julius_amd import lib

FS, SH = 400, 160
KINDS = (("MFCC", 12), ("MFCC_D", 24), ("MFCC_E_D_A_Z", 39))


@pytest.mark.parametrize("delwin,accwin", [(2, 2), (3, 1)])
@pytest.mark.parametrize("kind,vecsize", KINDS)
@pytest.mark.parametrize("splice", [1, 3])
def test_frame_count_is_the_reference_loops(ref, kind, vecsize, delwin, accwin, splice):
    """Every n from 0 to framesize + 1 + 12 * frameshift: the rows the reference's window loop and flush loop store."""
    v = RefFrontend(ref).para(lib.param_kind(kind), vecsize, delWin=delwin, accWin=accwin, framesize=FS, frameshift=SH)
    d = lib.Frontend.desc_for(kind, vecsize, delWin=delwin, accWin=accwin, framesize=FS, frameshift=SH, splice=splice)
    fn = lib.load().jamd_frontend_live_frames
    bad = [(n, fn(C.byref(d), n), L.live_frames(ref, v, splice, n)) for n in range(FS + 1 + 12 * SH + 1)]
    bad = [b for b in bad if b[1] != b[2]]
    assert not bad, f"(n, library, reference) {bad[:6]}"
    assert fn(C.byref(d), FS + 1 + 12 * SH) == 13 - (splice - 1)   # the sweep reached segments that emit


def test_one_frame_fewer_than_the_buffered_front_end():
    """A file of exactly framesize + k * frameshift samples: the live window is one sample longer."""
    d = lib.Frontend.desc_for("MFCC_E_D_A_Z", 39, framesize=FS, frameshift=SH)
    l = lib.load()
    for k in (4, 9, 40):
        n = FS + k * SH
        assert l.jamd_frontend_frames(C.byref(d), n) == k + 1
        assert l.jamd_frontend_live_frames(C.byref(d), n) == k
        assert l.jamd_frontend_live_frames(C.byref(d), n + 1) == k + 1
    assert l.jamd_frontend_live_frames(None, 100) == -1


def _cmnwork(ref, v):
    L._bind(ref.lib)
    return ref.lib.CMN_realtime_new(C.byref(v), 100.0, 1)


def _ref_load(ref, v, path):
    """CMN_load_from_file() -> (mean, variance or None) or None where it refuses."""
    c = _cmnwork(ref, v)
    V = v.veclen
    if c.contents.var:                           # (malloc()ed, not cleared: a file without a variance leaves it alone)
        C.memset(c.contents.cvar_init, 0, 4 * V)
    ok = ref.lib.CMN_load_from_file(c, str(path).encode())
    out = None
    if ok:
        out = (L._vec(c.contents.cmean_init, V), L._vec(c.contents.cvar_init, V) if c.contents.var else None)
    ref.lib.CMN_realtime_free(c)
    return out


@pytest.mark.parametrize("cvn", [0, 1])
def test_cmn_write_is_byte_identical(ref, tmp_path, cvn):
    v = RefFrontend(ref).para(lib.param_kind("MFCC_E_D_A_Z"), 39, cvn=cvn)
    rng = np.random.default_rng(5)
    cm = (rng.normal(0, 7, 39) * 10.0 ** rng.integers(-12, 9, 39)).astype(np.float32)
    cm[3], cm[4] = 0.0, -0.0
    cv = (np.abs(rng.normal(0, 3, 39)) * 10.0 ** rng.integers(-6, 6, 39)).astype(np.float32)
    c = _cmnwork(ref, v)
    C.memmove(c.contents.cmean_init, cm.ctypes.data, 4 * 39)
    if cvn:
        C.memmove(c.contents.cvar_init, cv.ctypes.data, 4 * 39)
    assert ref.lib.CMN_save_to_file(c, str(tmp_path / "ref.cmn").encode())
    ref.lib.CMN_realtime_free(c)
    lib.cmn_write(tmp_path / "got.cmn", cm, cv if cvn else None)
    assert (tmp_path / "got.cmn").read_bytes() == (tmp_path / "ref.cmn").read_bytes()
    # and read back as the reference reads it
    want = _ref_load(ref, v, tmp_path / "ref.cmn")
    got = lib.cmn_read(tmp_path / "got.cmn", 39, 13, want_var=bool(cvn))
    assert same(got[0], want[0]) and (not cvn or same(got[1], want[1]))
    assert (got[1] is None) == (not cvn)


def test_cmn_read_forms_and_refusals(ref, tmp_path):
    fe = RefFrontend(ref)
    kind = lib.param_kind("MFCC_E_0_D_A_Z")        # vecsize 42: 12 cepstra, c0 and energy, three blocks
    v = fe.para(kind, 42, cvn=1)
    V, M = v.veclen, v.mfcc_dim + 1
    assert (V, M) == (42, 13)
    rng = np.random.default_rng(9)
    vals = lambda n: " ".join(f"{x:.7e}" for x in rng.normal(0, 5, n))
    # a <MEAN> of mfcc_dim + c0 entries
    p = tmp_path / "short.cmn"
    p.write_text(f"<CEPSNORM> <MFCC_E_0_D_A_Z>\n<MEAN> {M}\n {vals(M)}\n")
    want = _ref_load(ref, v, p)
    got = lib.cmn_read(p, V, M, want_var=True)
    assert want is not None and same(got[0], want[0]) and got[1] is None and not got[0][M:].any() and got[0][:M].all()
    # full mean and variance over several lines, lower-case header
    p = tmp_path / "full.cmn"
    p.write_text(f"<cepsnorm> <>\n<MEAN> {V}\n {vals(20)}\n{vals(22)}\n<VARIANCE> {V}\n{vals(42)}\n")
    want = _ref_load(ref, v, p)
    got = lib.cmn_read(p, V, M, want_var=True)
    assert same(got[0], want[0]) and same(got[1], want[1])
    # the binary form (big-endian)
    cm, cv = rng.normal(0, 5, V).astype(np.float32), np.abs(rng.normal(1, 5, V)).astype(np.float32)
    p = tmp_path / "old.bin"
    p.write_bytes(struct.pack(">i", V) + cm.astype(">f4").tobytes() + cv.astype(">f4").tobytes())
    want = _ref_load(ref, v, p)
    got = lib.cmn_read(p, V, M, want_var=True)
    assert same(want[0], cm) and same(got[0], cm) and same(got[1], want[1]) and same(got[1], cv)
    v0 = fe.para(kind, 42, cvn=0)
    assert same(_ref_load(ref, v0, p)[0], cm) and lib.cmn_read(p, V, M, want_var=False)[1] is None
    # refused by both: a wrong dimension (ASCII and binary), a truncated variance block, a truncated binary variance
    bad = {"dim.cmn": f"<CEPSNORM> <>\n<MEAN> {V - 1}\n {vals(V - 1)}\n".encode(),
           "dim.bin": struct.pack(">i", V + 1) + bytes(4 * (V + 1)),
           "truncvar.cmn": f"<CEPSNORM> <>\n<MEAN> {V}\n {vals(V)}\n<VARIANCE> {V}\n {vals(V - 5)}\n".encode(),
           "truncmean.cmn": f"<CEPSNORM> <>\n<MEAN> {V}\n {vals(V - 1)}\n".encode(),
           "truncvar.bin": struct.pack(">i", V) + bytes(4 * V + 4 * (V - 1))}
    for name, body in bad.items():
        (tmp_path / name).write_bytes(body)
        assert _ref_load(ref, v, tmp_path / name) is None, name
        with pytest.raises(lib.JamdError):
            lib.cmn_read(tmp_path / name, V, M, want_var=True)
    with pytest.raises(lib.JamdError):
        lib.cmn_read(tmp_path / "missing", V, M)


def test_file_reader_and_writer_under_sanitizers(tmp_path):
    """tests/cmn_file_check.cpp (its own main over csrc/cmn_file.h) built with -fsanitize=address,undefined, the
    runtimes linked statically, run as a child process: every case as expected and no report."""
    exe = tmp_path / "cmn_file_check"
    root = lib._PKG.parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    str(root / "tests" / "cmn_file_check.cpp"), "-o", str(exe)], check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") >= 20 and "Sanitizer" not in r.stderr
