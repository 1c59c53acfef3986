"""Host half of the audio front end (csrc/frontend_tables.h behind csrc/frontend_api.hip) against the compiled
reference: the descriptor defaults, the HTK config parser, every table WMP_work_new() builds, and the frame count; and
that header as a stand-alone program under the host sanitizers.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from julius_amd import lib
from frontendref import DESC_FIELDS, EDGE_GEOMETRY, EDGE_TABLES, RefFrontend

KINDS = [("MFCC_E_D_A_Z", 39), ("MFCC_E_D_N_Z", 25), ("MFCC_E_D_A", 39), ("MFCC_0_D_A_Z", 39), ("MFCC_E_Z", 13),
         ("MFCC_0_E_D_A", 42), ("MFCC_E_D_A_Z", 36), ("FBANK_D_A_Z", 72), ("MELSPEC", 24), ("FBANK", 40),
         ("MFCC_E_D_N", 38)]


@pytest.fixture(scope="module")
def rf(ref):
    return RefFrontend(ref)


def _desc(kind, vecsize, htkconf=None, **fields):
    return lib.Frontend.desc_for(kind, vecsize, htkconf=htkconf, **fields)


def _same_fields(d, v):
    bad = [(k, getattr(d, k), getattr(v, k)) for k in DESC_FIELDS
           if np.float32(getattr(d, k)).tobytes() != np.float32(getattr(v, k)).tobytes()
           and getattr(d, k) != getattr(v, k)]
    return bad


@pytest.mark.parametrize("kind,vecsize", KINDS)
def test_defaults_match_reference(rf, kind, vecsize):
    d = _desc(kind, vecsize)
    v = rf.para(lib.param_kind(kind), vecsize)
    assert _same_fields(d, v) == []
    assert d.splice == 1 and d.ss == 0 and d.realtime == 0


CONFIGS = {
    "htk16k": "# a comment\nSOURCERATE = 625\nTARGETKIND = MFCC_E_D_A_Z\nTARGETRATE = 100000.0\nWINDOWSIZE = 250000.0\n"
              "USEHAMMING = T\nPREEMCOEF = 0.97\nNUMCHANS = 24\nCEPLIFTER = 22\nNUMCEPS = 12\nENORMALISE = F\n",
    "htk8k": "SOURCERATE=1250\nTARGETRATE=100000\nWINDOWSIZE=256000\nNUMCHANS=20\nLOFREQ=64\nHIFREQ=3800\n"
             "RAWENERGY=T\nENORMALISE=T\nESCALE=0.1\nSILFLOOR=40.0\nZMEANSOURCE=T\nUSEPOWER=T\n\n",
    "vtln": "  SOURCERATE =\t625  \r\nWINDOWSIZE = 400000.0\nTARGETRATE = 80000\nWARPFREQ = 1.1\nWARPLCUTOFF = 300\n"
            "WARPUCUTOFF = 6000\nDELTAWINDOW = 3\nACCWINDOW = 1\nCEPLIFTER = 0\nPREEMCOEF = 0.0\n",
    "norate": "WINDOWSIZE = 250000.0\nTARGETRATE = 100000.0\nNUMCHANS = 26\n",
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_htkconf_matches_reference(rf, tmp_path, name):
    p = tmp_path / f"{name}.conf"
    p.write_text(CONFIGS[name])
    d = lib.FrontendDesc()
    assert lib.load().jamd_frontend_default_desc(lib.param_kind("MFCC_E_D_A_Z"), 39, C.byref(d)) == 0
    assert lib.load().jamd_frontend_htkconf(str(p).encode(), C.byref(d)) == 0, lib.load().jamd_last_error()
    v = rf.para(lib.param_kind("MFCC_E_D_A_Z"), 39, htkconf=p)
    assert _same_fields(d, v) == []
    assert (d.vtln_lower, d.vtln_upper) == (v.vtln_lower, v.vtln_upper)


def test_htkconf_refuses_unknown_keys(tmp_path):
    p = tmp_path / "bad.conf"
    p.write_text("SOURCERATE = 625\nSAVECOMPRESSED = T\n")
    d = lib.FrontendDesc()
    assert lib.load().jamd_frontend_default_desc(lib.param_kind("MFCC_E_D_A_Z"), 39, C.byref(d)) == 0
    before = bytes(d)
    assert lib.load().jamd_frontend_htkconf(str(p).encode(), C.byref(d)) == -1
    assert b"SAVECOMPRESSED" in lib.load().jamd_last_error()
    assert bytes(d) == before
    p.write_text("USEHAMMING = F\n")
    assert lib.load().jamd_frontend_htkconf(str(p).encode(), C.byref(d)) == -1


def _table(d, name, dtype):
    n = lib.load().jamd_frontend_table(C.byref(d), name.encode(), None, 0)
    assert n >= 0, lib.load().jamd_last_error()
    a = np.zeros(n, dtype)
    assert lib.load().jamd_frontend_table(C.byref(d), name.encode(), a.ctypes.data, n) == n
    return a


def _arr(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


TABLE_CASES = [
    ("MFCC_E_D_A_Z", 39, {}),
    ("MFCC_E_D_N_Z", 25, {}),
    ("MFCC_0_D_A_Z", 39, dict(lifter=0)),
    ("MFCC_E_D_A_Z", 39, dict(lifter=15, fbank_num=26)),
    ("MFCC_E_D_A_Z", 39, dict(lopass=200, hipass=7000)),
    ("MFCC_E_D_A_Z", 39, dict(lopass=0, hipass=9000)),
    ("MFCC_E_D_A_Z", 39, dict(vtln_alpha=1.08, vtln_lower=250.0, vtln_upper=6500.0)),
    ("MFCC_E_D_A_Z", 39, dict(vtln_alpha=0.9, vtln_lower=200.0, vtln_upper=5000.0, lopass=100, hipass=7600)),
    ("MFCC_E_D_A_Z", 39, dict(smp_period=227, smp_freq=44100, framesize=1102, frameshift=441, fbank_num=40)),
    ("MFCC_E_D_A_Z", 39, dict(smp_period=1250, smp_freq=8000, framesize=200, frameshift=80, fbank_num=20)),
    ("FBANK_D_A_Z", 72, {}),
    ("MELSPEC", 24, dict(usepower=1)),
] + [EDGE_GEOMETRY[k] for k in EDGE_TABLES]   # windows of 16 .. 4096 samples, 4 .. 128 channels, 20 cepstra, clamped bands


@pytest.mark.parametrize("kind,vecsize,fields", TABLE_CASES)
def test_tables_match_reference(rf, kind, vecsize, fields):
    d = _desc(kind, vecsize, **fields)
    v = rf.para(lib.param_kind(kind), vecsize, **fields)
    w = rf.work(v).contents
    try:
        fftN, n, klo, khi = _table(d, "info", np.int32)
        assert (fftN, n, klo, khi) == (w.fb.fftN, w.fb.n, w.fb.klo, w.fb.khi)
        fres, sqrt2var = _table(d, "scalars", np.float32)
        assert fres.tobytes() == np.float32(w.fb.fres).tobytes()
        assert sqrt2var.tobytes() == np.float32(w.sqrt2var).tobytes()
        nv2 = fftN // 2
        maxChan = v.fbank_num + 1
        pairs = [("hamming", np.float64, w.costbl_hamming, w.costbl_hamming_len),
                 ("fft_cos", np.float64, w.costbl_fft, w.tbllen), ("fft_sin", np.float64, w.sintbl_fft, w.tbllen),
                 ("dct", np.float64, w.costbl_makemfcc, w.costbl_makemfcc_len),
                 ("wcep", np.float64, w.sintbl_wcep, w.sintbl_wcep_len)]
        for name, dt, ptr, ln in pairs:
            got = _table(d, name, dt)
            assert np.array_equal(got, _arr(ptr, ln, dt)), name
        # index 0 of the 1-based arrays is never written by the reference
        assert np.array_equal(_table(d, "cf", np.float32)[1:], _arr(w.fb.cf, maxChan + 1, np.float32)[1:])
        assert np.array_equal(_table(d, "lochan", np.int16)[1:], _arr(w.fb.loChan, nv2 + 1, np.int16)[1:])
        assert np.array_equal(_table(d, "lowt", np.float32)[1:], _arr(w.fb.loWt, nv2 + 1, np.float32)[1:])
        # the twiddle sequence of every stage = the serial loop's own recurrence over the reference's tables
        cs, sn = _arr(w.costbl_fft, n, np.float64), _arr(w.sintbl_fft, n, np.float64)
        tre, tim = _table(d, "twiddle_re", np.float64), _table(d, "twiddle_im", np.float64)
        assert len(tre) == fftN - 1
        for m in range(1, n + 1):
            me1 = 1 << (m - 1)
            uRe, uIm = 1.0, 0.0
            for j in range(me1):
                assert tre[me1 - 1 + j] == uRe and tim[me1 - 1 + j] == uIm, (m, j)
                uRe, uIm = uRe * cs[m - 1] - uIm * sn[m - 1], uRe * sn[m - 1] + uIm * cs[m - 1]
    finally:
        rf.lib.WMP_free(C.pointer(w))


def test_vtln_out_of_range_is_refused():
    d = _desc("MFCC_E_D_A_Z", 39, vtln_alpha=1.1, vtln_lower=100.0, vtln_upper=9000.0)
    assert lib.load().jamd_frontend_table(C.byref(d), b"cf", None, 0) == -1
    assert b"VTLN" in lib.load().jamd_last_error()


@pytest.mark.parametrize("n,splice", [(0, 1), (399, 1), (400, 1), (559, 1), (560, 1), (16000, 1), (16000, 3),
                                      (400 + 160 * 2, 3), (400 + 160, 3), (160000 * 6, 1)])
def test_frames(n, splice):
    d = _desc("MFCC_E_D_N_Z", 25, splice=splice)
    want = (n - 400) // 160 + 1 - (splice - 1) if n >= 400 else 1 - splice
    got = lib.load().jamd_frontend_frames(C.byref(d), n)
    assert got == want if want > 0 else got <= 0


def test_tables_parser_and_counts_under_sanitizers(tmp_path):
    """tests/frontend_tables_check.cpp (its own main over csrc/frontend_tables.h, which includes no HIP header) built
    with -fsanitize=address,undefined, the runtimes linked statically: HTK configs with CRLF ends, missing values and
    over-long lines, refused keys, tables for windows of 2 to 4096 samples, band limits, VTLN accepted and refused, one
    channel, and the live counts of every sample count cut at every point: every case as expected and no report."""
    exe = tmp_path / "frontend_tables_check"
    root = lib._PKG.parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    "-I", str(root / "include"), str(root / "tests" / "frontend_tables_check.cpp"), "-o", str(exe)],
                   check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") >= 40 and "Sanitizer" not in r.stderr


def test_param_kind_codes():
    assert lib.param_kind("MFCC_E_D_N_Z") == 6 | 0x40 | 0x100 | 0x80 | 0x800
    assert lib.param_kind("FBANK_D_A_Z") == 7 | 0x100 | 0x200 | 0x800
    with pytest.raises(lib.JamdError):
        lib.param_kind("LPC_E")


def test_make_audio_is_seeded_and_has_edges():
    from julius_amd import synth
    a = synth.make_audio(48000, seed=3)
    assert a.dtype == np.int16 and len(a) == 48000
    assert np.array_equal(a, synth.make_audio(48000, seed=3))
    assert (a == 32767).any() or (a == -32768).any()
    zr = np.flatnonzero(np.diff(np.concatenate([[1], (a == 0).astype(np.int8), [1]])))
    assert len(zr) >= 2
