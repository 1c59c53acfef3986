"""Host half of the spectral subtraction (csrc/frontend_api.hip, csrc/ss_file.h): the mkss / -ssload file format against
the reference's new_SS_load_from_file(), the defaults of jamd_frontend_ss_default() against the reference's, and the
file reader and writer as a stand-alone program under the host sanitizers.  No GPU."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

from julius_amd import lib
from frontendref import same
from frontendssref import RefFrontendSS


@pytest.fixture(scope="module")
def rf(ref):
    return RefFrontendSS(ref)


def spectrum(n, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 5000.0, n).astype(np.float32)
    a[::17] = 0.0                                      # exact zeros, and values whose four bytes all differ
    a[1::17] = np.float32(1.2345678e-3)
    return a


def mkss_bytes(a):
    """The layout mkss writes (mkss/mkss.c:219-233): big-endian int32 count, then big-endian float32."""
    a = np.ascontiguousarray(a, np.float32)
    return struct.pack(">i", len(a)) + a.astype(">f4").tobytes()


@pytest.mark.parametrize("n", [0, 1, 16, 255, 256, 257, 512, 4096])
def test_write_read_round_trip(tmp_path, n):
    a = spectrum(n, seed=n)
    p = tmp_path / "noise.ss"
    lib.ss_write(p, a)
    assert p.read_bytes() == mkss_bytes(a)
    got = lib.ss_read(p)
    assert got.dtype == np.float32 and got.shape == (n,) and got.tobytes() == a.tobytes()


@pytest.mark.parametrize("n", [16, 512, 700])
def test_mkss_layout_is_read_as_the_reference_reads_it(rf, tmp_path, n):
    a = spectrum(n, seed=100 + n)
    p = tmp_path / "mkss.ss"
    p.write_bytes(mkss_bytes(a))
    want = rf.load(p)
    assert want is not None and want.tobytes() == a.tobytes()
    got = lib.ss_read(p)
    assert got.tobytes() == want.tobytes()
    lib.ss_write(tmp_path / "ours.ss", a)             # and the reference reads what ss_write wrote
    assert rf.load(tmp_path / "ours.ss").tobytes() == a.tobytes()


@pytest.mark.parametrize("cut", [0, 2, 4, 5, 4 + 4 * 511, 4 + 4 * 512 - 1])
def test_truncated_file_is_refused(tmp_path, cut):
    p = tmp_path / "trunc.ss"
    p.write_bytes(mkss_bytes(spectrum(512))[:cut])
    out = np.full(512, 7.0, np.float32)
    L = lib.load()
    assert L.jamd_frontend_ss_read(str(p).encode(), out.ctypes.data, 512) == -1
    assert L.jamd_last_error()
    with pytest.raises(lib.JamdError):
        lib.ss_read(p)


def test_negative_count_and_missing_file_are_refused(tmp_path):
    p = tmp_path / "neg.ss"
    p.write_bytes(struct.pack(">i", -4) + b"\0" * 64)
    L = lib.load()
    assert L.jamd_frontend_ss_read(str(p).encode(), None, 0) == -1
    assert L.jamd_frontend_ss_read(str(tmp_path / "none.ss").encode(), None, 0) == -1
    assert L.jamd_frontend_ss_write(str(tmp_path / "no" / "dir.ss").encode(), spectrum(4).ctypes.data, 4) == -1
    assert L.jamd_frontend_ss_write(str(p).encode(), None, 4) == -1
    assert L.jamd_frontend_ss_read(None, None, 0) == -1


def test_cap_smaller_than_the_count_returns_the_count(tmp_path):
    a = spectrum(512, seed=3)
    p = tmp_path / "noise.ss"
    lib.ss_write(p, a)
    out = np.full(20, -1.0, np.float32)
    L = lib.load()
    assert L.jamd_frontend_ss_read(str(p).encode(), out.ctypes.data, 7) == 512
    assert out[:7].tobytes() == a[:7].tobytes() and (out[7:] == -1.0).all()
    assert L.jamd_frontend_ss_read(str(p).encode(), None, 0) == 512
    assert L.jamd_frontend_ss_read(str(p).encode(), out.ctypes.data, -3) == 512 and (out[7:] == -1.0).all()


def test_bytes_after_the_declared_values_are_ignored_as_in_the_reference(rf, tmp_path):
    a = spectrum(16, seed=4)
    p = tmp_path / "long.ss"
    p.write_bytes(mkss_bytes(a) + b"\x01\x02\x03" * 50)
    assert rf.load(p).tobytes() == a.tobytes()
    assert lib.ss_read(p).tobytes() == a.tobytes()


def test_ss_default_equals_the_reference_defaults(rf, tmp_path):
    ss = lib.FrontendSS(9, 9, 9.0, 9.0, 1234, 9)
    assert lib.load().jamd_frontend_ss_default(C.byref(ss)) == 0
    calclen, alpha, floor = rf.defaults(tmp_path)
    assert (calclen, alpha, floor) == (300, 2.0, 0.5)            # default.c:158-162, mfcc.h:68-69
    assert (ss.mode, ss.calc_len_ms, ss.noise, ss.noise_len) == (lib.SS_OFF, calclen, None, 0)
    assert same(np.float32([ss.alpha, ss.floor]), np.float32([alpha, floor]))
    assert lib.load().jamd_frontend_ss_default(None) == -1
    assert (lib.SS_OFF, lib.SS_CALC, lib.SS_LOAD) == (0, 1, 2)


def test_file_reader_and_writer_under_sanitizers(tmp_path):
    """tests/ss_file_check.cpp (its own main over csrc/ss_file.h) built with -fsanitize=address,undefined, the
    runtimes linked statically, over a good, an empty, a truncated and an over-long file: every case as expected and
    no report."""
    exe = tmp_path / "ss_file_check"
    root = lib._PKG.parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    str(root / "tests" / "ss_file_check.cpp"), "-o", str(exe)], check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") >= 12 and "Sanitizer" not in r.stderr
