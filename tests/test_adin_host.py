"""What the audio conditioning stage works out without a device (csrc/adin_plan.h through the C ABI) against the
compiled reference: the closed-form count of 16 kHz samples a push completes (jamd_adin_ds_count) against what
ds48to16() returns, for every input length 0 ... 1600 and for random cuts of 100000 samples; the coefficient file reader
against the tables the reference holds; and that header as a stand-alone program under the host sanitizers.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import adinref as R
from julius_amd import lib


@pytest.fixture(scope="module")
def tabs(ref):
    return R.tables(ref)


@pytest.fixture(scope="module")
def desc(tabs):
    return lib.Adin.desc_for(fir_3to4=tabs[0], fir_2to1=tabs[1])


def _count(desc, before, chunk):
    return lib.load().jamd_adin_ds_count(C.byref(desc), before, chunk)


def test_defaults():
    d = lib.AdinDesc()
    assert lib.load().jamd_adin_default(C.byref(d)) == 0
    assert (d.down48, d.fir_3to4, d.n_3to4, d.fir_2to1, d.n_2to1, d.level_coef, d.strip_zero, d.zmean) == \
        (0, None, 0, None, 0, 1.0, 1, 0)
    assert _count(d, 5, 1234) == 1234                      # without down48 a push yields its chunk
    assert lib.load().jamd_abi_version() == 4


def test_ds_count_every_length_to_1600(ref, desc):
    w = np.random.default_rng(0).integers(-20000, 20000, 1600).astype(np.int16)
    for n in range(1601):
        r = R.RefAdin(ref, 1, down48=True, strip_zero=False)
        assert len(r.push([w[:n]])[0]) == _count(desc, 0, n), n
        r.close()


def test_ds_count_random_cuts(ref, desc):
    rng = np.random.default_rng(1)
    w = rng.integers(-20000, 20000, 100000).astype(np.int16)
    for trial in range(4):
        r = R.RefAdin(ref, 1, down48=True, strip_zero=False)
        at, total = 0, 0
        while at < len(w):
            k = min(int(rng.integers(1, (300, 3000, 20000, 70000)[trial])), len(w) - at)
            got = len(r.push([w[at:at + k]])[0])
            assert got == _count(desc, at, k) == lib.load().jamd_adin_push_cap(C.byref(desc), at, k), (trial, at, k)
            at += k
            total += got
        assert total == 33052 == _count(desc, 0, len(w))
        r.close()


def test_ds_count_refusals(desc):
    assert _count(desc, -1, 5) < 0 and _count(desc, 0, -5) < 0
    bad = lib.Adin.desc_for(down48=True)
    assert _count(bad, 0, 1000) < 0 and b"513" in lib.load().jamd_last_error()


def test_fir_read_round_trip_and_refusals(tabs, tmp_path):
    for name, t in zip(("lpfcoef.3to4", "lpfcoef.2to1"), tabs):
        p = tmp_path / name
        p.write_text("".join(f"{x:.17g}\n" for x in t))
        assert np.array_equal(lib.adin_fir_read(p), t)     # 17 significant digits: atof() gives the double back
        with pytest.raises(lib.JamdError, match="room"):
            lib.adin_fir_read(p, cap=len(t) - 1)
    with pytest.raises(lib.JamdError, match="open"):
        lib.adin_fir_read(tmp_path / "missing")
    (tmp_path / "empty").write_text("")
    with pytest.raises(lib.JamdError, match="no coefficient"):
        lib.adin_fir_read(tmp_path / "empty")
    (tmp_path / "many").write_text("1\n" * 600)
    assert len(lib.adin_fir_read(tmp_path / "many")) == 513     # load_filter() stops there


def test_plan_under_sanitizers(tmp_path):
    """tests/adin_plan_check.cpp (its own main over csrc/adin_plan.h, which includes no HIP header) built with
    -fsanitize=address,undefined, the runtimes linked statically: the counts against a walk of do_filter()'s counters
    for seven pairs of table lengths, the index bounds the kernels rely on, the descriptor checks, coefficient files that
    are missing, empty, over-long or not numbers: every case as expected and no report."""
    exe = tmp_path / "adin_plan_check"
    root = lib._PKG.parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    "-I", str(root / "include"), str(root / "tests" / "adin_plan_check.cpp"), "-o", str(exe)],
                   check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 3 and "Sanitizer" not in r.stderr
