"""CPU: what the voice-activity detector (jamd_fvad) does without a device.  tests/fvad_core_check.cpp is compiled
alone, under the host sanitizers, from julius_amd/csrc/fvad_core.h -- the arithmetic the kernel runs -- and
fvad_plan.h: its decisions and final state over the committed streams equal the fixtures in every mode, and the frame
counts, the gate's smallest count and the model reader equal the helper (tests/fvadref.py).  The library's own
host-only entries are checked through the C ABI."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import fvadref as F   # noqa: E402
from julius_amd import lib   # noqa: E402

ROOT = F.ROOT


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("fvad_check") / "fvad_core_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I", str(ROOT / "include"), "-I", str(ROOT / "julius_amd" / "csrc"),
                    str(ROOT / "tests" / "fvad_core_check.cpp"), "-o", str(exe)], check=True)

    def run(*args, ok=True):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert (r.returncode == 0) == ok and not r.stderr, r.stderr[-2000:]
        return r.stdout
    return run


@pytest.mark.parametrize("name", list(F.STREAMS))
def test_core_equals_fixture(check, tmp_path, name):
    z = F.load(name)
    pcm = tmp_path / "pcm.raw"
    z["samples"].tofile(pcm)
    for mode in range(4):
        raw, state = check("run", F.MODEL, int(z["sfreq"]), mode, pcm).splitlines()
        assert np.array_equal(np.array(raw.split(), int), z[f"raw{mode}"]), mode
        assert np.array_equal(np.array(state.split(), int), z[f"state{mode}"][:-1]), mode


def test_frame_counts(check):
    es = [0, 1, 79, 80, 81, 159, 160, 161, 320, 321, 1000, 108000]
    for fs in (80, 160):
        assert [int(v) for v in check("gate", fs, *es).split()] == [F.gate_frames(e, fs) for e in es]
        assert [int(v) for v in check("frames", fs, *es).split()] == [e // fs for e in es]
    assert [F.gate_frames(e, 160) for e in (0, 1, 159, 160, 161, 320, 321)] == [0, 0, 0, 0, 1, 1, 2]


def test_frames_entry():
    """jamd_fvad_frames(): floor((before + chunk) / fs) - floor(before / fs)."""
    for sfreq in (8000, 16000):
        fs = sfreq // 100
        for before in (0, 1, fs - 1, fs, fs + 1, 12345):
            for chunk in (0, 1, fs - 1, fs, fs + 1, 4000, 227441):
                assert lib.Fvad.frames(sfreq, before, chunk) == (before + chunk) // fs - before // fs
    for sfreq, text in [(11025, "takes 8000 or 16000"), (32000, "takes 8000 or 16000"), (0, "takes 8000 or 16000")]:
        with pytest.raises(lib.JamdError, match=text):
            lib.Fvad.frames(sfreq, 0, 1)
    with pytest.raises(lib.JamdError, match="negative sample count"):
        lib.Fvad.frames(16000, -1, 1)
    with pytest.raises(lib.JamdError, match="negative sample count"):
        lib.Fvad.frames(16000, 0, -1)


def test_cmin(check):
    for N in range(1, 31):
        for thres in (0, 0.2, 0.5, 0.99, 1):
            assert int(check("cmin", N, thres)) == F.cmin(N, thres), (N, thres)
    assert F.cmin(5, 0) == 0 and F.cmin(5, 0.5) == 3 and F.cmin(5, 1) == 5 and F.cmin(5, 1.5) == 6


def test_model_reader(check, tmp_path):
    want = F.model_ints()
    assert len(want) == lib.FVAD_MODEL_INTS
    assert lib.FvadModel.read(F.MODEL).ints() == want
    assert [int(v) for v in check("read", F.MODEL).split()[1:]] == want
    plain = tmp_path / "plain.txt"               # no comments, blank lines, trailing blanks
    plain.write_text("\n".join(f" {v} " for v in want) + "\n\n")
    assert lib.FvadModel.read(plain).ints() == want
    bad = tmp_path / "bad.txt"
    for text, why in [("\n".join(map(str, want[:-1])) + "\n", "129 entries, the model has 130"),
                      ("\n".join(map(str, want + [1])) + "\n", "more than 130 entries"),
                      ("\n".join(map(str, want[:5] + ["1.5"] + want[6:])) + "\n", "line 6 is no integer"),
                      ("\n".join(map(str, want[:5] + ["x"] + want[6:])) + "\n", "line 6 is no integer"),
                      ("\n".join(map(str, want[:5] + [32768] + want[6:])) + "\n", "line 6 is no 16-bit value"),
                      ("", "0 entries, the model has 130")]:
        bad.write_text(text)
        with pytest.raises(lib.JamdError, match=why):
            lib.FvadModel.read(bad)
        assert check("read", bad, ok=False).startswith("refused: " + why)
    with pytest.raises(lib.JamdError, match="cannot open the file"):
        lib.FvadModel.read(tmp_path / "none.txt")
