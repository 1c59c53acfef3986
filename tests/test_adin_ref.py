"""tests/adinref.py held to the real program.  The helper restates the control flow of adin_cut()'s sample stage in
Python around the reference's own functions; here the unmodified `julius` (oracle/_ref/bin/julius) reads three 48 kHz
files with -48 -zmean (zero stripping is its default), and the same program reads, with -nostrip -nozmean, the helper's
16 kHz output for the three files: one file one chunk (each is shorter than the 20 s the first ad_read() asks for), the
DC state reset per file (zmean_reset() at every stream start), the down-sampling state carried from file to file (the
DS_BUFFER is made once).  Both must report the same frame counts (read off the word alignment, -walign) and print the
same first-pass word sequences, scores and alignments.  No GPU."""
import re
import subprocess
import wave

import numpy as np
import pytest

import adinref as R
from julius_amd import synth
from oracle import pyoracle

BIN = pyoracle.HERE / "_ref" / "bin" / "julius"
KEEP = ("pass1_best", "sentence1", "wseq1", "phseq1", "score1", "<search failed>", "<input rejected", "re-computed AM score")
ALIGNED = re.compile(r"\[\s*(\d+)\s+(\d+)\]")


def _run(args):
    out = subprocess.run([str(BIN)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-2000:])
    return out.stdout.replace("\r", "\n")


def _results(stdout):
    """(frame counts: last aligned frame + 1 per input, the first-pass and alignment lines)."""
    keep = [ln.rstrip() for ln in stdout.splitlines() if ln.startswith(KEEP) or ALIGNED.match(ln)]
    frames, last = [], None
    for ln in stdout.splitlines():
        m = ALIGNED.match(ln)
        if m:
            last = int(m.group(2))
        elif ln.startswith("=== end forced alignment") and last is not None:
            frames.append(last + 1)
            last = None
    return frames, keep


def _write_wavs(tmp_path, stem, waves, rate):
    paths = []
    for i, w in enumerate(waves):
        p = tmp_path / f"{stem}{i}.wav"
        with wave.open(str(p), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate)
            f.writeframes(np.asarray(w).astype("<i2").tobytes())
        paths.append(str(p))
    lst = tmp_path / f"{stem}list"
    lst.write_text("\n".join(paths) + "\n")
    return lst


def test_helper_samples_decode_as_the_program_with_48_zmean_and_stripping(ref, tmp_path):
    if not BIN.exists():
        pytest.skip("oracle/_ref/bin/julius not built")
    task = synth.make_triphone_task(tmp_path, seed=43, nword=80, nphone=8, S=120, M=2)
    waves = [synth.make_audio(n, seed=400 + i, sfreq=48000, dc=900.0 - 700.0 * i, zero_runs=4, silent_frac=0, clip=False)
             for i, n in enumerate((60000, 27000, 93000))]
    for w in waves:
        w[5000:6500] = 0                                     # half a second of digital silence in each: 500 samples gone
    common = ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-nlr", task["arpa"],
              "-b", "300", "-1pass", "-gprune", "none", "-sepnum", "5", "-walign", "-input", "rawfile", "-norealtime",
              "-nocutsilence"]
    prog = _run(common + ["-filelist", _write_wavs(tmp_path, "a", waves, 48000), "-48", "-zmean"])

    r = R.RefAdin(ref, 1, down48=True, strip_zero=True, zmean=True)
    fed_waves = []
    for w in waves:
        r.reset(what=R.ZMEAN)                                # a stream starts; the DS_BUFFER goes on
        out = r.push([w])[0]
        fed_waves.append(out)
    stripped = r.ds_out[0] - sum(len(x) for x in fed_waves)
    r.close()
    assert stripped >= 3 * 400                               # the stripping has bitten
    fed = _run(common + ["-filelist", _write_wavs(tmp_path, "b", fed_waves, 16000), "-nostrip", "-nozmean"])

    pframes, pres = _results(prog)
    fframes, fres = _results(fed)
    print("-48 -zmean :", pframes, [ln for ln in pres if ln.startswith("pass1_best")])
    print("helper fed :", fframes, [ln for ln in fres if ln.startswith("pass1_best")])
    assert len(pframes) == 3 and pframes == fframes
    assert pframes == [(len(w) - 400) // 160 + 1 for w in fed_waves]
    assert len([ln for ln in pres if ln.startswith("pass1_best_score:")]) == 3, prog[-3000:]
    assert pres == fres                                      # word sequences, scores and alignments as printed
    assert len(set(ln for ln in pres if ln.startswith("pass1_best:"))) > 1    # not one constant answer
