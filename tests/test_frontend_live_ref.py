"""tests/frontendliveref.py held to the real program.  The helper restates the control flow of the reference's live
front end in Python around the reference's own functions; here the unmodified `julius` (oracle/_ref/bin/julius) reads
three audio files with -realtime, and the same program reads, with -norealtime -input htkparam, the helper's features
for the three segments (committed between them, as the program updates its cepstral mean after every input).  Both must
report the same frame counts (read off the word alignment, -walign: the live run prints no count of its own) and print
the same first-pass word sequences, scores and alignments: the second and third file depend on the state carried over.
No -notypecheck is needed: the model is declared MFCC_E_D_A_Z and so are the parameter files."""
import re
import subprocess
import wave

import pytest

import frontendliveref as L
from frontendref import RefFrontend
from julius_amd import lib, synth
from oracle import pyoracle

BIN = pyoracle.HERE / "_ref" / "bin" / "julius"
KIND = "MFCC_E_D_A_Z"


def _run(args):
    out = subprocess.run([str(BIN)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-2000:])
    return out.stdout.replace("\r", "\n")


KEEP = ("pass1_best", "sentence1", "wseq1", "phseq1", "score1", "<search failed>", "<input rejected", "re-computed AM score")
ALIGNED = re.compile(r"\[\s*(\d+)\s+(\d+)\]")


def _results(stdout):
    """What the program prints per input: the first-pass result, and the word alignment (-walign) with its frame
    numbers and scores.  Returns (frame counts: last aligned frame + 1, the kept lines)."""
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


def test_helper_features_decode_as_the_live_program(ref, tmp_path):
    if not BIN.exists():
        pytest.skip("oracle/_ref/bin/julius not built")
    task = synth.make_triphone_task(tmp_path, seed=41, nword=80, nphone=8, S=120, M=2)
    # the same model declared as MFCC_E_D_A_Z, so that the live front end normalises the cepstral mean
    synth.write_hmmdefs(task["hmmdefs"], task["model"], phones=list(task["phys"].items()), kind=KIND)
    waves = [synth.make_audio(n, seed=300 + i, zero_runs=0, silent_frac=0, clip=False) for i, n in enumerate((20000, 9000, 31000))]
    for w in waves:
        w[w == 0] = 1                                        # no zero samples at all
    wavs = []
    for i, w in enumerate(waves):
        p = tmp_path / f"a{i}.wav"
        with wave.open(str(p), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes(w.astype("<i2").tobytes())
        wavs.append(str(p))
    (tmp_path / "wavlist").write_text("\n".join(wavs) + "\n")
    common = ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-nlr", task["arpa"],
              "-b", "300", "-1pass", "-gprune", "none", "-sepnum", "5", "-walign"]
    live = _run(common + ["-input", "rawfile", "-filelist", tmp_path / "wavlist", "-realtime", "-nostrip", "-nocutsilence"])

    v = RefFrontend(ref).para(lib.param_kind(KIND), 39)
    rc = L.RefLiveChannel(ref, v)                            # default.c: MAP-CMN, weight 100, nothing loaded
    mfcs, counts = [], []
    for i, w in enumerate(waves):
        feat = rc.segment(w)
        rc.commit()
        counts.append(len(feat))
        p = tmp_path / f"a{i}.mfc"
        synth.write_htk_param(p, feat, parmkind=lib.param_kind(KIND))
        mfcs.append(str(p))
    rc.close()
    (tmp_path / "mfclist").write_text("\n".join(mfcs) + "\n")
    fed = _run(common + ["-input", "htkparam", "-filelist", tmp_path / "mfclist", "-norealtime"])

    lframes, lres = _results(live)
    fframes, fres = _results(fed)
    print("live:", lframes, [ln for ln in lres if ln.startswith("pass1_best")])
    print("fed :", counts, [ln for ln in fres if ln.startswith("pass1_best")])
    assert lframes == counts == fframes                      # equal frame counts, all three files
    assert len([ln for ln in lres if ln.startswith("pass1_best_score:")]) == 3, live[-3000:]
    assert lres == fres                                      # word sequences, scores and alignments as printed
    assert len(set(ln for ln in lres if ln.startswith("pass1_best:"))) > 1    # not one constant answer
