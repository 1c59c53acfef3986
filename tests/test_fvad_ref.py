"""CPU, where the reference tree is readable: the committed fixtures of the voice-activity detector are the
reference's -- tests/golden/fvad_*.npz equal a fresh recording from libfvad compiled into a temp directory, the model
file equals what julius_amd/shim/jamd_fvad_export writes when built against the reference -- and they cover what the
GPU tests rely on them to cover.  The restated fvad_proceed(), its closed-form frame count and the gated helper
RefCutFvad are checked against the reference's own static fvad_proceed() and adin_cut(): adin-cut.c taken into a tap
with HAVE_LIBFVAD defined, built in a temp directory and linked with oracle/_ref/libjref.so for the rest."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import fvadref as F   # noqa: E402


@pytest.fixture(scope="module")
def libfvad(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("libfvad"))


@pytest.mark.parametrize("name", list(F.STREAMS))
def test_fixture_equals_fresh_recording(libfvad, name):
    """Recorded again from the committed stream (the generator behind it may give other numbers on another install)."""
    have = F.load(name)
    assert have["samples"].dtype == np.int16 and int(have["sfreq"]) == F.STREAMS[name][1]
    fresh = F.record_from(libfvad, have["samples"], int(have["sfreq"]))
    assert sorted(have) == sorted(fresh)
    for k in fresh:
        assert np.array_equal(have[k], fresh[k]), k


def test_streams_are_the_documented_ones():
    """The committed streams carry the documented edits (the zeros in front, the rails in the middle) and are no longer
    than 8 s; where this install's generator gives the numbers it gave when they were recorded, they are make_stream()'s
    sample for sample, and where it does not, the noise between the bursts still has its level."""
    for name, (seed, sfreq) in F.STREAMS.items():
        x = F.load(name)["samples"]
        assert len(x) <= 8 * sfreq
        half = (len(x) - 3200) // 2
        assert not x[:1600].any() and np.array_equal(x[1600 + half:3200 + half], F.rails())
        fresh = F.make_stream(name)
        assert len(fresh) == len(x)
        if np.array_equal(fresh[1600:1600 + 2000], x[1600:1600 + 2000]):     # (the first gap's noise: the generator agrees)
            assert np.array_equal(fresh, x)
        else:
            assert 20 < x[1600:1600 + 2000].astype(float).std() < 40         # N(0, 30)


def test_model_file_equals_export(tmp_path):
    if not F.FVAD_SRC.is_dir():
        pytest.skip("no reference tree")
    subprocess.run(["make", "-s", "-C", str(F.ROOT / "julius_amd" / "shim"), f"JULIUS_SRC={F.REFERENCE}",
                    f"BINDIR={tmp_path}", "fvad_export"], check=True)
    out = tmp_path / "model.txt"
    subprocess.run([str(tmp_path / "jamd_fvad_export"), str(out)], check=True)
    assert out.read_text() == F.MODEL.read_text()


@pytest.mark.parametrize("name", list(F.STREAMS))
def test_fixture_coverage(name):
    """Asserted here, so that a fixture cannot quietly lose what the GPU tests need it for."""
    z = F.load(name)
    for mode in range(4):
        raw, st = z[f"raw{mode}"].astype(int), z[f"state{mode}"]
        assert (raw == 0).any() and (raw == 1).any() and (raw > 1).any(), mode
        run = best = 0
        for v in raw:                            # num_of_speech counts the frames the core itself called speech
            run = run + 1 if v == 1 else 0
            best = max(best, run)
        assert best > F.MAX_SPEECH_FRAMES, mode    # ... and reaches its cap
        assert 100 < st[50] < len(raw), mode       # frame_counter: behind by the frames of power 0


@pytest.fixture(scope="module")
def cut_tap(tmp_path_factory, ref):
    """The reference's adin-cut.c compiled with HAVE_LIBFVAD into a temp directory (fvadref.CUT_TAP)."""
    return F.build_cut_tap(tmp_path_factory.mktemp("cut_tap"))


@pytest.mark.parametrize("step,first,second", [(1, 9000, 5000), (159, 40000, 30001), (160, 40000, 30001), (161, 40000, 30001),
                                               (1000, 40000, 30001), (4001, 60000, 40000)])
def test_proceed_against_the_reference(libfvad, cut_tap, step, first, second):
    """The restated fvad_proceed() against the reference's own static function, block by block of `step` samples over
    two streams with need_init between them (executed by the reference's adin_cut() on an empty stream): the gate, the
    samples kept -- which is the frames consumed, `i + fs < len` strictly -- and the results held are equal, the frames
    consumed are max(0, ceil(e / fs) - 1), and the gate is the closed form over the recorded decisions that the device
    uses.  The detectors behind both end in the same state."""
    z = F.load("fvad_b2_16k")
    x, fs, N, thres, mode = z["samples"][1600:], 160, 5, 0.5, 1
    tap = F.CutTap(cut_tap, mode, N, thres)
    det = F.RefFvad(libfvad, 16000, mode)
    seen = []
    p = F.Proceed(lambda fr: seen.append(det.frame(fr)[0]) or seen[-1], fs, N, thres)
    for w in (x[:first], x[first:first + second]):
        base = len(seen)
        for a in range(0, len(w), step):
            blk = w[a:a + step]
            e = a + len(blk)
            got = tap.proceed(blk)
            assert got == (p(blk), len(p.pend), sum(p.ring)), (a, got)
            n = F.gate_frames(e, fs)
            assert len(seen) - base == n and got[1] == e - n * fs
            assert got[0] == int(sum(seen[base + max(0, n - N):base + n]) >= F.cmin(N, thres))
        assert tap.stream(np.zeros(0, np.int16)) == []       # need_init, adin-cut.c:412-431
        p.init()
        assert tap.proceed(np.zeros(0, np.int16)) == (0, 0, 0)
    assert np.array_equal(tap.raw_state()[:-1], det.state()[:-1])
    det.close()


CUSTOM = dict(level_thres=500, zero_cross_num=40, head_margin_msec=200, tail_margin_msec=250, chunk_size=800)


@pytest.mark.parametrize("mode,smoothnum,thres", [(0, 5, 0.5), (1, 5, 1.0), (2, 1, 0.5), (3, 30, 1.0), (3, 30, 0.5)])
@pytest.mark.parametrize("desc", [{}, CUSTOM], ids=["default", "custom"])
def test_helper_equals_the_reference_adin_cut(libfvad, cut_tap, ref, desc, mode, smoothnum, thres):
    """RefCutFvad, which the GPU tests of the gate are held to, against the reference's own adin_cut() built with
    HAVE_LIBFVAD, fed whole streams: three streams on one ADIn and one core (need_init between them), read in one piece
    and in reads of 1 234 samples.  Every segment passed to ad_process() is equal, and the detectors end alike."""
    import adincutref as K
    x = F.load("fvad_b2_16k")["samples"]
    tap = F.CutTap(cut_tap, mode, smoothnum, thres, **desc)
    det = F.RefFvad(libfvad, 16000, mode)
    r = F.ref_cut_fvad(K)(ref, [lambda fr: det.frame(fr)[0]], smoothnum, thres, nchan=1, **desc)
    for w, read_max in ((x, 1 << 30), (x[:48000], 1234), (x[30001:], 1 << 30)):
        segs = tap.stream(w, read_max)
        mine = [q.data() for q in r.push([w], [True])[0] if q.final or len(q.data())]
        assert [len(s) for s in segs] == [len(s) for s in mine]
        assert all(np.array_equal(a, b) for a, b in zip(segs, mine))
        assert len(segs) >= 2
    assert sum(1 for over, gate in r.gates[0] if over and not gate) >= 1
    assert np.array_equal(tap.raw_state()[:-1], det.state()[:-1])
    det.close()
    r.close()


@pytest.mark.parametrize("mode", range(4))
def test_gate_coverage(ref, mode):
    """Under default cutting parameters and -fvad_param 5 0.5 the gate of every mode vetoes at least one block whose
    zero-cross count is over the threshold and changes value at least twice, and the delivered samples differ from the
    plain cutting's: the GPU tests of the gate rely on it."""
    import adincutref as K
    z = F.load("fvad_b2_16k")
    x = z["samples"]
    replay = F.Replay(z[f"raw{mode}"])
    r = F.ref_cut_fvad(K)(ref, [replay], 5, 0.5, nchan=1)
    got = K.layout(r.push([x], [True]), 1)[0]
    replay.finish(F.gate_frames(len(x), 160))
    g = r.gates[0]
    assert len(g) == len(x) // 1000
    assert sum(1 for over, gate in g if over and not gate) >= 1
    assert sum(1 for i in range(1, len(g)) if g[i][1] != g[i - 1][1]) >= 2
    p = K.RefCut(ref, 1)
    assert not np.array_equal(K.layout(p.push([x], [True]), 1)[0], got)
    r.close()
    p.close()
