"""GPU: the voice-activity detector behind -fvad (jamd_fvad) against libfvad's recorded decisions and final state
(tests/golden/fvad_*.npz, proven to be the reference's by tests/test_fvad_ref.py): whole streams, the same streams cut
into pushes of every awkward size, 130 channels with idle ones in one call, masked resets, the device-pointer entry
and the refusals."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import fvadref as F   # noqa: E402
from julius_amd import lib   # noqa: E402

pytestmark = pytest.mark.gpu

_fix = {}


def fixture(name):
    if name not in _fix:
        _fix[name] = F.load(name)
        for v in _fix[name].values():
            v.setflags(write=False)
    return _fix[name]


@pytest.fixture(scope="module")
def model():
    return lib.FvadModel.read(F.MODEL)


def pushes(fv, x, cuts):
    """One channel: x cut at `cuts` -> every raw value."""
    out = []
    for a, b in zip([0] + list(cuts), list(cuts) + [len(x)]):
        r, off = fv.push_host([x[a:b]])
        assert list(off) == [0, len(r)]
        out.append(r)
    return np.concatenate(out)


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("name", list(F.STREAMS))
def test_whole_stream(engine, model, name, mode):
    z = fixture(name)
    fv = lib.Fvad(engine, 1, model, sfreq=int(z["sfreq"]), mode=mode)
    raw, off = fv.push_host([z["samples"]])
    assert raw.dtype == np.uint8 and list(off) == [0, len(z[f"raw{mode}"])]
    assert np.array_equal(raw, z[f"raw{mode}"])
    assert np.array_equal(fv.state(0), z[f"state{mode}"])
    fv.close()


def test_one_sample_pushes_across_the_rails(engine, model):
    """4 000 pushes of one sample each -- 25 frames whose every sample comes out of the waiting ones -- placed where the
    models adapt hardest: from the last frames of speech in front of the rail stretch across its first 1 200 samples."""
    z, mode = fixture("fvad_b3_16k"), 2
    x = z["samples"]
    start = 1600 + (len(x) - 3200) // 2 - 2800 + 37          # (not on the frame grid)
    fv = lib.Fvad(engine, 1, model, sfreq=16000, mode=mode)
    assert np.array_equal(pushes(fv, x, [start + i for i in range(4001)]), z[f"raw{mode}"])
    assert np.array_equal(fv.state(0), z[f"state{mode}"])
    fv.close()


@pytest.mark.parametrize("step", [1, 159, 160, 161, 1000, 4001, "random"])
@pytest.mark.parametrize("name,mode", [("fvad_b2_16k", 1), ("fvad_b2_8k", 2)])
def test_pushes_give_identical_bytes(engine, model, name, mode, step):
    """The leading zeros in one push, then up to 400 pushes of `step` samples (random: 0 ... 5000 each), then the rest."""
    z = fixture(name)
    x = z["samples"]
    if step == "random":
        rng = np.random.default_rng(7)
        cuts = np.cumsum(rng.integers(0, 5001, 400))
    else:
        cuts = 1600 + step * np.arange(401)
    cuts = [int(c) for c in cuts if c < len(x)]
    fv = lib.Fvad(engine, 1, model, sfreq=int(z["sfreq"]), mode=mode)
    assert np.array_equal(pushes(fv, x, cuts), z[f"raw{mode}"])
    assert np.array_equal(fv.state(0), z[f"state{mode}"])
    fv.close()


@pytest.mark.parametrize("sfreq,names", [(16000, ("fvad_b2_16k", "fvad_b3_16k")), (8000, ("fvad_b2_8k",))])
def test_130_channels_with_idle_ones(engine, model, sfreq, names):
    """More than two waves in one call.  A prefix of a stream has the prefix of its decisions, so the channels are
    prefixes of different lengths (every 13th the whole stream, whose final state the fixture has), given in six pushes
    of unequal chunks, in each of which some channels get nothing."""
    nchan, mode, fs = 130, 2, sfreq // 100
    rng = np.random.default_rng(11)
    zs = [fixture(n) for n in names]
    src = [zs[c % len(zs)] for c in range(nchan)]
    length = [len(src[c]["samples"]) if c % 13 == 0 else int(rng.integers(1, len(src[c]["samples"]))) for c in range(nchan)]
    fv = lib.Fvad(engine, nchan, model, sfreq=sfreq, mode=mode)
    at, got = [0] * nchan, [[] for _ in range(nchan)]
    for push in range(6):
        chunks = []
        for c in range(nchan):
            left = length[c] - at[c]
            n = left if push == 5 else 0 if rng.random() < 0.25 else int(rng.integers(0, left + 1))
            chunks.append(src[c]["samples"][at[c]:at[c] + n])
            at[c] += n
        raw, off = fv.push_host(chunks)
        for c in range(nchan):
            assert off[c + 1] - off[c] == at[c] // fs - (at[c] - len(chunks[c])) // fs
            got[c].append(raw[off[c]:off[c + 1]])
    for c in range(nchan):
        assert np.array_equal(np.concatenate(got[c]), src[c][f"raw{mode}"][:length[c] // fs]), c
        if c % 13 == 0:
            assert np.array_equal(fv.state(c), src[c][f"state{mode}"]), c
        else:
            assert fv.state(c)[-1] == length[c] % fs
    fv.close()


def test_reset_with_mask(engine, model):
    """Reset channels repeat from the start (their waiting samples gone), the others go on."""
    z, mode = fixture("fvad_b3_16k"), 3
    x, want = z["samples"], z[f"raw{mode}"]
    half = 50007                                 # (47 samples wait)
    fv = lib.Fvad(engine, 4, model, sfreq=16000, mode=mode)
    raw, off = fv.push_host([x[:half]] * 4)
    for c in range(4):
        assert np.array_equal(raw[off[c]:off[c + 1]], want[:half // 160])
    fv.reset(mask=[1, 0, 1, 0])
    raw, off = fv.push_host([x, x[half:], x[:half], x[half:]])
    assert np.array_equal(raw[off[0]:off[1]], want)
    assert np.array_equal(raw[off[2]:off[3]], want[:half // 160])
    for c in (1, 3):
        assert np.array_equal(raw[off[c]:off[c + 1]], want[half // 160:])
    for c in (0, 1, 3):
        assert np.array_equal(fv.state(c), z[f"state{mode}"])
    fv.reset()
    raw, off = fv.push_host([x[:1000]] * 4)
    assert all(np.array_equal(raw[off[c]:off[c + 1]], want[:6]) for c in range(4))
    fv.close()


def test_device_entry(engine, model):
    """jamd_fvad_push_dev(): samples and bytes stay on the device, the offsets are closed-form."""
    z, mode = fixture("fvad_b2_16k"), 0
    x = z["samples"]
    fv = lib.Fvad(engine, 2, model, sfreq=16000, mode=mode)
    d_in = lib.DevBuf(engine, 2 * x.nbytes).upload(np.concatenate([x, x[:40000]]))
    d_out = lib.DevBuf(engine, 2 * len(x) // 160)
    off = fv.push_dev(d_in.ptr, [0, len(x), len(x) + 40000], d_out.ptr)
    assert list(off) == [0, len(x) // 160, len(x) // 160 + 250]
    got = d_out.download((int(off[2]),), np.uint8)
    assert np.array_equal(got[:off[1]], z[f"raw{mode}"]) and np.array_equal(got[off[1]:], z[f"raw{mode}"][:250])
    fv.close()


def test_refusals(engine, model):
    for kw, text in [(dict(sfreq=11025), "takes 8000 or 16000"), (dict(sfreq=32000), "not served"),
                     (dict(sfreq=48000), "not served"), (dict(mode=4), "mode 4 is not in 0 ... 3"),
                     (dict(mode=-1), "mode -1 is not in 0 ... 3")]:
        with pytest.raises(lib.JamdError, match=text):
            lib.Fvad(engine, 1, model, **kw)
    with pytest.raises(lib.JamdError, match="the model is NULL"):
        lib.Fvad(engine, 1, None)
    ints = model.ints()
    ints[17] = 40000
    with pytest.raises(lib.JamdError, match=r"model entry 17 \(40000\) is no 16-bit value"):
        lib.Fvad(engine, 1, lib.FvadModel.from_ints(ints))
    with pytest.raises(lib.JamdError, match="nchan not in"):
        lib.Fvad(engine, 0, model)
    fv = lib.Fvad(engine, 1, model)
    with pytest.raises(lib.JamdError, match="negative, descending"):
        fv.push_dev(0, [5, 3], 0)
    fv.close()


# ---- the gate inside the silence cutting (jamd_adin_cut_create_fvad) against RefCutFvad in replay

import adincutref as K   # noqa: E402

CUSTOM = dict(level_thres=500, zero_cross_num=40, head_margin_msec=200, tail_margin_msec=250, chunk_size=800)


def gated_pair(engine, ref, model, raws, mode, smoothnum, thres, desc, sfreq=16000):
    """The product with the gate and the helper replaying the recorded decisions `raws` (one array per channel)."""
    replay = [F.Replay(r) for r in raws]
    a = lib.AdinCut(engine, len(raws), fvad=lib.AdinCut.fvad_for(model, mode, smoothnum, thres, sfreq), sfreq=sfreq, **desc)
    r = F.ref_cut_fvad(K)(ref, replay, smoothnum, thres, nchan=len(raws), sfreq=sfreq, **desc)
    return a, r, replay


def same_push(a, r, chunks, eos=None, max_parts=None):
    """One push on both sides: samples, part_off, part_final, part_start and every channel's state are equal."""
    want = K.layout(r.push(chunks, eos), a.nchan)
    got = a.push_host(chunks, eos, max_parts=max_parts)
    for g, w, name in zip(got, want, ("samples", "part_off", "part_final", "part_start")):
        assert g.shape == w.shape and np.array_equal(g, w), name
    for c in range(a.nchan):
        assert a.state(c) == r.state(c), c
    return got


def feed(a, r, x, step, eos=True):
    out = []
    cuts = list(range(0, len(x), step)) + [len(x)]
    for i in range(len(cuts) - 1):
        out.append(same_push(a, r, [x[cuts[i]:cuts[i + 1]]], [eos and i == len(cuts) - 2])[0])
    return np.concatenate(out)


@pytest.mark.parametrize("step", [None, 4000], ids=["whole", "live4000"])
@pytest.mark.parametrize("thres", [0.5, 1.0])
@pytest.mark.parametrize("smoothnum", [1, 5, 30])
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("desc", [{}, CUSTOM], ids=["default", "custom"])
def test_cut_with_gate(engine, ref, model, desc, mode, smoothnum, thres, step):
    z = fixture("fvad_b2_16k")
    x = z["samples"]
    a, r, replay = gated_pair(engine, ref, model, [z[f"raw{mode}"]], mode, smoothnum, thres, desc)
    got = feed(a, r, x, step or len(x))
    replay[0].finish(F.gate_frames(len(x), 160))
    assert np.array_equal(a.fvad_state(0)[:-1], z[f"gstate{mode}"][:-1])
    vetoed = sum(1 for over, gate in r.gates[0] if over and not gate)
    assert vetoed > 0
    plain = lib.AdinCut(engine, 1, **desc)                    # the same object without the gate gives something else
    cuts = list(range(0, len(x), step or len(x))) + [len(x)]
    free = np.concatenate([plain.push_host([x[cuts[i]:cuts[i + 1]]], [i == len(cuts) - 2])[0] for i in range(len(cuts) - 1)])
    assert len(free) != len(got) or not np.array_equal(free, got)
    for o in (a, r, plain):
        o.close()


@pytest.mark.parametrize("step", [None, 4000], ids=["whole", "live4000"])
def test_thres_zero_is_the_plain_cutting(engine, ref, model, step):
    """cmin is 0: the gate never closes.  Equal to plain RefCut and to an object made by the old entry."""
    z = fixture("fvad_b3_16k")
    x = z["samples"]
    a = lib.AdinCut(engine, 1, fvad=lib.AdinCut.fvad_for(model, 2, 5, 0.0))
    r = K.RefCut(ref, 1)
    old = lib.AdinCut(engine, 1)
    cuts = list(range(0, len(x), step or len(x))) + [len(x)]
    for i in range(len(cuts) - 1):
        chunk, eos = [x[cuts[i]:cuts[i + 1]]], [i == len(cuts) - 2]
        got = same_push(a, r, chunk, eos)
        for g, w in zip(got, old.push_host(chunk, eos)):
            assert np.array_equal(g, w)
    assert np.array_equal(a.fvad_state(0)[:-1], z["gstate2"][:-1])     # (the detector ran all the same)
    for o in (a, r, old):
        o.close()


@pytest.mark.parametrize("tag,first", [("A", F.TWO_FIRST), ("B", F.TWO_FIRST + 1)])
def test_two_streams_on_one_core(engine, ref, model, tag, first):
    """End of stream at 160 k and 160 k + 1 samples, then a second stream on the same channels: the count ring and the
    frame grid start over, the core goes on.  After jamd_adin_cut_fvad_reset() the second stream alone is the
    single-stream fixture."""
    z, mode = fixture("fvad_b2_16k"), 1
    x = z["samples"]
    a, r, replay = gated_pair(engine, ref, model, [z[f"two{tag}{mode}"]] * 2, mode, 5, 0.5, {})
    same_push(a, r, [x[:first - 7000], x[:first]], [False, True])
    same_push(a, r, [x[first - 7000:first], x[:50000]], [True, False])
    same_push(a, r, [x, x[50000:]], [True, True])
    for c in range(2):
        replay[c].finish(len(z[f"two{tag}{mode}"]))
        assert np.array_equal(a.fvad_state(c)[:-1], z[f"two{tag}state{mode}"][:-1]), c
    a.fvad_reset(mask=[0, 1])
    r.ch[1].proceed.process = F.Replay(z[f"raw{mode}"])
    same_push(a, r, [np.zeros(0, np.int16), x], [False, True])
    r.ch[1].proceed.process.finish(F.gate_frames(len(x), 160))
    assert np.array_equal(a.fvad_state(1)[:-1], z[f"gstate{mode}"][:-1])
    assert np.array_equal(a.fvad_state(0)[:-1], z[f"two{tag}state{mode}"][:-1])
    a.close()
    r.close()


def test_refused_push_changes_nothing(engine, ref, model):
    """A push that needs more parts than max_parts returns JAMD_EINVAL and leaves the detector where it was: repeated
    with room it gives what an undisturbed run gives, detector state included."""
    z, mode = fixture("fvad_b2_16k"), 0
    x = z["samples"]
    a, r, replay = gated_pair(engine, ref, model, [z[f"raw{mode}"]], mode, 5, 0.5, {})
    same_push(a, r, [x[:30000]])
    before, det = a.state(0), a.fvad_state(0)
    with pytest.raises(lib.JamdError, match="max_parts is 1"):
        a.push_host([x[30000:]], [True], max_parts=1)
    assert a.state(0) == before and np.array_equal(a.fvad_state(0), det)
    same_push(a, r, [x[30000:]], [True])
    replay[0].finish(F.gate_frames(len(x), 160))
    assert np.array_equal(a.fvad_state(0)[:-1], z[f"gstate{mode}"][:-1])
    a.close()
    r.close()


LONG = dict(head_margin_msec=25000, tail_margin_msec=60000)    # margins with which a chunk_size of 320 000 is accepted


def test_gate_refusals(engine, model):
    ok = dict(mode=1, smoothnum=5, thres=0.5)
    for kw, desc, text in [(dict(sfreq=11025), dict(sfreq=11025), "takes 8000 or 16000"),
                           (dict(sfreq=32000), dict(sfreq=32000), "not served"),
                           (dict(sfreq=8000), {}, r"the detector's sfreq \(8000\) is not the cutting's \(16000\)"),
                           (dict(mode=4), {}, "mode 4 is not in 0 ... 3"),
                           (dict(smoothnum=0), {}, "smoothnum 0 is not in 1 ... 1000"),
                           (dict(smoothnum=1001), {}, "smoothnum 1001 is not in 1 ... 1000"),
                           (dict(thres=-0.1), {}, "thres -0.1 is not in 0 ... 1"),
                           (dict(thres=1.5), {}, "thres 1.5 is not in 0 ... 1"),
                           (dict(thres=float("nan")), {}, "thres -?nan is not in 0 ... 1"),
                           ({}, dict(chunk_size=319841, **LONG), "MAXSPEECHLEN")]:
        with pytest.raises(lib.JamdError, match=text):
            lib.AdinCut(engine, 1, fvad=lib.AdinCut.fvad_for(model, **{**ok, **kw}), **desc)
    with pytest.raises(lib.JamdError, match="the model is NULL"):
        lib.AdinCut(engine, 1, fvad=lib.AdinCut.fvad_for(None, **ok))
    lib.AdinCut(engine, 1, fvad=lib.AdinCut.fvad_for(model, **ok), chunk_size=319840, **LONG).close()
    plain = lib.AdinCut(engine, 1)
    with pytest.raises(lib.JamdError, match="made without the gate"):
        plain.fvad_reset()
    with pytest.raises(lib.JamdError, match="made without the gate"):
        plain.fvad_state(0)
    plain.close()


@pytest.mark.parametrize("sfreq,names,nchan", [(16000, ("fvad_b2_16k", "fvad_b3_16k"), 70), (8000, ("fvad_b2_8k",), 3)])
def test_gate_many_channels(engine, ref, model, sfreq, names, nchan):
    """More than a wave of gated channels in one call, each on its own schedule of unequal chunks with idle pushes in
    between, ending at different pushes; at 8 kHz the frame is 80 samples."""
    mode, fs = 2, sfreq // 100
    rng = np.random.default_rng(5)
    zs = [fixture(n) for n in names]
    src = [zs[c % len(zs)] for c in range(nchan)]
    a, r, replay = gated_pair(engine, ref, model, [s[f"raw{mode}"] for s in src], mode, 5, 0.5, {}, sfreq=sfreq)
    at, done = [0] * nchan, [False] * nchan
    for push in range(8):
        chunks, eos = [], []
        for c in range(nchan):
            left = len(src[c]["samples"]) - at[c]
            n = 0 if done[c] or rng.random() < 0.25 else left if push == 7 else int(rng.integers(0, min(left, 30000) + 1))
            chunks.append(src[c]["samples"][at[c]:at[c] + n])
            at[c] += n
            end = not done[c] and at[c] == len(src[c]["samples"]) and (n > 0 or push == 7)
            eos.append(end)
            done[c] = done[c] or end
        same_push(a, r, chunks, eos)
    for c in range(nchan):
        if done[c]:
            replay[c].finish(F.gate_frames(len(src[c]["samples"]), fs))
            assert np.array_equal(a.fvad_state(c)[:-1], src[c][f"gstate{mode}"][:-1]), c
    assert sum(done) > nchan // 2
    a.close()
    r.close()
