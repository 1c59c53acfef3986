"""Device audio front end (csrc/frontend.hip behind csrc/frontend_api.hip) where its kernels change path, bit for bit against the
compiled reference's Wav2MFCC() plus splicing (tests/test_frontend_gpu.py holds it at speech defaults):
windows from 16 to 4096 samples with and without zero padding, more than 64 channels / coefficients,
calls smaller than one workgroup of the frame kernel, delta windows longer than the utterance,
the per-utterance reductions at their block sizes, a thousand utterances in one call, one work area
reused by calls of different sizes, and the refusals that come before any launch.

The corpora are small and hold no runs of exact zeros (the -inf / NaN path is test_frontend_gpu.py's), and
every case first asserts that the REFERENCE's values are finite, so that no comparison is NaN == NaN."""
import ctypes as C

import numpy as np
import pytest

from julius_amd import lib, synth
from frontendref import EDGE_GEOMETRY, RefFrontend, first_diff, same

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 5, 11, 23, 64, 257)     # output frames per utterance of the geometry corpus: 366 in all
SENTINEL = np.float32(123.0)


@pytest.fixture(scope="module")
def rf(ref):
    return RefFrontend(ref)


def utt(fields, T, seed, spare=0):
    """Audio of exactly T frames: framesize + (T - 1) * frameshift samples plus `spare` (< frameshift)."""
    fs, sh = fields.get("framesize", 400), fields.get("frameshift", 160)
    assert 0 <= spare < sh
    return synth.make_audio(fs + (T - 1) * sh + spare, seed=seed, zero_runs=0)


def utts_of(fields, frames, seed):
    return [utt(fields, T, seed * 1000 + i, spare=i % 3) for i, T in enumerate(frames)]


def reference(rf, kind, vecsize, fields, utts, splice=1, min_finite=0.95):
    v = rf.para(lib.param_kind(kind), vecsize, **fields)
    want = [rf.wav2mfcc(u, v, splice=splice) for u in utts]
    finite = np.isfinite(np.concatenate(want)).mean()
    assert finite >= min_finite, f"only {finite:.3f} of the reference's values are finite"
    return want


def assert_equal(got, foff, want, what):
    assert list(foff) == list(np.concatenate([[0], np.cumsum([len(w) for w in want])])), what
    assert len(got) == foff[-1]
    for u, w in enumerate(want):
        g = got[foff[u]:foff[u + 1]]
        assert same(g, w), f"{what} utterance {u} ({len(w)} frames): {first_diff(g, w)}"


def check(engine, rf, kind, vecsize, fields, utts, splice=1, fe=None, what=""):
    fe = fe or lib.Frontend.from_kind(engine, kind, vecsize, splice=splice, **fields)
    want = reference(rf, kind, vecsize, fields, utts, splice)
    got, foff = fe.run_host(utts)
    assert_equal(got, foff, want, what)
    return want


def run_dev_spare_row(engine, fe, utts, stream=None):
    """run_dev into a buffer one row longer than the result, pre-filled: (features, frame_off, the spare row)."""
    samples, off = lib.Frontend._pack(utts)
    T = sum(fe.frames(len(u)) for u in utts)
    d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
    d_out = lib.DevBuf(engine, 4 * (T + 1) * fe.veclen).upload(np.full((T + 1, fe.veclen), SENTINEL))
    foff = fe.run_dev(d_in.ptr, off, d_out.ptr, stream=stream.value if stream else 0)
    if stream:
        assert lib.load().jamd_stream_sync(engine.h, stream) == 0
    out = d_out.download((T + 1, fe.veclen), np.float32)
    return out[:T], foff, out[T]


# ------------------------------------------------------------------ (a) window and filter-bank geometry
@pytest.mark.parametrize("name", list(EDGE_GEOMETRY))
def test_geometry(engine, rf, name):
    kind, vecsize, fields = EDGE_GEOMETRY[name]
    utts = utts_of(fields, FRAMES, list(EDGE_GEOMETRY).index(name) + 1)
    check(engine, rf, kind, vecsize, fields, utts, what=name)


# ------------------------------------------------------------------ (b) calls smaller than a workgroup
@pytest.mark.parametrize("name", ["fs512", "fs4096"])   # four and two frames per workgroup
def test_calls_smaller_than_a_workgroup(engine, rf, name):
    """Calls in which some or most waves of the last workgroup have no frame of their own: the features equal
    the reference's.  (Those waves would store into the work area, which no output shows; the spare row
    after the result guards the write kernel's bound only.)"""
    kind, vecsize, fields = EDGE_GEOMETRY[name]
    fe = lib.Frontend.from_kind(engine, kind, vecsize, **fields)
    calls = [utts_of(fields, (T,), 50 + T) for T in (1, 2, 3, 5)] + [utts_of(fields, (1, 1), 60)]
    for utts in calls:
        what = f"{name} call of {[fe.frames(len(u)) for u in utts]} frames"
        want = check(engine, rf, kind, vecsize, fields, utts, fe=fe, what=what)
        got, foff, spare = run_dev_spare_row(engine, fe, utts)
        assert_equal(got, foff, want, what + " (device entry)")
        assert (spare.view(np.uint32) == SENTINEL.view(np.uint32)).all(), what


# ------------------------------------------------------------------ (c) windows longer than the utterance
@pytest.mark.parametrize("delWin,accWin", [(1, 1), (2, 2), (5, 4), (1, 9), (9, 1)])
def test_windows_longer_than_the_utterance(engine, rf, delWin, accWin):
    fields = dict(delWin=delWin, accWin=accWin)
    utts = utts_of(fields, range(1, 2 * (delWin + accWin) + 3), 70 + delWin * 10 + accWin)
    check(engine, rf, "MFCC_E_D_A_Z", 39, fields, utts, what=f"delWin {delWin} accWin {accWin}")


# ------------------------------------------------------------------ (d) per-utterance reductions
# (frames, frame of the loudest window): the maximum of ENORMALISE sits where fe_emax_kernel changes path -- the
# last thread's first trip (254, 255), thread 0's second and third trip (256, 512), and, at 400 and 2900, a
# frame t with t % 512 >= 256, which a loop striding too far or a tree that drops its upper half never sees
REDUCTIONS = ((1, 0), (255, 254), (256, 255), (257, 256), (513, 512), (513, 400), (3000, 2900))


def reduction_utts(fields, seed):
    utts = utts_of(fields, [T for T, _ in REDUCTIONS], seed)
    fs, sh = fields.get("framesize", 400), fields.get("frameshift", 160)
    rng = np.random.default_rng(seed)
    for u, (T, loud) in zip(utts, REDUCTIONS):     # full-scale noise over exactly one window
        u[loud * sh:loud * sh + fs] = rng.integers(-30000, 30001, fs)
    return utts


@pytest.mark.parametrize("kind,vecsize,fields", [("MFCC_E_D_N_Z", 25, dict(enormal=1)), ("MFCC_E_D_A_Z", 39, dict(cvn=1))],
                         ids=["enormal", "mvn"])
def test_per_utterance_reductions(engine, rf, kind, vecsize, fields):
    """The 256-thread max of ENORMALISE and the serial sums of CMN / MVN at 1, 255, 256, 257, 513 and 3000
    frames (one frame under CVN divides 0 by 0 in the reference as well: 39 values of 178 000).  The
    reference's own un-normalised energy column has its maximum at the frames of REDUCTIONS."""
    utts = reduction_utts(fields, 90 + vecsize)
    v = rf.para(lib.param_kind("MFCC_E"), 13)
    assert [int(np.argmax(rf.wav2mfcc(u, v)[:, 12])) for u in utts] == [loud for _, loud in REDUCTIONS]
    check(engine, rf, kind, vecsize, fields, utts, what=kind)


# ------------------------------------------------------------------ (e) batch layout
@pytest.mark.parametrize("kind,vecsize", [("MFCC_E_D_A_Z", 39), ("MFCC_E_D_A", 39)])
def test_thousand_single_frame_utterances(engine, rf, kind, vecsize):
    utts = utts_of({}, [1] * 1000, 110)
    check(engine, rf, kind, vecsize, {}, utts, what=f"1000 x 1 frame {kind}")


@pytest.mark.parametrize("splice", [1, 2])
def test_thousand_short_utterances_spliced(engine, rf, splice):
    frames = np.random.default_rng(120).integers(1, 4, 1000)
    utts = [u for u, T in zip(utts_of({}, frames, 120), frames) if T >= splice]   # shorter than the splice: left out
    assert len(utts) >= 600
    check(engine, rf, "MFCC_E_D_N_Z", 25, {}, utts, splice=splice, what=f"1-3 frames, splice {splice}")


def test_one_utterance_less_than_a_wave_of_statistics(engine, rf):
    check(engine, rf, "MFCC_Z", 12, {}, utts_of({}, (37,), 130), what="MFCC_Z")   # nutt * veclen == 12


# ------------------------------------------------------------------ (f) work-area reuse
# ENORMALISE + CVN uses every buffer of the work area, but its one-frame call is all 0 / 0 in the reference
# too (a NaN pattern, which stale statistics would still break); ENORMALISE + CMN gives that call numbers
REUSE = {"enormal_cvn": ("MFCC_E_D_A_Z", 39, dict(enormal=1, cvn=1)), "enormal_cmn": ("MFCC_E_D_A_Z", 39, dict(enormal=1))}


def reuse_calls():
    rng = np.random.default_rng(140)
    large = [int(T) for T in rng.integers(2, 200, 200)]           # about 20 000 frames
    return [utts_of({}, (7, 40, 2), 141), utts_of({}, large, 142), utts_of({}, (3, 19, 5, 64, 2), 143),
            utts_of({}, (1,), 144)]


@pytest.fixture(scope="module", params=list(REUSE))
def reuse_reference(rf, request):
    calls = reuse_calls()
    kind, vecsize, fields = REUSE[request.param]
    want = [reference(rf, kind, vecsize, fields, utts, min_finite=0.0) for utts in calls]
    assert np.isfinite(np.concatenate([w for call in want for w in call])).mean() >= 0.95
    assert all(np.isfinite(np.concatenate(call)).mean() >= 0.95 for call in want[:3])
    assert request.param == "enormal_cvn" or np.isfinite(want[3][0]).all()
    return REUSE[request.param], calls, want


def test_work_area_reuse(engine, reuse_reference):
    """Small, large, small with another nutt, one frame: the buffers grow once and are then reused, and the
    per-utterance statistics are laid out anew for every nutt."""
    (kind, vecsize, fields), calls, want = reuse_reference
    fe = lib.Frontend.from_kind(engine, kind, vecsize, **fields)
    for i, (utts, w) in enumerate(zip(calls, want)):
        got, foff = fe.run_host(utts)
        assert_equal(got, foff, w, f"call {i} on the reused object")
        fresh, foff1 = lib.Frontend.from_kind(engine, kind, vecsize, **fields).run_host(utts)
        assert np.array_equal(foff, foff1) and same(got, fresh), f"call {i}: reused and fresh objects differ"


def test_work_area_reuse_device_entry(engine, reuse_reference):
    (kind, vecsize, fields), calls, want = reuse_reference
    fe = lib.Frontend.from_kind(engine, kind, vecsize, **fields)
    s = C.c_void_p()
    assert lib.load().jamd_stream_create(engine.h, C.byref(s)) == 0
    try:
        for i in (1, 2):                                           # small after large, on the caller's stream
            got, foff, spare = run_dev_spare_row(engine, fe, calls[i], stream=s)
            assert_equal(got, foff, want[i], f"call {i} on a caller's stream")
            assert (spare.view(np.uint32) == SENTINEL.view(np.uint32)).all()
    finally:
        lib.load().jamd_stream_destroy(engine.h, s)


# ------------------------------------------------------------------ (g) refusals before any launch
@pytest.mark.parametrize("fields", [dict(framesize=1), dict(framesize=4097), dict(frameshift=0), dict(fbank_num=0)],
                         ids=["framesize1", "framesize4097", "frameshift0", "fbank_num0"])
def test_refused_geometry(engine, fields):
    d = lib.Frontend.desc_for("MFCC_E_D_A_Z", 39, **fields)
    h = C.c_void_p()
    assert lib.load().jamd_frontend_create(engine.h, C.byref(d), C.byref(h)) == -1
    assert h.value is None and b"out of range" in lib.load().jamd_last_error()


@pytest.mark.parametrize("nutt,off", [(0, [0, 4000]), (2, [0, 4000, 3000])], ids=["nutt0", "decreasing"])
def test_refused_calls_write_nothing(engine, nutt, off):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_N_Z", 25)
    samples = synth.make_audio(8000, seed=150, zero_runs=0)
    off = np.array(off, np.int64)
    out = np.full((64, fe.veclen), SENTINEL)
    foff = np.full(3, -7, np.int32)
    L = lib.load()
    rc = L.jamd_frontend_run_host(fe.h, samples.ctypes.data, off.ctypes.data, nutt, out.ctypes.data, foff.ctypes.data)
    assert rc == -1 and L.jamd_last_error()
    assert (out == SENTINEL).all() and (foff == -7).all()
    d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
    d_out = lib.DevBuf(engine, out.nbytes).upload(out)
    rc = L.jamd_frontend_run_dev(fe.h, d_in.ptr, off.ctypes.data, nutt, d_out.ptr, foff.ctypes.data, None)
    assert rc == -1 and L.jamd_last_error()
    assert L.jamd_engine_sync(engine.h) == 0
    assert (d_out.download(out.shape, np.float32) == SENTINEL).all() and (foff == -7).all()
