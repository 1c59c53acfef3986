"""Spectral subtraction of the device front end (jamd_frontend_set_ss, jamd_frontend_noise_*; csrc/frontend.hip behind csrc/frontend_api.hip)
against the compiled reference, bit for bit (NaN as NaN): the noise spectrum against new_SS_calculate(), the features
of -sscalc / -ssload against Wav2MFCC() with that spectrum on its work area plus libjulius' splicing.

Every corpus of a feature test with alpha >= 0.5 is first shown to take BOTH branches of the subtraction: the share
of (frame, FFT index) pairs that are floored, computed from the samples by a plain numpy restatement
(frontendssref.floor_share), lies in [0.10, 0.90].  The alpha 0 and NaN cases are edge cases by design and exempt."""
import ctypes as C

import numpy as np
import pytest

from julius_amd import lib, synth
from frontendref import EDGE_GEOMETRY, first_diff, same
from frontendssref import RefFrontendSS, floor_share, frame_spectra

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(123.0)


@pytest.fixture(scope="module")
def rf(ref):
    return RefFrontendSS(ref)


# ------------------------------------------------------------------ corpora (pure functions of their arguments)
def speech(n, seed, loud_head=False, sfreq=16000):
    """Synthetic speech without runs of exact zeros; loud_head overwrites the first 0.3 s (or a third of a short
    utterance) with Gaussian noise of sigma 3000, so that its own head spectrum floors much of what follows."""
    a = synth.make_audio(int(n), seed=seed, sfreq=sfreq, zero_runs=0)
    if loud_head:
        h = min(int(0.3 * sfreq), int(n) // 3)
        a[:h] = np.clip(np.round(np.random.default_rng(seed + 7000).normal(0, 3000, h)), -32768, 32767)
    return a


def frames_len(fields, T, spare=0):
    return fields.get("framesize", 400) + (T - 1) * fields.get("frameshift", 160) + spare


def corpus(fields, seed, frames=(1, 2, 3, 5, 11, 40, 97, 190)):
    """Utterances of exactly `frames` frames (plus a few spare samples), every second one with a loud head."""
    return [speech(frames_len(fields, T, spare=i % 3), seed * 100 + i, loud_head=i % 2 == 1) for i, T in enumerate(frames)]


def table_info(kind, vecsize, fields):
    d = lib.Frontend.desc_for(kind, vecsize, **fields)
    a = np.zeros(4, np.int32)
    assert lib.load().jamd_frontend_table(C.byref(d), b"info", a.ctypes.data, 4) == 4
    return d, tuple(int(x) for x in a)            # fftN, n, klo, khi


def head_of(d, calc_len_ms, n):
    return min(calc_len_ms * d.smp_freq // 1000, n)


def share_calc(d, info, utts, calc_len_ms, alpha):
    """Floored share of a -sscalc corpus in numpy: the noise of an utterance is the mean |X| of its head frames."""
    fftN, _, klo, khi = info
    fl, n = 0.0, 0
    for u in utts:
        sp = frame_spectra(u, d.framesize, d.frameshift, fftN, d.preEmph)
        H = (head_of(d, calc_len_ms, len(u)) - d.framesize) // d.frameshift + 1
        w = sp.shape[0] * (khi - klo + 1)
        fl += floor_share(sp, sp[:H].mean(axis=0), alpha, klo, khi) * w
        n += w
    return fl / n


def share_load(d, info, utts, noise, alpha):
    fftN, _, klo, khi = info
    sp = np.concatenate([frame_spectra(u, d.framesize, d.frameshift, fftN, d.preEmph) for u in utts])
    return floor_share(sp, noise, alpha, klo, khi)


def assert_both_branches(share, what):
    assert 0.10 <= share <= 0.90, f"{what}: {share:.3f} of the (frame, index) pairs are floored -- the corpus shows one branch only"


def assert_equal(got, foff, want, what):
    assert list(foff) == list(np.concatenate([[0], np.cumsum([len(w) for w in want])])), what
    for u, w in enumerate(want):
        g = got[foff[u]:foff[u + 1]]
        assert same(g, w), f"{what} utterance {u} ({len(w)} frames): {first_diff(g, w)}"


# ------------------------------------------------------------------ (a) the noise spectrum
def check_noise(engine, rf, kind, vecsize, fields, utts, head, what):
    fe = lib.Frontend.from_kind(engine, kind, vecsize, **fields)
    v = rf.para(lib.param_kind(kind), vecsize, **fields)
    want = np.stack([rf.noise(u, v, min(head, len(u)) if head > 0 else len(u)) for u in utts])
    assert want.shape == (len(utts), fe.fftn) and np.isfinite(want).all() and (want > 0).mean() > 0.9
    got = fe.noise_host(utts, head)
    assert same(got, want), f"{what}: {first_diff(got, want)}"
    return fe, want


NOISE_CONFIGS = {"defaults": ("MFCC_E_D_A_Z", 39, {}), "zmeanframe": ("MFCC_E_D_A_Z", 39, dict(zmeanframe=1)),
                 "preEmph0": ("MFCC_E_D_A_Z", 39, dict(preEmph=0.0))}
NOISE_CONFIGS.update({k: EDGE_GEOMETRY[k] for k in ("fs16", "fs33", "fs257", "fs512", "fs4096", "gap")})


@pytest.mark.parametrize("name", list(NOISE_CONFIGS))
def test_noise_spectrum(engine, rf, name):
    """noise_host == new_SS_calculate() over a head of 12 frames and a few samples (shorter utterances: all of them)."""
    kind, vecsize, fields = NOISE_CONFIGS[name]
    utts = corpus(fields, 10 + list(NOISE_CONFIGS).index(name), frames=(1, 2, 3, 5, 11, 12, 13, 40))
    check_noise(engine, rf, kind, vecsize, fields, utts, frames_len(fields, 12, spare=5), name)


@pytest.mark.parametrize("head", [400, 400 + 160 - 1, 400 + 160, 10 ** 7], ids=["one_frame", "still_one_frame", "two_frames", "capped"])
def test_noise_head_lengths(engine, rf, head):
    """A head of exactly one frame, of framesize + frameshift - 1 samples (still one frame), of two frames, and one
    longer than every utterance (capped at the utterance)."""
    utts = corpus({}, 30)
    fe, want = check_noise(engine, rf, "MFCC_E_D_A_Z", 39, {}, utts, head, f"head {head}")
    if head == 400 + 160 - 1:
        assert same(want, fe.noise_host(utts, 400))
    if head == 400 + 160:
        assert not same(want, fe.noise_host(utts, 400))


def test_noise_whole_utterance_long_chain(engine, rf):
    """head_samples = 0: the whole utterance, as mkss.  The first has 330 frames: summed as a tree instead of the
    reference's chain of float roundings, its spectrum would differ (shown on the inputs in numpy)."""
    utts = [speech(frames_len({}, 330), 41), speech(frames_len({}, 7, spare=100), 42), speech(400, 43)]
    mags = frame_spectra(utts[0])
    chain = np.zeros(512, np.float32)
    for row in mags:
        chain = (chain.astype(np.float64) + row).astype(np.float32)
    assert (chain != mags.astype(np.float32).sum(axis=0, dtype=np.float32)).any()
    check_noise(engine, rf, "MFCC_E_D_A_Z", 39, {}, utts, 0, "whole utterance")


def ragged(seed, n=40):
    rng = np.random.default_rng(seed)
    return [speech(int(rng.integers(1600, 48000)), seed * 100 + i, loud_head=i % 2 == 1) for i in range(n)]


def test_noise_ragged_batch_equals_single_calls(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    utts = ragged(50)
    got = fe.noise_host(utts, 4800)
    assert np.isfinite(got).all() and got[1].mean() > 5 * got[0].mean()      # loud and quiet heads
    for u, a in enumerate(utts):
        assert same(got[u:u + 1], fe.noise_host([a], 4800)), u


def test_noise_device_entry_on_a_callers_stream(engine, rf):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    utts = corpus({}, 60)
    want = fe.noise_host(utts, 4800)
    v = rf.para(lib.param_kind("MFCC_E_D_A_Z"), 39)
    assert same(want[5], rf.noise(utts[5], v, 4800))
    samples, off = lib.Frontend._pack(utts)
    d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
    d_out = lib.DevBuf(engine, 4 * (len(utts) + 1) * fe.fftn).upload(np.full((len(utts) + 1, fe.fftn), SENTINEL))
    s = C.c_void_p()
    assert lib.load().jamd_stream_create(engine.h, C.byref(s)) == 0
    try:
        fe.noise_dev(d_in.ptr, off, d_out.ptr, head_samples=4800, stream=s.value)
        assert lib.load().jamd_stream_sync(engine.h, s) == 0
    finally:
        lib.load().jamd_stream_destroy(engine.h, s)
    out = d_out.download((len(utts) + 1, fe.fftn), np.float32)
    assert same(out[:-1], want) and (out[-1].view(np.uint32) == SENTINEL.view(np.uint32)).all()


def test_noise_head_without_a_frame_writes_nothing(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    utts = [speech(4000, 70), speech(399, 71)]
    samples, off = lib.Frontend._pack(utts)
    out = np.full((2, fe.fftn), SENTINEL)
    L = lib.load()
    assert L.jamd_frontend_noise_host(fe.h, samples.ctypes.data, off.ctypes.data, 2, 0, out.ctypes.data) == -1
    assert b"no full frame" in L.jamd_last_error() and (out == SENTINEL).all()
    assert L.jamd_frontend_noise_host(fe.h, samples.ctypes.data, off.ctypes.data, 1, 399, out.ctypes.data) == -1
    d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
    d_out = lib.DevBuf(engine, out.nbytes).upload(out)
    assert L.jamd_frontend_noise_dev(fe.h, d_in.ptr, off.ctypes.data, 2, 0, d_out.ptr, None) == -1
    assert L.jamd_engine_sync(engine.h) == 0 and (d_out.download(out.shape, np.float32) == SENTINEL).all()


# ------------------------------------------------------------------ (b) -sscalc features
def reference_calc(rf, kind, vecsize, fields, utts, calc_len_ms, alpha, floor, splice=1):
    v = rf.para(lib.param_kind(kind), vecsize, **fields)
    want = []
    for u in utts:
        nz = rf.noise(u, v, min(calc_len_ms * v.smp_freq // 1000, len(u)))
        want.append(rf.wav2mfcc_ss(u, v, nz, alpha, floor, splice=splice))
    return want


def check_calc(engine, rf, kind, vecsize, fields, utts, calc_len_ms=300, alpha=2.0, floor=0.5, splice=1, what="",
               both_branches=True, min_finite=0.95):
    d, info = table_info(kind, vecsize, fields)
    if both_branches:
        assert_both_branches(share_calc(d, info, utts, calc_len_ms, alpha), what)
    want = reference_calc(rf, kind, vecsize, fields, utts, calc_len_ms, alpha, floor, splice)
    assert np.isfinite(np.concatenate(want)).mean() >= min_finite, what
    fe = lib.Frontend.from_kind(engine, kind, vecsize, splice=splice, **fields)
    fe.set_ss(lib.SS_CALC, calc_len_ms=calc_len_ms, alpha=alpha, floor=floor)
    got, foff = fe.run_host(utts)
    assert_equal(got, foff, want, what)
    return fe, want


CALC_KINDS = {
    "mfcc_e_d_a_z": ("MFCC_E_D_A_Z", 39, {}, 1),
    "mfcc_e_d_n_z_splice3": ("MFCC_E_D_N_Z", 25, {}, 3),
    "mfcc_0_d_a_z": ("MFCC_0_D_A_Z", 39, {}, 1),
    "fbank_d_a_z": ("FBANK_D_A_Z", 72, {}, 1),
    "melspec_power": ("MELSPEC", 24, dict(usepower=1), 1),          # |X|^2 behind the subtraction
    "cvn": ("MFCC_E_D_A_Z", 39, dict(cvn=1), 1),
}
CALC_KINDS.update({k: EDGE_GEOMETRY[k] + (1,) for k in ("band_clamps", "narrow_band", "fs16", "fs512", "fs4096")})
FEATURE_FRAMES = (3, 5, 11, 40, 97, 190, 64, 33)     # every utterance holds the splice and more than one frame under CVN


@pytest.mark.parametrize("name", list(CALC_KINDS))
def test_sscalc_features(engine, rf, name):
    kind, vecsize, fields, splice = CALC_KINDS[name]
    utts = corpus(fields, 80 + list(CALC_KINDS).index(name), frames=FEATURE_FRAMES)
    # (a quarter of a second of fs4096's 256 ms window would be refused: 300 ms holds one frame of every geometry)
    check_calc(engine, rf, kind, vecsize, fields, utts, splice=splice, what=name)


@pytest.mark.parametrize("calc_len_ms", [25, 300, 5000])
def test_sscalc_head_lengths(engine, rf, calc_len_ms):
    """25 ms is one frame at the defaults, 5000 ms longer than every utterance here (capped at its length)."""
    utts = corpus({}, 100, frames=FEATURE_FRAMES)
    assert max(len(u) for u in utts) < 5000 * 16
    check_calc(engine, rf, "MFCC_E_D_A_Z", 39, {}, utts, calc_len_ms=calc_len_ms, what=f"{calc_len_ms} ms")


@pytest.mark.parametrize("alpha,floor", [(2.0, 0.5), (0.5, 0.1), (0.0, 0.5), (2.0, 0.0)],
                         ids=["a2_f05", "a05_f01", "alpha0", "floor0"])
def test_sscalc_alpha_and_floor(engine, rf, alpha, floor):
    """alpha 0 never floors (H is 1, or NaN where |X| is 0); floor 0 zeroes what it floors, and a channel of zeros is
    clamped to 1 before the log."""
    utts = corpus({}, 110, frames=FEATURE_FRAMES)
    check_calc(engine, rf, "MFCC_E_D_A_Z", 39, {}, utts, alpha=alpha, floor=floor, what=f"alpha {alpha} floor {floor}",
               both_branches=alpha >= 0.5)


# ------------------------------------------------------------------ (c) where the reference divides 0 by 0
def test_nan_edge(engine, rf):
    """A head of exact zeros gives a zero noise spectrum: alpha * NP^2 is 0, and in a frame of exact zeros |X| is 0
    too, so H = sqrt(0) / 0.  The reference carries that NaN through the log, the DCT and the CMN sums."""
    a = speech(16000, 120)
    a[:4800] = 0
    a[9000:9000 + 2 * 400 + 100] = 0                 # a run of more than two windows: whole frames of zeros
    utts = [a, np.zeros(4000, np.int16), speech(8000, 121)]
    want = reference_calc(rf, "MFCC_E_D_A_Z", 39, {}, utts, 300, 2.0, 0.5)
    assert np.isnan(want[0]).any() and np.isnan(want[1][:, :12]).all() and np.isfinite(want[2]).all()
    v = rf.para(lib.param_kind("MFCC_E_D_A", ), 39)   # without CMN the NaN stays in the frames of zeros
    nz = rf.noise(a, v, 4800)
    assert (nz == 0).all()
    plain = rf.wav2mfcc_ss(a, v, nz)
    rows = np.isnan(plain[:, :12]).any(axis=1)
    assert 0 < rows.sum() < len(rows)
    for kind, w in (("MFCC_E_D_A_Z", want), ("MFCC_E_D_A", None)):
        fe = lib.Frontend.from_kind(engine, kind, 39)
        fe.set_ss(lib.SS_CALC)
        w = w or reference_calc(rf, kind, 39, {}, utts, 300, 2.0, 0.5)
        got, foff = fe.run_host(utts)
        assert_equal(got, foff, w, f"NaN edge {kind}")


# ------------------------------------------------------------------ (d) -ssload
def noise_recording(seed=130, n=16000):
    """Background noise of its own: Gaussian, sigma 1500, slightly coloured."""
    x = np.random.default_rng(seed).normal(0, 1500, n + 1)
    return np.clip(np.round(x[1:] + 0.5 * x[:-1]), -32768, 32767).astype(np.int16)


def check_load(engine, rf, fe, noise, utts, alpha=2.0, floor=0.5, what=""):
    d, info = table_info("MFCC_E_D_A_Z", 39, {})
    assert_both_branches(share_load(d, info, utts, noise, alpha), what)
    v = rf.para(lib.param_kind("MFCC_E_D_A_Z"), 39)
    want = [rf.wav2mfcc_ss(u, v, noise, alpha, floor) for u in utts]
    assert np.isfinite(np.concatenate(want)).mean() >= 0.95
    fe.set_ss(lib.SS_LOAD, alpha=alpha, floor=floor, noise=noise)
    got, foff = fe.run_host(utts)
    assert_equal(got, foff, want, what)
    return want


def test_ssload(engine, rf, tmp_path):
    """One spectrum -- noise_host over a separate noise recording, through ss_write / ss_read -- for a whole batch;
    then the same with exact zeros in it (alpha * 0 subtracts nothing: H = sqrt(P^2) / P)."""
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    spec = fe.noise_host([noise_recording()])[0]
    lib.ss_write(tmp_path / "noise.ss", spec)
    noise = lib.ss_read(tmp_path / "noise.ss")
    assert noise.tobytes() == spec.tobytes() and len(noise) == fe.fftn == 512
    assert rf.load(tmp_path / "noise.ss").tobytes() == spec.tobytes()
    utts = corpus({}, 140, frames=FEATURE_FRAMES)
    check_load(engine, rf, fe, noise, utts, what="-ssload")
    holes = noise.copy()
    holes[::5] = 0.0
    check_load(engine, rf, fe, holes, utts, alpha=0.5, floor=0.1, what="-ssload with zero entries")


def test_ssload_wrong_length_is_refused(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    utts = corpus({}, 150, frames=(3, 20))
    before, _ = fe.run_host(utts)
    for n in (511, 513, 256, 0):
        with pytest.raises(lib.JamdError, match="fftN"):
            fe.set_ss(lib.SS_LOAD, noise=np.ones(n, np.float32))
    after, _ = fe.run_host(utts)
    assert same(before, after)


# ------------------------------------------------------------------ (e) isolation
def test_sscalc_ragged_batch_equals_single_calls(engine):
    """40 ragged utterances, every second one with a loud head: the spectra differ by an order of magnitude, so a
    frame that took a neighbour's spectrum would show."""
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    fe.set_ss(lib.SS_CALC)
    utts = ragged(160)
    d, info = table_info("MFCC_E_D_A_Z", 39, {})
    assert_both_branches(share_calc(d, info, utts, 300, 2.0), "ragged batch")
    nz = fe.noise_host(utts, 4800)
    assert nz[1::2].mean() > 5 * nz[0::2].mean()
    got, foff = fe.run_host(utts)
    for u, a in enumerate(utts):
        one, _ = fe.run_host([a])
        assert same(got[foff[u]:foff[u + 1]], one), u


def test_scratch_reuse_large_then_small(engine, rf):
    """A call of 64 utterances, then one of 3 on the same object: the head-frame scratch and the per-utterance spectra
    are laid out anew."""
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    fe.set_ss(lib.SS_CALC)
    large = ragged(170, n=64)
    small = corpus({}, 171, frames=(5, 64, 12))
    got_large, foff_large = fe.run_host(large)
    got, foff = fe.run_host(small)
    assert_equal(got, foff, reference_calc(rf, "MFCC_E_D_A_Z", 39, {}, small, 300, 2.0, 0.5), "3 after 64")
    again, foff2 = fe.run_host(large)
    assert np.array_equal(foff2, foff_large) and same(again, got_large)
    want7 = reference_calc(rf, "MFCC_E_D_A_Z", 39, {}, large[7:8], 300, 2.0, 0.5)[0]
    assert same(got_large[foff_large[7]:foff_large[8]], want7)


def test_mode_switches_equal_fresh_objects(engine):
    """OFF after CALC is the front end without SS, bit for bit; CALC after LOAD and LOAD after CALC equal fresh objects."""
    utts = corpus({}, 180, frames=FEATURE_FRAMES)
    new = lambda: lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    noise = new().noise_host([noise_recording(181)])[0]
    plain, _ = new().run_host(utts)
    f = new(); f.set_ss(lib.SS_CALC)
    calc, _ = f.run_host(utts)
    f = new(); f.set_ss(lib.SS_LOAD, noise=noise)
    load, _ = f.run_host(utts)
    assert not same(plain, calc) and not same(plain, load) and not same(calc, load)
    fe = new()
    for mode, want in ((lib.SS_CALC, calc), (lib.SS_OFF, plain), (lib.SS_LOAD, load), (lib.SS_CALC, calc), (lib.SS_LOAD, load),
                       (lib.SS_OFF, plain)):
        fe.set_ss(mode, noise=noise if mode == lib.SS_LOAD else None)
        got, _ = fe.run_host(utts)
        assert same(got, want), f"after switching to mode {mode}"


# ------------------------------------------------------------------ (f) refusals
def test_refusals_leave_the_previous_mode_working(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    utts = corpus({}, 190, frames=(3, 40, 11))
    fe.set_ss(lib.SS_CALC, calc_len_ms=200, alpha=1.5, floor=0.2)
    before, _ = fe.run_host(utts)
    L = lib.load()
    for bad, word in ((dict(mode=lib.SS_CALC, calc_len_ms=24), b"shorter than a frame"),     # 24 * 16000 / 1000 = 384 < 400
                      (dict(mode=lib.SS_CALC, calc_len_ms=0), b"shorter than a frame"),
                      (dict(mode=7), b"unknown mode"), (dict(mode=-1), b"unknown mode"),
                      (dict(mode=lib.SS_LOAD), b"JAMD_SS_LOAD")):
        with pytest.raises(lib.JamdError):
            fe.set_ss(**bad)
        assert word in L.jamd_last_error()
        after, _ = fe.run_host(utts)
        assert same(before, after), bad
    fe.set_ss(lib.SS_CALC, calc_len_ms=25)           # 400 samples: exactly a frame is taken
    assert L.jamd_frontend_set_ss(fe.h, None) == -1 and L.jamd_frontend_set_ss(None, None) == -1
    assert L.jamd_frontend_fftn(fe.h) == 512 and L.jamd_frontend_fftn(None) == -1
