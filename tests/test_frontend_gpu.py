"""Device audio front end (csrc/frontend.hip behind csrc/frontend_api.hip) against the compiled reference's Wav2MFCC()
(libsent/src/wav2mfcc/wav2mfcc-buffer.c) plus libjulius' splicing, bit for bit.

Where the reference produces NaN (an all-zero utterance under ENORMALISE: -inf - -inf), the device
must produce NaN too; the payload differs by architecture (x86's default NaN has the sign bit set), so
NaN is compared as NaN and every other value by its bits."""
import ctypes as C

import numpy as np
import pytest

from julius_amd import lib, synth
from frontendref import RefFrontend, first_diff, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rf(ref):
    return RefFrontend(ref)


# (name, kind, vecsize, fields, extra) -- extra: splice, cmean / cvar generation, static_cvn_only
CONFIGS = [
    ("mfcc_e_d_a_z", "MFCC_E_D_A_Z", 39, {}, {}),
    ("mfcc_e_d_n_z", "MFCC_E_D_N_Z", 25, {}, {}),
    ("mfcc_e_d_a", "MFCC_E_D_A", 39, {}, {}),
    ("mfcc_0_d_a_z", "MFCC_0_D_A_Z", 39, {}, {}),
    ("fbank_d_a_z", "FBANK_D_A_Z", 72, {}, {}),
    ("melspec", "MELSPEC", 24, {}, {}),
    ("raw_e_enormal", "MFCC_E_D_A_Z", 39, dict(raw_e=1, enormal=1, escale=0.1, silFloor=50.0), {}),
    ("enormal_windowed", "MFCC_E_D_N_Z", 25, dict(enormal=1, escale=0.3, silFloor=30.0), {}),
    ("zmean_power", "MFCC_E_D_N_Z", 25, dict(zmeanframe=1, usepower=1), {}),
    ("mvn", "MFCC_E_D_A_Z", 39, dict(cvn=1), {}),
    ("cvn_only", "MFCC_E_D_A", 39, dict(cvn=1), {}),
    ("static_cmn", "MFCC_E_D_A_Z", 39, {}, dict(cmean=True)),
    ("static_cmn_cvn", "MFCC_E_D_A_Z", 39, dict(cvn=1), dict(cmean=True, cvar=True)),
    ("static_cvn_only", "MFCC_E_D_A_Z", 39, dict(cvn=1), dict(cmean=True, cvar=True, static_cvn_only=True)),
    ("lifter_windows", "MFCC_0_E_D_A", 42, dict(lifter=0, fbank_num=26, delWin=3, accWin=1, preEmph=0.0), {}),
    ("lifter15", "MFCC_E_D_A_Z", 39, dict(lifter=15, frameshift=100, framesize=300), {}),
    ("vtln_cut", "MFCC_E_D_A_Z", 39, dict(vtln_alpha=1.08, vtln_lower=250.0, vtln_upper=6500.0, lopass=100,
                                          hipass=7600), {}),
    ("fft1024", "MFCC_E_D_N_Z", 25, dict(framesize=640, frameshift=160), {}),
    ("fft2048_48k", "MFCC_E_D_A_Z", 39, dict(smp_period=208, smp_freq=48000, framesize=1200, frameshift=480,
                                             fbank_num=40), {}),
    ("fft4096_48k", "MFCC_E_D_N_Z", 25, dict(smp_period=208, smp_freq=48000, framesize=2400, frameshift=480,
                                             fbank_num=40), {}),   # 50 ms: two frames per workgroup
    ("splice3", "MFCC_E_D_N_Z", 25, {}, dict(splice=3)),
    ("fbank_8k", "FBANK_D_A_Z", 60, dict(smp_period=1250, smp_freq=8000, framesize=200, frameshift=80), {}),
]


def corpus(fields, seed, seconds=120.0, long_utt=False, splice=1):
    """Utterances for one configuration: one output frame exactly, fewer frames than the delta window,
    an all-zero one, one clipped at both rails, then synthetic speech of random lengths (every fourth
    with a run of exact zeros: frames inside one have -inf energy, which the reference carries on)."""
    fs = fields.get("framesize", 400)
    sh = fields.get("frameshift", 160)
    sfreq = 10000000 // fields.get("smp_period", 625)
    rng = np.random.default_rng(seed)
    one = fs + (splice - 1) * sh
    utts = [synth.make_audio(one, seed=seed * 100 + 1), synth.make_audio(one + 2 * sh, seed=seed * 100 + 2),
            np.zeros(one + 10 * sh, np.int16)]
    clipped = synth.make_audio(fs + 50 * sh, seed=seed * 100 + 3)
    clipped[::7] = 32767
    clipped[3::7] = -32768
    utts.append(clipped)
    total = sum(len(u) for u in utts)
    k = 4
    while total < seconds * sfreq:
        n = int(rng.uniform(0.3, 6.0) * sfreq)
        utts.append(synth.make_audio(n, seed=seed * 100 + k, sfreq=sfreq, zero_runs=int(k % 4 == 0)))
        total += n
        k += 1
    if long_utt:
        utts.append(synth.make_audio(60 * sfreq, seed=seed * 100 + 99, sfreq=sfreq))
    return utts


def build(engine, kind, vecsize, fields, extra):
    d = lib.Frontend.desc_for(kind, vecsize, splice=extra.get("splice", 1),
                              static_cvn_only=int(extra.get("static_cvn_only", False)), **fields)
    rng = np.random.default_rng(7)
    cmean = rng.normal(0, 3, d.veclen).astype(np.float32) if extra.get("cmean") else None
    cvar = rng.uniform(0.5, 4.0, d.veclen).astype(np.float32) if extra.get("cvar") else None
    return lib.Frontend(engine, d, cmean, cvar), cmean, cvar


def reference(rf, kind, vecsize, fields, extra, utts, cmean, cvar):
    v = rf.para(lib.param_kind(kind), vecsize, **fields)
    return [rf.wav2mfcc(u, v, splice=extra.get("splice", 1), cmean=cmean, cvar=cvar,
                        static_cvn_only=extra.get("static_cvn_only", False)) for u in utts]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_features_match_reference(engine, rf, cfg):
    name, kind, vecsize, fields, extra = cfg
    seed = CONFIGS.index(cfg) + 1
    utts = corpus(fields, seed, long_utt=name in ("mfcc_e_d_n_z", "mfcc_e_d_a_z"), splice=extra.get("splice", 1))
    fe, cmean, cvar = build(engine, kind, vecsize, fields, extra)
    want = reference(rf, kind, vecsize, fields, extra, utts, cmean, cvar)
    got, foff = fe.run_host(utts)
    assert list(np.diff(foff)) == [len(w) for w in want]
    for u, w in enumerate(want):
        g = got[foff[u]:foff[u + 1]]
        assert same(g, w), f"{name} utterance {u} ({len(utts[u])} samples): {first_diff(g, w)}"
    if name in ("mfcc_e_d_n_z", "raw_e_enormal"):   # the all-zero utterance: -inf energies, NaN after ENORMALISE
        assert np.isinf(want[2]).any() or np.isnan(want[2]).any()


def test_corpus_size():
    n = 0
    for i, (name, kind, vecsize, fields, extra) in enumerate(CONFIGS):
        fs, sh = fields.get("framesize", 400), fields.get("frameshift", 160)
        n += sum((len(u) - fs) // sh + 1 for u in corpus(fields, i + 1, long_utt=name in ("mfcc_e_d_n_z", "mfcc_e_d_a_z"),
                                                         splice=extra.get("splice", 1)))
    assert n >= 200000, n


def test_ragged_batch_equals_single_calls(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_N_Z", 25, enormal=1, raw_e=1, splice=2)
    rng = np.random.default_rng(11)
    utts = [synth.make_audio(int(rng.integers(400 + 160, 16000 * 3)), seed=500 + i) for i in range(80)]
    got, foff = fe.run_host(utts)
    for u in range(len(utts)):
        one, f1 = fe.run_host([utts[u]])
        assert same(got[foff[u]:foff[u + 1]], one), u


def test_device_entry_equals_host_entry(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39, cvn=1)
    utts = [synth.make_audio(n, seed=900 + i) for i, n in enumerate((4000, 16000, 400, 32123, 720))]
    want, foff = fe.run_host(utts)
    samples, off = lib.Frontend._pack(utts)
    d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
    d_out = lib.DevBuf(engine, want.nbytes)
    s = C.c_void_p()
    assert lib.load().jamd_stream_create(engine.h, C.byref(s)) == 0
    try:
        f2 = fe.run_dev(d_in.ptr, off, d_out.ptr, stream=s.value)
        assert lib.load().jamd_stream_sync(engine.h, s) == 0
    finally:
        lib.load().jamd_stream_destroy(engine.h, s)
    assert np.array_equal(f2, foff)
    assert same(d_out.download(want.shape, np.float32), want)


@pytest.mark.parametrize("fields", [dict(ss=1), dict(realtime=1), dict(basetype=1), dict(paramtype=7 | 0x40, basetype=7,
                                                                                          energy=1)])
def test_refused_configurations(engine, fields):
    d = lib.Frontend.desc_for("MFCC_E_D_A_Z", 39, **fields)
    h = C.c_void_p()
    assert lib.load().jamd_frontend_create(engine.h, C.byref(d), C.byref(h)) == -1
    assert h.value is None and lib.load().jamd_last_error()


def test_too_short_utterance_writes_nothing(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_N_Z", 25, splice=3)
    utts = [synth.make_audio(4000, seed=1), synth.make_audio(400 + 160, seed=2)]   # 2 frames < splice 3
    samples, off = lib.Frontend._pack(utts)
    out = np.full((64, fe.veclen), 123.0, np.float32)
    foff = np.full(3, -7, np.int32)
    rc = lib.load().jamd_frontend_run_host(fe.h, samples.ctypes.data, off.ctypes.data, 2, out.ctypes.data,
                                           foff.ctypes.data)
    assert rc == -1 and b"too short" in lib.load().jamd_last_error()
    assert (out == 123.0).all() and (foff == -7).all()


def test_features_feed_scoring(engine, rf):
    """samples -> device features -> jamd_gmm_outprob_utts_dev, no host copy, equals scoring the
    reference's features."""
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_N_Z", 25)
    m = synth.make_gmm(S=300, M=8, D=25, seed=3)
    gm = lib.Gmm(engine, m)
    utts = [synth.make_audio(n, seed=40 + i) for i, n in enumerate((16000, 8000, 24000, 561))]
    v = rf.para(lib.param_kind("MFCC_E_D_N_Z"), 25)
    ref_feat = np.concatenate([rf.wav2mfcc(u, v) for u in utts])
    want = gm.outprob_host(ref_feat)
    samples, off = lib.Frontend._pack(utts)
    d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
    d_feat = lib.DevBuf(engine, ref_feat.nbytes)
    foff = fe.run_dev(d_in.ptr, off, d_feat.ptr)
    d_sc = lib.DevBuf(engine, 4 * len(ref_feat) * gm.S)
    gm.outprob_utts_dev(d_feat.ptr, foff, d_sc.ptr)
    got = d_sc.download((len(ref_feat), gm.S), np.float32)
    assert np.array_equal(got, want)
