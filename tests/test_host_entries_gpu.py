"""GPU: the _host form of every entry against its _dev form, and what the entries refuse.

A _host entry stages its input and output in buffers the object keeps between calls (csrc/jamd_host.h,
jamd_host_call()).  Every object is therefore called three times -- small, larger, smaller again -- so that the staging
grows once and is then reused with stale content behind the live part; every result must equal, bit for bit, the _dev
entry run on buffers the test owns.  Objects that keep state on the device (live front end, adin, adin_cut) are made
twice and fed the same pushes, one through _host and one through _dev.  The refusal table gives, per entry point, the
return code and the exact text a caller has always got."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu

SIZES = (1, 70, 3)                 # frames of the three calls: the staging grows at the second, is reused by the third
EINVAL = -1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same(a, b):
    """Bit-equal (a NaN equals only the same NaN)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def up(engine, a, room=0):
    """A device buffer of the test's own holding `a` (at least `room` bytes, never none)."""
    a = np.ascontiguousarray(a)
    buf = lib.DevBuf(engine, max(a.nbytes, room, 16))
    if a.nbytes:
        buf.upload(a)
    return buf


def down(engine, buf, shape, dtype):
    engine.sync()
    n = int(np.prod(shape))
    return buf.download(shape, dtype) if n else np.zeros(shape, dtype)


def last_error():
    return lib.load().jamd_last_error().decode()


def sub(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def pieces(a):
    """Three different pieces of `a`, of SIZES rows."""
    assert len(a) >= 100
    return [a[0:1], a[20:90], a[5:8]]


# ---------------------------------------------------------------------------------------------- the scorers
@pytest.fixture(scope="module")
def gmm(engine):
    model = synth.make_gmm(S=40, M=4, D=39, seed=1)
    return lib.Gmm(engine, model), synth.make_frames(model, T=100, seed=2)


def test_gmm_outprob_host(engine, gmm):
    gm, frames = gmm
    for fr in pieces(frames):
        T = len(fr)
        d_fr, d_out = up(engine, fr), lib.DevBuf(engine, 4 * T * gm.S)
        gm.outprob_dev(d_fr.ptr, T, d_out.ptr)
        assert same(gm.outprob_host(fr), down(engine, d_out, (T, gm.S), np.float32)), T
    out = np.full(8, 7.0, np.float32)                     # T = 0: nothing is touched
    assert lib.load().jamd_gmm_outprob_host(gm.h, frames.ctypes.data, 0, out.ctypes.data) == 0
    assert np.all(out == 7.0)


def test_gmm_dens_host(engine, gmm):
    gm, frames = gmm
    E = lib.load().jamd_gmm_nentry(gm.h)
    assert E == 160
    for fr in pieces(frames):
        T = len(fr)
        d_fr, d_out = up(engine, fr), lib.DevBuf(engine, 4 * T * E)
        assert lib.load().jamd_gmm_dens_dev(gm.h, d_fr.ptr, T, d_out.ptr, None) == 0
        assert same(gm.dens_host(fr), down(engine, d_out, (T, E), np.float32)), T
    out = np.full(8, 7.0, np.float32)
    assert lib.load().jamd_gmm_dens_host(gm.h, frames.ctypes.data, 0, out.ctypes.data) == 0
    assert np.all(out == 7.0)


def test_gms_apply_host(engine):
    z = np.load(GOLDEN / "gms.npz")
    gm = lib.Gmm(engine, sub(z, "full_"))
    stage = lib.Gms(engine, sub(z, "gs_"), z["state2gs"], 8)
    real = gm.outprob_host(z["frames"])
    changed = 0
    for a, b, off in ((0, 1, None), (20, 90, [0, 30, 70]), (5, 8, None)):
        fr, sc, T = z["frames"][a:b], real[a:b], b - a
        d_fr, d_sc = up(engine, fr), up(engine, sc)
        stage.apply_dev(d_fr.ptr, T, d_sc.ptr, utt_off=off)
        got = stage.apply_host(fr, sc, off)
        assert same(got, down(engine, d_sc, (T, stage.S), np.float32)), T
        changed += int((got != sc).sum())
    assert changed > 0                                    # (the stage did replace scores)
    sc = np.full(8, 7.0, np.float32)
    assert lib.load().jamd_gms_apply_host(stage.h, z["frames"].ctypes.data, 0, None, 0, sc.ctypes.data) == 0
    assert np.all(sc == 7.0)


def test_rejgmm_scores_host(engine):
    z = np.load(GOLDEN / "rejgmm.npz")
    keys = ("mean", "ivar", "gconst", "st_off", "ent_dens", "ent_logw")
    m = lib.RejGmm(engine, {k: z[k] for k in keys}, z["model_state"], 5)
    l = lib.load()
    for a, b, off in ((0, 1, [0, 1]), (20, 90, [0, 30, 30, 70]), (5, 8, [0, 3])):
        fr, T, off = z["frames"][a:b], b - a, np.array(off, np.int32)
        nutt = len(off) - 1
        d_fr, d_fs, d_us = up(engine, fr), lib.DevBuf(engine, 4 * T * m.nmodel), lib.DevBuf(engine, 4 * nutt * m.nmodel)
        assert l.jamd_rejgmm_frame_scores_dev(m.h, d_fr.ptr, T, d_fs.ptr, None) == 0
        assert l.jamd_rejgmm_utt_scores_dev(m.h, d_fs.ptr, T, off.ctypes.data, nutt, d_us.ptr, None) == 0
        fs, us = m.scores_host(fr, off)
        assert same(fs, down(engine, d_fs, (T, m.nmodel), np.float32)), T
        assert same(us, down(engine, d_us, (nutt, m.nmodel), np.float32)), T
        # either output alone: the other pointer NULL
        fs1, us1 = np.zeros_like(fs), np.zeros_like(us)
        assert l.jamd_rejgmm_scores_host(m.h, fr.ctypes.data, T, None, 0, fs1.ctypes.data, None) == 0
        assert l.jamd_rejgmm_scores_host(m.h, fr.ctypes.data, T, off.ctypes.data, nutt, None, us1.ctypes.data) == 0
        assert same(fs1, fs) and same(us1, us)
    # T = 0: the sums of empty utterances are 0, no frame score is written
    fs, us = np.full(8, 7.0, np.float32), np.full(m.nmodel, 7.0, np.float32)
    off = np.zeros(2, np.int32)
    assert l.jamd_rejgmm_scores_host(m.h, z["frames"].ctypes.data, 0, off.ctypes.data, 1, fs.ctypes.data, us.ctypes.data) == 0
    assert np.all(fs == 7.0) and np.all(us == 0.0)


def test_dnn_outprob_host(engine):
    dnn = synth.make_dnn(dims=(48, 72, 64, 40), seed=1)
    net = lib.Dnn(engine, dnn)
    frames = np.random.default_rng(3).normal(0, 1.5, (100, 48)).astype(np.float32)
    for fr in pieces(frames):
        T = len(fr)
        d_fr, d_out = up(engine, fr), lib.DevBuf(engine, 4 * T * net.S)
        net.outprob_dev(d_fr.ptr, T, d_out.ptr)
        assert same(net.outprob_host(fr), down(engine, d_out, (T, net.S), np.float32)), T
    out = np.full(8, 7.0, np.float32)
    assert lib.load().jamd_dnn_outprob_host(net.h, frames.ctypes.data, 0, out.ctypes.data) == 0
    assert np.all(out == 7.0)


@pytest.mark.parametrize("method", [lib.IWCD_MAX, lib.IWCD_AVG, lib.IWCD_NBEST])
def test_cdset_outprob_host(engine, method):
    rng = np.random.default_rng(4)
    S, nset = 50, 300
    n = rng.integers(0, 9, nset)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    cd = lib.CdSet(engine, off, rng.integers(0, S, int(off[-1])).astype(np.int32), method=method, nbest=3)
    scores = rng.normal(-60, 20, (100, S)).astype(np.float32)
    for sc in pieces(scores):
        T = len(sc)
        d_sc, d_cd = up(engine, sc), lib.DevBuf(engine, 4 * T * nset)
        cd.outprob_dev(d_sc.ptr, T, S, d_cd.ptr)
        assert same(cd.outprob_host(sc), down(engine, d_cd, (T, nset), np.float32)), T
    d_cd = up(engine, np.full(8, 7.0, np.float32))
    cd.outprob_dev(d_sc.ptr, 0, S, d_cd.ptr)
    assert np.all(down(engine, d_cd, (8,), np.float32) == 7.0)


# ---------------------------------------------------------------------------------------------- the front ends
FS, SH = 400, 160


def wave(frames, seed, extra=0):
    """Audio of `frames` whole buffered windows (and `extra` samples more), without runs of zeros."""
    return synth.make_audio(FS + (frames - 1) * SH + extra, seed=seed, zero_runs=0, silent_frac=0, clip=False)


def test_frontend_run_host(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    for utts in ([wave(1, 1)], [wave(70, 2, 37), wave(9, 3)], [wave(3, 4)]):
        got, foff = fe.run_host(utts)
        samples, off = lib.Frontend._pack(utts)
        d_s, d_out = up(engine, samples), lib.DevBuf(engine, max(got.nbytes, 16))
        foff_d = fe.run_dev(d_s.ptr, off, d_out.ptr)
        assert list(foff) == list(foff_d) and foff[-1] == len(got) > 0
        assert same(got, down(engine, d_out, got.shape, np.float32)), len(got)


def test_frontend_noise_host(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_N_Z", 25)
    for utts, head in (([wave(1, 5)], 0), ([wave(70, 6), wave(40, 7)], 4000), ([wave(3, 8)], 0)):
        got = fe.noise_host(utts, head)
        samples, off = lib.Frontend._pack(utts)
        d_s, d_nz = up(engine, samples), lib.DevBuf(engine, got.nbytes)
        fe.noise_dev(d_s.ptr, off, d_nz.ptr, head)
        assert got.shape == (len(utts), fe.fftn) and np.any(got != 0)
        assert same(got, down(engine, d_nz, got.shape, np.float32)), len(utts)


def live_wave(frames, seed):
    return synth.make_audio(FS + 1 + (frames - 1) * SH, seed=seed, zero_runs=0, silent_frac=0, clip=False)


def same_live_state(lv_h, lv_d):
    for c in range(lv_h.nchan):
        for x, y in zip(lv_h.state(c), lv_d.state(c)):
            assert same(np.asarray(x), np.asarray(y)), c


def test_live_run_host(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39, cvn=1)
    lv_h, lv_d = lib.LiveFrontend(fe, 2), lib.LiveFrontend(fe, 2)
    empty = np.zeros(0, np.int16)
    rows = 0
    for segs in ([live_wave(6, 1), empty], [live_wave(70, 2), live_wave(30, 3)], [empty, live_wave(9, 4)], [empty, empty]):
        got, foff = lv_h.run_host(segs)
        samples, off = lib.Frontend._pack(segs)
        d_s, d_out = up(engine, samples), lib.DevBuf(engine, max(got.nbytes, 16))
        foff_d = lv_d.run_dev(d_s.ptr, off, d_out.ptr)
        assert list(foff) == list(foff_d) and foff[-1] == len(got)
        assert same(got, down(engine, d_out, got.shape, np.float32)), len(got)
        same_live_state(lv_h, lv_d)
        rows += len(got)
    assert rows > 70 and len(got) == 0                    # (the last call: every channel idle)


def test_live_push_host(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    lv_h, lv_d = lib.LiveFrontend(fe, 2), lib.LiveFrontend(fe, 2)
    a, b = live_wave(90, 5), live_wave(60, 6)
    empty = np.zeros(0, np.int16)
    # a chunk shorter than a window (no row yet), a long one, every channel idle, a short one that ends the segments
    pushes = [([a[:100], empty], None), ([a[100:12000], b[:7000]], None), ([empty, empty], None),
              ([a[12000:12500], b[7000:7300]], [True, True])]
    rows = []
    for chunks, final in pushes:
        got, foff = lv_h.push_host(chunks, final)
        samples, off = lib.Frontend._pack(chunks)
        d_s, d_out = up(engine, samples), lib.DevBuf(engine, max(got.nbytes, 16))
        foff_d = lv_d.push_dev(d_s.ptr if len(samples) else 0, off, d_out.ptr if len(got) else 0, final)
        assert list(foff) == list(foff_d) and foff[-1] == len(got)
        assert same(got, down(engine, d_out, got.shape, np.float32)), len(got)
        same_live_state(lv_h, lv_d)
        rows.append(len(got))
    assert rows[0] == 0 and rows[2] == 0 and rows[1] > 70 and 0 < rows[3] < rows[1], rows


# ---------------------------------------------------------------------------------------------- adin, adin_cut
def test_adin_push_host(engine):
    a_h, a_d = (lib.Adin(engine, 2, strip_zero=True, zmean=True, level_coef=0.5) for _ in range(2))
    w = [synth.make_audio(9000, seed=11 + c, dc=300.0, zero_runs=0) for c in range(2)]
    empty = np.zeros(0, np.int16)
    # small; larger, one channel all zeros (stripped: the output is shorter than the staging); smaller; every channel idle
    pushes = [[w[0][:50], w[1][:20]], [w[0][50:5050], np.zeros(5000, np.int16)], [w[0][5050:5350], w[1][20:90]],
              [empty, empty]]
    lens = []
    for chunks in pushes:
        got, ooff = a_h.push_host(chunks)
        samples, ioff = lib.Frontend._pack(chunks)
        d_in, d_out = up(engine, samples), lib.DevBuf(engine, max(2 * len(samples), 16))
        ooff_d = a_d.push_dev(d_in.ptr if len(samples) else 0, ioff, d_out.ptr if len(samples) else 0)
        assert list(ooff) == list(ooff_d) and ooff[-1] == len(got)
        assert same(got, down(engine, d_out, got.shape, np.int16)), len(got)
        for c in range(2):
            for x, y in zip(a_h.state(c), a_d.state(c)):
                assert same(np.asarray(x), np.asarray(y)), c
        lens.append((int(ioff[-1]), len(got)))
    assert lens[1][1] < lens[1][0] - 4900 and lens[2][1] > 0 and lens[3] == (0, 0), lens


def cut_push_host(k, samples, in_off, eos, max_parts):
    """jamd_adin_cut_push_host() with offsets as given (lib.AdinCut.push_host always packs from 0)."""
    lens = np.diff(in_off)
    out = np.zeros(max(1, sum(k.push_cap(int(n)) for n in lens)), np.int16)
    poff, pfin, pst = k._tables(max_parts)
    n = C.c_int(0)
    m = k._eos(eos)
    rc = lib.load().jamd_adin_cut_push_host(k.h, samples.ctypes.data, in_off.ctypes.data, m.ctypes.data if m is not None else None,
                                            out.ctypes.data, max_parts, C.addressof(n), poff.ctypes.data, pfin.ctypes.data,
                                            pst.ctypes.data)
    assert rc == 0, last_error()
    total = int(poff[n.value - 1, -1]) if n.value else 0
    return out[:total].copy(), poff[:n.value].copy(), pfin[:n.value].copy(), pst[:n.value].copy()


def test_adin_cut_push_host(engine):
    small = dict(head_margin_msec=30, tail_margin_msec=40, chunk_size=100, level_thres=1000)
    k_h, k_d = lib.AdinCut(engine, 2, **small), lib.AdinCut(engine, 2, **small)
    w = [synth.make_audio(12000, seed=21 + c, zero_runs=0) for c in range(2)]
    empty = np.zeros(0, np.int16)
    pushes = [([w[0][:150], w[1][:60]], None), ([w[0][150:9150], w[1][60:7060]], None), ([empty, empty], None),
              ([w[0][9150:9500], w[1][7060:7200]], [True, True])]
    delivered = []
    for i, (chunks, eos) in enumerate(pushes):
        samples, off = lib.Frontend._pack(chunks)
        max_parts = max(1, max(k_h.parts_cap(len(c)) for c in chunks))
        # the host entry takes the samples 37 * i behind the start of the caller's buffer
        lead = 37 * i
        shifted = np.concatenate([np.full(lead, 12345, np.int16), samples, np.zeros(1, np.int16)])
        got = cut_push_host(k_h, shifted, off + lead, eos, max_parts)
        room = sum(k_d.push_cap(len(c)) for c in chunks)
        d_in, d_out = up(engine, samples), lib.DevBuf(engine, max(2 * room, 16))
        poff, pfin, pst = k_d.push_dev(d_in.ptr if len(samples) else 0, off, d_out.ptr, eos, max_parts=max_parts)
        assert same(got[1], poff) and same(got[2], pfin) and same(got[3], pst), i
        assert same(got[0], down(engine, d_out, got[0].shape, np.int16)), i
        for c in range(2):
            assert k_h.state(c) == k_d.state(c), (i, c)
        delivered.append(len(got[0]))
    assert delivered[2] == 0 and delivered[1] > 1000 and 0 < delivered[3] < delivered[1], delivered


# ---------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def objs(engine, gmm):
    """One object of every kind, and arrays to hand in."""
    z = np.load(GOLDEN / "rejgmm.npz")
    g = np.load(GOLDEN / "gms.npz")
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    o = dict(gmm=gmm[0], dnn=lib.Dnn(engine, synth.make_dnn(dims=(16, 8, 5), seed=1)),
             gms=lib.Gms(engine, sub(g, "gs_"), g["state2gs"], 8),
             rej=lib.RejGmm(engine, {k: z[k] for k in ("mean", "ivar", "gconst", "st_off", "ent_dens", "ent_logw")},
                            z["model_state"], 5),
             cd=lib.CdSet(engine, [0, 2], [0, 1]), fe=fe, lv=lib.LiveFrontend(fe, 1), adin=lib.Adin(engine, 1),
             cut=lib.AdinCut(engine, 1))
    o["f"] = np.zeros(4096, np.float32)
    o["s"] = np.zeros(4096, np.int16)
    o["i"] = np.zeros(64, np.int32)
    o["i64"] = np.zeros(64, np.int64)
    o["u8"] = np.zeros(64, np.uint8)
    o["down"] = np.array([5, 3], np.int64)                # a descending offset table
    o["n"] = C.c_int(0)
    return o


def p(a):
    return a.ctypes.data


# (arrays a refusal row hands in live here, so that they outlive the call)
OFF9, OFF900 = np.array([0, 9], np.int64), np.array([0, 900], np.int64)
SET_OFF, I01, I06, I0, I099 = (np.array(v, np.int32) for v in ([0, 2], [0, 1], [0, 6], [0], [0, 99]))


ENTRY_REFUSALS = [
    ("gmm_outprob_host NULL handle", lambda l, o: l.jamd_gmm_outprob_host(None, p(o["f"]), 1, p(o["f"])),
     "jamd_gmm_outprob_host: bad argument"),
    ("gmm_dens_host negative count", lambda l, o: l.jamd_gmm_dens_host(o["gmm"].h, p(o["f"]), -1, p(o["f"])),
     "jamd_gmm_dens_host: bad argument"),
    ("gms_apply_host NULL scores", lambda l, o: l.jamd_gms_apply_host(o["gms"].h, p(o["f"]), 1, None, 0, None),
     "jamd_gms_apply_host: bad argument"),
    ("rejgmm_scores_host negative count",
     lambda l, o: l.jamd_rejgmm_scores_host(o["rej"].h, p(o["f"]), -1, None, 0, p(o["f"]), None),
     "jamd_rejgmm_scores_host: bad argument"),
    ("rejgmm_scores_host sums without utterances",
     lambda l, o: l.jamd_rejgmm_scores_host(o["rej"].h, p(o["f"]), 1, None, 0, None, p(o["f"])),
     "jamd_rejgmm_scores_host: bad argument"),
    ("dnn_outprob_host NULL frames", lambda l, o: l.jamd_dnn_outprob_host(o["dnn"].h, None, 1, p(o["f"])),
     "jamd_dnn_outprob_host: bad argument"),
    ("dnn_outprob_dev negative count", lambda l, o: l.jamd_dnn_outprob_dev(o["dnn"].h, p(o["f"]), -1, p(o["f"]), None),
     "jamd_dnn_outprob_dev: bad argument"),
    ("cdset_outprob_dev NULL scores", lambda l, o: l.jamd_cdset_outprob_dev(o["cd"].h, None, 1, 2, p(o["f"]), None),
     "jamd_cdset_outprob_dev: bad argument"),
    ("frontend_run_host nutt 0", lambda l, o: l.jamd_frontend_run_host(o["fe"].h, p(o["s"]), p(o["i64"]), 0, p(o["f"]), None),
     "jamd_frontend_run_host: NULL argument or nutt < 1"),
    ("frontend_run_host descending", lambda l, o: l.jamd_frontend_run_host(o["fe"].h, p(o["s"]), p(o["down"]), 1, p(o["f"]), None),
     "jamd_frontend_run_host: sample_off is not non-decreasing from 0 at utterance 0"),
    ("frontend_noise_host NULL handle",
     lambda l, o: l.jamd_frontend_noise_host(None, p(o["s"]), p(o["i64"]), 1, 0, p(o["f"])),
     "jamd_frontend_noise_host: NULL argument or nutt < 1"),
    ("live_run_host NULL samples", lambda l, o: l.jamd_frontend_live_run_host(o["lv"].h, None, p(o["i64"]), p(o["f"]), None),
     "jamd_frontend_live_run_host: NULL argument"),
    ("live_push_host descending",
     lambda l, o: l.jamd_frontend_live_push_host(o["lv"].h, p(o["s"]), p(o["down"]), None, p(o["f"]), None),
     "jamd_frontend_live_push_host: sample_off is not non-decreasing from 0 at channel 0"),
    ("live_push_host NULL buffer",
     lambda l, o: l.jamd_frontend_live_push_host(o["lv"].h, None, p(OFF900), None, p(o["f"]), None),
     "jamd_frontend_live_push_host: NULL buffer"),
    ("adin_push_host descending", lambda l, o: l.jamd_adin_push_host(o["adin"].h, p(o["s"]), p(o["down"]), p(o["s"]), p(o["i64"])),
     "jamd_adin_push_host: channel 0: offsets [5, 3) are negative, descending or more than 1073741823 samples"),
    ("adin_push_host NULL buffer",
     lambda l, o: l.jamd_adin_push_host(o["adin"].h, None, p(OFF9), p(o["s"]), p(o["i64"])),
     "jamd_adin_push_host: NULL buffer"),
    ("adin_push_dev descending",
     lambda l, o: l.jamd_adin_push_dev(o["adin"].h, None, p(o["down"]), None, p(o["i64"]), None),
     "jamd_adin_push_dev: channel 0: offsets [5, 3) are negative, descending or more than 1073741823 samples"),
    ("adin_cut_push_host descending",
     lambda l, o: l.jamd_adin_cut_push_host(o["cut"].h, p(o["s"]), p(o["down"]), None, p(o["s"]), 4, C.addressof(o["n"]),
                                            p(o["i64"]), p(o["u8"]), p(o["i64"])),
     "jamd_adin_cut_push_host: channel 0: offsets [5, 3) are negative, descending or more than 1073741823 samples"),
    ("adin_cut_push_host max_parts 0",
     lambda l, o: l.jamd_adin_cut_push_host(o["cut"].h, p(o["s"]), p(OFF9), None, p(o["s"]), 0,
                                            C.addressof(o["n"]), p(o["i64"]), p(o["u8"]), p(o["i64"])),
     "jamd_adin_cut_push_dev: max_parts not in 1 ... 65535"),
    ("adin_cut_push_host max_parts 65536",
     lambda l, o: l.jamd_adin_cut_push_host(o["cut"].h, p(o["s"]), p(OFF9), None, p(o["s"]), 65536,
                                            C.addressof(o["n"]), p(o["i64"]), p(o["u8"]), p(o["i64"])),
     "jamd_adin_cut_push_dev: max_parts not in 1 ... 65535"),
    ("adin_cut_push_host NULL input",
     lambda l, o: l.jamd_adin_cut_push_host(o["cut"].h, None, p(OFF9), None, p(o["s"]), 4,
                                            C.addressof(o["n"]), p(o["i64"]), p(o["u8"]), p(o["i64"])),
     "jamd_adin_cut_push_host: NULL input"),
]


@pytest.mark.parametrize("what,call,text", ENTRY_REFUSALS, ids=[r[0] for r in ENTRY_REFUSALS])
def test_entry_refusals(objs, what, call, text):
    assert call(lib.load(), objs) == EINVAL
    assert last_error() == text


def gmm_desc(model, **over):
    keep = {k: np.ascontiguousarray(model[k], np.int32 if k in ("st_off", "ent_dens") else np.float32)
            for k in ("mean", "ivar", "gconst", "st_off", "ent_dens", "ent_logw")}
    d = lib.GmmDesc()
    d.nstate, d.veclen, d.ndens, d.nentry = len(keep["st_off"]) - 1, keep["mean"].shape[1], len(keep["mean"]), len(keep["ent_dens"])
    d.nbook, d.nstream, d.st_book = 0, 1, None
    for k, v in keep.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    d._keep = keep
    return d


def dnn_desc(dims):
    dnn = synth.make_dnn(dims=dims, seed=1)
    nl = len(dims) - 1
    keep = [np.array(dims, np.int32), [np.ascontiguousarray(w, np.float32) for w in dnn["w"]],
            [np.ascontiguousarray(b, np.float32) for b in dnn["b"]], np.ascontiguousarray(dnn["prior"], np.float32)]
    wp = (C.c_void_p * nl)(*[w.ctypes.data for w in keep[1]])
    bp = (C.c_void_p * nl)(*[b.ctypes.data for b in keep[2]])
    d = lib.DnnDesc()
    d.nlayer, d.dims, d.state_prior = nl, keep[0].ctypes.data, keep[3].ctypes.data
    d.w, d.b = C.cast(wp, C.c_void_p), C.cast(bp, C.c_void_p)
    d._keep = (keep, wp, bp)
    return d


def _model():
    return synth.make_gmm(S=6, M=3, D=13, seed=5)


def _bad_dens():
    m = _model()
    m["ent_dens"] = m["ent_dens"].copy()
    m["ent_dens"][7] = 99                                 # (refused once the object exists)
    return m


CREATE_REFUSALS = [
    ("dnn layer width", lambda l, e, h: l.jamd_dnn_create(e.h, C.byref(dnn_desc((12, 8, 5))), C.byref(h)),
     "jamd_dnn_create: layer 0 input length 12 is not a multiple of 8 (same restriction as the reference's SIMD path)"),
    ("dnn hidden width", lambda l, e, h: l.jamd_dnn_create(e.h, C.byref(dnn_desc((16, 12, 5))), C.byref(h)),
     "jamd_dnn_create: layer 1 input length 12 is not a multiple of 8 (same restriction as the reference's SIMD path)"),
    ("cdset nbest 0", lambda l, e, h: l.jamd_cdset_create(e.h, 1, p(SET_OFF), p(I01), lib.IWCD_NBEST, 0, C.byref(h)),
     "jamd_cdset_create: nbest=0 outside [1,16]"),
    ("cdset nbest 17", lambda l, e, h: l.jamd_cdset_create(e.h, 1, p(SET_OFF), p(I01), lib.IWCD_NBEST, 17, C.byref(h)),
     "jamd_cdset_create: nbest=17 outside [1,16]"),
    ("cdset method", lambda l, e, h: l.jamd_cdset_create(e.h, 1, p(SET_OFF), p(I01), 77, 3, C.byref(h)),
     "jamd_cdset_create: unknown method 77"),
    ("gmm nstream", lambda l, e, h: l.jamd_gmm_create(e.h, C.byref(gmm_desc(_model(), nstream=2)), lib.GPRUNE_NONE, 0, C.byref(h)),
     "jamd_gmm_create: nstream=2; only single-stream models are supported"),
    ("gmm density index", lambda l, e, h: l.jamd_gmm_create(e.h, C.byref(gmm_desc(_bad_dens())), lib.GPRUNE_NONE, 0, C.byref(h)),
     "jamd_gmm_create: density index 99 out of range"),
    ("gmm gprune_num", lambda l, e, h: l.jamd_gmm_create(e.h, C.byref(gmm_desc(_model())), lib.GPRUNE_SAFE, 0, C.byref(h)),
     "jamd_gmm_create: gprune safe needs gprune_num >= 1"),
    ("gms nbest 0", lambda l, e, h: l.jamd_gms_create(e.h, C.byref(gmm_desc(_model())), p(I01), 2, 0, C.byref(h)),
     "jamd_gms_create: bad argument"),
    ("gms state2gs", lambda l, e, h: l.jamd_gms_create(e.h, C.byref(gmm_desc(_model())), p(I06), 2, 1, C.byref(h)),
     "jamd_gms_create: state2gs[1] out of range"),
    ("rejgmm gprune_num 0", lambda l, e, h: l.jamd_rejgmm_create(e.h, C.byref(gmm_desc(_model())), p(I0), 1, 0, C.byref(h)),
     "jamd_rejgmm_create: bad argument"),
    ("rejgmm model_state", lambda l, e, h: l.jamd_rejgmm_create(e.h, C.byref(gmm_desc(_model())), p(I099), 2, 5, C.byref(h)),
     "jamd_rejgmm_create: model_state[1] out of range"),
    ("adin nchan 0", lambda l, e, h: l.jamd_adin_create(e.h, C.byref(lib.Adin.desc_for()), 0, C.byref(h)),
     "jamd_adin_create: NULL argument or nchan < 1"),
    ("adin_cut nchan 0", lambda l, e, h: l.jamd_adin_cut_create(e.h, C.byref(lib.AdinCut.desc_for()), 0, C.byref(h)),
     "jamd_adin_cut_create: NULL argument or nchan not in 1 ... 65535"),
    ("adin_cut nchan 65536", lambda l, e, h: l.jamd_adin_cut_create(e.h, C.byref(lib.AdinCut.desc_for()), 65536, C.byref(h)),
     "jamd_adin_cut_create: NULL argument or nchan not in 1 ... 65535"),
    ("frontend realtime",
     lambda l, e, h: l.jamd_frontend_create(e.h, C.byref(lib.Frontend.desc_for("MFCC_E_D_A_Z", 39, realtime=1)), C.byref(h)),
     "jamd_frontend_create: realtime input / MAP-CMN is not served (buffered front end only)"),
    ("frontend _A without _D",
     lambda l, e, h: l.jamd_frontend_create(e.h, C.byref(lib.Frontend.desc_for("MFCC_E_D_A_Z", 39, delta=0)), C.byref(h)),
     "jamd_frontend_create: _N needs _E and _D, _A needs _D"),
]

VALID_CREATES = {
    "dnn": lambda e: lib.Dnn(e, synth.make_dnn(dims=(16, 8, 5), seed=1)),
    "cdset": lambda e: lib.CdSet(e, [0, 2], [0, 1], method=lib.IWCD_NBEST, nbest=3),
    "gmm": lambda e: lib.Gmm(e, _model()),
    "gms": lambda e: lib.Gms(e, _model(), [0, 1], 1),
    "rejgmm": lambda e: lib.RejGmm(e, _model(), [0], 5),
    "adin": lambda e: lib.Adin(e, 1),
    "adin_cut": lambda e: lib.AdinCut(e, 1),
    "frontend": lambda e: lib.Frontend.from_kind(e, "MFCC_E_D_A_Z", 39),
}


@pytest.mark.parametrize("what,call,text", CREATE_REFUSALS, ids=[r[0] for r in CREATE_REFUSALS])
def test_create_refusals(engine, what, call, text):
    h = C.c_void_p()
    assert call(lib.load(), engine, h) == EINVAL
    assert last_error() == text
    assert not h.value                                    # no handle
    obj = VALID_CREATES[what.split()[0]](engine)          # and the engine still serves a valid create
    assert obj.h
    obj.close()


def test_live_create_refusals(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    h = C.c_void_p()
    d = lib.FrontendLiveDesc(1, 100.0, None, None)
    assert lib.load().jamd_frontend_live_create(fe.h, C.byref(d), 0, C.byref(h)) == EINVAL
    assert last_error() == "jamd_frontend_live_create: NULL argument or nchan < 1"
    assert not h.value
    fe2 = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39, cvn=1)
    cm = np.zeros(39, np.float32)
    d = lib.FrontendLiveDesc(1, 100.0, cm.ctypes.data, None)
    assert lib.load().jamd_frontend_live_create(fe2.h, C.byref(d), 1, C.byref(h)) == EINVAL
    assert last_error() == "jamd_frontend_live_create: the kind has cvn: an initial mean needs an initial variance"
    assert not h.value
    lv = lib.LiveFrontend(fe2, 1)
    assert lv.h
    lv.close()


def test_engine_create_refusals(engine):
    l = lib.load()
    assert l.jamd_engine_create(0, None) == EINVAL
    assert last_error() == "jamd_engine_create: out is NULL"
    n = l.jamd_device_count()
    h = C.c_void_p()
    assert l.jamd_engine_create(n, C.byref(h)) == EINVAL
    assert last_error() == f"jamd_engine_create: device {n} out of range [0,{n})"
    assert not h.value
    e2 = lib.Engine(0)
    assert e2.h
    e2.close()
