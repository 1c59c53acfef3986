"""The live-input front end on the device (lib.LiveFrontend) against the compiled reference driven by
tests/frontendliveref.py: every vector and every carried value bit for bit (frontendref.same: bits for numbers, NaN for
NaN; no tolerance anywhere).  Segments are a few hundred frames at most."""
import ctypes as C

import numpy as np
import pytest

import frontendliveref as L
from beamutil import ref_task
from frontendref import RefFrontend, first_diff, same
from frontendssref import RefFrontendSS, floor_share, frame_spectra
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu

FS, SH = 400, 160


def nsamp(frames):
    """Samples of a segment of `frames` base frames (live window: framesize + 1)."""
    return FS + 1 + (frames - 1) * SH if frames > 0 else 0


_AUDIO = {}


def audio(frames, seed, gain=1.0):
    """Seeded audio without runs of zero samples, cut to `frames` base frames."""
    if seed not in _AUDIO:
        _AUDIO[seed] = synth.make_audio(nsamp(240), seed=seed, zero_runs=0, silent_frac=0, clip=False)
    a = _AUDIO[seed][:nsamp(frames)]
    return a if gain == 1.0 else np.clip(np.round(a * gain), -32768, 32767).astype(np.int16)


def pair(engine, ref, kind, vecsize, nchan=1, splice=1, live=None, ss=None, **fields):
    """(parent Frontend, LiveFrontend, maker of a reference channel) for one configuration."""
    live = dict(live or {})
    v = RefFrontend(ref).para(lib.param_kind(kind), vecsize, **fields)
    fe = lib.Frontend.from_kind(engine, kind, vecsize, splice=splice, **fields)
    if ss is not None:
        fe.set_ss("load", alpha=ss[1], floor=ss[2], noise=ss[0])
    lv = lib.LiveFrontend(fe, nchan, **live)
    return fe, lv, (lambda: L.RefLiveChannel(ref, v, splice=splice, ss=ss, **live))


def check_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert same(got, want), (what, first_diff(got, want))


def check_state(lv, chan, rc, v, what, emax=False):
    cm, cv, em, fl = lv.state(chan)
    wcm, wcv, wem, wset = rc.state()
    if wset:                                       # (the reference's vector is not initialised before)
        assert same(cm, wcm), (what, "cmean_init", first_diff(cm[None], wcm[None]))
    if v.cvn and wset:
        assert same(cv, wcv), (what, "cvar_init", first_diff(cv[None], wcv[None]))
    if emax:
        assert same(np.array([em]), np.array([wem])), (what, "energy maximum", em, wem)
    assert (fl & lib.LIVE_CMEAN_SET) == wset, (what, "cmean_init_set")


# ------------------------------------------------------------------------------------------------ delta edges
@pytest.mark.parametrize("delwin,accwin", [(2, 2), (1, 3), (4, 1)])
def test_delta_edges(engine, ref, delwin, accwin):
    """First segments of every length around the buffers' delays (and one long one): the frame count, which includes
    the segments that emit nothing, and every vector.  The last delWin + accWin frames of a segment come out of the
    reference's flush loop, whose third block is not the main loop's (tests/frontendliveref.py)."""
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, delWin=delwin, accWin=accwin)
    empty = 0
    for Tb in list(range(1, 2 * (delwin + accwin) + 4)) + [40]:
        rc = mk()
        want = rc.segment(audio(Tb, 11))
        lv1 = lib.LiveFrontend(fe, 1)             # a first segment: fresh state
        got, foff = lv1.run_host([audio(Tb, 11)])
        assert list(foff) == [0, len(want)], (Tb, foff, len(want))
        assert lv1.frames(nsamp(Tb)) == len(want)
        check_rows(got, want, f"Tb {Tb}")
        empty += len(want) == 0
        lv1.close(); rc.close()
    assert empty == max(delwin, accwin) - 1       # Tb = 1 .. max(delWin, accWin) - 1 emit nothing


# ------------------------------------------------------------------------------------------------ state over segments
SEGS = (37, 230, 180, 60, 40, 41, 50, 45, 38)


def _history_plan(lens, skip=()):
    """What CMN_realtime_update() meets over `lens` (restated from its loop, to hold the inputs to the issue's terms):
    per commit (entries in the list, entries summed, whether CPMAX was reached, clist_max after)."""
    lst, cmax, out = [], 5, []
    for i, now in enumerate(lens):
        if i in skip:
            continue
        frames, used = now, 0
        for fn in lst:
            frames += fn
            used += 1
            if frames >= 500:
                break
        n = len(lst)
        if n == cmax and frames < 500:
            cmax += 5
        lst = ([now] + lst)[:cmax]
        out.append((n, used, frames >= 500, cmax))
    return out


_rng = np.random.default_rng(77)
CM0 = _rng.normal(0, 4, 39).astype(np.float32)
CV0 = _rng.uniform(0.5, 40, 39).astype(np.float32)
STATE_CASES = {
    "map_default": (dict(), dict(), ()),
    "map_weight_10": (dict(map_weight=10.0), dict(enormal=1), ()),       # (enormal: the energy maximum is carried too)
    "cmnstatic_loaded_mean": (dict(map_cmn=False, cmean=CM0), dict(), ()),
    "loaded_mean_and_variance_cvn": (dict(cmean=CM0, cvar=CV0), dict(cvn=1), ()),
    "cvn_nothing_loaded": (dict(), dict(cvn=1, enormal=1), ()),
    "cmnnoupdate": (dict(), dict(), tuple(range(9))),
    "commit_skipped_after_3_and_4": (dict(), dict(enormal=1), (2, 3)),
}


@pytest.mark.parametrize("case", list(STATE_CASES))
def test_state_over_segments(engine, ref, case):
    live, fields, skip = STATE_CASES[case]
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, live=live, **fields)
    rc = mk()
    if not skip:                                   # the segment lengths meet the issue's terms
        plan = _history_plan(SEGS)
        assert all(37 <= x <= 230 for x in SEGS) and len(SEGS) == 9
        assert sum(SEGS[:5]) >= 500                                   # CPMAX passed before the sixth segment
        assert plan[-1][3] > 5                                        # more than CPSTEP segments enter the history
        assert any(cut and used < n for n, used, cut, _ in plan)      # the cut inside the list
        assert any(cut and used == n and n > 0 for n, used, cut, _ in plan)   # and at its end
    if not live:
        assert not rc.state()[3]                   # the first segment has no initial mean
    for i, Tb in enumerate(SEGS):
        wav = audio(Tb, 20 + i)
        want = rc.segment(wav)
        got, foff = lv.run_host([wav])
        assert len(want) == Tb
        check_rows(got, want, f"{case} segment {i + 1}")
        if i not in skip:
            rc.commit()
            lv.commit()
        check_state(lv, 0, rc, rc.v, f"{case} after segment {i + 1}", emax=bool(fields.get("enormal")))
    if not skip:
        assert rc.history()[1] > 5                 # the reference lengthened its list
    rc.close()


# ------------------------------------------------------------------------------------------------ kinds
KIND_CASES = {
    "MFCC_E_D_N_Z_25": ("MFCC_E_D_N_Z", 25, 1, {}),
    "MFCC_E_0_D_Z": ("MFCC_E_0_D_Z", 28, 1, {}),
    "MFCC_0_D_A": ("MFCC_0_D_A", 39, 1, {}),
    "FBANK_D_A_Z_40": ("FBANK_D_A_Z", 120, 1, dict(fbank_num=40)),
    "MFCC_plain": ("MFCC", 12, 1, {}),
    "enormal_escale01": ("MFCC_E_D_A_Z", 39, 1, dict(enormal=1, escale=0.1, silFloor=50.0)),
    "enormal_defaults": ("MFCC_E_D_A_Z", 39, 1, dict(enormal=1)),
    "splice3": ("MFCC_E_D_A_Z", 39, 3, {}),
    "splice3_cvn": ("MFCC_E_D_A_Z", 39, 3, dict(cvn=1)),
}


@pytest.mark.parametrize("case", list(KIND_CASES))
def test_kinds(engine, ref, case):
    """Three segments (loud, quiet, very loud: the energy passes the previous maximum and falls below the floor),
    committed after each; the fourth is too short to emit and still moves the energy maximum."""
    kind, vecsize, splice, fields = KIND_CASES[case]
    fe, lv, mk = pair(engine, ref, kind, vecsize, splice=splice, **fields)
    rc = mk()
    en = bool(fields.get("enormal"))
    ecol = rc.v.baselen - 1
    for i, (Tb, gain) in enumerate(((50, 1.0), (33, 0.004), (70, 3.0), (1, 1.0))):
        wav = audio(Tb, 40 + i, gain)
        want = rc.segment(wav)
        got, foff = lv.run_host([wav])
        check_rows(got, want, f"{case} segment {i + 1}")
        if en and i == 1:                          # quiet after loud: frames on the floor (min_last)
            assert (want[:, ecol] == want[:, ecol].min()).sum() > 3
        if en and i == 2:                          # very loud after quiet: frames above the previous maximum
            assert (want[:, ecol] > 1.0).any()
        rc.commit()
        lv.commit()
        check_state(lv, 0, rc, rc.v, f"{case} after segment {i + 1}", emax=en)
    assert lv.frames(nsamp(1)) == len(want) == (1 if kind == "MFCC" else 0)
    rc.close()


def test_refusals(engine):
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_N_A", 38)
    with pytest.raises(lib.JamdError, match=r"realtime-1stpass\.c:1233-1241"):
        lib.LiveFrontend(fe, 1)
    fe = lib.Frontend.from_kind(engine, "MFCC_E_D_A_Z", 39)
    lv = lib.LiveFrontend(fe, 1)
    fe.set_ss("calc", calc_len_ms=100)
    with pytest.raises(lib.JamdError, match="JAMD_SS_CALC"):
        lv.run_host([audio(20, 3)])
    fe.set_ss("off")
    assert len(lv.run_host([audio(20, 3)])[0]) == 20
    d = lib.Frontend.desc_for("MFCC_E_D_A_Z", 39, realtime=1)      # the buffered descriptor keeps refusing it
    h = C.c_void_p()
    assert lib.load().jamd_frontend_create(engine.h, C.byref(d), C.byref(h)) == -1


# ------------------------------------------------------------------------------------------------ channels
@pytest.mark.parametrize("nchan", [1, 3, 65, 130])
def test_channels(engine, ref, nchan):
    """Three calls queued on one stream without a host synchronisation, ragged lengths, idle channels, one channel too
    short for a frame, a different commit mask per call; a second object on the same parent runs alternately on the
    same stream over the channels in reverse.  Every channel equals the reference run alone on its own segments."""
    kind, vecsize, fields = "MFCC_E_D_A_Z", 39, dict(enormal=1, cvn=1)
    fe, lv, mk = pair(engine, ref, kind, vecsize, nchan=nchan, **fields)
    lv2 = lib.LiveFrontend(fe, nchan)
    rng = np.random.default_rng(1000 + nchan)
    ncall = 3
    plan = []                                      # per call: (segments per channel, commit mask)
    for k in range(ncall):
        segs = []
        for c in range(nchan):
            r = rng.random()
            if nchan > 1 and r < 0.15:
                segs.append(np.zeros(0, np.int16))                       # idle in this call
            elif (c == nchan // 2 and k == 1) or r < 0.22:
                segs.append(audio(3, 60 + c % 5)[:rng.integers(1, FS + 1)])   # samples, but no frame
            elif r < 0.3:
                segs.append(audio(int(rng.integers(1, 4)), 60 + (c + k) % 5))   # base frames, but too few to emit
            else:
                segs.append(audio(int(rng.integers(4, 26)), 60 + (c + k) % 5, gain=float(rng.choice([0.01, 0.3, 2.0]))))
        plan.append((segs, rng.random(nchan) < 0.7))
    # the reference, every channel alone
    refs = [mk() for _ in range(nchan)]
    want = [[None] * nchan for _ in range(ncall)]
    wstate = [None] * nchan
    for c, rc in enumerate(refs):
        for k, (segs, mask) in enumerate(plan):
            want[k][c] = rc.segment(segs[c]) if len(segs[c]) else np.zeros((0, 39), np.float32)
            ran = any(len(plan[j][0][c]) for j in range(k + 1))
            # also over a channel idle in this call (its last segment again), but not before its first segment: the
            # reference's now.framenum is not initialised until CMN_realtime_prepare(); the device's is 0
            if mask[c] and ran:
                rc.commit()
        wstate[c] = rc.state()
    # the device: everything queued, then one wait
    d_in, d_out, d_out2, foffs, foffs2, offs = [], [], [], [], [], []
    for segs, mask in plan:
        samples, off = lib.Frontend._pack(segs)
        s2, off2 = lib.Frontend._pack(segs[::-1])
        d_in.append((lib.DevBuf(engine, max(samples.nbytes, 2)).upload(samples), lib.DevBuf(engine, max(s2.nbytes, 2)).upload(s2)))
        offs.append((off, off2))
        rows = sum(lv.frames(len(s)) for s in segs)
        d_out.append(lib.DevBuf(engine, max(rows, 1) * 39 * 4))
        d_out2.append(lib.DevBuf(engine, max(rows, 1) * 39 * 4))
    engine.sync()
    for k, (segs, mask) in enumerate(plan):
        foffs.append(lv.run_dev(d_in[k][0].ptr, offs[k][0], d_out[k].ptr))
        foffs2.append(lv2.run_dev(d_in[k][1].ptr, offs[k][1], d_out2[k].ptr))
        lv.commit(mask)
        lv2.commit(mask[::-1])
    engine.sync()
    lvh = lib.LiveFrontend(fe, nchan)             # the host entry over the same calls
    for k, (segs, mask) in enumerate(plan):
        foff, foff2 = foffs[k], foffs2[k]
        got = d_out[k].download((int(foff[-1]), 39), np.float32) if foff[-1] else np.zeros((0, 39), np.float32)
        got2 = d_out2[k].download((int(foff2[-1]), 39), np.float32) if foff2[-1] else np.zeros((0, 39), np.float32)
        for c in range(nchan):
            check_rows(got[foff[c]:foff[c + 1]], want[k][c], f"call {k} channel {c}")
            r = nchan - 1 - c
            check_rows(got2[foff2[r]:foff2[r + 1]], want[k][c], f"second object, call {k} channel {c}")
        hgot, hfoff = lvh.run_host(segs)
        lvh.commit(mask)
        assert np.array_equal(hfoff, foff) and same(hgot, got), f"run_host differs from run_dev in call {k}"
    for c, rc in enumerate(refs):
        check_state(lv, c, rc, rc.v, f"channel {c}", emax=True)
        check_state(lv2, nchan - 1 - c, rc, rc.v, f"second object, channel {c}", emax=True)
        rc.close()


# ------------------------------------------------------------------------------------------------ spectral subtraction
def test_spectral_subtraction_load(engine, ref):
    alpha, floor = 2.0, 0.5
    rs = RefFrontendSS(ref)
    v = rs.para(lib.param_kind("MFCC_E_D_A_Z"), 39)
    wavs = [audio(60, 70), audio(45, 71)]
    noise = rs.noise(audio(80, 72), v)
    share = floor_share(np.concatenate([frame_spectra(w) for w in wavs]), noise, alpha, 2, 256)
    print("floored share", share)
    assert 0.2 < share < 0.8, share
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, ss=(noise, alpha, floor))
    rc = mk()
    plain = L.RefLiveChannel(ref, v)
    for i, w in enumerate(wavs):
        want = rc.segment(w)
        assert not same(want, plain.segment(w))   # the subtraction changes the features
        got, _ = lv.run_host([w])
        check_rows(got, want, f"segment {i + 1}")
        rc.commit(); lv.commit(); plain.commit()
        check_state(lv, 0, rc, rc.v, f"after segment {i + 1}")
    rc.close(); plain.close()


# ------------------------------------------------------------------------------------------------ into the first pass
def test_into_the_first_pass(engine, oracle, ref, tmp_path):
    """8 channels x 2 segments: LiveFrontend.run_dev -> Gmm.outprob_utts_dev -> Beam.pass1_dev without a host copy of
    the features; sentences and scores equal the oracle's first pass over the helper's features."""
    eng, lex, am, task = ref_task(ref, tmp_path, 5, 300, nword=80, nphone=8, S=120, M=2)
    nchan, D = 8, 39
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", D, nchan=nchan)
    gm = lib.Gmm(engine, am)
    lx = lib.Lexicon(engine, lex)
    bm = lib.Beam(engine, lx, eng.beam_width, -1.0, max_utts=nchan)
    refs = [mk() for _ in range(nchan)]
    rng = np.random.default_rng(4)
    for k in range(2):
        segs = [audio(int(rng.integers(30, 90)), 80 + (c + 3 * k) % 6, gain=float(rng.choice([0.2, 1.0]))) for c in range(nchan)]
        samples, off = lib.Frontend._pack(segs)
        d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
        rows = sum(lv.frames(len(s)) for s in segs)
        d_feat = lib.DevBuf(engine, rows * D * 4)
        d_sc = lib.DevBuf(engine, rows * gm.S * 4)
        foff = lv.run_dev(d_in.ptr, off, d_feat.ptr)
        lv.commit()
        gm.outprob_utts_dev(d_feat.ptr, foff, d_sc.ptr)
        bm.pass1_dev(d_sc.ptr, gm.S, foff)
        res = bm.results()
        for c, rc in enumerate(refs):
            feat = rc.segment(segs[c])
            rc.commit()
            assert foff[c + 1] - foff[c] == len(feat)
            oatoms, owseq, oscore, orc, died = oracle.beam_pass1(lex, oracle.gmm_outprob(am, feat), eng.beam_width, -1.0)
            assert res[c].status == orc, (k, c)
            if orc == 0:
                assert list(res[c].wseq[:res[c].wnum]) == list(owseq) and res[c].score == oscore, (k, c)
    for rc in refs:
        rc.close()
