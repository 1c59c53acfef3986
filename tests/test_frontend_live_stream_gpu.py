"""Chunked live input on the device (lib.LiveFrontend.push_*): however a segment is cut, the pushes deliver, concatenated,
the rows of the compiled reference driven by tests/frontendliveref.py (and of one run_host over the whole segment) and
leave the same channel state; bit for bit (frontendref.same), no tolerance anywhere.  Geometry, audio and the helpers
are those of tests/test_frontend_live_gpu.py."""
import numpy as np
import pytest

import frontendliveref as L
from beamutil import ref_task
from frontendref import RefFrontend, same
from frontendssref import RefFrontendSS
from julius_amd import lexblob, lib
from test_frontend_live_gpu import CM0, CV0, FS, SEGS, SH, audio, check_rows, check_state, nsamp, pair

pytestmark = pytest.mark.gpu

ESTATE = r"\(-5\)"
EINVAL = r"\(-1\)"


def tb_of(n):
    return 0 if n < FS + 1 else (n - FS - 1) // SH + 1


def feed(lv, wav, chunks, final_last=True):
    """One channel: the chunk sizes in turn (the last push final) -> rows of every push.  Every push's row count is
    push_frames() of the samples before it."""
    assert sum(chunks) == len(wav)
    out, pos = [], 0
    for i, n in enumerate(chunks):
        fin = final_last and i == len(chunks) - 1
        rows, foff = lv.push_host([wav[pos:pos + n]], [fin])
        assert list(foff) == [0, len(rows)]
        assert len(rows) == lv.push_frames(pos, n, fin), (i, pos, n, fin, len(rows))
        out.append(rows)
        pos += n
    return out


def cat(parts, width):
    return np.concatenate(parts) if parts else np.zeros((0, width), np.float32)


def to_chunks(total, cuts):
    edges = [0] + sorted(cuts) + [total]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


# ------------------------------------------------------------------------------------------------ 1. cut points
L4 = 4                                             # delWin 2 + accWin 2
N40 = nsamp(40)


def _cycle(total, sizes):
    out, i = [], 0
    while sum(out) < total:
        out.append(min(sizes[i % len(sizes)], total - sum(out)))
        i += 1
    return out


CUT_PLANS = {
    "single_samples_for_600": [1] * 600 + [N40 - 600],
    "159_160_161": _cycle(N40, [159, 160, 161]),
    "first_400": [400, 3000, N40 - 3400],
    "first_401": [401, 3000, N40 - 3401],
    "first_402": [402, 3000, N40 - 3402],
    "frames_to_L-1_L_L+1": to_chunks(N40, [nsamp(L4 - 1), nsamp(L4), nsamp(L4 + 1)]),
    "history_wraps_7_8_9_frames": to_chunks(N40, [nsamp(2 * L4 - 1), nsamp(4 * L4 - 1), nsamp(6 * L4)]),
    "final_push_of_nothing": [3000, N40 - 3000, 0],
    "final_push_carries_the_last_frames": to_chunks(N40, [nsamp(20), nsamp(38)]),
    "whole_segment_in_one_final_push": [N40],
}
_WHOLE40 = {}


@pytest.mark.parametrize("plan", list(CUT_PLANS))
def test_cut_points(engine, ref, plan):
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39)
    wav = audio(40, 11)
    if not _WHOLE40:                               # the two yardsticks, once
        rc = mk()
        _WHOLE40["ref"] = rc.segment(wav)
        rc.close()
        lv1 = lib.LiveFrontend(fe, 1)
        _WHOLE40["run"] = lv1.run_host([wav])[0]
        lv1.close()
        check_rows(_WHOLE40["run"], _WHOLE40["ref"], "run_host")
    chunks = CUT_PLANS[plan]
    parts = feed(lv, wav, chunks)
    counts = [len(p) for p in parts]
    got = cat(parts, 39)
    check_rows(got, _WHOLE40["ref"], plan)
    check_rows(got, _WHOLE40["run"], plan + " against run_host")
    frames = [tb_of(x) for x in np.cumsum(chunks)]
    if plan == "frames_to_L-1_L_L+1":
        assert frames[:3] == [L4 - 1, L4, L4 + 1] and counts[:3] == [0, 0, 1]
    if plan == "history_wraps_7_8_9_frames":
        assert np.diff([0] + frames)[:3].tolist() == [2 * L4 - 1, 2 * L4, 2 * L4 + 1]
    if plan.startswith("first_40"):
        assert frames[0] == (0 if chunks[0] == 400 else 1) and counts[0] == 0
    if plan == "final_push_of_nothing":
        assert counts[-1] == L4
    if plan == "final_push_carries_the_last_frames":
        assert frames[-1] - frames[-2] == 2 and counts[-1] == 2 + L4
    lv.close()


# ------------------------------------------------------------------------------------------------ 2. short segments
@pytest.mark.parametrize("delwin,accwin", [(2, 2), (1, 3), (4, 1)])
def test_short_segments(engine, ref, delwin, accwin):
    """First segments of 1 .. 2 L + 3 base frames, one frame's worth per push: the rows, also of the segments that
    emit nothing, and the energy maximum the segment leaves."""
    fe, lv0, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, delWin=delwin, accWin=accwin, enormal=1)
    empty = 0
    for Tb in range(1, 2 * (delwin + accwin) + 4):
        wav = audio(Tb, 11)
        rc = mk()
        want = rc.segment(wav)
        lv = lib.LiveFrontend(fe, 1)
        got = cat(feed(lv, wav, to_chunks(len(wav), [nsamp(k) for k in range(1, Tb)])), 39)
        check_rows(got, want, f"Tb {Tb}")
        check_state(lv, 0, rc, rc.v, f"Tb {Tb}", emax=True)
        assert lv.state(0)[2] != np.float32(5.0)   # the maximum moved, also where nothing was emitted
        empty += len(want) == 0
        lv.close(); rc.close()
    assert empty == max(delwin, accwin) - 1


# ------------------------------------------------------------------------------------------------ 3. state over segments
STATE_CASES = {
    "map_default": (dict(), dict()),
    "map_weight_10": (dict(map_weight=10.0), dict(enormal=1)),
    "cmnstatic_loaded_mean": (dict(map_cmn=False, cmean=CM0), dict()),
    "loaded_mean_and_variance_cvn": (dict(cmean=CM0, cvar=CV0), dict(cvn=1)),
    "cvn_nothing_loaded": (dict(), dict(cvn=1, enormal=1)),      # the variance is re-estimated from the stored rows
}


def _loudest(ref, wav):
    """The base frame with the largest log energy (WMP_calc() of the reference, no normalisation)."""
    v = RefFrontend(ref).para(lib.param_kind("MFCC_E"), 13)
    rc = L.RefLiveChannel(ref, v)
    e = rc.segment(wav)[:, 12]
    rc.close()
    return int(np.argmax(e))


def _seg_plan(ref, i, wav, rng):
    """Segment i cut at seeded random samples into 1 - 6 pushes; segment 1 keeps its loudest frame in the first push,
    segment 2 in the last."""
    n = len(wav)
    cuts = sorted(set(rng.integers(1, n, rng.integers(0, 6)).tolist()))
    if i in (1, 2):
        am = _loudest(ref, wav)
        lo, hi = nsamp(am + 1), nsamp(am + 1) - 1  # frame am is complete with lo samples and not with hi
        if i == 1:
            cuts = [c for c in cuts if c >= lo] or [lo]
        else:
            cuts = [c for c in cuts if c <= hi] or [hi]
        chunks = to_chunks(n, cuts)
        done = np.cumsum(chunks)
        push_of = int(np.searchsorted(done, lo))   # the push that completes frame am
        assert len(chunks) >= 2 and push_of == (0 if i == 1 else len(chunks) - 1), (i, am, chunks)
    return to_chunks(n, cuts)


@pytest.mark.parametrize("case", list(STATE_CASES))
def test_state_over_segments(engine, ref, case):
    live, fields = STATE_CASES[case]
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, live=live, **fields)
    assert fe.desc.splice == 1
    rc = mk()
    rng = np.random.default_rng(300)
    npush = set()
    for i, Tb in enumerate(SEGS):
        wav = audio(Tb, 20 + i)
        chunks = _seg_plan(ref, i, wav, rng)
        npush.add(len(chunks))
        want = rc.segment(wav)
        got = cat(feed(lv, wav, chunks), 39)
        check_rows(got, want, f"{case} segment {i + 1} {chunks}")
        rc.commit()
        lv.commit()
        check_state(lv, 0, rc, rc.v, f"{case} after segment {i + 1}", emax=bool(fields.get("enormal")))
    assert min(npush) == 1 and max(npush) >= 5
    rc.close()


# ------------------------------------------------------------------------------------------------ 4. kinds
KIND_CASES = {
    "MFCC_E_D_N_Z_25": ("MFCC_E_D_N_Z", 25, 1, {}, False),
    "MFCC_0_D_A": ("MFCC_0_D_A", 39, 1, {}, False),
    "FBANK_D_A_Z_40": ("FBANK_D_A_Z", 120, 1, dict(fbank_num=40), False),
    "MFCC_plain": ("MFCC", 12, 1, {}, False),
    "enormal_escale01": ("MFCC_E_D_A_Z", 39, 1, dict(enormal=1, escale=0.1, silFloor=50.0), False),
    "splice3": ("MFCC_E_D_A_Z", 39, 3, {}, False),
    "splice3_cvn": ("MFCC_E_D_A_Z", 39, 3, dict(cvn=1), False),
    "ss_load": ("MFCC_E_D_A_Z", 39, 1, {}, True),
}


@pytest.mark.parametrize("case", list(KIND_CASES))
def test_kinds(engine, ref, case):
    """Three segments (loud, quiet, very loud) in 3 - 4 pushes each, committed after each.  The first pushes complete
    one vector, then two (segment 1) and two, then one (segment 2): with splice 3 that is no row and the first row."""
    kind, vecsize, splice, fields, with_ss = KIND_CASES[case]
    ss = None
    if with_ss:
        rs = RefFrontendSS(ref)
        ss = (rs.noise(audio(80, 72), rs.para(lib.param_kind(kind), vecsize)), 2.0, 0.5)
    fe, lv, mk = pair(engine, ref, kind, vecsize, splice=splice, ss=ss, **fields)
    rc = mk()
    v = rc.v
    Ld = (v.delWin if v.delta else 0) + (v.accWin if v.acc else 0)
    width = v.veclen * splice
    plans = ([Ld + 1, Ld + 3, 30], [Ld + 2, Ld + 3, 20], [17, 43, 69])      # base frames after each push but the last
    for i, (Tb, gain) in enumerate(((50, 1.0), (33, 0.004), (70, 3.0))):
        wav = audio(Tb, 40 + i, gain)
        chunks = to_chunks(len(wav), [nsamp(k) + 13 * i for k in plans[i]])
        want = rc.segment(wav)
        parts = feed(lv, wav, chunks)
        check_rows(cat(parts, width), want, f"{case} segment {i + 1}")
        vecs = np.diff([0] + [max(0, tb_of(x) - Ld) for x in np.cumsum(chunks)[:-1]])
        if i == 0:
            assert vecs[:2].tolist() == [1, 2]
            assert [len(p) for p in parts[:2]] == ([0, 1] if splice == 3 else [1, 2])
        if i == 1:
            assert vecs[:2].tolist() == [2, 1]
            assert [len(p) for p in parts[:2]] == ([0, 1] if splice == 3 else [2, 1])
        rc.commit()
        lv.commit()
        check_state(lv, 0, rc, v, f"{case} after segment {i + 1}", emax=bool(fields.get("enormal")))
    rc.close()


# ------------------------------------------------------------------------------------------------ 5. channels
def _channel_plan(nchan, ncall=6):
    """Per call (chunk of every channel, final bytes): seeded; the last call ends every open segment."""
    rng = np.random.default_rng(2000 + nchan)
    is_open = [False] * nchan
    pos = [0] * nchan                              # samples of the open segment
    nseg = [0] * nchan
    calls, kinds_seen = [], []
    for k in range(ncall):
        chunks, fin, what = [], np.zeros(nchan, bool), []
        for c in range(nchan):
            r = rng.random()
            if r < 0.2 and not (nchan == 3 and c == k % 3):
                chunks.append(np.zeros(0, np.int16))
                fin[c] = is_open[c] and (k == ncall - 1 or rng.random() < 0.3)   # idle, or an end without samples
                what.append("end" if fin[c] else "idle")
            else:
                n = int(rng.integers(1, 13 * SH))
                src = audio(240, 60 + (c + nseg[c]) % 5)
                gain = (0.05, 0.5, 2.0)[(c + nseg[c]) % 3]
                seg = src if gain == 1.0 else np.clip(np.round(src * gain), -32768, 32767).astype(np.int16)
                chunks.append(seg[pos[c]:pos[c] + n])
                fin[c] = k == ncall - 1 or rng.random() < 0.35
                what.append(("cont" if is_open[c] else "open") + ("+end" if fin[c] else ""))
                pos[c] += n
                is_open[c] = True
            if fin[c]:
                is_open[c], pos[c] = False, 0
                nseg[c] += 1
        calls.append((chunks, fin))
        kinds_seen.append(set(what))
    every = {"idle", "end", "cont", "cont+end", "open", "open+end"}
    if nchan > 3:                                  # all of it in one call
        assert any(every <= s for s in kinds_seen), kinds_seen
    else:
        assert {"idle", "cont", "cont+end", "open"} <= set().union(*kinds_seen), kinds_seen
    return calls


@pytest.mark.parametrize("nchan", [3, 65, 130])
def test_channels(engine, ref, nchan):
    """Six push_dev calls queued on one stream with a commit behind each, ragged chunks: in one call some channels are
    idle, some continue, some end and some open a segment.  Every channel equals the reference channel fed its own
    segments whole."""
    fields = dict(enormal=1, cvn=1)
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, nchan=nchan, **fields)
    calls = _channel_plan(nchan)
    # the reference, every channel alone over its whole segments
    refs = [mk() for _ in range(nchan)]
    want = [[] for _ in range(nchan)]              # rows per finished segment
    wstate = [None] * nchan
    for c, rc in enumerate(refs):
        acc = []
        for chunks, fin in calls:
            acc.append(chunks[c])
            if fin[c]:
                seg = np.concatenate(acc)
                acc = []
                if len(seg):                       # (an end without an open segment is nothing)
                    want[c].append(rc.segment(seg))
                    rc.commit()
    # the device: everything queued, then one wait
    bufs = []
    for chunks, fin in calls:
        samples, off = lib.Frontend._pack(chunks)
        rows = int(off[-1]) // SH + 8 * nchan
        bufs.append((lib.DevBuf(engine, max(samples.nbytes, 2)).upload(samples), off, lib.DevBuf(engine, rows * 39 * 4), rows))
    engine.sync()
    idle_state = {}
    foffs = []
    ended_any = [False] * nchan
    seg_open = [False] * nchan
    for k, (chunks, fin) in enumerate(calls):
        idle = [c for c in range(nchan) if len(chunks[c]) == 0 and not fin[c] and not seg_open[c]][:3]
        before = {c: lv.state(c) for c in idle} if k == 3 else {}
        foffs.append(lv.push_dev(bufs[k][0].ptr, bufs[k][1], bufs[k][2].ptr, final=fin))
        mask = np.zeros(nchan, bool)
        for c in range(nchan):
            had = seg_open[c] or len(chunks[c]) > 0
            if len(chunks[c]):
                seg_open[c] = True
            if fin[c] and had:
                mask[c] = True
                seg_open[c] = False
        lv.commit(mask)
        for c, st in before.items():               # a channel idle in this call and not committed: untouched
            now = lv.state(c)
            assert all(same(np.asarray(a), np.asarray(b)) for a, b in zip(st, now)), (k, c)
        idle_state.update(before)
    engine.sync()
    assert idle_state or nchan == 3
    got = [[] for _ in range(nchan)]
    for k, (chunks, fin) in enumerate(calls):
        foff = foffs[k]
        assert foff[0] == 0 and np.all(np.diff(foff) >= 0) and foff[-1] <= bufs[k][3]
        rows = bufs[k][2].download((int(foff[-1]), 39), np.float32) if foff[-1] else np.zeros((0, 39), np.float32)
        for c in range(nchan):
            got[c].append(rows[foff[c]:foff[c + 1]])
            if len(chunks[c]) == 0 and not fin[c]:
                assert foff[c + 1] == foff[c]
    for c, rc in enumerate(refs):
        allwant = cat(want[c], 39)
        check_rows(cat(got[c], 39), allwant, f"channel {c}")
        if want[c]:
            check_state(lv, c, rc, rc.v, f"channel {c}", emax=True)
        rc.close()


# ------------------------------------------------------------------------------------------------ 6. mixing, refusals
def test_mixing_and_refusals(engine, ref):
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, nchan=2, enormal=1, cvn=1)
    rc = mk()
    wavs = [audio(60, 30), audio(45, 31, 0.3), audio(52, 32, 2.0)]
    none = np.zeros(0, np.int16)
    # chunked, whole, chunked on channel 0; channel 1 stays idle
    rows, _ = lv.push_host([wavs[0][:3000], none])
    with pytest.raises(lib.JamdError, match=ESTATE):       # a whole-segment run while a segment is open
        lv.run_host([none, wavs[1]])
    with pytest.raises(lib.JamdError, match=ESTATE):
        lv.commit()
    with pytest.raises(lib.JamdError, match=ESTATE):
        lv.commit([True, False])
    with pytest.raises(lib.JamdError, match=ESTATE):
        lv.set_state(0, CM0, CV0)
    with pytest.raises(lib.JamdError, match=ESTATE):
        lv.stream_cap(100)
    lv.commit([False, True])                               # the idle channel may be committed (nothing to enter)
    rows2, _ = lv.push_host([wavs[0][3000:], none], [True, False])
    check_rows(np.concatenate([rows, rows2]), rc.segment(wavs[0]), "chunked segment 1")
    rc.commit(); lv.commit([True, False])
    got, foff = lv.run_host([wavs[1], none])
    check_rows(got, rc.segment(wavs[1]), "whole segment 2")
    rc.commit(); lv.commit([True, False])
    parts = [lv.push_host([wavs[2][:5000], none])[0], lv.push_host([wavs[2][5000:], none])[0],
             lv.push_host([none, none], [True, True])[0]]   # (channel 1 has no segment: nothing happens)
    check_rows(np.concatenate(parts), rc.segment(wavs[2]), "chunked segment 3")
    rc.commit(); lv.commit([True, False])
    check_state(lv, 0, rc, rc.v, "after three segments", emax=True)
    fresh = lib.LiveFrontend(fe, 1)
    st1, st0 = lv.state(1), fresh.state(0)
    assert st1[3] == 0 and same(np.float32(st1[2]), np.float32(st0[2]))    # channel 1 never ran
    # the cap on the stored rows (cvn with splice 1)
    lv.stream_cap(50)
    wav = audio(70, 33)
    want = rc.segment(wav)
    a = lv.push_host([wav[:nsamp(30)], none])[0]
    with pytest.raises(lib.JamdError, match=EINVAL):       # 60 frames in all: 56 rows before the end
        lv.push_host([wav[nsamp(30):nsamp(60)], none])
    b = lv.push_host([wav[nsamp(30):nsamp(50)], none])[0]  # 46 rows: fits, the segment goes on where it was
    assert len(a) == 26 and len(b) == 20
    with pytest.raises(lib.JamdError, match=EINVAL):       # the end would make 70
        lv.push_host([wav[nsamp(50):], none], [True, False])
    check_rows(np.concatenate([a, b]), want[:46], "under the cap")
    rc.close(); fresh.close()
    # a kind without cvn keeps no rows: no cap
    fe2, lv2, mk2 = pair(engine, ref, "MFCC_E_D_A_Z", 39)
    lv2.stream_cap(5)
    rc2 = mk2()
    check_rows(cat(feed(lv2, wav, [4000, len(wav) - 4000]), 39), rc2.segment(wav), "no cap without cvn")
    rc2.close()


def test_history_grows_to_the_cap(engine, ref):
    """A segment longer than the first allocation of the row history (cvn, splice 1): the stored rows move over and the
    re-estimated variance equals the reference's."""
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", 39, nchan=2, cvn=1)
    rc = mk()
    wav = np.concatenate([audio(240, 50), audio(240, 51), audio(200, 52)])
    want = rc.segment(wav)
    assert len(want) > 2 * 256
    none = np.zeros(0, np.int16)
    cuts = [nsamp(100), nsamp(300), nsamp(600)]
    parts = []
    for i, n in enumerate(to_chunks(len(wav), cuts)):
        pos = sum(to_chunks(len(wav), cuts)[:i])
        parts.append(lv.push_host([none, wav[pos:pos + n]], [False, i == len(cuts)])[0])
    check_rows(np.concatenate(parts), want, "long segment")
    rc.commit(); lv.commit([False, True])
    check_state(lv, 1, rc, rc.v, "after the long segment")
    rc.close()


# ------------------------------------------------------------------------------------------------ 7. into the first pass
def test_into_the_first_pass(engine, ref, tmp_path):
    """8 channels in pushes of 25 frames: push_dev -> Gmm.outprob_dev (the narrow kernel) -> Beam.stream_push_dev
    without a host copy; trellis and sentence equal run_dev -> outprob_utts_dev -> pass1_dev over the same segments."""
    eng, lex, am, task = ref_task(ref, tmp_path, 5, 300, nword=80, nphone=8, S=120, M=2)
    nchan, D, step = 8, 39, 25 * SH
    fe, lv, mk = pair(engine, ref, "MFCC_E_D_A_Z", D, nchan=nchan)
    lvw = lib.LiveFrontend(fe, nchan)             # the whole-segment side
    gm = lib.Gmm(engine, am)
    lx = lib.Lexicon(engine, lex)
    bm = lib.Beam(engine, lx, eng.beam_width, -1.0, max_utts=nchan)
    rng = np.random.default_rng(4)
    d_feat = lib.DevBuf(engine, nchan * 40 * D * 4)
    d_sc = lib.DevBuf(engine, nchan * 40 * gm.S * 4)
    for k in range(2):
        segs = [audio(int(rng.integers(30, 90)), 80 + (c + 3 * k) % 6, gain=float(rng.choice([0.2, 1.0]))) for c in range(nchan)]
        npush = max((len(s) + step - 1) // step for s in segs)
        bm.stream_begin(nchan)
        total = np.zeros(nchan, np.int64)
        for j in range(npush):
            chunks = [s[j * step:(j + 1) * step] for s in segs]
            fin = [len(s) <= (j + 1) * step and len(s) > j * step for s in segs]
            samples, off = lib.Frontend._pack(chunks)
            d_in = lib.DevBuf(engine, max(samples.nbytes, 2)).upload(samples)
            foff = lv.push_dev(d_in.ptr, off, d_feat.ptr, final=fin)
            assert foff[-1] <= nchan * 40
            if foff[-1]:
                gm.outprob_dev(d_feat.ptr, int(foff[-1]), d_sc.ptr)
                assert "gmm_narrow<D=39" in gm.last_kernel()
            bm.stream_push_dev(d_sc.ptr, gm.S, foff, final=j == npush - 1)
            total += np.diff(foff)
            engine.sync()
            d_in.free()
        lv.commit()
        res = bm.results(nchan)
        sres = [(r.status, r.natom, r.wnum, r.score, list(r.wseq[:r.wnum])) for r in res]
        stre = [lexblob.canonical_trellis(bm.trellis(c)) for c in range(nchan)]
        # the same segments whole
        samples, off = lib.Frontend._pack(segs)
        d_in = lib.DevBuf(engine, samples.nbytes).upload(samples)
        rows = sum(lvw.frames(len(s)) for s in segs)
        w_feat = lib.DevBuf(engine, rows * D * 4)
        w_sc = lib.DevBuf(engine, rows * gm.S * 4)
        woff = lvw.run_dev(d_in.ptr, off, w_feat.ptr)
        lvw.commit()
        assert list(np.diff(woff)) == list(total)
        gm.outprob_utts_dev(w_feat.ptr, woff, w_sc.ptr)
        bm.pass1_dev(w_sc.ptr, gm.S, woff)
        wres = bm.results()
        assert any(r.status == 0 and r.wnum > 0 for r in wres)
        for c in range(nchan):
            r = wres[c]
            assert sres[c] == (r.status, r.natom, r.wnum, r.score, list(r.wseq[:r.wnum])), (k, c)
            wt = lexblob.canonical_trellis(bm.trellis(c))
            assert all(np.array_equal(stre[c][key], wt[key]) for key in wt), (k, c)
        for b in (d_in, w_feat, w_sc):
            b.free()
