"""The silence cutting stage on the device (jamd_adin_cut, csrc/adin_cut.hip) against the reference helper
(adincutref.RefCut: the compiled count_zc_e() under a Python restatement of adin_cut()'s block loop), bit for bit after
every push: the samples delivered, the three part tables and the state of every channel.  Apart from one run with the
default parameters the tests use -headmargin 30 -tailmargin 40 -chunksize 100 (c_length 480, threshold 1, nc_max 8,
sbsize 784) on streams of about 10000 samples, where every branch of the block loop is taken several times."""
import collections

import numpy as np
import pytest

import adincutref as K
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu

SMALL = dict(head_margin_msec=30, tail_margin_msec=40, chunk_size=100)


class Pair:
    """The product and the helper side by side."""

    def __init__(self, engine, ref, nchan=1, **desc):
        self.engine, self.nchan = engine, nchan
        self.a = lib.AdinCut(engine, nchan, **desc)
        self.r = K.RefCut(ref, nchan, **desc)
        assert self.a.params() == (self.r.c_length, self.r.noise_zerocross, self.r.nc_max, self.r.sbsize)
        self.segs = [[] for _ in range(nchan)]   # per channel [start, [arrays], ended]
        self.most_parts = 0

    def close(self):
        self.a.close()
        self.r.close()

    def _record(self, parts):
        for c, ps in enumerate(parts):
            for p in ps:
                if p.start >= 0:
                    self.segs[c].append([p.start, [], False])
                if len(p.data()):
                    self.segs[c][-1][1].append(p.data())
                if p.final:
                    self.segs[c][-1][2] = True

    def check_state(self, chans=None):
        for c in range(self.nchan) if chans is None else chans:
            assert self.a.state(c) == self.r.state(c), c

    def push(self, chunks, eos=None, how="host", max_parts=None, chans=None):
        parts = self.r.push(chunks, eos)
        want = K.layout(parts, self.nchan)
        self.most_parts = max(self.most_parts, len(want[1]))
        if how == "host":
            got = self.a.push_host(chunks, eos, max_parts=max_parts)
        else:
            samples, off = lib.Frontend._pack(chunks)
            d_in = lib.DevBuf(self.engine, 2 * max(1, len(samples)))
            if len(samples):
                d_in.upload(samples)
            room = sum(self.a.push_cap(len(w)) for w in chunks)
            d_out = lib.DevBuf(self.engine, 2 * room)
            tabs = self.a.push_dev(d_in.ptr, off, d_out.ptr, eos, max_parts=max_parts)
            self.engine.sync()
            n = int(tabs[0][-1, -1]) if len(tabs[0]) else 0
            got = (d_out.download((room,), np.int16)[:n],) + tabs
            d_in.free()
            d_out.free()
        for g, w, name in zip(got, want, ("samples", "part_off", "part_final", "part_start")):
            assert g.shape == w.shape and np.array_equal(g, w), name
        self.check_state(chans)
        self._record(parts)
        return want

    def feed(self, w, cuts, c=0, eos=True, how="host"):
        """Channel c takes w[cuts[i]:cuts[i + 1]] push by push (the others nothing)."""
        for i in range(len(cuts) - 1):
            chunks = [np.zeros(0, np.int16)] * self.nchan
            chunks[c] = w[cuts[i]:cuts[i + 1]]
            flags = [False] * self.nchan
            flags[c] = eos and i == len(cuts) - 2
            self.push(chunks, flags, how=how)

    def delivered(self, c=0):
        return [(s, np.concatenate(a) if a else np.zeros(0, np.int16), e) for s, a, e in self.segs[c]]


def _steps(n, k):
    return list(range(0, n, k)) + [n]


def _random_cuts(n, rng, top):
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + (0 if rng.random() < 0.2 else int(rng.integers(1, top)))))
    return cuts


def _square(n, half, amp):
    return (amp * (1 - 2 * ((np.arange(n) // half) % 2))).astype(np.int32)


# ---- every branch of the block loop

def test_default_parameters_six_seconds(engine, ref):
    w = K.bursts(2)
    p = Pair(engine, ref)
    p.feed(w, _steps(len(w), 4000))
    segs = p.delivered()
    assert [len(s[1]) for s in segs] == [18800, 17800, 26800, 9600] and all(s[2] for s in segs)
    ev = p.r.events
    assert ev["retrigger_swap"] and ev["swapped"] and ev["tail_delivered"] and ev["end_eos"] == 1
    p.close()


def test_event_coverage(engine, ref):
    ev = collections.Counter()
    rng = np.random.default_rng(5)
    for seed in (1, 2, 3, 5):
        w = K.bursts(seed, 0.1)
        p = Pair(engine, ref, **SMALL)
        p.feed(w, _random_cuts(len(w), rng, 900))
        ev.update(p.r.events)
        p.close()
    p = Pair(engine, ref, 4, **SMALL)
    loud = _square(1000, 3, 7000).astype(np.int16)
    p.feed(loud, [0, 250, 1000], c=0)                        # loud from the first sample: a trigger in the first block
    p.feed(np.zeros(300, np.int16), [0, 300], c=1)           # end of stream while idle, nothing waiting
    p.feed(loud[:37], [0, 37], c=2)                          # a stream shorter than a block
    p.feed(loud[:337], [0, 337], c=3)                        # a short last block inside a segment
    p.feed(loud, [0, 1000], c=0)                             # ... and the channels serve their next streams as new
    ev.update(p.r.events)
    p.close()
    print(dict(ev))
    missing = [k for k in K.EVENTS if not ev[k]]
    assert not missing, missing


# ---- however the stream is cut

def test_cut_invariance(engine, ref):
    w = K.bursts(2, 0.1)
    rng = np.random.default_rng(9)
    ways = [[0, len(w)], _steps(len(w), 99), _steps(len(w), 100), _steps(len(w), 101), _random_cuts(len(w), rng, 700),
            _random_cuts(len(w), rng, 2500)]
    results = []
    for i, cuts in enumerate(ways):
        p = Pair(engine, ref, **SMALL)
        p.feed(w, cuts, eos=False, how="dev" if i % 2 else "host")
        results.append((p.delivered(), p.a.state(0)))
        p.close()
    assert len(results[0][0]) == 4
    for got, state in results[1:]:
        assert state == results[0][1] and len(got) == len(results[0][0])
        for x, y in zip(got, results[0][0]):
            assert x[0] == y[0] and x[2] == y[2] and np.array_equal(x[1], y[1])


def test_pushes_of_one_sample(engine, ref):
    w = K.bursts(3, 0.1)[:1400]                              # a trigger at sample 20, speech for 800, silence
    whole = Pair(engine, ref, **SMALL)
    whole.feed(w, [0, len(w)])
    p = Pair(engine, ref, **SMALL)
    p.feed(w, _steps(len(w), 1))
    a, b = p.delivered(), whole.delivered()
    assert len(b) >= 1 and len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[2] == y[2] and np.array_equal(x[1], y[1])
    whole.close()
    p.close()


# ---- sample-level edges

def _edge(engine, ref, w, desc, expect_segments, steps=(None, 100, 7)):
    w = np.asarray(w).astype(np.int16)
    for k in steps:
        p = Pair(engine, ref, **desc)
        p.feed(w, [0, len(w)] if k is None else _steps(len(w), k))
        assert len(p.delivered()) == expect_segments, (k, len(p.delivered()))
        p.close()


def test_level_exactly_at_the_trigger_does_not_arm(engine, ref):
    quiet = np.zeros(500, np.int32)
    for amp, n in ((2000, 0), (2001, 1)):
        _edge(engine, ref, np.concatenate([quiet, _square(400, 5, amp), quiet]), SMALL, n)
        _edge(engine, ref, np.concatenate([quiet, -_square(400, 5, amp), quiet]), SMALL, n)


def test_minus_32768_arms(engine, ref):
    quiet = np.zeros(500, np.int32)
    for low, n in ((-32767, 0), (-32768, 1)):
        w = np.concatenate([quiet, np.tile(np.array([low, low, 1, 1], np.int32), 100), quiet])
        _edge(engine, ref, w, dict(SMALL, level_thres=32767), n)


def test_zeros_between_the_signs_and_the_threshold_count(engine, ref):
    quiet = np.zeros(600, np.int32)
    up, down, zeros = np.full(6, 5000, np.int32), np.full(6, -5000, np.int32), np.zeros(9, np.int32)
    # one crossing in the window is noise_zerocross itself: no trigger; a second one triggers
    _edge(engine, ref, np.concatenate([quiet, up, zeros, down, quiet]), SMALL, 0)
    _edge(engine, ref, np.concatenate([quiet, up, zeros, down, zeros, up, quiet]), SMALL, 1)
    # two crossings more than c_length apart never share a window
    _edge(engine, ref, np.concatenate([quiet, up, down, np.zeros(480, np.int32), up, quiet]), SMALL, 0)


def test_crossings_leave_the_count_c_length_later(engine, ref):
    """Crossings at every sample around stream index 120 (20 behind a block end, as 480 behind a later block end is):
    the counts of the blocks that end 480 samples later must drop exactly there.  Block by block against the helper."""
    w = np.zeros(1500, np.int32)
    w[112:129] = _square(17, 1, 4000)
    w[600:603] = [3000, -3000, 3000]
    p = Pair(engine, ref, **SMALL)
    counts = []
    for i in range(15):
        p.push([w[100 * i:100 * i + 100].astype(np.int16)], [i == 14])
        counts.append(p.r.state(0)[4] if i < 14 else None)
    print(counts)
    assert counts[:11] == [0, 16, 16, 16, 16, 9, 2, 2, 2, 2, 0]   # 9: the crossings at 120 ... 128 are still inside [120, 600)
    p.close()


def test_armed_in_one_push_crossing_in_the_next_and_across_a_tile_edge(engine, ref):
    w = np.zeros(3700, np.int32)
    w[1023], w[1024], w[1025] = 5000, -5000, 5000            # armed by the last sample of a 1024-sample step
    w[3071], w[3072] = -5000, 5000                           # ... and of the third, after the first segment has ended
    _edge(engine, ref, w, SMALL, 2, steps=(None,))
    for cut in (1023, 1024, 1025):
        p = Pair(engine, ref, **SMALL)
        p.feed(w.astype(np.int16), [0, cut, len(w)])
        assert len(p.delivered()) == 2
        p.close()


@pytest.mark.parametrize("thres", [0, -5])
def test_level_zero_and_negative(engine, ref, thres):
    rng = np.random.default_rng(3)
    w = np.round(rng.normal(0, 30, 3000)).astype(np.int16)
    w[1000:2200] = 0                                         # with -lv 0 a zero does not arm; below 0 everything does
    p = Pair(engine, ref, **dict(SMALL, level_thres=thres))
    p.feed(w, _steps(len(w), 333))
    assert len(p.delivered()) >= 1
    p.close()


# ---- many channels

@pytest.mark.parametrize("nchan", [1, 3, 65, 130])
def test_ragged_channels(engine, ref, nchan):
    rng = np.random.default_rng(nchan)
    base = [K.bursts(s, 0.1) for s in (2, 3, 4, 5, 1)]
    ws = [base[c % 5][(37 * c) % 900:] for c in range(nchan)]
    at = [0] * nchan
    p = Pair(engine, ref, nchan, **SMALL)
    watch = None if nchan <= 3 else sorted(set([0, 1, 63, 64, nchan - 1]) | set(int(x) for x in rng.integers(0, nchan, 6)))
    for push in range(8):
        chunks, eos = [], []
        for c in range(nchan):
            if push == 0 and c % 4 == 0:
                n = len(ws[c])                               # a whole stream at once: several segment ends in one push
            elif (c + push) % 5 == 0:
                n = 0                                        # idle
            else:
                n = int(rng.integers(1, 3000))
            n = min(n, len(ws[c]) - at[c])
            chunks.append(ws[c][at[c]:at[c] + n])
            at[c] += n
            done = at[c] == len(ws[c]) and n > 0
            eos.append(done)
            if done:
                at[c] = 0                                    # the channel's next stream: the same samples again
        if push == 0:                                        # one part too few: refused, and nothing has moved
            t = K.RefCut(ref, nchan, **SMALL)
            need = len(K.layout(t.push(chunks, eos), nchan)[1])
            t.close()
            assert need >= 3
            with pytest.raises(lib.JamdError, match="parts"):
                p.a.push_host(chunks, eos, max_parts=need - 1)
            p.check_state(watch)
        p.push(chunks, eos, how="dev" if push % 2 == 0 else "host", chans=watch)
    assert p.most_parts >= 3
    p.check_state()
    p.close()


def test_reset_of_some_channels_mid_segment(engine, ref):
    w = K.bursts(2, 0.1)
    p = Pair(engine, ref, 3, **SMALL)
    p.push([w[:1750], w[:1750], w[:1633]])
    assert [p.r.state(c)[0] for c in range(3)] == [1, 1, 1]  # all three inside their first segment
    p.a.reset([0, 1, 0])
    p.r.reset([0, 1, 0])
    p.check_state()
    assert p.a.state(1) == (0, 0, 0, 0, 0, 0, 0)
    p.push([w[1750:4000], w[:2500], w[1633:4000]])           # channel 1 starts over, the others go on
    p.a.reset()
    p.r.reset()
    p.check_state()
    p.push([w[:3000]] * 3, [False, True, False])
    p.close()


def test_host_and_device_entry_points_agree(engine, ref):
    w = K.bursts(5, 0.1)
    a, b = Pair(engine, ref, 2, **SMALL), Pair(engine, ref, 2, **SMALL)
    for lo, hi in ((0, 2999), (2999, 3000), (3000, 8000), (8000, len(w))):
        chunks, eos = [w[lo:hi], w[lo // 2:hi // 2]], [hi == len(w), False]
        x = a.push(chunks, eos, how="host")
        y = b.push(chunks, eos, how="dev")
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    a.close()
    b.close()


def test_refusals(engine):
    with pytest.raises(lib.JamdError, match="swap buffer"):
        lib.AdinCut(engine, 1, head_margin_msec=30, tail_margin_msec=40, chunk_size=480)
    with pytest.raises(lib.JamdError, match="header margin"):
        lib.AdinCut(engine, 1, chunk_size=4801)
    a = lib.AdinCut(engine, 2, **SMALL)
    with pytest.raises(lib.JamdError, match="max_parts"):
        a.push_host([np.zeros(5, np.int16)] * 2, max_parts=0)
    with pytest.raises(lib.JamdError, match="descending"):
        a.push_dev(0, [0, 5, 3], 0, max_parts=4)
    with pytest.raises(lib.JamdError, match="NULL input"):
        a.push_dev(0, [0, 5, 9], 0, max_parts=4)
    with pytest.raises(lib.JamdError, match="out of range"):
        a.state(2)
    assert a.state(0) == (0, 0, 0, 0, 0, 0, 0)
    a.close()


# ---- from 48 kHz samples to feature rows without a host copy between the stages

KIND = "MFCC_E_D_A_Z"


@pytest.mark.parametrize("nchan", [1, 3])
def test_adin_cut_live_chain(engine, ref, nchan):
    import adinref as R
    import frontendliveref as L
    from frontendref import RefFrontend
    tabs = R.tables(ref)
    rng = np.random.default_rng(40 + nchan)
    ws = []
    for c in range(nchan):                                   # 48 kHz: three bursts between noise, DC, runs of zeros
        parts = []
        for i, (g, b) in enumerate(((0.3, 0.5), (1.0, 0.35), (0.9, 0.4))):
            parts.append(rng.normal(0, 30, int((g + 0.1 * c) * 48000)))
            parts.append(synth.make_audio(int(b * 48000), seed=70 + 10 * c + i, sfreq=48000, dc=0.0, zero_runs=0,
                                          silent_frac=0, clip=False).astype(np.float64))
        w = np.round(np.concatenate(parts) + 250.0 * (c + 1)).clip(-32768, 32767).astype(np.int16)
        w[20000:20600] = 0
        w[70000 + 999 * c:70040 + 999 * c] = 0
        ws.append(w)
    ad = lib.Adin(engine, nchan, fir_3to4=tabs[0], fir_2to1=tabs[1], zmean=True)
    rad = R.RefAdin(ref, nchan, down48=True, strip_zero=True, zmean=True)
    cut = lib.AdinCut(engine, nchan)
    rcut = K.RefCut(ref, nchan)
    fe = lib.Frontend.from_kind(engine, KIND, 39)
    lv = lib.LiveFrontend(fe, nchan)
    step = 36000                                             # 0.75 s per push
    npush = max(-(-len(w) // step) for w in ws)
    d_in = lib.DevBuf(engine, 2 * nchan * step)
    d_mid = lib.DevBuf(engine, 2 * nchan * step)
    d_cut = lib.DevBuf(engine, 2 * nchan * cut.push_cap(step))
    max_rows = nchan * (cut.push_cap(step) // 160 + 32)
    d_out = lib.DevBuf(engine, 4 * max_rows * lv.veclen)
    got = [[] for _ in range(nchan)]                         # per channel the rows, and where its segments end
    ends = [[] for _ in range(nchan)]
    want_segs = [[] for _ in range(nchan)]
    for i in range(npush):
        chunks = [w[i * step:(i + 1) * step] for w in ws]
        eos = [len(w) <= (i + 1) * step and len(w) > i * step for w in ws]
        samples, off = lib.Frontend._pack(chunks)
        if len(samples):
            d_in.upload(samples)
        moff = ad.push_dev(d_in.ptr, off, d_mid.ptr)
        poff, pfin, pst = cut.push_dev(d_mid.ptr, moff, d_cut.ptr, eos)
        for row in range(len(poff)):
            foff = lv.push_dev(d_cut.ptr, poff[row], d_out.ptr, final=pfin[row])
            engine.sync()
            rows = d_out.download((max_rows, lv.veclen), np.float32)
            for c in range(nchan):
                got[c].append(rows[foff[c]:foff[c + 1]].copy())
                if pfin[row, c]:
                    ends[c].append(sum(len(r) for r in got[c]))
        for c, ps in enumerate(rcut.push(rad.push(chunks), eos)):
            for p in ps:
                if p.start >= 0:
                    want_segs[c].append([])
                if len(p.data()):
                    want_segs[c][-1].append(p.data())
    v = RefFrontend(ref).para(lib.param_kind(KIND), 39)
    for c in range(nchan):
        rc = L.RefLiveChannel(ref, v)
        want = [rc.segment(np.concatenate(s)) for s in want_segs[c]]
        rc.close()
        assert len(want) >= 3 and rcut.events["trigger_head"] >= 3 * nchan
        rows = np.concatenate(got[c])
        assert ends[c] == list(np.cumsum([len(x) for x in want]))
        assert np.array_equal(rows, np.concatenate(want)), c
    for o in (lv, fe, cut, ad):
        o.close()
    rad.close()
    rcut.close()
