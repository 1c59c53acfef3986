"""The audio conditioning stage (jamd_adin: -48, -lvscale, zero stripping, -zmean) on the device against the compiled
reference (tests/adinref.py: ds48to16(), strip_zero(), sub_zmean() of oracle/_ref/libjref.so): samples, counts and
state, all with np.array_equal.  Sizes are the smallest at which a kernel takes another path: the FIR stages consume
blocks of 256 and drop 36 / 100 / 100 outputs, a FIR workgroup computes 1024 outputs, the strip workgroup steps
through a chunk 1024 samples at a time with 15 neighbours each side, ZMEANSAMPLES is 48000."""
import numpy as np
import pytest

import adinref as R
from frontendref import RefFrontend
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu
TILE = 1024                        # kAdPostTile / kAdFirTile (csrc/adin_host.h)


@pytest.fixture(scope="module")
def tabs(ref):
    return R.tables(ref)


def _pair(engine, ref, tabs, nchan=1, down48=False, **kw):
    d = lib.Adin.desc_for(fir_3to4=tabs[0] if down48 else None, fir_2to1=tabs[1] if down48 else None, **kw)
    return lib.Adin(engine, nchan, d), R.RefAdin(ref, nchan, down48=down48, **kw)


def _check_state(a, r, c):
    zlen, zmean, arrived, emitted = a.state(c)
    if r.zmean:
        assert zlen == r.zlen[c], (c, zlen, r.zlen[c])
    if r.down48:
        st, n_in, n_out = r.ds_state(c)
        assert arrived[0] == n_in and emitted[2] == n_out, (c, arrived, emitted, n_in, n_out)
        assert arrived[1] == emitted[0] and arrived[2] == emitted[1]
        for s in range(3):
            assert arrived[s] % 256 == st[s][0], (c, s, arrived, st)
            if emitted[s] > 0:
                assert st[s][1] == 0                       # the delay is spent
    return zlen, zmean


def _push_both(a, r, chunks, how="host"):
    """One push on both; the outputs, the offsets and every channel's state must agree.  Returns the per-channel output."""
    chunks = [np.ascontiguousarray(w, np.int16) for w in chunks]
    want = r.push(chunks)
    if how == "host":
        got, off = a.push_host(chunks)
    else:
        samples, ioff = lib.Frontend._pack(chunks)
        cap = sum(len(w) for w in chunks)
        d_in = lib.DevBuf(a.eng, max(2, 2 * len(samples))).upload(samples if len(samples) else np.zeros(1, np.int16))
        d_out = lib.DevBuf(a.eng, max(2, 2 * cap))
        off = a.push_dev(d_in.ptr, ioff, d_out.ptr)
        a.eng.sync()
        got = d_out.download((max(1, cap),), np.int16)[:int(off[-1])]
    lens = [len(w) for w in want]
    assert list(np.diff(off)) == lens, (list(np.diff(off))[:8], lens[:8])
    for c in range(a.nchan):
        g = got[off[c]:off[c + 1]]
        if not np.array_equal(g, want[c]):
            bad = np.flatnonzero(g != want[c])
            raise AssertionError(f"channel {c}: {len(bad)} of {len(g)} samples differ, first at {bad[0]}: "
                                 f"{g[bad[0]]} != {want[c][bad[0]]}")
        _check_state(a, r, c)
    return want


def _close(a, r):
    a.close()
    r.close()


# ---- down-sampling

@pytest.fixture(scope="module")
def audio48():
    return synth.make_audio(144000, seed=7, sfreq=48000, zero_runs=0)


@pytest.mark.parametrize("n", [767, 768, 769, 144000])
def test_downsample_one_channel(engine, ref, tabs, audio48, n):
    a, r = _pair(engine, ref, tabs, down48=True, strip_zero=False)
    out = _push_both(a, r, [audio48[:n]])
    assert len(out[0]) == a.ds_count(0, n) == {767: 0, 768: 28, 769: 28, 144000: 47772}[n]
    _close(a, r)


@pytest.mark.parametrize("step", [1, 255, 256, 257, "random"])
def test_downsample_does_not_depend_on_the_cuts(engine, ref, tabs, audio48, step):
    n = 144000
    w = audio48
    whole = R.RefAdin(ref, 1, down48=True, strip_zero=False)
    want = whole.push([w])[0]
    whole.close()
    a = lib.Adin(engine, 1, lib.Adin.desc_for(fir_3to4=tabs[0], fir_2to1=tabs[1], strip_zero=False))
    rng = np.random.default_rng(5)
    got, at, before = [], 0, 0
    while at < n:
        # (one sample per push over the first 10000 -- 39, 51 and 25 block edges of the three stages, the first output
        # at 768 -- then the rest at once: 144000 such pushes would take minutes)
        k = int(rng.integers(1, 9000)) if step == "random" else (n if step == 1 and at >= 10000 else step)
        k = min(k, n - at)
        o, off = a.push_host([w[at:at + k]])
        assert off[1] == a.ds_count(before, k)
        got.append(o)
        at += k
        before += k
    assert np.array_equal(np.concatenate(got), want)
    assert a.state(0)[3][2] == len(want)
    a.close()


def test_downsample_ragged_channels(engine, ref, tabs):
    nchan = 130
    rng = np.random.default_rng(11)
    a, r = _pair(engine, ref, tabs, nchan=nchan, down48=True, strip_zero=False)
    for push in range(2):
        lens = rng.integers(0, 6001, nchan)
        lens[rng.integers(0, nchan, 20)] = 0               # idle channels
        lens[0], lens[1] = (0, 6000) if push == 0 else (6000, 0)
        chunks = [synth.make_audio(int(k), seed=1000 * push + c, sfreq=48000, zero_runs=0) for c, k in enumerate(lens)]
        _push_both(a, r, chunks, how="dev" if push else "host")
    _close(a, r)


def test_downsample_state_carried_across_files(engine, ref, tabs):
    f1 = synth.make_audio(20000, seed=21, sfreq=48000, zero_runs=0)
    f2 = synth.make_audio(15000, seed=22, sfreq=48000, zero_runs=0)
    a, r = _pair(engine, ref, tabs, down48=True, strip_zero=False)
    _push_both(a, r, [f1])
    carried = _push_both(a, r, [f2])[0]                    # the program: pending samples and history of file 1 go on
    a.reset(what=lib.ADIN_DS)
    r.reset(what=R.DS)
    assert a.state(0)[2].tolist() == [0, 0, 0]
    fresh = _push_both(a, r, [f2])[0]
    assert len(carried) != len(fresh) or not np.array_equal(carried, fresh)
    _close(a, r)


def test_downsample_full_scale_square_wave(engine, ref, tabs):
    w = np.where((np.arange(20000) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    a, r = _pair(engine, ref, tabs, down48=True, strip_zero=False)
    _push_both(a, r, [w])
    _close(a, r)


@pytest.mark.parametrize("n34,n21", [(1, 1), (2, 3), (7, 8), (216, 400), (217, 6), (12, 401)])
def test_downsample_other_table_lengths(engine, ref, tabs, n34, n21):
    """The descriptor takes tables of 1 ... 513 entries: lengths at which a kernel's unguarded middle loop is empty, the
    filter length is odd (the history is rounded up to even) or a delay is 0, against the reference made with the same
    tables, two channels in three pushes."""
    rng = np.random.default_rng(n34 * 1000 + n21)
    t = (rng.normal(0, 1.0 / n34, n34), rng.normal(0, 1.0 / n21, n21))
    a = lib.Adin(engine, 2, lib.Adin.desc_for(fir_3to4=t[0], fir_2to1=t[1], strip_zero=False))
    r = R.RefAdin(ref, 2, down48=True, strip_zero=False, tabs=t)
    assert R.tables(ref)[0].tobytes() == tabs[0].tobytes() and R.tables(ref)[1].tobytes() == tabs[1].tobytes()
    ws = [synth.make_audio(9000, seed=70 + c, sfreq=48000, zero_runs=0) for c in range(2)]
    for lo, hi in ((0, 700), (700, 4097), (4097, 9000)):
        _push_both(a, r, [ws[0][lo:hi], ws[1][lo // 2:hi]])
    assert a.state(0)[3][2] > 0
    _close(a, r)


# ---- level

@pytest.mark.parametrize("coef", [0.5, 2.0])
def test_level_on_rail_values(engine, ref, tabs, coef):
    w = np.array([32767, -32768, 20000, -20000, 16384, -16384, 16383, 1, -1, 3, -3, 0, 12345, -32767] * 20, np.int16)
    a, r = _pair(engine, ref, tabs, level_coef=coef, strip_zero=False)
    out = _push_both(a, r, [w])[0]
    if coef == 2.0:
        assert out[2] == -25536                            # 40000 wraps
    _close(a, r)


# ---- zero stripping

def _noise(n, seed):
    w = np.random.default_rng(seed).integers(-3000, 3000, n).astype(np.int16)
    w[(w == 0) | (w == -32767)] = 5
    return w


@pytest.mark.parametrize("run", [15, 16, 17])
def test_strip_run_lengths(engine, ref, tabs, run):
    w = _noise(500, 1)
    w[100:100 + run] = 0
    a, r = _pair(engine, ref, tabs)
    out = _push_both(a, r, [w])[0]
    assert len(out) == (500 if run < 16 else 500 - run)
    _close(a, r)


def test_strip_runs_at_the_ends_mixed_values_and_minus_32768(engine, ref, tabs):
    w = _noise(3000, 2)
    w[:20] = 0                                             # from the first sample
    w[-18:] = -32767                                       # to the last
    w[500:540:2], w[501:540:2] = 0, -32767                 # 0 and -32767 mixed: one run
    w[800:830] = 0
    w[815] = -32768                                        # valid: cuts the run into 15 + 14
    w[1000:1015] = 0                                       # a run of 15 that ends at a run start: kept
    a, r = _pair(engine, ref, tabs)
    out = _push_both(a, r, [w])[0]
    assert len(out) == 3000 - 20 - 18 - 40
    _close(a, r)


def test_strip_run_across_a_push_boundary_is_kept(engine, ref, tabs):
    w = _noise(400, 3)
    w[192:208] = 0
    a, r = _pair(engine, ref, tabs)
    o1 = _push_both(a, r, [w[:200]])[0]
    o2 = _push_both(a, r, [w[200:]])[0]
    assert len(o1) + len(o2) == 400                        # 8 + 8: neither chunk holds a run of 16
    _close(a, r)


def test_strip_runs_at_tile_edges(engine, ref, tabs):
    w = _noise(5 * TILE + 100, 4)
    for k in range(1, 6):
        for d, ln in ((-1, 16), (0, 17), (1, 15)):
            at = k * TILE + d - (8 if k % 2 else 0)        # starting at the edge, and straddling it
            w[at + 40 * d:at + 40 * d + ln] = 0
    w[2 * TILE - 16:2 * TILE] = 0                          # ends exactly at an edge
    w[3 * TILE:3 * TILE + 16] = -32767                     # starts exactly at one
    w[4 * TILE - 1:4 * TILE + 1] = 0                       # two samples over an edge: kept
    a, r = _pair(engine, ref, tabs, nchan=2)
    _push_both(a, r, [w, w[::-1].copy()], how="dev")
    _close(a, r)


def test_strip_wholly_invalid_chunk(engine, ref, tabs):
    a, r = _pair(engine, ref, tabs, nchan=3)
    out = _push_both(a, r, [np.zeros(2500, np.int16), _noise(100, 5), np.full(16, -32767, np.int16)])
    assert [len(o) for o in out] == [0, 100, 0]
    _close(a, r)


# ---- DC removal

def test_zmean_one_long_chunk(engine, ref, tabs):
    w = synth.make_audio(60000, seed=31, dc=700.0, zero_runs=0)
    a, r = _pair(engine, ref, tabs, zmean=True, strip_zero=False)
    _push_both(a, r, [w])
    assert a.state(0)[0] == 60000
    _close(a, r)


def test_zmean_estimate_stops_at_48000(engine, ref, tabs):
    w = synth.make_audio(60000, seed=32, dc=-450.0, zero_runs=0)
    a, r = _pair(engine, ref, tabs, zmean=True, strip_zero=False)
    at, means = 0, []
    for k in (1000, 19000, 30000, 10000):
        _push_both(a, r, [w[at:at + k]])
        at += k
        means.append(a.state(0)[:2])
    assert [m[0] for m in means] == [1000, 20000, 50000, 50000]
    assert means[2][1] == means[3][1] and means[0][1] != means[1][1]   # the last chunk no longer updates
    _close(a, r)


def test_zmean_float_chain_is_walked_in_order(engine, ref, tabs):
    rng = np.random.default_rng(33)
    w = (30001 + rng.integers(-40, 40, 40000)).astype(np.int16)        # prefix sums pass 2^24: float adds round
    a, r = _pair(engine, ref, tabs, zmean=True, strip_zero=False)
    out = _push_both(a, r, [w])[0]
    exact = np.round(w.astype(np.float32) - np.float32(w.astype(np.int64).sum() / len(w))).astype(np.int16)
    assert not np.array_equal(out, exact)                  # (what an exact mean would have given: the case bites)
    _close(a, r)


def test_zmean_rounding_and_both_clips(engine, ref, tabs):
    a, r = _pair(engine, ref, tabs, nchan=3, zmean=True, strip_zero=False)
    up = np.array([32767] * 50 + [-32768] * 3, np.int16)   # positive mean under -32768: clipped at the lower rail
    dn = np.array([-32768] * 50 + [32767] * 3, np.int16)
    out = _push_both(a, r, [np.array([1, 2], np.int16), up, dn])
    assert out[0].tolist() == [-1, 1]                      # mean 1.5: -0.5 and 0.5, both away from zero
    assert out[1][-1] == -32768 and out[2][-1] == 32767
    _close(a, r)


def test_zmean_chunk_stripped_to_nothing_gives_nan(engine, ref, tabs):
    a, r = _pair(engine, ref, tabs, nchan=2, zmean=True)
    w = _noise(300, 6)
    _push_both(a, r, [np.zeros(40, np.int16), np.zeros(0, np.int16)])     # channel 1 idle: untouched
    assert np.isnan(a.state(0)[1]) and a.state(1)[:2] == (0, 0.0)
    out = _push_both(a, r, [w, w])
    assert not out[0].any() and out[1].any()               # NaN mean: every later sample 0
    a.reset(mask=[1, 0], what=lib.ADIN_ZMEAN)
    r.reset(mask=[1, 0], what=R.ZMEAN)
    out = _push_both(a, r, [w, w])
    assert out[0].any()
    _close(a, r)


# ---- everything on

def test_all_steps_in_three_pushes(engine, ref, tabs):
    nchan = 3
    a, r = _pair(engine, ref, tabs, nchan=nchan, down48=True, level_coef=1.7, zmean=True)
    ws = [synth.make_audio(90000, seed=40 + c, sfreq=48000, dc=500.0 * (c - 1), zero_runs=6) for c in range(nchan)]
    for w in ws:
        w[30000:33000] = 0                                 # digital silence: about 1000 samples at 16 kHz
    cuts = [(0, 25000, 60001, 90000), (0, 30000, 30000, 90000), (0, 1000, 50000, 89000)]
    for p in range(3):
        _push_both(a, r, [ws[c][cuts[c][p]:cuts[c][p + 1]] for c in range(nchan)], how="dev" if p == 1 else "host")
    _close(a, r)


# ---- into the front ends

KIND = "MFCC_E_D_A_Z"


def test_push_dev_feeds_the_buffered_front_end(engine, ref, tabs):
    ws = [synth.make_audio(n, seed=50 + i, sfreq=48000, dc=300.0, zero_runs=3) for i, n in enumerate((40000, 61000))]
    a, r = _pair(engine, ref, tabs, nchan=2, down48=True, zmean=True)
    want = r.push(ws)
    samples, ioff = lib.Frontend._pack(ws)
    d_in = lib.DevBuf(engine, 2 * len(samples)).upload(samples)
    d_mid = lib.DevBuf(engine, 2 * sum(a.push_cap(0, len(w)) for w in ws))
    off = a.push_dev(d_in.ptr, ioff, d_mid.ptr)
    assert list(np.diff(off)) == [len(w) for w in want]
    fe = lib.Frontend.from_kind(engine, KIND, 39)
    rf = RefFrontend(ref)
    v = rf.para(lib.param_kind(KIND), 39)
    T = [fe.frames(len(w)) for w in want]
    d_out = lib.DevBuf(engine, 4 * max(1, sum(T)) * fe.veclen)
    foff = fe.run_dev(d_mid.ptr, off, d_out.ptr)
    engine.sync()
    got = d_out.download((sum(T), fe.veclen), np.float32)
    assert list(np.diff(foff)) == T
    for c in (0, 1):
        assert np.array_equal(got[foff[c]:foff[c + 1]], rf.wav2mfcc(want[c], v))
    fe.close()
    _close(a, r)


def test_push_dev_feeds_the_live_front_end(engine, ref, tabs):
    import frontendliveref as L
    w = synth.make_audio(100000, seed=60, sfreq=48000, dc=-200.0, zero_runs=3)
    cuts = (0, 30000, 70001, 100000)
    a, r = _pair(engine, ref, tabs, down48=True, zmean=True)
    fe = lib.Frontend.from_kind(engine, KIND, 39)
    lv = lib.LiveFrontend(fe, 1)
    d_in = lib.DevBuf(engine, 2 * len(w))
    d_mid = lib.DevBuf(engine, 2 * len(w))
    d_out = lib.DevBuf(engine, 4 * 400 * lv.veclen)
    conditioned, rows = [], []
    for p in range(3):
        chunk = w[cuts[p]:cuts[p + 1]]
        conditioned.append(r.push([chunk])[0])
        d_in.upload(chunk)
        off = a.push_dev(d_in.ptr, [0, len(chunk)], d_mid.ptr)
        assert off[1] == len(conditioned[-1])
        foff = lv.push_dev(d_mid.ptr, off, d_out.ptr, final=[p == 2])
        engine.sync()
        rows.append(d_out.download((400, lv.veclen), np.float32)[:foff[1]].copy())
    v = RefFrontend(ref).para(lib.param_kind(KIND), 39)
    rc = L.RefLiveChannel(ref, v)
    want = rc.segment(np.concatenate(conditioned))
    rc.close()
    assert np.array_equal(np.concatenate(rows), want)
    lv.close()
    fe.close()
    _close(a, r)


# ---- refusals

def test_refusals(engine, tabs):
    with pytest.raises(lib.JamdError, match="tables"):
        lib.Adin(engine, 1, lib.Adin.desc_for(down48=True))
    with pytest.raises(lib.JamdError, match="513"):
        lib.Adin(engine, 1, lib.Adin.desc_for(fir_3to4=np.zeros(514), fir_2to1=tabs[1]))
    with pytest.raises(lib.JamdError, match="level_coef"):
        lib.Adin(engine, 1, lib.Adin.desc_for(level_coef=65536.0))
    lib.Adin(engine, 1, lib.Adin.desc_for(level_coef=65535.0)).close()
    a = lib.Adin(engine, 2)
    with pytest.raises(lib.JamdError, match="what"):
        a.reset(what=0)
    a.close()
