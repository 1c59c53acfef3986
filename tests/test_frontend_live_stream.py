"""The host half of chunked live input, without a device: the rows one push yields (jamd_frontend_live_push_frames())
against the rows the compiled reference stores, counted off its own cyclic buffers driven by tests/frontendliveref.py
(no WMP_calc(): the counts depend on the number of windows alone).  Before the end of a segment that is what
RealTimeMFCC() has stored after each window; at the end it is what the flush loop adds."""
import ctypes as C

import numpy as np
import pytest

import frontendliveref as L
from frontendref import RefFrontend
from julius_amd import lib

FS, SH = 400, 160
KINDS = (("MFCC", 12), ("MFCC_D", 24), ("MFCC_E_D_A_Z", 39))
WINS = [(2, 2), (1, 3), (4, 1)]


def nsamp(frames):
    return FS + 1 + (frames - 1) * SH if frames > 0 else 0


class Counting(L.RefLiveChannel):
    """cum[k]: rows stored once the main loop has seen k windows (RealTimeMFCC() returned TRUE that often)."""

    def segment(self, wave, calc=True):
        self.cum = [0]
        return super().segment(wave, calc)

    def _realtime_mfcc(self, window, calc):
        ok = super()._realtime_mfcc(window, calc)
        self.cum.append(self.cum[-1] + (1 if ok else 0))
        return ok


def setup(ref, kind, vecsize, delwin, accwin, splice):
    v = RefFrontend(ref).para(lib.param_kind(kind), vecsize, delWin=delwin, accWin=accwin, framesize=FS, frameshift=SH)
    d = lib.Frontend.desc_for(kind, vecsize, delWin=delwin, accWin=accwin, framesize=FS, frameshift=SH, splice=splice)
    vv = type(v).from_buffer_copy(v)
    vv.cmn = vv.cvn = vv.enormal = 0              # (the counts do not depend on the normalisations)
    L_ = (delwin if v.delta else 0) + (accwin if v.acc else 0)
    return vv, d, L_


def ref_counts(ref, vv, splice, Tb):
    """(rows after each window of the main loop, rows of the whole segment) for a segment of Tb base frames."""
    ch = Counting(ref, vv, splice=splice)
    total = len(ch.segment(np.zeros(nsamp(Tb), np.int16), calc=False))
    cum = ch.cum
    ch.close()
    assert len(cum) == Tb + 1
    return cum, total


@pytest.mark.parametrize("delwin,accwin", WINS)
@pytest.mark.parametrize("kind,vecsize", KINDS)
@pytest.mark.parametrize("splice", [1, 3])
def test_push_frames_is_the_reference_loops(ref, kind, vecsize, delwin, accwin, splice):
    vv, d, L_ = setup(ref, kind, vecsize, delwin, accwin, splice)
    pf = lib.load().jamd_frontend_live_push_frames
    fr = lib.load().jamd_frontend_live_frames
    dp = C.byref(d)
    # totals of 1 .. 2 L + 4 and 40 base frames: what the end of the segment delivers in all
    for Tb in list(range(1, 2 * L_ + 5)) + [40]:
        cum, total = ref_counts(ref, vv, splice, Tb)
        assert pf(dp, 0, nsamp(Tb), 1) == total == fr(dp, nsamp(Tb)), (Tb, total)
        # the segment fed one frame's worth per push: each push as the main loop stored, the last with the flush
        before, rows = 0, []
        for k in range(1, Tb + 1):
            n = nsamp(k)
            rows.append(pf(dp, before, n - before, 1 if k == Tb else 0))
            before = n
        want = [cum[k] - cum[k - 1] for k in range(1, Tb)] + [total - cum[Tb - 1]]
        assert rows == want, (Tb, rows, want)
        assert pf(dp, nsamp(Tb), 0, 1) == total - cum[Tb]          # an end without samples: the flush loop alone
    # every prefix of 40 frames, at the sample: cumulative rows = max(0, max(0, Tb - L) - (splice - 1))
    cum, total = ref_counts(ref, vv, splice, 40)
    for n in range(nsamp(40) + 1):
        Tb = 0 if n < FS + 1 else (n - FS - 1) // SH + 1
        got = pf(dp, 0, n, 0)
        assert got == cum[Tb] == max(0, max(0, Tb - L_) - (splice - 1)), (n, Tb, got, cum[Tb])
    assert cum[40] == 40 - L_ - (splice - 1) and total == 40 - (splice - 1)


@pytest.mark.parametrize("delwin,accwin", WINS)
@pytest.mark.parametrize("splice", [1, 3])
def test_pushes_of_a_plan_sum_to_the_segment(ref, delwin, accwin, splice):
    """Seeded cuts at any sample, empty pushes among them: each push is a difference of the cumulative count, and the
    sum is jamd_frontend_live_frames() of the whole."""
    vv, d, L_ = setup(ref, "MFCC_E_D_A_Z", 39, delwin, accwin, splice)
    pf = lib.load().jamd_frontend_live_push_frames
    dp = C.byref(d)
    rng = np.random.default_rng(delwin * 10 + accwin + splice)
    for total_n in [0, 1, FS, FS + 1, nsamp(L_), nsamp(L_ + 1) + 7, nsamp(2 * L_ + 3) - 1, nsamp(40) + 100]:
        whole = lib.load().jamd_frontend_live_frames(dp, total_n)
        assert whole == L.live_frames(ref, vv, splice, total_n)
        for _ in range(6):
            cuts = sorted(rng.integers(0, total_n + 1, rng.integers(0, 7)).tolist()) + [total_n]
            before, got = 0, []
            for i, c in enumerate(cuts):
                got.append(pf(dp, before, c - before, 1 if i == len(cuts) - 1 else 0))
                assert got[-1] >= 0
                if i < len(cuts) - 1:
                    assert got[-1] == pf(dp, 0, c, 0) - pf(dp, 0, before, 0)
                before = c
            assert sum(got) == whole, (total_n, cuts, got, whole)


def test_push_frames_refuses():
    pf = lib.load().jamd_frontend_live_push_frames
    d = lib.Frontend.desc_for("MFCC_E_D_A_Z", 39, framesize=FS, frameshift=SH)
    assert pf(None, 0, 10, 0) == -1
    assert pf(C.byref(d), -1, 10, 0) == -1 and pf(C.byref(d), 0, -1, 0) == -1
