"""CPU: the inputs of test_iwcd_first_pass_gpu.py reach what they were chosen for (tests/iwcdref.py).

The GPU tests compare the first pass with the compiled reference (case A) and, on the lexicon with resized sets that
the reference cannot load, with the CPU oracle (case B).  Here, without a device: the oracle equals the reference for
every method on a stream with dead members, the streams hold no all-dead set, and the oracle's tap (per-frame count of
state-set reductions) shows that the chosen beams put frames into each lane split of the exact-order kernel in each
workgroup shape, with sets of more than 32 members (a second round at four lanes) reduced in each of them."""
import numpy as np
import pytest

import iwcdref
from beamutil import TR_KEYS
from iwcdref import BEAMS, METHODS, NT, WIDE_BEAM_B


@pytest.fixture(scope="module")
def tk(ref, oracle, tmp_path_factory):
    return iwcdref.Task(ref, oracle, tmp_path_factory.mktemp("iwcd"))


def test_task_is_the_one_described(tk):
    lex = tk.lex("max")
    assert lex["nnode"] == 8001 and lex["nset"] == 969
    size, count = np.unique(np.diff(lex["set_off"]), return_counts=True)
    groups = {"1": count[size == 1].sum(), "7-14": count[(size >= 7) & (size <= 14)].sum(), "42-53": count[(size >= 42) & (size <= 53)].sum()}
    assert groups == {"1": 6, "7-14": 927, "42-53": 36}
    sizes_b = np.diff(tk.lex_b["set_off"])
    assert np.array_equal(sizes_b, np.array(iwcdref.SIZES)[np.arange(lex["nset"]) % len(iwcdref.SIZES)])
    for i in range(lex["nset"]):                       # the original members first
        a = lex["set_states"][lex["set_off"][i]:lex["set_off"][i + 1]]
        b = tk.lex_b["set_states"][tk.lex_b["set_off"][i]:tk.lex_b["set_off"][i + 1]]
        n = min(len(a), len(b))
        assert np.array_equal(a[:n], b[:n]) and len(set(b.tolist())) == len(b) and b.max() < iwcdref.S


def test_streams_hold_no_dead_set(tk):
    """The helper's condition, and that the holes are there: both kinds of dead score, and at 0.9 sets on both sides
    of every N: fewer live members than N (the reference then averages what there is) and at least N."""
    for lex, streams in ((tk.lex("max"), tk.streams), (tk.lex_b, tk.streams_b)):
        for kind, sc in streams.items():
            assert sc.shape == (iwcdref.T, iwcdref.S) and sc.dtype == np.float32
            iwcdref.assert_no_dead_set(lex, sc)
            if kind.startswith("holes"):
                assert (sc == iwcdref.LOG_ZERO).any() and (sc == iwcdref.BELOW_LOG_ZERO).any()
            else:
                assert (sc > iwcdref.LOG_ZERO).all()
    lex = tk.lex("max")
    live = np.add.reduceat((tk.streams["holes90"][:, lex["set_states"]] > iwcdref.LOG_ZERO).astype(np.int32), lex["set_off"][:-1], axis=1)
    assert live.min() >= 1
    for n in (2, 3, 4, 5):
        assert (live < n).mean() > 0.01 and (live >= n).mean() > 0.01, n
    assert (live < 16).mean() > 0.9


@pytest.mark.parametrize("method", list(METHODS))
def test_oracle_equals_reference(tk, method):
    """Bit for bit on holes(0.5) at beam 400: members at and below LOG_ZERO, sets with fewer live members than N."""
    rtr, (rwseq, rscore) = tk.want(method, 400, "holes50")
    otr, owseq, oscore, rc, calls, big = tk.oracle_run("A", method, 400, "holes50")
    assert len(otr["wid"]) == len(rtr["wid"]) > 0
    for k in TR_KEYS:
        assert np.array_equal(otr[k], rtr[k]), k
    assert np.isfinite(otr["backscore"]).all()
    if rc == 0:
        assert np.array_equal(owseq, rwseq) and oscore == rscore
    assert calls.sum() > 0 and calls[0] == 1           # frame 0: the initial token stands on a set node


def _classes(tk, case, method, shape, beams, kinds):
    """Frames per lane split (four, two, one lanes) over the beams and streams, and those of them that reduce a set of
    more than 32 members."""
    n, nbig = np.zeros(3, int), np.zeros(3, int)
    for beam in beams:
        for kind in kinds:
            calls, big = (iwcdref.device_frames(x) for x in tk.oracle_run(case, method, beam, kind)[4:6])
            cls = np.where(calls > NT[shape] // 2, 2, np.where(calls > NT[shape] // 4, 1, 0))
            two, one = iwcdref.lane_classes(calls, NT[shape])
            assert ((cls == 1).sum(), (cls == 2).sum()) == (two, one)
            for c in range(3):
                n[c] += (cls == c).sum()
                nbig[c] += ((cls == c) & (big > 0)).sum()
    return n, nbig


@pytest.mark.parametrize("shape", ["full", "half"])
@pytest.mark.parametrize("method", list(METHODS))
def test_every_lane_class_is_reached(tk, method, shape):
    """At least 5 frames in each of the three lane classes per workgroup shape over the beam list, on each case; with
    resized sets every class also reduces sets of more than 32 members."""
    # (the half shape ends between beams 900 and 2 000 -- half a CU's LDS must hold a typical frame --, so its classes
    # are counted over the beams below; the GPU test finds the limit on the device and runs there as well)
    beams = BEAMS if shape == "full" else tuple(b for b in BEAMS if b <= 900)
    n, _ = _classes(tk, "A", method, shape, beams, tk.streams)
    assert (n >= 5).all(), (method, shape, n)
    beams_b = beams + ((WIDE_BEAM_B,) if shape == "full" else ())
    n, nbig = _classes(tk, "B", method, shape, beams_b, tk.streams_b)
    assert (n >= 5).all() and (nbig >= 5).all(), (method, shape, n, nbig)
    # the wide beam is what gives the full shape its one-lane frames on the flat stream
    if shape == "full":
        assert iwcdref.lane_classes(iwcdref.device_frames(tk.oracle_run("B", method, WIDE_BEAM_B, "flat")[4]), NT["full"])[1] >= 5


def test_tap_counts_every_reduction(tk, oracle):
    """The tap is off unless asked for, leaves the result alone, counts the same twice, and reproduces the per-frame
    counts the beams were chosen from."""
    lex, sc = tk.lex("best4"), tk.streams["flat"]
    out = oracle.beam_pass1(lex, sc, 400)
    assert len(out) == 5
    a = oracle.beam_pass1(lex, sc, 400, counts=True)
    b = oracle.beam_pass1(lex, sc, 400, counts=True)
    assert len(a) == 7 and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6])
    assert np.array_equal(a[0], out[0]) and a[5].shape == (iwcdref.T,) and (a[6] <= a[5]).all()
    assert a[6].sum() == 0                                  # the reference-built sets of 42..53 members are never reduced
    assert (tk.oracle_run("B", "best4", 400, "flat")[5] > 0).all()
    # the lane-split table of the issue on this stream: frames with <= 128 / 129..256 / 257..512 / > 512 reductions
    table = {40: (30, 0, 0, 0), 400: (4, 26, 0, 0), 900: (4, 2, 24, 0), 2000: (4, 2, 15, 9)}
    for beam, want in table.items():
        c = tk.oracle_run("A", "best4", beam, "flat")[4]
        got = ((c <= 128).sum(), ((c > 128) & (c <= 256)).sum(), ((c > 256) & (c <= 512)).sum(), (c > 512).sum())
        assert got == want, (beam, got)
