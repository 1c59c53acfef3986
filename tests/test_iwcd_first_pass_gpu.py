"""GPU: the state-set reductions INSIDE the first pass -- every method, lane split and set size (tests/iwcdref.py).

The stand-alone set kernel has its own edge tests (test_gmm_gpu.py); the first pass does not call it.  The exact-order
kernel's step C gives a set 4, 2 or 1 lanes per frame, the canonical-tie kernel's drain always 4, the multipath frame
and strict order reduce on one lane.  Here the whole trellis, the sentence and the score are compared
  A  with the compiled reference, on the lexicon it built, for 8 methods x 4 beams x 2 workgroup shapes x 4 streams;
  B  with the CPU oracle on the same lexicon with its sets resized to both sides of every round of the member loops;
  C  in strict order, on the canonical-tie kernel and on the multipath frame;
and in A and B jamd_beam_prune_stats()[13..15] must equal what the oracle's tap counted for that utterance, so that a
case cannot pass on another lane split than the one it was chosen for.  D: an N outside [1, 16] is refused."""
import numpy as np
import pytest

import iwcdref
from beamutil import assert_trellis_equal, assert_trellis_equal_modulo_ties, ref_task
from iwcdref import BEAMS, METHODS, NT, WIDE_BEAM_B
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu

SHAPES = ("full", "half")
T_STRICT = 12
# case B: the wide beam is there for the one-lane class of the FULL shape (the half shape has it from beam 900 on)
CASES_B = [(b, s) for b in BEAMS for s in SHAPES] + [(WIDE_BEAM_B, "full")]


@pytest.fixture(scope="module")
def tk(ref, oracle, tmp_path_factory):
    return iwcdref.Task(ref, oracle, tmp_path_factory.mktemp("iwcd"))


@pytest.fixture(scope="module")
def lexicons(engine, tk):
    """Device lexicons, one per (case, method), made on first use."""
    made = {}

    def get(case, method):
        if (case, method) not in made:
            made[case, method] = lib.Lexicon(engine, tk.lex(method) if case == "A" else tk.lex_resized(method))
        return made[case, method]
    return get


def _beam(engine, lx, beam, nutt):
    return lib.Beam(engine, lx, beam, -1.0, max_utts=nutt, atoms_per_utt=1 << 17)


def _half_ok(engine, lx, beam):
    bm = _beam(engine, lx, beam, 1)
    try:
        bm.set_workgroup_shape("half")
        return True
    except lib.JamdError:
        return False
    finally:
        bm.close()


@pytest.fixture(scope="module")
def half_limit(engine, lexicons):
    """The widest beam the half shape takes on this lexicon.  Half a CU's LDS must hold a typical frame (xbeam_layout():
    heap >= 5 beams, cells >= 3 beams), which ends between beams 900 and 2 000: jamd_beam_set_workgroup_shape() refuses
    the half shape beyond.  The half-shape cases of beam 2 000 assert that refusal and run at this beam instead, the
    widest the shape has; its one-lane frames are there from beam 900 on."""
    lx = lexicons("A", "max")
    lo, hi = 900, 2000
    assert _half_ok(engine, lx, lo) and not _half_ok(engine, lx, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _half_ok(engine, lx, mid) else (lo, mid)
    print(f"\nhalf shape: beams <= {lo}")
    return lo


def _shape_beam(engine, lx, beam, shape, half_limit):
    """The beam a case runs at: its own, or the half shape's widest where the half shape refuses it (asserted here)."""
    if shape != "half" or beam <= half_limit:
        return beam
    bm = _beam(engine, lx, beam, 1)
    try:
        with pytest.raises(lib.JamdError, match="does not fit the half shape"):
            bm.set_workgroup_shape("half")
        assert bm.workgroup_shape(1) == "full" and bm.order_mode() == "exact"
    finally:
        bm.close()
    return half_limit


def _check_result(r, atoms, want_trellis, want_rc, want_wseq, want_score, what):
    assert r.status in (0, 1) and r.status == want_rc, (what, r.status, want_rc)
    assert_trellis_equal(atoms, want_trellis)
    if r.status == 0:
        assert np.array_equal(np.array(r.wseq[:r.wnum]), want_wseq) and r.score == want_score, what


def _check_counters(bm, u, calls, shape, what):
    st = bm.prune_stats(u, reset=True)
    calls = iwcdref.device_frames(calls)
    two, one = iwcdref.lane_classes(calls, NT[shape])
    print(f"{what}: frames {st[11]}, two-lane {st[13]} (oracle {two}), one-lane {st[14]} (oracle {one}), "
          f"reductions {st[15]} (oracle {int(calls.sum())})")
    assert st[11] == len(calls), (what, st)
    assert st[15] == int(calls.sum()), (what, st[15], int(calls.sum()))
    assert (st[13], st[14]) == (two, one), (what, st[13], st[14], two, one)


def _run_exact(engine, tk, lexicons, half_limit, case, method, beam, shape):
    kinds = list(tk.streams if case == "A" else tk.streams_b)
    streams = tk.streams if case == "A" else tk.streams_b
    beam = _shape_beam(engine, lexicons(case, method), beam, shape, half_limit)
    bm = _beam(engine, lexicons(case, method), beam, len(kinds))
    try:
        assert bm.order_mode() == "exact"
        bm.set_workgroup_shape(shape)
        assert bm.workgroup_shape(len(kinds)) == shape
        for u in range(len(kinds)):
            bm.prune_stats(u, reset=True)
        res, tre = bm.pass1_host([streams[k] for k in kinds])
        for u, (kind, r, atoms) in enumerate(zip(kinds, res, tre)):
            what = (case, method, beam, shape, kind)
            otr, owseq, oscore, orc, calls, big = tk.oracle_run(case, method, beam, kind)
            if case == "A":
                rtr, (rwseq, rscore) = tk.want(method, beam, kind)
                _check_result(r, atoms, rtr, orc, rwseq, rscore, what)
            else:
                _check_result(r, atoms, otr, orc, owseq, oscore, what)
            _check_counters(bm, u, calls, shape, what)
    finally:
        bm.close()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("beam", BEAMS)
@pytest.mark.parametrize("method", list(METHODS))
def test_a_exact_order_vs_reference(engine, tk, lexicons, half_limit, method, beam, shape):
    _run_exact(engine, tk, lexicons, half_limit, "A", method, beam, shape)


@pytest.mark.parametrize("beam,shape", CASES_B)
@pytest.mark.parametrize("method", list(METHODS))
def test_b_resized_sets_vs_oracle(engine, tk, lexicons, half_limit, method, beam, shape):
    _run_exact(engine, tk, lexicons, half_limit, "B", method, beam, shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("method", list(METHODS))
def test_every_lane_class_is_met(tk, half_limit, method, shape):
    """The cap on the cases above: over the beams they run at, each method meets the four-, two- and one-lane split in
    each shape (the cases hold the device's counters to these counts one by one)."""
    for case, streams, beams in (("A", tk.streams, BEAMS), ("B", tk.streams_b, [b for b, s in CASES_B if s == shape])):
        four = two = one = 0
        for beam in beams:
            beam = min(beam, half_limit) if shape == "half" else beam
            for kind in streams:
                calls = iwcdref.device_frames(tk.oracle_run(case, method, beam, kind)[4])
                c2, c1 = iwcdref.lane_classes(calls, NT[shape])
                four, two, one = four + len(calls) - c2 - c1, two + c2, one + c1
        assert four > 0 and two > 0 and one > 0, (case, method, shape, four, two, one)


@pytest.mark.parametrize("beam", [40, 400])
@pytest.mark.parametrize("method", list(METHODS))
def test_c_strict_order(engine, tk, lexicons, method, beam):
    """One lane per utterance, cd_reduce() per token: 12 frames of A's streams against the reference and of B's against
    the oracle."""
    for case, streams in (("A", tk.streams), ("B", tk.streams_b)):
        kinds = list(streams)
        bm = _beam(engine, lexicons(case, method), beam, len(kinds)).set_order_mode("strict")
        try:
            assert bm.order_mode() == "strict"
            res, tre = bm.pass1_host([streams[k][:T_STRICT] for k in kinds])
            for kind, r, atoms in zip(kinds, res, tre):
                otr, owseq, oscore, orc, _, _ = tk.oracle_run(case, method, beam, kind, T_STRICT)
                if case == "A":
                    rtr, (rwseq, rscore) = tk.want(method, beam, kind, T_STRICT)
                    _check_result(r, atoms, rtr, orc, rwseq, rscore, (case, method, beam, kind))
                else:
                    _check_result(r, atoms, otr, orc, owseq, oscore, (case, method, beam, kind))
        finally:
            bm.close()


@pytest.mark.parametrize("beam", [40, 400, 2000])
@pytest.mark.parametrize("method", list(METHODS))
def test_c_canonical_tie_kernel(engine, tk, lexicons, method, beam):
    """The drain: four lanes per set, four members per lane and round (a round = 16 members), its own 4-slot list for
    best <= 4.  Exact where the kernel met no tie, else equal up to the tied atoms."""
    for case, streams in (("A", tk.streams), ("B", tk.streams_b)):
        kinds = list(streams)
        bm = _beam(engine, lexicons(case, method), beam, len(kinds)).set_order_mode("fast")
        try:
            assert bm.order_mode() == "fast"
            res, tre = bm.pass1_host([streams[k] for k in kinds])
            for kind, r, atoms in zip(kinds, res, tre):
                what = (case, method, beam, kind)
                otr, owseq, oscore, orc, _, _ = tk.oracle_run(case, method, beam, kind)
                if case == "A":
                    otr, (owseq, oscore) = tk.want(method, beam, kind)
                assert r.status in (0, 1), what
                assert_trellis_equal_modulo_ties(atoms, otr, r.ties)
                if r.ties == 0:
                    assert r.status == orc, what
                    if r.status == 0:
                        assert np.array_equal(np.array(r.wseq[:r.wnum]), owseq) and r.score == oscore, what
        finally:
            bm.close()


@pytest.mark.parametrize("beam", [40, 900])
@pytest.mark.parametrize("method", ["avg", "best2", "best5", "best16"])
def test_c_multipath_frame(engine, oracle, ref, tmp_path, method, beam):
    """The multipath frame (step O): cd_reduce() on one lane per token, both shapes, against the compiled reference;
    it has no lane split and leaves the three counters at 0."""
    kw = {k: v for k, v in iwcdref.TASK_KW.items() if k != "seed"}
    eng, lex, am, task = ref_task(ref, tmp_path, iwcdref.TASK_KW["seed"], beam, ["-multipath", "-iwcd1"] + METHODS[method], **kw)
    assert eng.multipath == 1 and lex["lm_type"] == 0x100 and eng.beam_width == beam
    utts = [synth.make_utterance(task, nwords=2 + u, seed=9042 + u)[0][:iwcdref.T] for u in range(2)]
    scores = [oracle.gmm_outprob(am, fr) for fr in utts]
    want = []
    for fr in utts:
        synth.write_htk_param(tmp_path / "u.mfc", fr)
        want.append(eng.recognize(tmp_path / "u.mfc"))
    bm = _beam(engine, lib.Lexicon(engine, lex), beam, len(utts))
    try:
        assert bm.order_mode() == "exact"
        for shape in SHAPES:
            bm.set_workgroup_shape(shape)
            assert bm.workgroup_shape(len(utts)) == shape
            res, tre = bm.pass1_host(scores)
            for u, (r, atoms, (rtr, (rwseq, rscore))) in enumerate(zip(res, tre, want)):
                assert r.status in (0, 1), (method, beam, shape, u)
                assert_trellis_equal(atoms, rtr)
                if r.status == 0:
                    assert np.array_equal(np.array(r.wseq[:r.wnum]), rwseq) and r.score == rscore, (method, beam, shape, u)
                st = bm.prune_stats(u, reset=True)
                assert st[11] > 0 and st[13:16] == [0, 0, 0], st
    finally:
        bm.close()


@pytest.mark.parametrize("n", [0, 17])
def test_d_nbest_outside_range_is_refused(engine, tk, n):
    lex = dict(tk.lex("best4"))
    assert lex["cdset_method"] == 2
    lex["cdmax_num"] = n
    with pytest.raises(lib.JamdError, match=rf"cdmax_num={n} outside \[1,16\]"):
        lib.Lexicon(engine, lex)
