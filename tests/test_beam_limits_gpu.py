"""First-pass kernel selection at its beam limits, against the compiled reference.

Which kernel runs a work area depends on the beam width: the exact-order kernel's narrow LDS image (survivors in LDS), its
wide image (survivors in the utterance's slice), its closed-form extraction and its half workgroup shape each end at a
beam, beyond the last of them the work area falls back to the canonical-tie kernel, whose own LDS image (cell table,
survivors in LDS or in HBM, score-row cache) changes at further beams.  The other GPU tests pin each kernel at beams chosen
inside a regime; here every threshold is found on the live work area (bisection over jamd_beam_exact_layout() /
jamd_beam_set_workgroup_shape() / jamd_beam_prune_stats(), or the arithmetic of jamd_beam_create() for the canonical-tie
kernel) and the whole first pass runs on BOTH sides of it, over the BASELINE-size lexicon (20 000 words, tree built by the
reference) and the three score streams of test_wide_beam_gpu.py, with rank pruning live in every case."""
import numpy as np
import pytest

from beamutil import assert_trellis_equal, assert_trellis_equal_modulo_ties
from julius_amd import lexblob, lib, synth
from oracle import pyoracle

pytestmark = pytest.mark.gpu

S = 3000
T_CHEAP = 50          # frames per stream where the closed-form extraction runs
T_LOOP = 40           # frames per stream where the extraction loop runs (a beam's worth of pops per frame on one wave)
T_STRICT = 16         # frames per stream in strict order at the widest beams (one lane per utterance)


def _last_true(pred, lo, hi):
    """Largest b in [lo, hi) with pred(b), for a pred that is true at lo, false at hi and changes once."""
    assert pred(lo) and not pred(hi), (lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def fast_lds_image(beam, nstate, tok_bytes=32):
    """The canonical-tie kernel's LDS image for a beam, restating fbeam_layout() and the score-row test of
    fbeam_launch() (csrc/beam.hip): (survivors in LDS, cell-table slots, score row cached)."""
    max_dyn, hist = 159 * 1024, 2048 * 4            # kMaxDynLds, kHistBytes (csrc/beam_common.h)
    hsize = 64
    while hsize < 2 * beam:
        hsize <<= 1
    sv = (beam * (tok_bytes + 8) + hsize * 8 + 15) & ~15
    use_lds = sv + hist <= max_dyn
    slots = 0
    if use_lds:
        s = 4096
        while sv + s * 24 <= max_dyn and s < 65536:
            s *= 2
        slots = s if sv + s * 12 <= max_dyn and s >= 8 * beam else 0
    cell_off = sv if use_lds else 0
    lds = cell_off + max(8 * slots, hist) + 4 * slots
    return use_lds, slots, lds + 4 * nstate <= max_dyn


def fast_limits(nstate=S):
    """(last beam with the LDS cell table, last beam with the survivors in LDS) of the canonical-tie kernel."""
    cells = _last_true(lambda b: fast_lds_image(b, nstate)[1] > 0, 1, 65536)
    surv = _last_true(lambda b: fast_lds_image(b, nstate)[0], 1, 65536)
    return cells, surv


def _streams(task, am, oracle, T):
    rng = np.random.default_rng(4242)
    fr = synth.make_utterance(task, nwords=3, seed=9042)[0]
    flat = rng.normal(-8.0, 0.33, (90, S)).astype(np.float32)
    st = {"gmm": oracle.gmm_outprob(am, fr), "flat": flat, "ties": (np.round(flat * 4.0) / 4.0).astype(np.float32)}
    return {k: v[:T] for k, v in st.items()}


class _Task:
    """One reference-built lexicon on the device, its streams, and the compiled reference at any beam (cached)."""

    def __init__(self, engine, oracle, ref, wd, task, args):
        self.engine, self.ref, self.wd, self.task, self.args = engine, ref, wd, task, args
        eng = pyoracle.RefEngine(ref, args + ["-b", "800"])
        eng.save_lexicon(wd / "lex.blob")
        self.lex = lexblob.load(wd / "lex.blob")
        self.am = ref.am_load(task["hmmdefs"], task["hmmlist"]).export()
        self.lx = lib.Lexicon(engine, self.lex)
        self.streams = _streams(task, self.am, oracle, max(T_CHEAP, T_LOOP))
        self._eng, self._want = {}, {}

    def want(self, beam, kind, T):
        """The compiled reference's (trellis, (wseq, score)) for the first T frames of a stream at this beam."""
        key = (beam, kind, T)
        if key not in self._want:
            if beam not in self._eng:
                self._eng[beam] = pyoracle.RefEngine(self.ref, self.args + ["-b", str(beam)])
                assert self._eng[beam].beam_width == beam
            synth.write_htk_param(self.wd / "u.prob", self.streams[kind][:T], parmkind=synth.PARM_USER)
            self._want[key] = self._eng[beam].recognize(self.wd / "u.prob")
        return self._want[key]

    def beam(self, beam, nutt=3):
        return lib.Beam(self.engine, self.lx, beam, -1.0, max_utts=nutt, atoms_per_utt=1 << 18)

    def run(self, bm, T, kinds=("gmm", "flat", "ties")):
        res, tre = bm.pass1_host([self.streams[k][:T] for k in kinds])
        return list(zip(kinds, res, tre))


def _task_args(task):
    return ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-nlr", task["arpa"], "-input", "outprob", "-1pass"]


@pytest.fixture(scope="module")
def big(engine, oracle, ref, tmp_path_factory):
    wd = tmp_path_factory.mktemp("limits")
    task = synth.make_triphone_task(wd, nphone=40, S=S, M=1, nword=20000, nvar=25, seed=0, maxlen=8, nbigram_per_word=10)
    t = _Task(engine, oracle, ref, wd, task, _task_args(task))
    assert t.lex["nnode"] > 200000
    return t


@pytest.fixture(scope="module")
def mid(engine, oracle, ref, tmp_path_factory):
    """A mid-size lexicon (nnode far above the canonical-tie kernel's LDS thresholds) with the big task's S."""
    wd = tmp_path_factory.mktemp("limits_mid")
    task = synth.make_triphone_task(wd, nphone=40, S=S, M=1, nword=4000, nvar=25, seed=1, maxlen=8, nbigram_per_word=10)
    t = _Task(engine, oracle, ref, wd, task, _task_args(task))
    assert t.lex["nnode"] > 20000
    return t


def _layout(t, beam):
    bm = lib.Beam(t.engine, t.lx, beam, -1.0, max_utts=1)
    try:
        return bm.exact_layout()
    finally:
        bm.close()


def _half_ok(t, beam):
    bm = lib.Beam(t.engine, t.lx, beam, -1.0, max_utts=1)
    try:
        bm.set_workgroup_shape("half")
        return True
    except lib.JamdError:
        return False
    finally:
        bm.close()


def _closed_form_frames(t, beam, T=10):
    """Pruned frames of a short flat stream whose extraction the exact-order kernel resolved in closed form."""
    bm = t.beam(beam, nutt=1)
    try:
        bm.pass1_host([t.streams["flat"][:T]])
        st = bm.prune_stats(0)
        assert st[0] > 0
        return st[0] - st[6]
    finally:
        bm.close()


@pytest.fixture(scope="module")
def limits(big):
    """The exact-order kernel's thresholds on the 20 000-word lexicon, found on live work areas."""
    lim = {}
    assert _layout(big, 1) == "narrow" and _layout(big, 65536) == "none"
    lim["narrow"] = _last_true(lambda b: _layout(big, b) == "narrow", 1, 65536)
    lim["max"] = _last_true(lambda b: _layout(big, b) != "none", lim["narrow"], 65536)
    lim["half"] = _last_true(lambda b: _half_ok(big, b), 1, lim["max"] + 1)
    # the closed-form extraction needs room for the top lists (b_cap > 0, beam_exact_layout.hip xbeam_place_with()): past it every
    # pruned frame goes to the extraction loop
    lim["closed"] = _last_true(lambda b: _closed_form_frames(big, b) > 0, lim["narrow"] + 1, lim["max"])
    print(f"\nexact-order limits on the {big.lex['nword']}-word lexicon ({big.lex['nnode']} nodes): "
          f"narrow <= {lim['narrow']}, half <= {lim['half']}, closed form <= {lim['closed']}, exact <= {lim['max']}")
    return lim


def test_thresholds_are_ordered(limits):
    """Sanity: the regimes the header describes, in their order, and each side of each threshold really different."""
    assert 1 <= limits["half"] <= limits["max"]
    assert 500 <= limits["narrow"] < limits["closed"] < limits["max"]
    assert limits["max"] >= 8000          # the reference recipe's DNN beam (4 000) with room to spare


def test_fast_lds_image_helper():
    """The restatement of jamd_beam_create()'s arithmetic: a change in the Tok record or the LDS budget must show up
    here rather than silently move the beams test_fast_kernel_lds_edges runs."""
    cells, surv = fast_limits()
    assert cells == 1024 and 2000 <= surv <= 4096, (cells, surv)
    # the score row of S = 3000 states is cached on one side and not on the other of both thresholds
    rows = [fast_lds_image(b, S)[2] for b in (cells, cells + 1, surv, surv + 1)]
    assert rows == [False, True, False, True], rows


def _check_exact(t, bm, beam, T):
    for kind, r, atoms in t.run(bm, T):
        rtr, (rwseq, rscore) = t.want(beam, kind, T)
        assert r.status in (0, 1), (beam, kind, r.status)
        assert r.max_tokens > beam, (beam, kind)                 # rank pruning is live
        assert_trellis_equal(atoms, rtr)
        if r.status == 0:
            assert np.array_equal(np.array(r.wseq[:r.wnum]), rwseq) and r.score == rscore, (beam, kind)


def _check_fast(t, bm, beam, T):
    for kind, r, atoms in t.run(bm, T):
        rtr, (rwseq, rscore) = t.want(beam, kind, T)
        assert r.status in (0, 1), (beam, kind, r.status)
        assert r.max_tokens > beam, (beam, kind)
        assert_trellis_equal_modulo_ties(atoms, rtr, r.ties)
        if r.ties == 0 and r.status == 0:
            assert np.array_equal(np.array(r.wseq[:r.wnum]), rwseq) and r.score == rscore, (beam, kind)


@pytest.mark.parametrize("side", [0, 1])
def test_narrow_layout_edge(big, limits, side):
    """Last narrow beam and the first wide one: exact and exact_serial both give the reference's trellis."""
    beam = limits["narrow"] + side
    bm = big.beam(beam)
    assert bm.exact_layout() == ("narrow", "wide")[side]
    for mode in ("exact", "exact_serial"):
        bm.set_order_mode(mode)
        assert bm.order_mode() == mode
        _check_exact(big, bm, beam, T_CHEAP)
    bm.close()


@pytest.mark.parametrize("side", [0, 1])
def test_closed_form_extraction_edge(big, limits, side):
    """Last beam of the closed-form extraction and the first without it: both the reference's trellis, and the pruning
    steps of the two resolved by different paths (jamd_beam_prune_stats: [1]-[3], [5] closed form, [6] extraction loop)."""
    beam = limits["closed"] + side
    bm = big.beam(beam)
    assert bm.exact_layout() == "wide" and bm.order_mode() == "exact"
    _check_exact(big, bm, beam, T_LOOP)
    for u in range(3):
        st = bm.prune_stats(u)
        closed = st[1] + st[2] + st[3] + st[5]
        assert st[0] > 0
        if side == 0:
            assert closed > 0, st
        else:
            assert closed == 0 and st[6] == st[0], st
    bm.close()


def test_half_shape_edge(big, limits):
    """The widest beam the half workgroup shape takes: half and full shape both give the reference's trellis; one more
    is refused for the half shape (and still runs in the full one)."""
    beam = limits["half"]
    bm = big.beam(beam)
    for shape in ("half", "full"):
        bm.set_workgroup_shape(shape)
        assert bm.workgroup_shape(3) == shape
        _check_exact(big, bm, beam, T_CHEAP)
    bm.close()
    bm = big.beam(beam + 1, nutt=1)
    with pytest.raises(lib.JamdError, match="half shape"):
        bm.set_workgroup_shape("half")
    assert bm.workgroup_shape(1) == "full" and bm.order_mode() == "exact"
    bm.close()


def test_widest_exact_beam(big, limits):
    beam = limits["max"]
    bm = big.beam(beam)
    assert bm.exact_layout() == "wide" and bm.order_mode() == "exact"
    _check_exact(big, bm, beam, T_LOOP)
    bm.close()


def test_one_past_the_widest_exact_beam(big, limits):
    """Past the exact-order kernel the work area falls back to the canonical-tie kernel; strict order still gives the
    reference, and the exact order is refused by name."""
    beam = limits["max"] + 1
    bm = big.beam(beam)
    assert bm.order_mode() == "fast" and bm.exact_layout() == "none"
    _check_fast(big, bm, beam, T_LOOP)
    with pytest.raises(lib.JamdError, match="beam too wide"):
        bm.set_order_mode("exact")
    assert bm.order_mode() == "fast"
    bm.set_order_mode("strict")
    assert bm.order_mode() == "strict"
    _check_exact(big, bm, beam, T_STRICT)
    bm.close()


@pytest.mark.parametrize("edge,side", [("cells", 0), ("cells", 1), ("surv", 0), ("surv", 1)])
def test_fast_kernel_lds_edges(mid, edge, side):
    """The canonical-tie kernel on both sides of its LDS cell table and of its LDS survivor image (the second
    instantiation, survivors in HBM, beyond); the score row is cached on one side of each (test_fast_lds_image_helper)."""
    cells, surv = fast_limits()
    beam = (cells if edge == "cells" else surv) + side
    bm = mid.beam(beam).set_order_mode("fast")
    assert bm.order_mode() == "fast"
    _check_fast(mid, bm, beam, T_CHEAP)
    bm.close()
