"""The order-mode state machine of a first-pass work area (jamd_beam_set_strict_order / _set_order_mode /
_set_workgroup_shape / _stream_*), over every kind of lexicon, at a beam the exact-order kernel serves and one past it.

Invariants, checked after every call of a table of call sequences:
  - a call either succeeds or raises JamdError and leaves order_mode() as it was;
  - order_mode() names the kernel that then runs: the next pass gives the compiled reference's trellis (exactly in the exact
    and strict modes, by the ties rule in the canonical-tie one) or is refused;
  - a lexicon with a forward DFA is never in the canonical-tie mode (that kernel carries no forward-DFA state); a multipath
    lexicon in it has every pass refused;
  - set_strict_order(False) returns to the mode the work area had right after create;
  - while a streaming session is open nothing changes the mode or the shape, and the session ends with the one-shot result.
Every refusal is asserted on the host before anything else is launched."""
import numpy as np
import pytest

from beamutil import assert_grammar_fast, assert_trellis_equal, assert_trellis_equal_modulo_ties, load_beam_golden
from julius_amd import lexblob, lib, synth
from oracle import pyoracle

pytestmark = pytest.mark.gpu

SERVED_BEAM = {"ngram": 100, "dfa": 100, "fwd": 60, "wordlist": 80, "mp": 100, "tee": None}


class _Lex:
    """A small lexicon on the device, two utterances' scores and the reference's result at any beam (cached)."""

    def __init__(self, engine, oracle, ref, wd, kind):
        self.kind, self.engine, self.oracle, self.ref, self.wd = kind, engine, oracle, ref, wd
        self.fwd, self.mp, self.loose = kind == "fwd", kind in ("mp", "tee"), kind in ("dfa", "fwd", "wordlist")
        self._want = {}
        if kind == "tee":
            # test_multipath_exact_gpu.py: a root that reaches a word end along its own arcs (the reference refuses such a
            # word when it builds the tree; its CPU restatement is the reference here)
            g = load_beam_golden("beam_multipath.npz")
            lex = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g["lex"].items()}
            root = int(lex["startnode"][0])
            end = int(np.flatnonzero(lex["stend"] >= 0)[0])
            at = int(lex["ac_off"][root + 1])
            lex["ac_to"] = np.insert(lex["ac_to"], at, end).astype(np.int32)
            lex["ac_a"] = np.insert(lex["ac_a"], at, np.float32(-1.0)).astype(np.float32)
            lex["ac_off"] = lex["ac_off"].copy()
            lex["ac_off"][root + 1:] += 1
            self.lex, self.args, self.served = lex, None, g["beam_width"]
            self.scores = [oracle.gmm_outprob(g["am"], u["frames"]) for u in g["utts"][:2]]
            self.frames = None
        else:
            self.served = SERVED_BEAM[kind]
            hl = ["-input", "htkparam", "-gprune", "none"]
            if kind == "wordlist":
                task = synth.make_wordlist_task(wd, seed=7, triphone=True, nword=80)
                self.args = ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-w", task["wordlist"], "-wsil", "silB", "silE", "silB"] + hl
                self.frames = [synth.make_wordlist_utterance(task, seed=u)[0] for u in range(2)]
            elif kind == "fwd":
                task = synth.make_forward_grammar(synth.make_triphone_task(wd, seed=63, nword=80), ncat=3, maxwords=3, seed=63)
                self.args = ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-dfa", task["dfa"], "-v", task["gdict"], "-1pass"] + hl
                self.frames = [synth.make_forward_grammar_utterance(task, seed=6300 + u, nwords=None if u == 0 else 5)[0] for u in range(2)]
            elif kind == "dfa":
                task = synth.make_triphone_grammar(synth.make_triphone_task(wd, seed=62, nword=80), ncat=3, seed=62, wrap=True)
                self.args = ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-dfa", task["dfa"], "-v", task["gdict"], "-1pass"] + hl
                self.frames = [synth.make_triphone_grammar_utterance(task, nwords=2 + 2 * u, seed=6200 + u)[0] for u in range(2)]
            else:
                task = synth.make_triphone_task(wd, seed=61 if kind == "ngram" else 64, nword=80)
                self.args = (["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-nlr", task["arpa"], "-1pass",
                              "-sepnum", "5"] + hl + (["-multipath"] if kind == "mp" else []))
                self.frames = [synth.make_utterance(task, nwords=3 + 2 * u, seed=6100 + u)[0] for u in range(2)]
            eng = pyoracle.RefEngine(ref, self.args + ["-b", str(self.served)])
            eng.save_lexicon(wd / "lex.blob")
            self.lex = lexblob.load(wd / "lex.blob")
            assert bool(self.lex["lm_type"] & 0x100) == self.mp and (self.lex["nfwd"] > 0) == self.fwd
            am = ref.am_load(task["hmmdefs"], task["hmmlist"]).export()
            self.scores = [oracle.gmm_outprob(am, fr) for fr in self.frames]
        self.lx = lib.Lexicon(engine, self.lex)
        # the widest beam the exact-order kernel serves on this lexicon (none for the tee-root one: no beam at all)
        self.wide = None
        if self._layout(self.served) != "none":
            assert self._layout(65536) == "none"
            lo, hi = self.served, 65536
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if self._layout(mid) != "none" else (lo, mid)
            self.wide = hi
            assert self.wide > self.lex["nnode"]       # a full search in the reference (m_chkparam.c clamps the beam to it)

    def _layout(self, beam):
        bm = lib.Beam(self.engine, self.lx, beam, -1.0, max_utts=1)
        try:
            return bm.exact_layout()
        finally:
            bm.close()

    def want(self, beam):
        """[(canonical trellis, wseq, score)] of the reference for the two utterances at this beam."""
        if beam not in self._want:
            out = []
            if self.args is None:
                for sc in self.scores:
                    oatoms, wseq, score, rc, died = self.oracle.beam_pass1(self.lex, sc, beam, -1.0)
                    out.append((lexblob.canonical_trellis(oatoms), np.array(wseq if rc == 0 else [], np.int32), score))
            else:
                eng = pyoracle.RefEngine(self.ref, self.args + ["-b", str(beam)])
                for fr in self.frames:
                    synth.write_htk_param(self.wd / "u.mfc", fr)
                    rtr, (rwseq, rscore) = eng.recognize(self.wd / "u.mfc")
                    if self.kind == "wordlist":
                        _, rwseq, rscore = eng.final_result()
                    out.append((rtr, rwseq, rscore))
            self._want[beam] = out
        return self._want[beam]

    def beam_width(self, which):
        return self.served if which == "served" else self.wide

    def beam(self, which):
        return lib.Beam(self.engine, self.lx, self.beam_width(which), -1.0, max_utts=2, atoms_per_utt=1 << 17)

    def check(self, which, res, tre, mode):
        """The pass's result against the reference, by the rule of the mode that ran it."""
        assert mode != "fast" or not self.mp
        for r, atoms, (rtr, rwseq, rscore) in zip(res, tre, self.want(self.beam_width(which))):
            if mode == "fast" and self.loose:
                assert_grammar_fast(atoms, rtr, r, rwseq, rscore)
                continue
            if mode == "fast":
                assert_trellis_equal_modulo_ties(atoms, rtr, r.ties)
                if r.ties:
                    continue
            else:
                assert_trellis_equal(atoms, rtr)
            if len(rwseq):
                assert r.status == 0 and list(r.wseq[:r.wnum]) == list(rwseq) and r.score == rscore, mode
            else:
                assert r.status != 0, mode


@pytest.fixture(scope="module")
def lexes(engine, oracle, ref, tmp_path_factory):
    """kind -> _Lex, built on first use."""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _Lex(engine, oracle, ref, tmp_path_factory.mktemp(f"modes_{kind}"), kind)
        return made[kind]
    yield get
    made.clear()


CASES = [(k, w) for k in ("ngram", "dfa", "fwd", "wordlist", "mp", "tee") for w in ("served", "wide") if (k, w) != ("tee", "wide")]
IDS = [f"{k}-{w}" for k, w in CASES]


def _default(L, which):
    """The mode create() picks: the exact-order kernel where it serves the work area; else strict order for a forward DFA
    (the canonical-tie kernel would drop its state) and the canonical-tie kernel otherwise (which refuses multipath passes)."""
    if which == "served" and L.wide is not None:
        return "exact"
    return "strict" if L.fwd else "fast"


@pytest.mark.parametrize("kind,which", CASES, ids=IDS)
def test_default_mode_after_create(lexes, kind, which):
    L = lexes(kind)
    bm = L.beam(which)
    mode = bm.order_mode()
    assert mode == _default(L, which)
    assert (bm.exact_layout() == "none") == (mode != "exact")
    if mode == "fast" and L.mp:
        with pytest.raises(lib.JamdError, match="strict-order kernel only"):
            bm.pass1_host(L.scores)
    else:
        res, tre = bm.pass1_host(L.scores)
        L.check(which, res, tre, mode)
    bm.close()


SEQS = {
    "strict-on-off": [("strict", True), ("strict", False)],
    "off": [("strict", False)],
    "serial-off": [("mode", "exact_serial"), ("strict", False)],
    "serial-strict-off": [("mode", "exact_serial"), ("mode", "strict"), ("strict", False)],
    "fast-strict-exact": [("mode", "fast"), ("mode", "strict"), ("mode", "exact")],
    "exact-strict-fast-off": [("mode", "exact"), ("strict", True), ("mode", "fast"), ("strict", False)],
    "half-fast-full-off": [("shape", "half"), ("mode", "fast"), ("shape", "full"), ("strict", False)],
}


def _apply(bm, op):
    what, arg = op
    if what == "strict":
        bm.set_strict_order(arg)
    elif what == "mode":
        bm.set_order_mode(arg)
    else:
        bm.set_workgroup_shape(arg)


def _must_accept(L, which, op):
    """Calls whose outcome the contract fixes (None: either way, the invariants decide)."""
    served = which == "served" and L.wide is not None
    if op in (("strict", True), ("mode", "strict"), ("shape", "full"), ("shape", "auto")):
        return True
    if op == ("strict", False):
        return served or not L.fwd               # a forward DFA past the exact-order kernel stays in strict order
    if op in (("mode", "exact"), ("mode", "exact_serial")):
        return served
    if op == ("mode", "fast"):
        return not L.fwd
    return None


@pytest.mark.parametrize("seq", list(SEQS))
@pytest.mark.parametrize("kind,which", CASES, ids=IDS)
def test_call_sequence(lexes, kind, which, seq):
    L = lexes(kind)
    bm = L.beam(which)
    default = bm.order_mode()
    for op in SEQS[seq]:
        before = bm.order_mode()
        try:
            _apply(bm, op)
            accepted = True
        except lib.JamdError as e:
            accepted = False
            err = str(e)
        mode = bm.order_mode()
        # host-side checks first: nothing is launched in a state they reject
        if not accepted:
            assert mode == before, (op, err)
        expect = _must_accept(L, which, op)
        if expect is not None:
            assert accepted == expect, (op, before, mode)
        if L.fwd:
            assert mode != "fast", op
            if op == ("strict", False) and not accepted:
                assert "forward DFA" in err and mode == "strict"
        if op == ("strict", False) and accepted:
            assert mode == default, (op, mode, default)
        # the reported mode is the one that runs
        if mode == "fast" and L.mp:
            with pytest.raises(lib.JamdError, match="strict-order kernel only"):
                bm.pass1_host(L.scores)
        else:
            res, tre = bm.pass1_host(L.scores)
            L.check(which, res, tre, mode)
    bm.close()


def _stream_modes(kind, which):
    """Modes a streaming session can run in on this work area (test_default_mode_after_create pins which beams the
    exact-order kernel serves; the canonical-tie kernel takes no forward DFA and refuses multipath passes)."""
    modes = ["exact", "exact_serial"] if which == "served" and kind != "tee" else []
    if kind not in ("fwd", "mp", "tee"):
        modes.append("fast")
    return modes + ["strict"]


STREAM_CASES = [(k, w, m) for k, w in CASES for m in _stream_modes(k, w)]


@pytest.mark.parametrize("kind,which,mode", STREAM_CASES, ids=[f"{k}-{w}-{m}" for k, w, m in STREAM_CASES])
def test_no_change_mid_stream(lexes, kind, which, mode):
    """After stream_begin and one non-final push (strict order: before its only push), every setter is refused and
    leaves the mode alone; the session then ends with the one-shot result."""
    L = lexes(kind)
    bm = L.beam(which).set_order_mode(mode)
    res1, tre1 = bm.pass1_host(L.scores)
    L.check(which, res1, tre1, mode)
    bm.stream_begin(2)
    split = [0, 0] if mode == "strict" else [len(s) // 2 for s in L.scores]
    if mode != "strict":
        _push(bm, L, split, final=False, start=[0, 0])
    for op in [("strict", False), ("strict", True)] + [("mode", m) for m in ("fast", "strict", "exact", "exact_serial")] + \
              [("shape", s) for s in ("auto", "full", "half")]:
        with pytest.raises(lib.JamdError, match="stream"):
            _apply(bm, op)
        assert bm.order_mode() == mode, op
    _push(bm, L, [len(s) for s in L.scores], final=True, start=split)
    res = bm.results(2)
    for u, r in enumerate(res):
        assert (r.status, r.natom, r.score, r.wnum) == (res1[u].status, res1[u].natom, res1[u].score, res1[u].wnum), (u, mode)
        a, b = lexblob.canonical_trellis(bm.trellis(u)), lexblob.canonical_trellis(tre1[u])
        assert all(np.array_equal(a[k], b[k]) for k in a), (u, mode)
    bm.close()


def _push(bm, L, upto, final, start=None):
    start = start or [0] * len(L.scores)
    S = L.scores[0].shape[1]
    part = [sc[a:b] for sc, a, b in zip(L.scores, start, upto)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in part])]).astype(np.int32)
    rows = np.concatenate(part) if off[-1] else np.zeros((1, S), np.float32)
    d = lib.DevBuf(L.engine, rows.nbytes).upload(np.ascontiguousarray(rows, np.float32))
    try:
        bm.stream_push_dev(d.ptr, S, off, final=final)
        bm.results(len(L.scores))
    finally:
        d.free()
