"""GPU: the first-pass kernels (csrc/beam.hip, beam_exact.hip, beam_exact_mp.h, beam_strict.hip), the cross-word table
builder (beam_lexicon.hip) and the table-less LM path (JAMD_NO_IWTAB) over the language-model forms of tests/lmforms.py:
word classes, pronunciation variants, <unk> and transparent words under classes, a backward N-gram alone (ng_mode 3),
in-category word probabilities under a grammar, and ng_mode 1.  Every run is compared with oracle.beam_pass1 AND the
compiled reference: bit for bit in the exact and strict modes, by the existing tie rules in the canonical-tie mode.
tests/test_lm_forms.py shows on the CPU that each form's value matters to the result."""
import numpy as np
import pytest

from beamutil import assert_grammar_fast, assert_trellis_equal, assert_trellis_equal_modulo_ties
from julius_amd import lexblob, lib
from lmforms import FORMS, GRAMMAR_FORMS, LmCase, assert_form, with_fields

pytestmark = pytest.mark.gpu

MODES = ("exact", "strict", "fast")
ATOMS = 1 << 17


@pytest.fixture(scope="module")
def cases(oracle, ref, tmp_path_factory):
    """LmCase over 4 utterances of 2 + 3u words by (form, multipath, wide, sepnum), built on first use and shared."""
    made = {}

    def get(form, multipath=False, wide=False, sepnum=4):
        key = (form, multipath, wide, sepnum)
        if key not in made:
            made[key] = LmCase(ref, oracle, tmp_path_factory.mktemp(f"lmg_{form}"), form, [2 + 3 * u for u in range(4)],
                               multipath=multipath, wide=wide, sepnum=sepnum)
        assert_form(made[key].lex, form)
        return made[key]
    yield get
    made.clear()


def _lexicon(engine, lex, monkeypatch, table=True):
    """The lexicon on the device with its cross-word LM table, or (JAMD_NO_IWTAB) without: lm_table() tells which."""
    with monkeypatch.context() as m:
        if table:
            m.delenv("JAMD_NO_IWTAB", raising=False)
        else:
            m.setenv("JAMD_NO_IWTAB", "1")
        lx = lib.Lexicon(engine, lex)
    ngram_roots = (lex["lm_type"] & 0xff) == 0 and lex["isolatenum"] > 0
    assert lx.lm_table() == (1 if table and ngram_roots else 0)
    return lx


def _run(engine, c, lx, mode, shape=None):
    # (the beam-5000 task fills up to 195 000 atoms per utterance)
    bm = lib.Beam(engine, lx, c.eng.beam_width, -1.0, max_utts=len(c.scores), atoms_per_utt=ATOMS if c.beam <= 150 else 1 << 19)
    bm.set_order_mode(mode)
    if shape is not None:
        try:
            bm.set_workgroup_shape(shape)
        except lib.JamdError:
            pytest.skip(f"the {shape} shape is not available for this work area")
        assert bm.workgroup_shape(len(c.scores)) == shape
    res, tre = bm.pass1_host(c.scores)
    return bm, res, tre


def _check(c, res, tre, mode):
    """One pass against the oracle and the compiled reference, by the rule of the mode that ran it."""
    for r, atoms, (rtr, rwseq, rscore), (otr, owseq, oscore, rc) in zip(res, tre, c.ref, c.orc):
        assert r.status == rc
        got = list(r.wseq[:r.wnum])
        if mode != "fast":
            assert_trellis_equal(atoms, otr)
            assert_trellis_equal(atoms, rtr)
            if r.status == 0:
                assert got == list(rwseq) == list(owseq) and r.score == rscore == oscore
        elif c.form in GRAMMAR_FORMS:
            assert_grammar_fast(atoms, otr, r, owseq, oscore)
            assert_grammar_fast(atoms, rtr, r, rwseq, rscore)
        else:
            assert_trellis_equal_modulo_ties(atoms, otr, r.ties)
            assert_trellis_equal_modulo_ties(atoms, rtr, r.ties)
            if r.status == 0 and r.ties == 0:
                assert got == list(rwseq) and r.score == rscore


def _bytes(res, tre):
    """Everything a pass returns, for byte-wise comparison of two runs."""
    out = []
    for r, atoms in zip(res, tre):
        ct = lexblob.canonical_trellis(atoms)
        out.append((r.status, r.natom, r.score, list(r.wseq[:r.wnum]), tuple(ct[k].tobytes() for k in sorted(ct))))
    return out


# ---- a. every form x order mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", FORMS + GRAMMAR_FORMS)
def test_form_vs_oracle_and_reference(engine, cases, monkeypatch, form, mode):
    c = cases(form)
    if form in FORMS:
        assert sum(o[3] == 0 for o in c.orc) >= 3
    bm, res, tre = _run(engine, c, _lexicon(engine, c.lex, monkeypatch), mode)
    _check(c, res, tre, mode)


# ---- b. with the cross-word table and without ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["class", "class_unk", "class_transp", "rlonly_class"])
def test_both_lm_paths(engine, cases, monkeypatch, form, mode):
    c = cases(form)
    outs = []
    for table in (True, False):
        lx = _lexicon(engine, c.lex, monkeypatch, table)
        assert lx.lm_table() == (1 if table else 0)
        bm, res, tre = _run(engine, c, lx, mode)
        _check(c, res, tre, mode)
        outs.append(_bytes(res, tre))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sepnum", [0, 20])
def test_table_less_at_other_tree_splits(engine, cases, monkeypatch, sepnum, mode):
    """-sepnum 0: no word is kept out of the tree for its frequency, so the most LM values come through the memo of
    max_successor_prob(); -sepnum 20: the twenty most frequent words are roots of their own and take the cross-word
    expressions instead."""
    c = cases("class", sepnum=sepnum)
    assert cases("class", sepnum=20).lex["isolatenum"] > cases("class", sepnum=0).lex["isolatenum"]
    lx = _lexicon(engine, c.lex, monkeypatch, table=False)
    assert lx.lm_table() == 0
    bm, res, tre = _run(engine, c, lx, mode)
    _check(c, res, tre, mode)


# ---- c. shapes and layouts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [True, False], ids=["table", "table-less"])
@pytest.mark.parametrize("form", ["class", "rlonly"])
def test_half_shape(engine, cases, monkeypatch, form, table):
    c = cases(form)
    bm, res, tre = _run(engine, c, _lexicon(engine, c.lex, monkeypatch, table), "exact", shape="half")
    _check(c, res, tre, "exact")


@pytest.mark.parametrize("form", ["class", "rlonly"])
def test_wide_layout(engine, cases, monkeypatch, form):
    c = cases(form, wide=True)
    assert c.eng.beam_width == 5000
    bm, res, tre = _run(engine, c, _lexicon(engine, c.lex, monkeypatch), "exact")
    assert bm.exact_layout() == "wide"                       # jamd_beam_exact_layout() == 2
    _check(c, res, tre, "exact")


@pytest.mark.parametrize("mode", ["exact", "strict"])
@pytest.mark.parametrize("form", ["class", "rlonly"])
def test_multipath(engine, cases, monkeypatch, form, mode):
    c = cases(form, multipath=True)
    outs = []
    for table in (True, False):
        bm, res, tre = _run(engine, c, _lexicon(engine, c.lex, monkeypatch, table), mode)
        _check(c, res, tre, mode)
        outs.append(_bytes(res, tre))
    assert outs[0] == outs[1]


# ---- d. streaming ------------------------------------------------------------------------------------------------------
CHUNKS = [1] * 5 + [7, 0, 10000]


@pytest.mark.parametrize("form,table", [("class", True), ("class", False), ("grammar_free", True)],
                         ids=["class", "class-table-less", "grammar_free"])
def test_streaming_equals_one_shot(engine, cases, monkeypatch, form, table):
    c = cases(form)
    lx = _lexicon(engine, c.lex, monkeypatch, table)
    one, res1, tre1 = _run(engine, c, lx, "exact")
    _check(c, res1, tre1, "exact")
    bm = lib.Beam(engine, lx, c.eng.beam_width, -1.0, max_utts=len(c.scores), atoms_per_utt=ATOMS)
    assert bm.order_mode() == "exact"
    S = c.scores[0].shape[1]
    bm.stream_begin(len(c.scores))
    pos = [0] * len(c.scores)
    for ci, ch in enumerate(CHUNKS):
        part, off = [], [0]
        for u, sc in enumerate(c.scores):             # utterance u advances by ch + u frames (until it runs out)
            n = min(len(sc) - pos[u], (ch + u) if ch else 0)
            part.append(sc[pos[u]:pos[u] + n]); pos[u] += n; off.append(off[-1] + n)
        rows = np.concatenate(part) if off[-1] else np.zeros((1, S), np.float32)
        d = lib.DevBuf(engine, rows.nbytes).upload(np.ascontiguousarray(rows, np.float32))
        bm.stream_push_dev(d.ptr, S, np.array(off, np.int32), final=ci == len(CHUNKS) - 1)
        assert [r.frames for r in bm.results(len(c.scores))] == pos
        d.free()
    res2 = bm.results(len(c.scores))
    for u, (a, b) in enumerate(zip(res1, res2)):
        assert (a.status, a.natom, a.wnum, a.score, a.frames) == (b.status, b.natom, b.wnum, b.score, b.frames)
        assert list(a.wseq[:a.wnum]) == list(b.wseq[:b.wnum])
        assert_trellis_equal(bm.trellis(u), lexblob.canonical_trellis(tre1[u]))


# ---- e. ng_mode 1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "strict"])
@pytest.mark.parametrize("form", ["plain", "class"])
def test_old_binary_format_mode(engine, cases, monkeypatch, form, mode):
    """JAMD_NG_ADDITIONAL_OLD: the descriptor is filled as for mode 0 (shim/jamd_flatten_lex.c:254-255), so the lexicon
    relabelled to it gives the same bytes, through the table and without it."""
    c = cases(form)
    assert c.lex["ng_mode"] == 0
    for table in (True, False):
        outs = []
        for ng_mode in (0, 1):
            lx = _lexicon(engine, with_fields(c.lex, ng_mode=ng_mode), monkeypatch, table)
            bm, res, tre = _run(engine, c, lx, mode)
            _check(c, res, tre, mode)
            outs.append(_bytes(res, tre))
        assert outs[0] == outs[1]


# ---- f. the forms are what they claim to be ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS + GRAMMAR_FORMS)
def test_descriptor_conditions(cases, form):
    c = cases(form)
    assert_form(c.lex, form)
    assert all(len(o[0]["wid"]) > 100 for o in c.orc)
