"""CPU: the language-model forms of tests/lmforms.py -- word classes (cprob != 0), pronunciation variants (several words
on one N-gram entry), <unk> and transparent words under classes, a backward N-gram alone (ng_mode 3) and in-category
word probabilities under a grammar -- in the first-pass oracle against the compiled reference, bit for bit; and the host
readers (binary N-gram, factoring values) over the same forms.  Every form must also be shown to matter: a test that
would pass with the form's value ignored fails here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from beamutil import TR_KEYS
from julius_amd import lexblob, lib, synth
from lmforms import (FORMS, GRAMMAR_FORMS, NENT, LmCase, assert_form, bigram_branches, classed_dict, form_counts,
                     same_trellis, shared_context_atoms, with_fields)
from test_readers import EXPORT, _blob_records, _fscore_of, _ref

CASES = [(f, False) for f in FORMS + GRAMMAR_FORMS] + [("class", True), ("rlonly", True)]
IDS = [f + ("-mp" if mp else "") for f, mp in CASES]


@pytest.fixture(scope="module")
def cases(oracle, ref, tmp_path_factory):
    """(form, multipath) -> LmCase over 3 utterances of 3 + 2u words, built on first use."""
    made = {}

    def get(form, multipath=False):
        if (form, multipath) not in made:
            made[form, multipath] = LmCase(ref, oracle, tmp_path_factory.mktemp(f"lm_{form}"), form,
                                           [3 + 2 * u for u in range(3)], multipath=multipath)
        return made[form, multipath]
    yield get
    made.clear()


def _scores_differ(a, b):
    return len(a["wid"]) != len(b["wid"]) or not (np.array_equal(a["lscore"], b["lscore"]) and
                                                 np.array_equal(a["backscore"], b["backscore"]))


@pytest.mark.parametrize("form,multipath", CASES, ids=IDS)
def test_oracle_matches_reference(cases, form, multipath):
    c = cases(form, multipath)
    assert_form(c.lex, form)
    for (rtr, rwseq, rscore), (otr, owseq, oscore, rc) in zip(c.ref, c.orc):
        assert rc in (0, 1)
        assert len(otr["wid"]) == len(rtr["wid"]) > 100
        for k in TR_KEYS:
            assert np.array_equal(otr[k], rtr[k]), k
        if rc == 0:
            assert np.array_equal(owseq, rwseq) and oscore == rscore
    print(f"{form}{'-mp' if multipath else ''}: seed {c.seed}, (ng_mode, distinct wton, non-zero cprob) = {form_counts(c.lex)}, "
          f"atoms {[len(o[0]['wid']) for o in c.orc]}, rc {[o[3] for o in c.orc]}")


@pytest.mark.parametrize("form,multipath", [x for x in CASES if "class" in x[0] or x[0] in GRAMMAR_FORMS],
                         ids=[i for i in IDS if "class" in i or i in GRAMMAR_FORMS])
def test_class_probabilities_matter(cases, form, multipath):
    """With cprob zeroed the search differs on every utterance: a device that dropped the term could not pass."""
    c = cases(form, multipath)
    zero = with_fields(c.lex, cprob=np.zeros_like(c.lex["cprob"]))
    for sc, (otr, _, _, _) in zip(c.scores, c.orc):
        assert _scores_differ(c.run_oracle(zero, sc)[0], otr)


@pytest.mark.parametrize("form", ["variants", "class"])
def test_contexts_are_shared_between_words(cases, form):
    """The kernels key their LM memo and the cross-word table by wton(last word): every utterance's trellis must hold
    word ends whose N-gram entry another dictionary word has too."""
    c = cases(form)
    for otr, _, _, _ in c.orc:
        assert shared_context_atoms(c.lex, otr) >= 1
    assert np.all(c.lex["cprob"] == 0) == (form == "variants")


@pytest.mark.parametrize("form,multipath", [("rlonly", False), ("rlonly_class", False), ("rlonly", True)],
                         ids=["rlonly", "rlonly_class", "rlonly-mp"])
def test_backward_only_lookup_matters(cases, form, multipath):
    """ng_mode 3 read as ng_mode 2 (the same tables without bi_prob_compute()'s 1-gram terms) is another search."""
    c = cases(form, multipath)
    assert c.lex["ng_mode"] == 3
    for sc, (otr, _, _, _) in zip(c.scores, c.orc):
        assert _scores_differ(c.run_oracle(with_fields(c.lex, ng_mode=2), sc)[0], otr)


@pytest.mark.parametrize("form,multipath", [x for x in CASES if x[0] in FORMS], ids=[i for i in IDS if i.split("-")[0] in FORMS])
def test_both_branches_of_the_bigram_lookup(cases, form, multipath):
    """Distinct (predecessor word, word) pairs of the trellises that search_bigram() finds, and that back off."""
    c = cases(form, multipath)
    hit, backoff = bigram_branches(c.lex, [o[0] for o in c.orc])
    print(f"{form}{'-mp' if multipath else ''}: {hit} pairs found, {backoff} backed off")
    assert hit >= 20 and backoff >= 20


@pytest.mark.parametrize("form", ["plain", "class"])
def test_old_binary_format_mode_is_the_normal_lookup(cases, form):
    """JAMD_NG_ADDITIONAL_OLD (ng_mode 1): the flattener fills the descriptor as for mode 0
    (shim/jamd_flatten_lex.c:254-255) and the reference tree has no writer for the old format, so the mode is
    relabelled here: identical results."""
    c = cases(form)
    assert c.lex["ng_mode"] == 0
    for sc, (otr, owseq, oscore, rc) in zip(c.scores, c.orc):
        tr1, wseq1, score1, rc1 = c.run_oracle(with_fields(c.lex, ng_mode=1), sc)
        assert same_trellis(tr1, otr) and rc1 == rc and score1 == oscore and np.array_equal(wseq1, owseq)


# ------------------------------------------------------------------------------------------------- host readers
def _export(tmp_path, task, name, lm, extra=()):
    subprocess.run([str(EXPORT), "-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-d", str(lm)] +
                   list(extra) + ["-input", "htkparam", "-jamdout", str(tmp_path / name)], check=True, capture_output=True)
    return tmp_path / f"{name}.lex"


@pytest.mark.parametrize("classed", [False, True], ids=["plain", "class"])
def test_backward_only_bingram(tmp_path, classed):
    """A binary N-gram written from the backward ARPA file alone: the direct reader's first-pass tables are the
    exported lexicon's byte for byte, and the lexicon says ng_mode 3 -- with or without a class dictionary."""
    ref = _ref()
    ref.lib.jref_write_bingram.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    task = synth.make_triphone_task(tmp_path, seed=81, nword=80, nphone=8, S=120, M=2, with_rl3=True)
    if classed:
        classed_dict(task["dict"], NENT, 81)
    bingram = tmp_path / "rl.bingram"
    assert ref.lib.jref_write_bingram(None, str(task["arpa_rl"]).encode(), str(bingram).encode()) == 0
    lexfile = _export(tmp_path, task, "exp", bingram)
    lex = lexblob.load(lexfile)
    assert_form(lex, "rlonly_class" if classed else "rlonly")
    L = lib.load()
    same = C.c_int(-1)
    rc = L.jamd_bingram_check(str(lexfile).encode(), str(bingram).encode(), C.byref(same))
    assert rc == 0 and same.value == 1, L.jamd_last_error()


TREE = ("self_a", "next_a", "ac_off", "ac_to", "ac_a", "stend", "scid", "startnode", "start2isolate", "word_head", "scword")


def test_retrained_ngram_under_a_class_dictionary(tmp_path):
    """jamd_bingram_fscore() where the words wchmm.c keeps out of the tree are ranked by uni_prob[wton[w]] + cprob[w]
    (wchmm.c:1490) and a factoring value is the best of that sum below a node (factoring_sub.c:447): a retrained N-gram
    that leaves the five best words alone gives the fresh export's values index by index; one that promotes another word
    into the five is refused."""
    ref = _ref()
    ref.lib.jref_write_bingram.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    seed, sepnum = 83, 5
    task = synth.make_triphone_task(tmp_path, seed=seed, nword=300, nphone=8, S=120, M=2)
    classed_dict(task["dict"], NENT, seed)

    def bingram(name, arpa):
        assert ref.lib.jref_write_bingram(str(arpa).encode(), None, str(tmp_path / f"{name}.bingram").encode()) == 0
        return tmp_path / f"{name}.bingram"

    lm1 = bingram("lm1", task["arpa"])
    exp1 = _export(tmp_path, task, "exp1", lm1, ["-sepnum", str(sepnum)])
    lex = lexblob.load(exp1)
    assert_form(lex, "class")
    names = [n.decode() for n in lex["ng_wname"].tobytes().split(b"\0")][:lex["ng_nword"]]
    rank = lex["ng_uni_prob"][lex["wton"]] + lex["cprob"]
    order = np.argsort(-rank, kind="stable")
    assert rank[order[sepnum - 1]] > rank[order[sepnum]]                  # the five are the five: no tie at the cut
    keep = {names[lex["wton"][w]] for w in order[:sepnum]}
    # a word of another entry, the one nearest to its entry's 1-gram, to be lifted over the best of the five
    outside = [w for w in order[sepnum:] if names[lex["wton"][w]] not in keep]
    lifted = max(outside, key=lambda w: lex["cprob"][w])
    rng = np.random.default_rng(seed)
    A = open(task["arpa"]).read().splitlines()
    a, b = A.index("\\1-grams:") + 1, A.index("\\2-grams:")

    def variant(name, promote):
        out = list(A)
        for i in range(a, b):
            f = A[i].split()
            if len(f) == 3 and f[1] not in keep:
                out[i] = f"{float(f[0]) - rng.uniform(0.05, 0.6):.6f}\t{f[1]}\t{f[2]}"
                if promote and f[1] == names[lex["wton"][lifted]]:
                    out[i] = f"{rank[order[0]] - lex['cprob'][lifted] + 0.2:.6f}\t{f[1]}\t{f[2]}"
        (tmp_path / f"{name}.arpa").write_text("\n".join(out) + "\n")
        return bingram(name, tmp_path / f"{name}.arpa")

    lm2, lm3 = variant("lm2", False), variant("lm3", True)
    exp2 = _export(tmp_path, task, "exp2", lm2, ["-sepnum", str(sepnum)])
    r1, r2 = _blob_records(exp1, b"JAMDLEX1"), _blob_records(exp2, b"JAMDLEX1")
    assert np.frombuffer(r1["sep_wnum"][1], np.int32)[0] == sepnum
    for k in TREE + ("wton", "cprob"):
        assert r1[k] == r2[k], k                                           # the same words stayed out: the same tree
    f1, f2 = np.frombuffer(r1["fscore"][1], np.float32), np.frombuffer(r2["fscore"][1], np.float32)
    assert len(f1) == len(f2) > 50 and (f1[1:] != f2[1:]).sum() > 10       # the values did move
    L = lib.load()
    rc, got = _fscore_of(L, exp1, lm2)
    assert rc == 0, L.jamd_last_error()
    assert np.array_equal(got[1:], f2[1:])                                 # == wchmm.c's own, from the fresh export
    rc, same = _fscore_of(L, exp1, lm1)
    assert rc == 0 and np.array_equal(same[1:], f1[1:])
    rc, _ = _fscore_of(L, exp1, lm3)
    assert rc != 0 and b"export the lexicon again" in L.jamd_last_error()
