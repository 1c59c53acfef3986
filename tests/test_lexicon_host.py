"""Host half of the tree lexicon (csrc/beam_lexicon_image.h behind csrc/beam_lexicon_api.hip): that header as a
stand-alone program under the host sanitizers, and the library's own jamd_lexicon_create() refusing corrupted golden
lexicons before it touches a device.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from beamutil import load_beam_golden
from julius_amd import lexblob, lib

GOLDEN_LEXICONS = ["beam_score", "beam_grammar", "beam_grammar_free", "beam_isolated", "beam_multipath", "beam_rank"]


def test_check_and_image_under_sanitizers(tmp_path):
    """tests/lexicon_image_check.cpp (its own main over csrc/beam_lexicon_image.h, which includes no HIP header) built
    with -fsanitize=address,undefined, the runtimes linked statically: an N-gram lexicon, its two multipath forms, a
    grammar with a forward DFA, its multipath form and the word-mode form, every array a heap block of exactly its
    length -- accepted, the image laid out and filled as the kernels read it -- then every refusal of lexicon_check()
    once, counted against the header's own: every case as expected and no report."""
    exe = tmp_path / "lexicon_image_check"
    root = lib._PKG.parent
    header = lib._PKG / "csrc" / "beam_lexicon_image.h"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    "-I", str(root / "include"), str(root / "tests" / "lexicon_image_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(header)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") >= 100 and "Sanitizer" not in r.stderr
    assert "0 failure(s)" in r.stdout


# One corruption of each family: (name, the lexicons it applies to, what it does to the lexicon dict, the refusal).
def _set(key, index, value):
    def f(lex):
        a = np.array(lex[key]).copy()
        a[index] = value(lex) if callable(value) else value
        lex[key] = a
    return f


def _scalar(key, value):
    def f(lex):
        lex[key] = value(lex) if callable(value) else value
    return f


def _forward_dfa(bad_to):
    def f(lex):      # a forward DFA of two states beside the golden grammar, its second arc leaving the automaton
        lex.update(nfwd=2, fwd_off=np.array([0, 1, 2], np.int32), fwd_label=np.array([0, 1], np.int32),
                   fwd_to=np.array([1, bad_to], np.int32), init_to_state=np.zeros(lex["ninit"], np.int32))
    return f


class _Null:
    """The pointer of one array set to NULL in the finished descriptor (make_desc() gives every array a block)."""

    def __init__(self, field):
        self.field = field


NGRAM = ("beam_score", "beam_isolated", "beam_multipath", "beam_rank")
GRAMMAR = ("beam_grammar", "beam_grammar_free")
ALL = NGRAM + GRAMMAR
CORRUPTIONS = [
    ("flag bits", ALL, _scalar("lm_type", lambda l: l.get("lm_type", 0) | 0x200), b"lm_type="),
    ("sizes", ALL, _scalar("nnode", 0), b"bad sizes"),
    ("negative table size", ALL, _scalar("nset", -1), b"bad table sizes"),
    ("ac_off descends", ALL, _set("ac_off", 3, -1), b"ac_off not monotone at node 2"),
    ("word end out of range by one", ALL, _set("stend", -1, lambda l: l["nword"]), b"ends word"),
    ("successor id out of range by one", ALL, _set("scid", 5, lambda l: l["nscword"]), b"node 5 has successor id"),
    ("successor table one short", NGRAM, _scalar("nscword", lambda l: l["nscword"] - 1), b"outside the tables"),
    ("state set out of range by one", ALL, lambda l: (_set("out_kind", 7, 1)(l), _set("out_id", 7, l["nset"])(l)), b"node 7 has output"),
    ("root out of range by one", ALL, _set("startnode", 1, lambda l: l["nnode"]), b"root 1 is node"),
    ("negative word head", ALL, _set("word_head", 2, -2), b"word 2 starts at node -2"),
    ("set_off descends", ALL, _set("set_off", 4, -1), b"set_off not monotone at 3"),
    ("lc_tab names a missing set", ALL, _set("lc_tab", 0, lambda l: ~l["nset"]), b"lc_tab entry 0 names state set"),
    ("left context out of range by one", ALL, _set("word_lc", 1, lambda l: l["nlc"] + 1), b"word 1 selects left context"),
    ("N-gram entry out of range by one", NGRAM, _set("wton", 3, lambda l: l["ng_nword"]), b"word 3 is N-gram entry"),
    ("2-grams one short", NGRAM, _scalar("ng_nbigram", lambda l: l["ng_nbigram"] - 1), b"leave the table"),
    ("node array NULL", ALL, _Null("scid"), b"NULL or malformed node arrays"),
    ("word array NULL", ALL, _Null("word_lc"), b"NULL root, word or successor arrays"),
    ("successor array NULL", NGRAM, _Null("scword"), b"NULL root, word or successor arrays"),
    ("N-gram array NULL", NGRAM, _Null("ng_bi_wid"), b"NULL N-gram arrays"),
    ("arc array NULL", tuple(g for g in ALL if g != "beam_isolated"), _Null("ac_to"), b"arc arrays missing"),   # (beam_isolated has no extra arc)
    ("state-set offsets NULL", ALL, _Null("set_off"), b"state-set table missing"),
    # ... and the ones that used to come behind the first device call
    ("isolated root not assigned", NGRAM, _scalar("isolatenum", lambda l: l["isolatenum"] + 1), b"is not assigned"),
    ("isolated number repeated", NGRAM, lambda l: _set("start2isolate", int(np.flatnonzero(l["start2isolate"] >= 0)[1]),
                                                        int(l["start2isolate"][np.flatnonzero(l["start2isolate"] >= 0)[0]]))(l),
     b"start2isolate out of range or repeated"),
    ("root category", GRAMMAR, _set("start2wid", 0, lambda l: l["nword"]), b"root 0 has no valid category"),
    ("word category", GRAMMAR, _set("wton", -1, lambda l: l["ncat"]), b"categor"),
    ("initial node out of range by one", GRAMMAR, _set("init_node", 0, lambda l: l["nnode"]), b"bad initial node"),
    ("forward-DFA arc target", GRAMMAR, _forward_dfa(2), b"forward DFA arc 1 leaves the automaton"),
    ("forward-DFA arc target negative", GRAMMAR, _forward_dfa(-1), b"forward DFA arc 1 leaves the automaton"),
]
CASES = [(g, c) for c in CORRUPTIONS for g in GOLDEN_LEXICONS if g in c[1]]


@pytest.mark.parametrize("golden,corruption", CASES, ids=[f"{g}-{c[0].replace(' ', '_')}" for g, c in CASES])
def test_library_refuses_corrupt_golden_without_a_device(golden, corruption):
    """jamd_lexicon_create() with a placeholder engine: every refusal comes before the first device call, so an invalid
    descriptor never gets as far as the engine -- JAMD_EINVAL, no handle, the matching text."""
    _, _, corrupt, text = corruption
    lex = dict(load_beam_golden(golden + ".npz")["lex"])
    if not isinstance(corrupt, _Null):
        corrupt(lex)
    d, keep = lexblob.make_desc(lex)
    if isinstance(corrupt, _Null):
        assert getattr(d, corrupt.field)
        setattr(d, corrupt.field, None)
    fake_engine = C.create_string_buffer(256)
    h = C.c_void_p()
    L = lib.load()
    assert L.jamd_lexicon_create(C.cast(fake_engine, C.c_void_p), C.byref(d), C.byref(h)) == -1     # JAMD_EINVAL
    assert not h.value
    assert text in L.jamd_last_error(), L.jamd_last_error()
