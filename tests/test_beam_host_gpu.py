"""The first pass's host layer (csrc/beam_api.hip, csrc/beam_lexicon_api.hip) where one work area changes what it owns:
the prune-order scratch across growth, the strict-order work area across order switches, the streaming state across
sessions, and the destroys in the order the engine goes first.  Smallest shapes: the golden beam_score lexicon."""
import numpy as np
import pytest

from beamutil import assert_trellis_equal, load_beam_golden
from julius_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(oracle):
    g = load_beam_golden("beam_score.npz")
    g["scores"] = [oracle.gmm_outprob(g["am"], u["frames"]) for u in g["utts"][:2]]
    return g


def _assert_golden(g, res, tre, utts):
    for r, atoms, i in zip(res, tre, utts):
        u = g["utts"][i]
        assert r.status == 0 and r.frames == len(u["frames"])
        assert_trellis_equal(atoms, u["trellis"])
        assert np.array_equal(np.array(r.wseq[:r.wnum]), u["wseq"]) and r.score == u["score"]


def test_prune_scratch_across_growth(engine, oracle, gold):
    """jamd_beam_prune_order() at 64 tokens, past the scratch's capacity (64 + 1024), at 64 again, then
    jamd_beam_prune_arrange() inside the grown capacity (5 000 and 6 000 of 6 024: the arrange buffer is made) and past it
    (8 000: the scratch is replaced once more and the arrange buffer follows it) -- every result the sequential sort's."""
    beam = 40
    lx = lib.Lexicon(engine, gold["lex"])
    bm = lib.Beam(engine, lx, beam, -1.0, max_utts=1)
    rng = np.random.default_rng(40)
    for n in (64, 5000, 64):
        sc = (-rng.integers(0, 50, n).astype(np.float32) * 0.5 - 2000.0).astype(np.float32)      # heavy ties
        assert np.array_equal(bm.prune_order(sc), oracle.sort_token_no_order(sc, beam)), n
    for n in (5000, 6000, 8000):
        sc = (-rng.random(n) * 300.0 - 5000.0).astype(np.float32)
        sc[rng.integers(0, n, n // 10)] = sc[rng.integers(0, n, n // 10)]
        order, arr = bm.prune_arrange(sc)
        worder, warr = oracle.sort_token_arrange(sc, beam)
        assert np.array_equal(order, worder) and np.array_equal(arr, warr), n
    bm.close()
    lx.close()


def test_strict_order_on_off_on(engine, gold):
    """A whole-utterance pass after each switch: the strict work area is made by the first and serves the third."""
    lx = lib.Lexicon(engine, gold["lex"])
    bm = lib.Beam(engine, lx, gold["beam_width"], gold["score_pruning_width"], max_utts=2)
    default = bm.order_mode()
    for on in (True, False, True):
        bm.set_strict_order(on)
        assert bm.order_mode() == ("strict" if on else default)
        res, tre = bm.pass1_host(gold["scores"])
        _assert_golden(gold, res, tre, [0, 1])
    bm.close()
    lx.close()


def test_stream_begin_twice(engine, gold):
    """Two sessions on one work area, of two utterances and then of one, each in two pushes: the streaming state is made
    by the first jamd_beam_stream_begin() and reset by the second -- both end with the whole-utterance result."""
    scores = gold["scores"]
    S = scores[0].shape[1]
    lx = lib.Lexicon(engine, gold["lex"])
    bm = lib.Beam(engine, lx, gold["beam_width"], gold["score_pruning_width"], max_utts=2)
    for utts in ([0, 1], [1]):
        bm.stream_begin(len(utts))
        for final in (False, True):
            part = [scores[u][len(scores[u]) // 2:] if final else scores[u][:len(scores[u]) // 2] for u in utts]
            off = np.concatenate([[0], np.cumsum([len(p) for p in part])]).astype(np.int32)
            rows = np.concatenate(part)
            d = lib.DevBuf(engine, rows.nbytes).upload(rows)
            bm.stream_push_dev(d.ptr, S, off, final=final)
            res = bm.results(len(utts))
            d.free()
        _assert_golden(gold, res, [bm.trellis(i) for i in range(len(utts))], utts)
    bm.close()
    lx.close()


def test_engine_destroyed_first(gold):
    """jamd_engine_destroy(), then jamd_beam_destroy() and jamd_lexicon_destroy(): each selects the device it stored when
    it was created and frees its own memory; neither looks at the engine."""
    eng = lib.Engine(0)
    lx = lib.Lexicon(eng, gold["lex"])
    bm = lib.Beam(eng, lx, gold["beam_width"], gold["score_pruning_width"], max_utts=2)
    bm.set_strict_order(True)                # (the strict work area is there to be freed)
    bm.set_strict_order(False)
    res, tre = bm.pass1_host(gold["scores"])
    _assert_golden(gold, res, tre, [0, 1])
    eng.sync()
    eng.close()
    bm.close()
    lx.close()
