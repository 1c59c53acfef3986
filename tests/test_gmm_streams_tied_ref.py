"""CPU: the tied-mixture multi-stream fixture tests/golden/gmm_streams_tied.npz against the live compiled reference, and
the helper's ascii hmmdefs against the reference's own binary writer and reader.  No device code runs here."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import streamstied as st  # noqa: E402


@pytest.mark.parametrize("name", list(st.CASES))
def test_fixture_equals_live_reference(ref, tmp_path, name):
    """The committed arrays are what the case's recipe makes, and the committed scores (and caches) are what the
    reference computes today for the hmmdefs written from the COMMITTED arrays, under every mode -- bit for bit."""
    c, made = st.load_case(name), st.CASES[name]()
    for k in st.MODEL_KEYS:
        assert np.array_equal(c["model"][k], made["model"][k]), k
    assert np.array_equal(c["frames"], made["frames"]) and np.array_equal(c["utt_off"], made["utt_off"])
    assert c["nums"] == made["nums"] and c["cache"] == made["cache"]
    path, S = tmp_path / "hmmdefs", c["model"]["st_pdf"].shape[0]
    st.write_tied_hmmdefs(path, c["model"])
    for gprune, n in st.modes(c):
        r = st.RefModel(ref, path, S, gprune, n)
        assert np.array_equal(r.scores(c["frames"], c["utt_off"]), c["scores"][st.key(gprune, n)]), (gprune, n)
        if gprune == "safe" and n in c["cache"]:
            for got, want in zip(r.cache(c["frames"], st.nbook(c["model"])), c["caches"][f"safe{n}"]):
                assert np.array_equal(got, want)
        r.close()


@pytest.mark.parametrize("name", [n for n in st.CASES if st.CASES[n]()["binhmm"]])
def test_binhmm_round_trip_scores_the_same(ref, tmp_path, name):
    """write_binhmm() -> read_binhmm() of the reference, fresh and committed: the binary file scores as the ascii one
    under both modes (codebooks, a NULL member, stream weights, plain pdfs beside tied ones)."""
    c = st.load_case(name)
    S = c["model"]["st_pdf"].shape[0]
    st.write_tied_hmmdefs(tmp_path / "hmmdefs", c["model"])
    fresh = st.write_binhmm(ref, tmp_path / "hmmdefs", tmp_path / "fresh.binhmm")
    committed = st.load_binhmm(name, tmp_path / "committed.binhmm")
    for gprune, n in st.modes(c):
        for path in (fresh, committed):
            r = st.RefModel(ref, path, S, gprune, n)
            assert np.array_equal(r.scores(c["frames"], c["utt_off"]), c["scores"][st.key(gprune, n)]), (gprune, n, path)
            r.close()


@pytest.mark.parametrize("name", [n for n in st.CASES if n != "e2e"])
def test_safe_differs_from_none_where_a_book_is_pruned(name):
    """Every case with a book larger than gprune_num: pruning shows in the scores, so a device path that ignored the
    mode could not pass both."""
    c = st.load_case(name)
    for n in c["nums"]:
        if max(st.book_sizes(c["model"])) > n:
            assert not np.array_equal(c["scores"][f"safe{n}"], c["scores"]["none"]), n


def test_history_shows_in_the_ties_case():
    """The same 17 frames as three utterances and as one: the reference alone scores them differently somewhere, and
    only from the second utterance on."""
    a, b = st.load_case("ties"), st.load_case("ties_one_utt")
    assert np.array_equal(a["frames"], b["frames"]) and list(a["utt_off"]) == [0, 7, 8, 17]
    differ = [n for n in a["nums"] if not np.array_equal(a["scores"][f"safe{n}"], b["scores"][f"safe{n}"])]
    assert differ
    for n in a["nums"]:
        assert np.array_equal(a["scores"][f"safe{n}"][:7], b["scores"][f"safe{n}"][:7])
    assert np.array_equal(a["scores"]["none"], b["scores"]["none"])


@pytest.mark.parametrize("name", ["branches", "compound", "lay_4_3_two_books"])
def test_float64_restatement_of_the_stream_loop(name):
    """calc_tied_mix() / calc_compound_mix() under -gprune none in float64 agree with the reference on every score, and
    `branches` does what its recipe says."""
    c = st.load_case(name)
    m, fr, sc = c["model"], c["frames"], c["scores"]["none"]
    soff = np.concatenate([[0], np.cumsum(m["vsize"])])
    want = np.empty(sc.shape)
    for t in range(sc.shape[0]):
        for s in range(sc.shape[1]):
            tot = 0.0
            for k in range(len(m["vsize"])):
                p = m["st_pdf"][s, k]
                x = fr[t, soff[k]:soff[k + 1]].astype(np.float64)
                terms = [-1e6]             # addlog_array() starts from LOG_ZERO as a value (addlog.c:109)
                for e in range(m["pdf_off"][p], m["pdf_off"][p + 1]):
                    g = m["ent_dens"][e]
                    if g < 0:                  # a NULL density scores LOG_ZERO and takes its weight like any other
                        terms.append(-1e6 + float(m["ent_logw"][e]))
                        continue
                    a, b = m["dens_off"][g], m["dens_off"][g + 1]
                    terms.append(-0.5 * (float(m["gconst"][g]) + np.sum((x - m["mean"][a:b]) ** 2 * m["ivar"][a:b].astype(np.float64)))
                                 + float(m["ent_logw"][e]))
                lp = np.logaddexp.reduce(terms)
                if np.float32(lp) <= -1e6:     # (the reference compares the fp32 value: spacing 1/16 there)
                    continue
                tot += lp * float(m["st_weight"][s, k])
            want[t, s] = -1e6 if tot == 0 or tot <= -1e6 else tot * 0.434294482
    # the bound tests/test_gmm_streams_ref.py derives: fp32 sums of at most 26 + 1 terms, 27 x 2^-24 = 1.6e-6 of the
    # magnitude, twice (Gaussian, stream sum) and the final product; the log-sum table's step is 3e-5 in the argument
    # of a function of slope <= 0.5, 1.5e-5 a step.  A pdf here has up to 7 entries where that file's had 3, but a step
    # whose smaller term lies more than ln 2 below the larger has slope <= 1/3, and of a book's members at most two
    # or three lie that close to the best on any frame: the same 1e-4 holds.
    assert (np.abs(want - sc) <= 4e-6 * np.abs(want) + 1e-4).all()
    if name == "branches":
        assert (sc[5, [0, 2, 4]] == st.LOG_ZERO).all() and (sc[:, 5] == st.LOG_ZERO).all()   # every stream skipped; all weights 0
        assert (sc[4, :5] > st.LOG_ZERO).all()                                       # one stream skipped, the others count
        assert not m["has_sw"][2] and m["st_weight"][4, 1] == 0.0 and (m["ent_dens"] < 0).sum() > 0
        assert len(set(m["pdf_book"])) == 4 and (m["pdf_book"] >= 0).all()           # books shared by every state
