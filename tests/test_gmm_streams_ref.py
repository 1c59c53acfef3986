"""CPU: the multi-stream fixture tests/golden/gmm_streams.npz against the live compiled reference, and the helper's
ascii hmmdefs against the reference's own binary writer and reader.  No device code runs here."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import streamsref  # noqa: E402


@pytest.mark.parametrize("name", list(streamsref.CASES))
def test_fixture_equals_live_reference(ref, tmp_path, name):
    """The committed model arrays are what the case's recipe makes, and the committed scores are what the reference
    computes today for the hmmdefs written from the COMMITTED arrays -- bit for bit."""
    model, frames, scores = streamsref.load_case(name)
    made, made_frames = streamsref.CASES[name]()
    for k in streamsref.MODEL_KEYS:
        assert np.array_equal(model[k], made[k]), k
    assert np.array_equal(frames, made_frames)
    path = tmp_path / "hmmdefs"
    streamsref.write_streams_hmmdefs(path, model)
    live = streamsref.ref_scores(ref, path, frames)
    assert live.shape == scores.shape and np.array_equal(live, scores)


@pytest.mark.parametrize("name", streamsref.BINHMM_CASES)
def test_binhmm_round_trip_scores_the_same(ref, tmp_path, name):
    """write_binhmm() -> read_binhmm() of the reference: the binary file of the helper's hmmdefs scores as the ascii
    one (stream weights, shared `~p` macros, NULL densities and all)."""
    model, frames, scores = streamsref.load_case(name)
    path = tmp_path / "hmmdefs"
    streamsref.write_streams_hmmdefs(path, model)
    bpath = streamsref.write_binhmm(ref, path, tmp_path / "binhmm")
    assert np.array_equal(streamsref.ref_scores(ref, bpath, frames, nstate=scores.shape[1]), scores)


@pytest.mark.parametrize("name", streamsref.BINHMM_CASES)
def test_committed_binhmm_scores_the_same(ref, tmp_path, name):
    """The binary HMM files of the fixture (what the GPU machine's reader test reads) say what the arrays say."""
    model, frames, scores = streamsref.load_case(name)
    bpath = streamsref.load_binhmm(name, tmp_path / "binhmm")
    assert np.array_equal(streamsref.ref_scores(ref, bpath, frames, nstate=scores.shape[1]), scores)


def test_fixture_holds_every_branch_of_calc_mix():
    """The `branches` case does what its recipe says: a skipped stream changes a frame's scores without zeroing
    them, a frame with every stream skipped and a state with all weights 0 score LOG_ZERO, and a float64 restatement
    of calc_mix() agrees with the reference on every finite score."""
    m, fr, sc = streamsref.load_case("branches")
    assert (sc[5] == streamsref.LOG_ZERO).all()               # every stream skipped
    assert (sc[:, 5] == streamsref.LOG_ZERO).all()            # all weights 0
    assert (sc[4, :5] > streamsref.LOG_ZERO).all()            # one stream skipped, the others count
    assert not m["has_sw"][2] and (m["st_weight"][2] == 1.0).all()
    assert m["st_weight"][4, 1] == 0.0 and (m["ent_dens"] < 0).sum() == 1
    assert m["st_pdf"][1, 1] == m["st_pdf"][0, 1] and m["st_pdf"][4, 0] == m["st_pdf"][2, 0]
    soff = np.concatenate([[0], np.cumsum(m["vsize"])])
    want = np.empty(sc.shape)
    for t in range(sc.shape[0]):
        for s in range(sc.shape[1]):
            tot = 0.0
            for k in range(len(m["vsize"])):
                p = m["st_pdf"][s, k]
                x = fr[t, soff[k]:soff[k + 1]].astype(np.float64)
                terms = []
                for e in range(m["pdf_off"][p], m["pdf_off"][p + 1]):
                    g = m["ent_dens"][e]
                    if g < 0:
                        continue
                    a, b = m["dens_off"][g], m["dens_off"][g + 1]
                    terms.append(-0.5 * (float(m["gconst"][g]) + np.sum((x - m["mean"][a:b]) ** 2 * m["ivar"][a:b].astype(np.float64)))
                                 + float(m["ent_logw"][e]))
                lp = np.logaddexp.reduce(terms)
                if lp <= -1e6:
                    continue
                tot += lp * float(m["st_weight"][s, k])
            want[t, s] = -1e6 if tot == 0 or tot <= -1e6 else tot * 0.434294482
    # fp32 sums of at most 26 + 1 terms: 27 x 2^-24 = 1.6e-6 of the magnitude, twice (Gaussian, stream sum) and the
    # final product; the log-sum table's step is 3e-5 in the argument of a function of slope <= 0.5: 1.5e-5 a step,
    # at most 2 steps x 3 streams x weight 1.5 x .4343 = 6e-5
    assert (np.abs(want - sc) <= 4e-6 * np.abs(want) + 1e-4).all()
