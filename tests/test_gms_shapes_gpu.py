"""GPU: Gaussian mixture selection (gms_select_kernel / gms_combine_kernel behind lib.Gms) against oracle.gms_apply(),
bit for bit and in both forms (set_strict_order(False / True)), at the shapes the golden fixture of test_gms_gpu.py
does not reach: mixture counts that enter the four-wide maximum loop, a tie inside a state, the LOG_ZERO floor and
NULL densities, the edges of the four-wide ranking loop, empty and one-frame utterances, LDS requests beyond 48 KB
and beyond the kernel's limit, other vector lengths, scratch buffers that grow between calls, a caller's stream and
the frame stride of the combining kernel.

Every case also checks its own inputs with the numpy restatements of densref.py: that the oracle's replaced scores
are the selection states' scores computed there, that no two selection states tie on the nbest boundary (only then
must the ranking form equal the reference's heap) and, where it is the point of the case, that the winners really
fall where the four-wide loop could go wrong."""
import ctypes as C

import numpy as np
import pytest

from densref import (LOG_ZERO, boundary_is_untied, dens_ref, gmax_winners, gms_state_scores,
                     visiting_order_covered)
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu


def make_map(Sgs, S, seed):
    """state2gs of S real states: about a sixth unmapped (-1), the rest spread over the selection states so that
    every selection state serves a real state whenever S allows and most serve several."""
    rng = np.random.default_rng(seed)
    s2g = rng.integers(0, Sgs, S).astype(np.int32)
    k = min(Sgs, S)
    s2g[:k] = rng.permutation(Sgs)[:k]
    s2g[rng.random(S) < 1 / 6] = -1
    if S > 1:
        s2g[-1] = -1
    return s2g[rng.permutation(S)]


def make_inputs(Sgs, M, D=39, T=40, seed=0, ragged=False, null_frac=0.0, S=None, noise=1.0):
    """(selection model, state2gs, frames, model of the real states)."""
    gs = synth.make_gmm(S=Sgs, M=M, D=D, seed=seed, ragged=ragged, null_frac=null_frac)
    S = S if S is not None else 2 * Sgs + 5
    fr = synth.make_frames(gs, T=T, seed=seed + 1, noise=noise)
    return gs, make_map(Sgs, S, seed + 2), fr, synth.make_gmm(S=S, M=2, D=D, seed=seed + 3)


def lds_bytes(Sgs, Egs):
    """The dynamic LDS jamd_gms_apply_dev() asks for: fs, idx, last [Sgs] each, st_off [Sgs + 1], logw [Egs], 64 floats
    of alignment slack and two rows of Egs rounded up to 64."""
    pad = (Egs + 63) & ~63
    return 4 * (3 * Sgs + Sgs + 1 + Egs + 64 + 2 * pad)


def utterances(utt_off, T):
    off = [0, T] if utt_off is None else [int(x) for x in utt_off]
    return [(a, b) for a, b in zip(off[:-1], off[1:]) if b > a]


def expected(oracle, gs, s2g, nbest, fr, real, utt_off=None):
    """The oracle utterance by utterance, after the checks of the inputs that every case shares.  Returns
    (want, dens, fs): the expected scores, the per-Gaussian scores and the selection states' scores."""
    T = len(fr)
    want = real.copy()
    for a, b in utterances(utt_off, T):
        want[a:b] = oracle.gms_apply(dict(model=gs, state2gs=s2g, nbest=nbest), fr[a:b], real[a:b])
    dens = dens_ref(gs, fr)
    fs = gms_state_scores(gs, dens, utt_off)
    assert boundary_is_untied(fs, nbest)
    mapped = s2g >= 0
    assert np.array_equal(want[:, ~mapped], real[:, ~mapped])
    by_state = fs[:, np.maximum(s2g, 0)]
    replaced = (want != real) & mapped[None, :]
    assert np.array_equal(want[replaced], by_state[replaced])   # the oracle and the numpy restatement agree on fs
    if nbest >= len(gs["st_off"]) - 1:
        assert not replaced.any()
    return want, dens, fs


def check_both_forms(engine, gs, s2g, nbest, fr, real, want, utt_off=None):
    for strict in (False, True):
        stage = lib.Gms(engine, gs, s2g, nbest).set_strict_order(strict)
        got = stage.apply_host(fr, real, utt_off)
        stage.close()
        assert np.array_equal(got, want), f"strict={strict}"


def real_scores(engine, real_model, fr):
    g = lib.Gmm(engine, real_model)
    out = g.outprob_host(fr)
    g.close()
    return out


MIXTURE_CASES = [(1, False), (2, False), (3, False), (4, False), (5, False), (7, False), (8, False), (16, False),
                 (64, False), (20, True)]


def mixture_inputs(M, ragged):
    gs, s2g, fr, rm = make_inputs(70, M, T=120, seed=100 + M, ragged=ragged)
    return gs, s2g, fr, rm, np.array([0, 37, 80, 120], np.int32)


@pytest.mark.parametrize("M,ragged", MIXTURE_CASES)
def test_mixture_counts(engine, oracle, M, ragged):
    """Sgs = 70 states of M Gaussians (ragged: 1 to 20), 120 frames in three utterances.  From M = 4 on the four-wide
    loop of the maximum runs, with a scalar tail unless M % 4 == 0; the winners of one state fall in every class of
    (n - 1 - k) % 4 that M leaves, in the groups of four and in the tail, and change between frames."""
    gs, s2g, fr, rm, utt_off = mixture_inputs(M, ragged)
    n = np.diff(gs["st_off"])
    assert (n.min(), n.max()) == ((1, 20) if ragged else (M, M))
    real = real_scores(engine, rm, fr)
    want, dens, _ = expected(oracle, gs, s2g, 12, fr, real, utt_off)
    assert 0.0 < (want != real).mean() < 1.0
    win, _ = gmax_winners(gs["st_off"], dens, utt_off)
    residues, changed, in_body, in_tail = visiting_order_covered(gs["st_off"], win, utt_off)
    assert residues == set(range(min(M, 4)))
    assert changed == (M > 1) and in_body == (M >= 4) and in_tail == (ragged or M % 4 != 0)
    check_both_forms(engine, gs, s2g, 12, fr, real, want, utt_off)


def tie_inputs():
    """Eight selection states; in six of them two entries are one Gaussian under two weights, placed at the state's
    centre so that the pair is often the state's best.  The four-wide loop holds entry k of a state of n at place
    (n - 1 - k) % 4 of a group; the pairs put their lower entry -- the one a wrong comparison would let win -- at each
    of the four places and in the scalar tail, with its twin in the same group, four entries above it, or across
    the border between the groups and the tail (state 2 has six entries: one group and a tail of two)."""
    gs, s2g, fr, rm = make_inputs(8, 8, T=90, seed=48, S=26)
    gs = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in gs.items()}
    gs["st_off"] = np.array([0, 8, 16, 22, 30, 38, 46, 54, 62], np.int32)   # state 2 gives up its last two entries
    keep = np.r_[0:22, 24:64]
    gs["ent_dens"], gs["ent_logw"] = gs["ent_dens"][keep], gs["ent_logw"][keep]
    pairs = {0: (5, 6), 1: (1, 5), 2: (1, 4), 3: (3, 7), 4: (6, 7), 5: (0, 2)}
    n = np.diff(gs["st_off"])
    assert sorted((int(n[i]) - 1 - a) % 4 if a >= n[i] % 4 else -1 for i, (a, _) in pairs.items()) == [-1, 0, 1, 2, 2, 3]
    for i, (a, b) in pairs.items():
        da, db = gs["ent_dens"][gs["st_off"][i] + a], gs["ent_dens"][gs["st_off"][i] + b]
        gs["mean"][da] = gs["centre"][i]
        for k in ("mean", "ivar", "gconst"):
            gs[k][db] = gs[k][da]
        assert gs["ent_logw"][gs["st_off"][i] + a] != gs["ent_logw"][gs["st_off"][i] + b]
    return gs, s2g, fr, rm, pairs


def test_tie_inside_a_state(engine, oracle):
    """Two entries of a state that score the same on every frame: compute_g_max() keeps the one it visits first, the
    higher index (and, once that one has won, visits it first of all on the next frame).  Which of the two wins shows
    in the state's score through the winner's weight, so the frames are run as one utterance and the expected
    scores are shown to be those of the higher entry and not those of the lower."""
    gs, s2g, fr, rm, pairs = tie_inputs()
    real = real_scores(engine, rm, fr)
    want, dens, fs = expected(oracle, gs, s2g, 2, fr, real)
    win, _ = gmax_winners(gs["st_off"], dens)
    other = win.copy()
    for i, (a, b) in pairs.items():
        e0 = int(gs["st_off"][i])
        assert np.array_equal(dens[:, e0 + a], dens[:, e0 + b])
        assert not (win[:, i] == a).any()                       # the lower entry of a pair never wins ...
        at = win[:, i] == b
        other[at, i] = a                                        # ... and this is what the score would be if it did
    fs_other = gms_state_scores(gs, dens, win=other)
    for i in pairs:
        col = int(np.nonzero(s2g == i)[0][0])
        shows = (win[:, i] == pairs[i][1]) & (want[:, col] != real[:, col])
        assert shows.sum() >= 5                                  # frames on which the state's score is in the output
        assert np.array_equal(want[shows, col], fs[shows, i]) and (fs[shows, i] != fs_other[shows, i]).all()
    check_both_forms(engine, gs, s2g, 2, fr, real, want)


def log_zero_inputs():
    """Narrow Gaussians (variances / 400) in every third state, every second frame scaled by 50: all Gaussians of such
    a state then lie below LOG_ZERO.  Every fourth state ends in a NULL density -- the first entry visited on an
    utterance's first frame -- and state 5 holds nothing but NULL densities."""
    gs, s2g, fr, rm = make_inputs(24, 6, T=64, seed=77, ragged=True, null_frac=0.1)
    gs = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in gs.items()}
    fr = fr.copy()
    fr[::2] *= 50.0
    for i in range(0, 24, 3):
        d = gs["ent_dens"][gs["st_off"][i]:gs["st_off"][i + 1]]
        d = d[d >= 0]
        var = (gs["var"][d] / np.float32(400.0)).astype(np.float32)
        gs["var"][d], gs["ivar"][d] = var, (1.0 / var.astype(np.float64)).astype(np.float32)
        gs["gconst"][d] = synth.gconst_of(var)
    null = [int(gs["st_off"][i + 1]) - 1 for i in range(1, 24, 4) if gs["st_off"][i + 1] - gs["st_off"][i] > 1]
    null += list(range(int(gs["st_off"][5]), int(gs["st_off"][6])))
    gs["ent_dens"][null] = -1
    gs["ent_logw"][null] = LOG_ZERO
    return gs, s2g, fr, rm, np.array([0, 21, 42, 64], np.int32)


def test_log_zero_floor_and_null_densities(engine, oracle):
    gs, s2g, fr, rm, utt_off = log_zero_inputs()
    real = real_scores(engine, rm, fr)
    for nbest in (3, 20):
        want, dens, fs = expected(oracle, gs, s2g, nbest, fr, real, utt_off)
        live = [i for i in range(24) if (gs["ent_dens"][gs["st_off"][i]:gs["st_off"][i + 1]] >= 0).all()]
        below = np.array([(dens[:, gs["st_off"][i]:gs["st_off"][i + 1]] < LOG_ZERO).all(axis=1) for i in live])
        assert below.any() and not below.all()                  # a state of real Gaussians, all of them under the floor
        assert (gs["ent_dens"][gs["st_off"][1:] - 1] < 0).sum() >= 3
        assert np.isfinite(fs).all() and (fs[:, 5] == fs[0, 5]).all()
        check_both_forms(engine, gs, s2g, nbest, fr, real, want, utt_off)


@pytest.mark.parametrize("Sgs", [1, 3, 63, 64, 65, 66, 67, 129, 256])
def test_selection_shapes(engine, oracle, Sgs):
    """The ranking loop reads fs four at a time with a scalar tail (Sgs % 4 entries) and every lane takes the states
    lane, lane + 64, ...: one pass up to 64 states, a ragged last pass beyond.  nbest at both ends."""
    gs, s2g, fr, rm = make_inputs(Sgs, 2, T=24, seed=200 + Sgs)
    real = real_scores(engine, rm, fr)
    for nbest in sorted({nb for nb in (1, Sgs - 1, Sgs, Sgs + 5) if nb >= 1}):
        want, _, _ = expected(oracle, gs, s2g, nbest, fr, real)
        if nbest >= Sgs:
            assert np.array_equal(want, real)
        else:
            assert (want != real).any()
        check_both_forms(engine, gs, s2g, nbest, fr, real, want)


def test_utterance_layout(engine, oracle):
    """Empty utterances first, in the middle and last, and one of a single frame: the batch equals its utterances run
    one by one, and the oracle."""
    gs, s2g, fr, rm = make_inputs(20, 5, T=50, seed=41, ragged=True)
    utt_off = np.array([0, 0, 1, 18, 18, 19, 50, 50], np.int32)
    real = real_scores(engine, rm, fr)
    want, _, _ = expected(oracle, gs, s2g, 4, fr, real, utt_off)
    check_both_forms(engine, gs, s2g, 4, fr, real, want, utt_off)
    for strict in (False, True):
        stage = lib.Gms(engine, gs, s2g, 4).set_strict_order(strict)
        for a, b in utterances(utt_off, 50):
            assert np.array_equal(stage.apply_host(fr[a:b], real[a:b]), want[a:b])


LDS_LIMIT = 159 * 1024


def _first_refused_sgs(M=64):
    return next(s for s in range(1, 4096) if lds_bytes(s, s * M) > LDS_LIMIT)


@pytest.mark.parametrize("Sgs", [62, 63, 65, 129, _first_refused_sgs() - 1])
def test_lds_up_to_the_limit(engine, oracle, Sgs):
    """64 Gaussians per state.  62 states are the last request within 48 KB and 63 the first beyond, where the kernel's
    attribute has to be raised; 65 states (a second pass of the lanes as well) and 129 states, about 100 KB, are
    models of the real size, and 207 states are the largest model of this shape within the kernel's limit."""
    Egs = Sgs * 64
    assert lds_bytes(62, 62 * 64) <= 48 * 1024 < lds_bytes(63, 63 * 64)
    assert lds_bytes(Sgs, Egs) <= LDS_LIMIT and (Sgs != 129 or lds_bytes(Sgs, Egs) > 96 * 1024)
    gs, s2g, fr, rm = make_inputs(Sgs, 64, T=40, seed=300 + Sgs, S=150)
    real = real_scores(engine, rm, fr)
    utt_off = np.array([0, 17, 40], np.int32)
    want, _, _ = expected(oracle, gs, s2g, 10, fr, real, utt_off)
    assert (want != real).any()
    check_both_forms(engine, gs, s2g, 10, fr, real, want, utt_off)


def test_lds_refusal(engine, oracle):
    """The smallest 64-Gaussian model whose request passes the kernel's 159 KB is refused, not launched, and the engine
    goes on serving a small model."""
    Sgs = _first_refused_sgs()
    assert Sgs == 208 and lds_bytes(Sgs - 1, (Sgs - 1) * 64) <= LDS_LIMIT < lds_bytes(Sgs, Sgs * 64)
    gs, s2g, fr, rm = make_inputs(Sgs, 64, T=4, seed=5, S=30)
    real = real_scores(engine, rm, fr)
    for strict in (False, True):
        stage = lib.Gms(engine, gs, s2g, 10).set_strict_order(strict)
        with pytest.raises(lib.JamdError, match=r"\(-1\).*208 states / 13312 Gaussians does not fit in LDS"):
            stage.apply_host(fr, real)
    gs, s2g, fr, rm = make_inputs(9, 3, T=12, seed=6)
    real = real_scores(engine, rm, fr)
    want, _, _ = expected(oracle, gs, s2g, 2, fr, real)
    check_both_forms(engine, gs, s2g, 2, fr, real, want)


@pytest.mark.parametrize("D", [13, 25, 60])
def test_vector_lengths(engine, oracle, D):
    gs, s2g, fr, rm = make_inputs(20, 5, D=D, T=30, seed=50 + D, ragged=True)
    real = real_scores(engine, rm, fr)
    want, _, _ = expected(oracle, gs, s2g, 5, fr, real)
    assert (want != real).any()
    check_both_forms(engine, gs, s2g, 5, fr, real, want)


@pytest.mark.parametrize("strict", [False, True])
def test_scratch_reuse_and_callers_stream(engine, oracle, strict):
    """One stage at T = 10, 700 and 10 again (its scratch buffers grow, then serve a smaller call), then through
    jamd_gms_apply_dev() on a stream and device buffers of the caller's."""
    gs, s2g, fr, rm = make_inputs(20, 4, T=700, seed=61)
    real = real_scores(engine, rm, fr)
    stage = lib.Gms(engine, gs, s2g, 6).set_strict_order(strict)
    for T, utt_off in ((10, None), (700, np.array([0, 300, 301, 700], np.int32)), (10, None)):
        want, _, _ = expected(oracle, gs, s2g, 6, fr[:T], real[:T], utt_off)
        assert np.array_equal(stage.apply_host(fr[:T], real[:T], utt_off), want)
    T, utt_off = 130, np.array([0, 60, 130], np.int32)
    want = stage.apply_host(fr[:T], real[:T], utt_off)
    assert np.array_equal(want, expected(oracle, gs, s2g, 6, fr[:T], real[:T], utt_off)[0])
    d_fr = lib.DevBuf(engine, fr[:T].nbytes).upload(fr[:T])
    d_sc = lib.DevBuf(engine, real[:T].nbytes).upload(real[:T])
    s = C.c_void_p()
    assert lib.load().jamd_stream_create(engine.h, C.byref(s)) == 0
    try:
        stage.apply_dev(d_fr.ptr, T, d_sc.ptr, utt_off, stream=s.value)
        assert lib.load().jamd_stream_sync(engine.h, s) == 0
    finally:
        lib.load().jamd_stream_destroy(engine.h, s)
    assert np.array_equal(d_sc.download((T, len(s2g)), np.float32), want)


@pytest.mark.parametrize("S", [257, 1000])
def test_combine_many_states_and_frames(engine, oracle, S):
    """gms_combine_kernel: more real states than one block of 256 and more frames than the 1024 its grid spans, so
    that a block walks on to frame t + gridDim.y.  Every unmapped column comes back as it went in."""
    gs, s2g, fr, rm = make_inputs(10, 2, T=1100, seed=70 + S, S=S)
    rm = synth.make_gmm(S=S, M=1, D=39, seed=71)
    real = real_scores(engine, rm, fr)
    utt_off = np.array([0, 500, 1100], np.int32)
    want, _, _ = expected(oracle, gs, s2g, 3, fr, real, utt_off)
    assert (s2g < 0).sum() > 10 and (want[1024:] != real[1024:]).any()
    for strict in (False, True):
        got = lib.Gms(engine, gs, s2g, 3).set_strict_order(strict).apply_host(fr, real, utt_off)
        assert np.array_equal(got[:, s2g < 0], real[:, s2g < 0])
        assert np.array_equal(got, want)
