"""GPU: K1's record ring (csrc/gmm_outprob.hip, gmm_tile_ring_kernel) -- the D = 39 tile kernel that keeps the next
Gaussian's record in flight while it works on this one -- at the shapes where the ring can go wrong: states of one, two
and three Gaussians (the prologue alone, the re-read in a block's last state, the hand-over to the next state's last
entry), empty states, the first and last record of a model, the ends of a block's state range, partial waves and
blocks, NULL densities at either end of a state, repeated calls and two models at once.  Bit-exact against the oracle
and the compiled reference's golden scores; every call is long enough (T >= 257) to take the tile kernel."""
import numpy as np
import pytest

from conftest import GOLDEN
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu


def with_counts(m, counts):
    """The model m (every state M Gaussians) cut down to counts[s] mixture entries in state s."""
    counts = np.asarray(counts)
    assert len(counts) == len(m["st_off"]) - 1 and (counts <= np.diff(m["st_off"])).all()
    idx = np.concatenate([np.arange(m["st_off"][s], m["st_off"][s] + n) for s, n in enumerate(counts)]).astype(np.int64)
    out = dict(m)
    out["st_off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out["ent_dens"], out["ent_logw"] = m["ent_dens"][idx].copy(), m["ent_logw"][idx].copy()
    return out


def ring_scores(engine, m, fr):
    gm = lib.Gmm(engine, m)
    got = gm.outprob_host(fr)
    assert "gmm_tile<D=39" in gm.last_kernel() and ",ring>" in gm.last_kernel(), gm.last_kernel()
    gm.close()
    return got


COUNTS = {
    # 20 states = one block of 16 and one of 4; a block that begins and one that ends with a single Gaussian
    "1_2_3_beside_16": [1, 2, 3, 16, 1, 1, 2, 16, 3, 3, 16, 2, 1, 16, 16, 1, 3, 16, 2, 1],
    "all_single": [1] * 18,
    "block_ends_on_16_next_begins_on_2": [16] * 16 + [2, 3],
    # empty states: behind one the ring holds another record than the state's last one
    "empty_states": [0, 3, 0, 0, 16, 1, 0, 2, 16, 0, 1, 1, 0, 16, 2, 0, 0, 1, 0],
}


@pytest.mark.parametrize("name", list(COUNTS))
def test_mixture_counts(engine, oracle, name):
    counts = COUNTS[name]
    m = with_counts(synth.make_gmm(S=len(counts), M=16, D=39, seed=11), counts)
    fr = synth.make_frames(m, T=257, seed=12)
    assert np.array_equal(ring_scores(engine, m, fr), oracle.gmm_outprob(m, fr))


@pytest.mark.parametrize("T", [257, 385, 513])      # a partial wave; a block less a wave; a block and one frame
@pytest.mark.parametrize("S", [1, 16, 17, 33])      # one state; one full block; a block and one state; two and one
def test_states_and_frames(engine, oracle, S, T):
    m = synth.make_gmm(S=S, M=16, D=39, seed=100 + S, ragged=(S == 33))
    fr = synth.make_frames(m, T=T, seed=T)
    got = ring_scores(engine, m, fr)
    assert got.shape == (T, S)
    assert np.array_equal(got, oracle.gmm_outprob(m, fr))


@pytest.mark.parametrize("ragged", [False, True])
def test_null_densities(engine, oracle, ragged):
    """The HAS_NULL instantiation: NULL densities scattered by the generator (never a state's first entry) and placed by
    hand at a state's last entry, at a state's first entry, and as the whole of a one-entry state."""
    m = synth.make_gmm(S=21, M=16, D=39, seed=31, ragged=ragged, null_frac=0.1)
    if not ragged:
        m = with_counts(m, [16, 16, 1, 16, 2, 3] + [16] * 15)
    m["ent_dens"] = m["ent_dens"].copy()
    so = m["st_off"]
    m["ent_dens"][so[1] - 1] = -1       # last entry of state 0: the first record the block reads
    m["ent_dens"][so[3]] = -1           # first entry of state 3: handed over to state 4's last entry
    m["ent_dens"][so[16] - 1] = -1      # last entry of the block's last state (the re-read)
    if not ragged:
        m["ent_dens"][so[2]] = -1       # a one-entry state that is a NULL density: LOG_ZERO
    fr = synth.make_frames(m, T=300, seed=32)
    want = oracle.gmm_outprob(m, fr)
    if not ragged:
        assert (want[:, 2] == np.float32(-1000000.0)).all()
    assert np.array_equal(ring_scores(engine, m, fr), want)


def test_golden_plain_through_the_ring(engine):
    """The compiled reference's golden scores (40 frames, 24 states x 8 Gaussians), the frames repeated to a tile-kernel call."""
    z = np.load(GOLDEN / "gmm_plain_none.npz")
    g = {k: z[k] for k in z.files}
    g["nbook"], g["st_book"] = 0, None
    T = len(g["frames"])
    reps = 7
    got = ring_scores(engine, g, np.tile(g["frames"], (reps, 1)))
    for r in range(reps):
        assert np.array_equal(got[r * T:(r + 1) * T], g["out"])


def test_repeated_calls_and_two_models(engine, oracle):
    """Three calls on the same input give the same floats (a home copied before its load has landed would not, every
    time), and two models alive at once keep their own ring copies whichever is destroyed first."""
    ma = with_counts(synth.make_gmm(S=35, M=16, D=39, seed=41), ([16, 1, 2, 3, 16] * 7))
    mb = synth.make_gmm(S=19, M=16, D=39, seed=42, ragged=True, null_frac=0.05)
    fa, fb = synth.make_frames(ma, T=513, seed=43), synth.make_frames(mb, T=385, seed=44)
    wa, wb = oracle.gmm_outprob(ma, fa), oracle.gmm_outprob(mb, fb)
    for first in ("a", "b"):
        ga, gb = lib.Gmm(engine, ma), lib.Gmm(engine, mb)
        for _ in range(3):
            assert np.array_equal(ga.outprob_host(fa), wa)
            assert np.array_equal(gb.outprob_host(fb), wb)
        assert ",ring>" in ga.last_kernel() and ",ring>" in gb.last_kernel()
        if first == "a":
            ga.close()
            assert np.array_equal(gb.outprob_host(fb), wb)
            gb.close()
        else:
            gb.close()
            assert np.array_equal(ga.outprob_host(fa), wa)
            ga.close()


@pytest.mark.parametrize("D", [38, 26, 25, 13])
def test_other_vector_lengths_keep_their_kernel(engine, oracle, D):
    """Only D = 39 has a ring copy; the other templated lengths and the generic-D kernel score as before."""
    m = synth.make_gmm(S=20, M=7, D=D, seed=50 + D, ragged=True, null_frac=0.05)
    fr = synth.make_frames(m, T=300, seed=D)
    gm = lib.Gmm(engine, m)
    got = gm.outprob_host(fr)
    assert ("gmm_tile_generic<" if D == 13 else f"gmm_tile<D={D},") in gm.last_kernel() and "ring" not in gm.last_kernel()
    assert np.array_equal(got, oracle.gmm_outprob(m, fr))


def test_golden_ragged_at_tile_length(engine):
    """The ragged golden model with NULL densities (D = 25), its 33 frames repeated to a tile-kernel call."""
    z = np.load(GOLDEN / "gmm_ragged.npz")
    g = {k: z[k] for k in z.files}
    g["nbook"], g["st_book"] = 0, None
    T = len(g["frames"])
    gm = lib.Gmm(engine, g)
    got = gm.outprob_host(np.tile(g["frames"], (9, 1)))
    assert "gmm_tile<D=25," in gm.last_kernel()
    for r in range(9):
        assert np.array_equal(got[r * T:(r + 1) * T], g["out"])
