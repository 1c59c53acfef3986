"""GPU: the fine-grained tail of K1's pull form (csrc/gmm_outprob.hip, gmm_tile_ring_kernel<.., PULL>; the deal in
csrc/gmm_deal.h, gd_tail_ticket) -- the last JAMD_GMM_PULL_TAIL tiles of every share are drawn in pieces of
JAMD_GMM_PULL_SUB states, so a ticket names its own first state and state count.  The form is forced at small shapes by
JAMD_GMM_PULL_MIN=0 (all three switches are read when the model is created): 8, 16 blocks and the default capacity;
1, 3, 4, 5 states (a range shorter than one piece, a ragged piece, empty pieces behind the model's end), 16, 17, 20 and
129 states; 3, 5 and 9 frame groups, the last one partial; no tail, one tile per share, and every tile in pieces; pieces
of 2 and 8 states; the 65-state model whose empty and one-Gaussian states make the ring's `held` cross piece boundaries,
without and with NULL densities; two calls and two models in a row.

Every call scores into a device buffer pre-filled with NaN, so a (state, frame) that no wave took shows up, and the
result is bit-exact against the oracle."""
import re

import numpy as np
import pytest

from julius_amd import lib, synth

pytestmark = pytest.mark.gpu


def score_into_nan(engine, gm, fr):
    """gm.outprob_dev() of the frames into a [T][S] device buffer that holds NaN everywhere before the call."""
    T = len(fr)
    d_fr = lib.DevBuf(engine, fr.nbytes).upload(fr)
    d_out = lib.DevBuf(engine, 4 * T * gm.S).upload(np.full((T, gm.S), np.nan, np.float32))
    gm.outprob_dev(d_fr.ptr, T, d_out.ptr)
    engine.sync()
    got = d_out.download((T, gm.S), np.float32)
    d_fr.free()
    d_out.free()
    return got


def with_counts(m, counts):
    """The model m (every state M Gaussians) cut down to counts[s] mixture entries in state s."""
    counts = np.asarray(counts)
    assert len(counts) == len(m["st_off"]) - 1 and (counts <= np.diff(m["st_off"])).all()
    idx = np.concatenate([np.arange(m["st_off"][s], m["st_off"][s] + n) for s, n in enumerate(counts)]).astype(np.int64)
    out = dict(m)
    out["st_off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out["ent_dens"], out["ent_logw"] = m["ent_dens"][idx].copy(), m["ent_logw"][idx].copy()
    return out


def forced(monkeypatch, grid, tail, sub=None):
    """The environment of a model that takes the pull form for every tile-kernel call, at `grid` blocks (None: capacity),
    with `tail` tiles per share in pieces (None: the default) of `sub` states (None: the default)."""
    monkeypatch.setenv("JAMD_GMM_PULL_MIN", "0")
    for name, value in (("JAMD_GMM_PULL_GRID", grid), ("JAMD_GMM_PULL_TAIL", tail), ("JAMD_GMM_PULL_SUB", sub)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def check_tail(kernel, grid, tail, sub=None):
    """The kernel string of a pull launch: the grid, and the tail as `tail=<tiles>x<states>`."""
    assert "gmm_tile<D=39" in kernel and ",ring,pull>" in kernel, kernel
    g = int(re.search(r"grid=(\d+)", kernel).group(1))
    assert g % 8 == 0 and (g == grid if grid else g >= 8), kernel
    m = re.search(r" tail=(\d+)x(\d+)$", kernel)
    assert m, kernel
    assert int(m.group(1)) == (tail if tail is not None else 2 * (4 * g // 8)), kernel
    assert int(m.group(2)) == (sub or 4), kernel


_CASES = {}


def case(oracle, key, make):
    """Model, frames and the oracle's scores of one shape, computed once."""
    if key not in _CASES:
        m, fr = make()
        want = oracle.gmm_outprob(m, fr)
        want.setflags(write=False)
        _CASES[key] = (m, fr, want)
    return _CASES[key]


def shape(oracle, S, T):
    def make():
        small = S < 128
        m = synth.make_gmm(S=S, M=16 if small else 4, D=39, seed=S + 39, ragged=small)
        return m, synth.make_frames(m, T=T, seed=T)
    return case(oracle, (S, T), make)


def run(engine, monkeypatch, m, fr, want, grid, tail, sub=None):
    forced(monkeypatch, grid, tail, sub)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    check_tail(kernel, grid, tail, sub)
    assert not np.isnan(got).any(), np.argwhere(np.isnan(got))[:4]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("tail", [0, 1, 1000])                # none, one tile per share, every tile in quarters
@pytest.mark.parametrize("grid", [8, 16, None])
@pytest.mark.parametrize("T", [257, 513, 1100])               # 3, 5, 9 frame groups, the last one partial
@pytest.mark.parametrize("S", [1, 3, 4, 5, 16, 17, 20, 129])
def test_states_groups_grids_and_tails(engine, oracle, monkeypatch, S, T, grid, tail):
    m, fr, want = shape(oracle, S, T)
    run(engine, monkeypatch, m, fr, want, grid, tail)


@pytest.mark.parametrize("sub", [2, 8])
@pytest.mark.parametrize("tail", [1, 1000])
def test_pieces_of_two_and_eight_states(engine, oracle, monkeypatch, sub, tail):
    """129 states x 1100 frames (81 tiles; a last range of one state: seven or one empty pieces) and 5 states x 513 at
    8 blocks."""
    for S, T in ((129, 1100), (5, 513)):
        m, fr, want = shape(oracle, S, T)
        run(engine, monkeypatch, m, fr, want, 8, tail, sub)


def test_default_tail(engine, oracle, monkeypatch):
    """No switch but the forcing one: twice as many tiles per share as wave slots start on it, in quarters."""
    m, fr, want = shape(oracle, 129, 1100)
    run(engine, monkeypatch, m, fr, want, None, None)
    run(engine, monkeypatch, m, fr, want, 16, None)


def carry_model(null):
    counts = [16, 0, 1, 3, 16] * 13                           # 65 states: 5 ranges, the last of one state
    m = with_counts(synth.make_gmm(S=len(counts), M=16, D=39, seed=77, null_frac=0.15 if null else 0.0), counts)
    if null:
        m["ent_dens"] = m["ent_dens"].copy()
        so = m["st_off"]
        m["ent_dens"][so[16] - 1] = -1                        # the last record of the first range (a tile's re-read)
        m["ent_dens"][so[18] - 1] = -1                        # the whole of a one-entry state
        assert (m["ent_dens"] < 0).sum() > 10
    return m


@pytest.mark.parametrize("tail,sub", [(1, 4), (1000, 4), (1000, 2), (1000, 8)])
@pytest.mark.parametrize("null", [False, True])
def test_ring_state_carried_over_pieces(engine, oracle, monkeypatch, null, tail, sub):
    """Empty and one-Gaussian states between full ones, without and with NULL densities (the HAS_NULL instantiation), at
    8 blocks: a wave goes from a piece to the next piece, to another tile or to another range with `held` naming the
    record the homes were left with; pieces begin and end on empty states and on one-Gaussian states."""
    def make():
        m = carry_model(null)
        return m, synth.make_frames(m, T=1100, seed=5)
    m, fr, want = case(oracle, ("carry", null), make)
    run(engine, monkeypatch, m, fr, want, 8, tail, sub)


def test_heads_reset_between_calls_and_models(engine, oracle, monkeypatch):
    """Two calls on one model give the same bytes, and two models used alternately on one stream each find their own
    heads at zero -- with tails, the heads run further than the tiles."""
    ma, fa, wa = shape(oracle, 129, 1100)
    mb, fb, wb = shape(oracle, 20, 513)
    forced(monkeypatch, 8, 1000)
    ga = lib.Gmm(engine, ma)
    forced(monkeypatch, 8, 1)
    gb = lib.Gmm(engine, mb)
    first = score_into_nan(engine, ga, fa)
    second = score_into_nan(engine, ga, fa)
    assert np.array_equal(first, wa) and first.tobytes() == second.tobytes()
    for _ in range(2):
        assert np.array_equal(score_into_nan(engine, gb, fb), wb)
        assert np.array_equal(score_into_nan(engine, ga, fa), wa)
    check_tail(ga.last_kernel(), 8, 1000)
    check_tail(gb.last_kernel(), 8, 1)
    ga.close()
    gb.close()
