"""GPU: the PULL form of K1's record-ring kernel (csrc/gmm_outprob.hip, gmm_tile_ring_kernel<.., PULL>; the deal in
csrc/gmm_deal.h) -- a launch of as many blocks as the device holds, whose waves draw (state range, 128-frame group) tiles
from eight ticket heads -- forced at small shapes by JAMD_GMM_PULL_MIN=0 (read when the model is created): 3, 5 and 9
frame groups, the last one partial, against 1 state, one range, a range and one state, 9 and 17 ranges (most shares
empty; a leftover range of one state; one and two full rounds), at 8 blocks (32 waves: several tickets per wave, fewer
waves than tiles at the larger shapes, shares that are stolen from), 16 blocks and the default capacity (nearly every
wave finds nothing).  The ring's state carried from one ticket to the next, the heads' reset between calls and between
models on one stream, and which calls take the form at all.

Every call scores into a device buffer pre-filled with NaN, so a tile that no wave took shows up, and the result is
bit-exact against the oracle."""
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


def forced(monkeypatch, grid):
    """The environment of a model that takes the pull form for every tile-kernel call, at `grid` blocks (None: capacity)."""
    monkeypatch.setenv("JAMD_GMM_PULL_MIN", "0")
    if grid is None:
        monkeypatch.delenv("JAMD_GMM_PULL_GRID", raising=False)
    else:
        monkeypatch.setenv("JAMD_GMM_PULL_GRID", str(grid))


def check_pull(kernel, grid):
    assert "gmm_tile<D=39" in kernel and ",ring,pull>" in kernel, kernel
    g = int(re.search(r"grid=(\d+)", kernel).group(1))
    assert g % 8 == 0 and (g == grid if grid else g >= 8), kernel


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


@pytest.mark.parametrize("grid", [8, 16, None])
@pytest.mark.parametrize("T", [257, 513, 1100])              # 3, 5, 9 frame groups, the last one partial
@pytest.mark.parametrize("S", [1, 16, 17, 129, 257])         # 1, 1, 2, 9, 17 state ranges
def test_ranges_groups_and_grids(engine, oracle, monkeypatch, S, T, grid):
    m, fr, want = shape(oracle, S, T)
    forced(monkeypatch, grid)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    check_pull(kernel, grid)
    assert not np.isnan(got).any(), np.argwhere(np.isnan(got))[:4]
    assert np.array_equal(got, want)


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


@pytest.mark.parametrize("null", [False, True])
def test_ring_state_carried_over_tickets(engine, oracle, monkeypatch, null):
    """Empty and one-Gaussian states between full ones, without and with NULL densities (the HAS_NULL instantiation), at
    8 blocks: 45 tiles over 32 waves, so waves go from a tile of one range to a tile of another with `held` naming
    the record the homes were left with."""
    def make():
        m = carry_model(null)
        return m, synth.make_frames(m, T=1100, seed=5)
    m, fr, want = case(oracle, ("carry", null), make)
    forced(monkeypatch, 8)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    check_pull(kernel, 8)
    assert not np.isnan(got).any(), np.argwhere(np.isnan(got))[:4]
    assert np.array_equal(got, want)


def test_heads_reset_between_calls_and_models(engine, oracle, monkeypatch):
    """Two calls on one model give the same bytes, and two models used alternately on one stream each find their own
    heads at zero."""
    ma, fa, wa = shape(oracle, 129, 1100)
    mb, fb, wb = shape(oracle, 257, 513)
    forced(monkeypatch, 8)
    ga, gb = lib.Gmm(engine, ma), lib.Gmm(engine, mb)
    first = score_into_nan(engine, ga, fa)
    second = score_into_nan(engine, ga, fa)
    assert np.array_equal(first, wa) and first.tobytes() == second.tobytes()
    for _ in range(2):
        assert np.array_equal(score_into_nan(engine, gb, fb), wb)
        assert np.array_equal(score_into_nan(engine, ga, fa), wa)
    check_pull(ga.last_kernel(), 8)
    check_pull(gb.last_kernel(), 8)
    ga.close()
    gb.close()


def test_which_calls_take_the_pull_form(engine, oracle, monkeypatch):
    """Unforced, a call whose blocks fit the device at once keeps the block form and its kernel string; a negative
    JAMD_GMM_PULL_MIN switches the pull form off; forced, a call of at most 256 frames still goes to K1n."""
    m, fr, want = shape(oracle, 129, 513)
    monkeypatch.delenv("JAMD_GMM_PULL_MIN", raising=False)
    monkeypatch.delenv("JAMD_GMM_PULL_GRID", raising=False)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    assert kernel == "gmm_tile<D=39,FPL=2,NS=16,ring> grid=24 nsb=16", kernel     # 8 x 2 pinned blocks + 2 dealt over 8
    assert np.array_equal(got, want)

    monkeypatch.setenv("JAMD_GMM_PULL_MIN", "-1")
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    assert ",ring>" in kernel and "pull" not in kernel, kernel
    assert np.array_equal(got, want)

    forced(monkeypatch, None)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr[:200])
    kernel = gm.last_kernel()
    gm.close()
    assert "gmm_narrow<D=39>" in kernel, kernel
    assert np.array_equal(got, want[:200])
