"""GPU: which (state range, frame block) a block index names (csrc/gmm_dev.h, decode_block() / xcd_grid()) -- the full
rounds of eight ranges pinned to one XCD each, the blocks of the leftover ranges dealt over all eight -- at the smallest
shapes at which that deal can go wrong: no full round, exactly one, one or two rounds and 1 / 7 leftover ranges, a last
range of 4 states and of 1 state, against 1, 2 and 3 frame blocks (fewer leftover blocks than XCDs, exactly 8, no
multiple of 8, a share that straddles two ranges).  Every user of the pair: the record-ring kernel (D = 39), the
straight templated kernel (D = 25), the generic-D kernel (D = 13) and K1n's density kernel.

Every call scores through outprob_dev() into a device buffer pre-filled with NaN, so a (range, frame block) that no
block took shows up, and the result is bit-exact against the oracle.  The tile kernels report their grid in
last_kernel(): at most 7 blocks more than ranges x frame blocks."""
import re

import numpy as np
import pytest

from julius_amd import lib, synth

pytestmark = pytest.mark.gpu

NS, FPB = 16, 512          # states per block, frames per block of the tile kernels (4 waves x 128 frames)


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


def check_grid(kernel, S, T):
    nstb, nfb = -(-S // NS), -(-T // FPB)
    grid = int(re.search(r"grid=(\d+)", kernel).group(1))
    assert 0 <= grid - nstb * nfb <= 7, (kernel, nstb, nfb)


_CASES = {}


def case(oracle, S, T, D=39):
    """Model, frames and the oracle's scores of one shape, computed once."""
    key = (S, T, D)
    if key not in _CASES:
        small = S < 128
        m = synth.make_gmm(S=S, M=16 if small else 4, D=D, seed=S + D, ragged=small)
        fr = synth.make_frames(m, T=T, seed=T)
        want = oracle.gmm_outprob(m, fr)
        want.setflags(write=False)
        _CASES[key] = (m, fr, want)
    return _CASES[key]


@pytest.mark.parametrize("T", [257, 513, 1100])                   # 1, 2, 3 frame blocks
@pytest.mark.parametrize("S", [16, 100, 128, 129, 240, 257])      # 1, 7, 8, 9, 15, 17 state ranges
def test_ranges_and_frame_blocks(engine, oracle, S, T):
    m, fr, want = case(oracle, S, T)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    assert "gmm_tile<D=39" in kernel and ",ring>" in kernel, kernel
    check_grid(kernel, S, T)
    assert not np.isnan(got).any(), np.argwhere(np.isnan(got))[:4]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("D", [25, 13])
def test_straight_and_generic_kernels(engine, oracle, D):
    S, T = 129, 513
    m, fr, want = case(oracle, S, T, D)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    assert ("gmm_tile_generic<" if D == 13 else "gmm_tile<D=25,") in kernel and "ring" not in kernel, kernel
    check_grid(kernel, S, T)
    assert not np.isnan(got).any()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("T", [25, 100])            # 4 and 13 frame blocks of 8 frames
@pytest.mark.parametrize("S", [24, 32, 36])         # 6, 8, 9 entry ranges of 64
def test_narrow_density_kernel(engine, oracle, S, T):
    m = synth.make_gmm(S=S, M=16, D=39, seed=700 + S)
    assert int(m["st_off"][-1]) == 64 * (S * 16 // 64)
    fr = synth.make_frames(m, T=T, seed=T)
    gm = lib.Gmm(engine, m)
    got = score_into_nan(engine, gm, fr)
    kernel = gm.last_kernel()
    gm.close()
    assert "gmm_narrow<D=39>" in kernel, kernel
    assert not np.isnan(got).any()
    assert np.array_equal(got, oracle.gmm_outprob(m, fr))


def test_second_call_gives_the_same_floats(engine, oracle):
    m, fr, want = case(oracle, 240, 1100)
    gm = lib.Gmm(engine, m)
    first = score_into_nan(engine, gm, fr)
    second = score_into_nan(engine, gm, fr)
    gm.close()
    assert np.array_equal(first, want)
    assert first.tobytes() == second.tobytes()
