"""GPU: per-Gaussian scores (jamd_gmm_dens_host / jamd_gmm_dens_dev, gmm_dens_kernel) against the fp32 restatement of
compute_g_base() in densref.py, bit for bit, at the shapes where the kernel takes another path: entry counts around
its 16-entry tile and its 1024-entry chunk (blockIdx.y > 0), frame counts around its 64-frame block, vector lengths
up to the last one its LDS request admits, all-tied-mixture models in codebook order, a caller's stream, and the
two refusals."""
import ctypes as C

import numpy as np
import pytest

from densref import dens_columns, dens_ref
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu


def _plain_model(E, D, seed):
    """A plain model of exactly E mixture entries in ragged states (1 to 20 entries each), about a tenth of the
    entries NULL densities -- the first one of the model never, the last one of some states always."""
    rng = np.random.default_rng(seed)
    m = synth.make_gmm(S=E, M=1, D=D, seed=seed)
    cuts = [0]
    while cuts[-1] < E:
        cuts.append(min(E, cuts[-1] + int(rng.integers(1, 21))))
    m["st_off"] = np.array(cuts, np.int32)
    kill = rng.random(E) < 0.1
    kill[m["st_off"][1::3] - 1] = True
    kill[0] = False
    m["ent_dens"] = np.where(kill, -1, np.arange(E)).astype(np.int32)
    m["ent_logw"][kill] = np.float32(lib.LOG_ZERO)
    return m


def _tied_model(sizes, D, seed):
    """An all-tied-mixture model whose codebooks have the given sizes.  The Gaussians of a codebook are scattered over
    the density pool, and the states come in an order in which the codebooks do not first appear by ascending id, so
    the column order can come from nothing but the codebook ids and each codebook's own entry order."""
    rng = np.random.default_rng(seed)
    nbook, G = len(sizes), int(sum(sizes))
    pool = synth.make_gmm(S=G, M=1, D=D, seed=seed)
    perm = rng.permutation(G)
    book_dens = np.split(perm, np.cumsum(sizes)[:-1])
    st_book = np.concatenate([np.arange(nbook)[::-1], rng.integers(0, nbook, 4)]).astype(np.int32)
    n = np.array([sizes[b] for b in st_book])
    return dict(mean=pool["mean"], ivar=pool["ivar"], gconst=pool["gconst"],
                st_off=np.concatenate([[0], np.cumsum(n)]).astype(np.int32),
                ent_dens=np.concatenate([book_dens[b] for b in st_book]).astype(np.int32),
                ent_logw=np.log(rng.uniform(0.01, 1.0, int(n.sum()))).astype(np.float32),
                st_book=st_book, nbook=nbook, nstream=1, book_dens=book_dens)


def _frames(D, T, seed):
    return np.random.default_rng(seed).normal(0.0, 1.5, (T, D)).astype(np.float32)


# every T beside an entry count on either side of the 1024-entry chunk
@pytest.mark.parametrize("E,T", [(1, 1), (1, 65), (15, 63), (16, 64), (17, 130), (1023, 1), (1023, 64), (1024, 65),
                                 (1024, 130), (1025, 1), (1025, 63), (1025, 64), (2064, 63), (2064, 65), (2064, 130)])
def test_entry_and_frame_counts(engine, E, T):
    m = _plain_model(E, 39, seed=E)
    assert len(m["ent_dens"]) == E and (E < 15 or (m["ent_dens"] < 0).any())
    fr = _frames(39, T, seed=T)
    g = lib.Gmm(engine, m)
    assert lib.load().jamd_gmm_nentry(g.h) == E
    got = g.dens_host(fr)
    assert got.shape == (T, E) and np.array_equal(got, dens_ref(m, fr))


# 239 is the last vector length whose LDS request (64 * D + 64 * 17 floats) is within the kernel's 64 KB
@pytest.mark.parametrize("D", [13, 25, 26, 39, 60, 96, 239])
def test_vector_lengths(engine, D):
    m = _plain_model(37, D, seed=D)
    fr = _frames(D, 70, seed=D + 1)
    got = lib.Gmm(engine, m).dens_host(fr)
    assert np.array_equal(got, dens_ref(m, fr))


def test_vector_length_beyond_lds_is_refused(engine):
    """The kernel asks for (64 * D + 64 * 17) floats of LDS and jamd_gmm_dens_dev() refuses a request above 64 KB: the
    first such D is 240 (jamd_gmm_create() accepts vector lengths up to 1024, so the model itself loads)."""
    D = next(d for d in range(1, 1025) if 4 * (64 * d + 64 * 17) > 64 * 1024)
    assert D == 240
    g = lib.Gmm(engine, _plain_model(5, D, seed=1))
    with pytest.raises(lib.JamdError, match=r"\(-1\).*jamd_gmm_dens_dev: vector length 240 too large"):
        g.dens_host(_frames(D, 3, seed=2))


@pytest.mark.parametrize("K", [16, 40, 129])
@pytest.mark.parametrize("nbook", [1, 3])
def test_all_tied_columns_are_in_codebook_order(engine, nbook, K):
    sizes = [K, K // 2 + 1, K + 3][:nbook]
    m = _tied_model(sizes, 39, seed=K + nbook)
    fr = _frames(39, 66, seed=K)
    g = lib.Gmm(engine, m)
    assert lib.load().jamd_gmm_nentry(g.h) == sum(sizes)
    off = np.zeros(nbook + 1, np.int32)
    assert lib.load().jamd_gmm_book_offsets(g.h, off.ctypes.data, nbook + 1) == 0
    cols, want_off = dens_columns(m)
    assert np.array_equal(off, want_off) and np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]))
    got = g.dens_host(fr)
    assert np.array_equal(got, dens_ref(m, fr))
    # column off[b] + k is Gaussian k of codebook b, said once more without the helper's column list
    plain = dict(m, st_book=None, nbook=0, ent_dens=np.arange(len(m["mean"]), dtype=np.int32),
                 st_off=np.array([0, len(m["mean"])], np.int32))
    by_density = dens_ref(plain, fr)
    for b in range(nbook):
        assert np.array_equal(cols[off[b]:off[b + 1]], m["book_dens"][b])
        assert np.array_equal(got[:, off[b]:off[b + 1]], by_density[:, m["book_dens"][b]])


def test_compound_model_is_refused(engine):
    """A model that mixes tied-mixture and plain states has no single column order: both entries say so."""
    m = _tied_model([16, 9], 39, seed=3)
    m["st_book"] = m["st_book"].copy()
    m["st_book"][-1] = -1                                      # the last state becomes a plain one
    g = lib.Gmm(engine, m)
    assert lib.load().jamd_gmm_nentry(g.h) == 0
    fr = _frames(39, 4, seed=4)
    with pytest.raises(lib.JamdError, match=r"\(-1\).*jamd_gmm_dens_host: no single column order for this model"):
        g.dens_host(fr)
    d_fr = lib.DevBuf(engine, fr.nbytes).upload(fr)
    d_out = lib.DevBuf(engine, 4 * 4 * 64)
    assert lib.load().jamd_gmm_dens_dev(g.h, d_fr.ptr, 4, d_out.ptr, None) == -1
    assert (b"jamd_gmm_dens_dev: models mixing plain and tied-mixture states have no single column order"
            in lib.load().jamd_last_error())


@pytest.mark.parametrize("E,T", [(1025, 65), (17, 63), (2064, 130)])
def test_device_entry_on_a_callers_stream(engine, E, T):
    """jamd_gmm_dens_dev() on a stream and buffers of the caller's: the host entry's values, and nothing written past
    the [T][E] matrix where the last chunk of entries and the last block of frames are both ragged."""
    m = _plain_model(E, 39, seed=E + 7)
    fr = _frames(39, T, seed=T + 7)
    g = lib.Gmm(engine, m)
    want = g.dens_host(fr)
    assert np.array_equal(want, dens_ref(m, fr))
    sentinel = np.float32(-12345.5)
    d_fr = lib.DevBuf(engine, fr.nbytes).upload(fr)
    d_out = lib.DevBuf(engine, 4 * (T * E + 4)).upload(np.full(T * E + 4, sentinel, np.float32))
    s = C.c_void_p()
    assert lib.load().jamd_stream_create(engine.h, C.byref(s)) == 0
    try:
        assert lib.load().jamd_gmm_dens_dev(g.h, d_fr.ptr, T, d_out.ptr, s) == 0, lib.load().jamd_last_error()
        assert lib.load().jamd_stream_sync(engine.h, s) == 0
    finally:
        lib.load().jamd_stream_destroy(engine.h, s)
    got = d_out.download((T * E + 4,), np.float32)
    assert np.array_equal(got[:T * E].reshape(T, E), want)
    assert (got[T * E:] == sentinel).all()
