"""GPU: the pruned and tied-mixture forms of GMM scoring (csrc/gmm_pruned.hip: gmm_safe_kernel, tmix_book_kernel,
tmix_book_hist_kernel, tmix_state_kernel) where their kernels change path: every list size dispatch_topn instantiates
(2 .. 64 register slots) at the compiled and the generic vector lengths, codebooks of unequal size, frame and state
counts around the wave / block / tile edges, empty states, NULL densities, frames far from every Gaussian, many and
empty utterances, and exactly tied scores.  Everything is bit-exact: against the oracle (licensed for these shapes by
test_oracle_vs_ref.py) and, wherever an hmmdefs file can express the model, against the compiled reference."""
import functools

import numpy as np
import pytest

import tiedref
from julius_amd import lib, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

LZ = np.float32(-1000000.0)
CODES = {"none": lib.GPRUNE_NONE, "safe": lib.GPRUNE_SAFE, "heu": lib.GPRUNE_HEU, "beam": lib.GPRUNE_BEAM}
HIST = pytest.mark.parametrize("method", ["heu", "beam"])


def maxmix(m):
    return int(np.diff(m["st_off"]).max())


def check_safe(engine, oracle, m, fr, n, want=None):
    """One gprune-safe call on a plain model: the kernel and list size it reports, and the oracle's scores."""
    gm = lib.Gmm(engine, m, lib.GPRUNE_SAFE, n)
    got = gm.outprob_host(fr)
    D = m["mean"].shape[1]
    assert gm.last_kernel() == f"gmm_safe<DT={D if D in (39, 38, 26, 25) else 0}> cap={min(n, maxmix(m))}"
    if want is None:
        want = oracle.gmm_outprob(m, fr, po.GPRUNE_SAFE, n)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} scores differ, first at (t, s) = {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    return got


def same_cache(dev, b, want, what=""):
    """The device's MIXCACHE of codebook b ([T][nbook][cap] score, id; [T][nbook] num) against (score, id, num) rows
    of the oracle or the reference: num, and the first num[t] slots of every frame."""
    sc, ids, num = dev
    wsc, wids, wnum = want
    assert np.array_equal(num[:, b], wnum), (what, b, "num")
    w = min(sc.shape[2], wsc.shape[1])
    assert wnum.max(initial=0) <= w
    live = np.arange(w)[None, :] < wnum[:, None]
    assert np.array_equal(ids[:, b, :w][live], wids[:, :w][live]), (what, b, "id")
    assert np.array_equal(sc[:, b, :w][live], wsc[:, :w][live]), (what, b, "score")


def check_tied(engine, oracle, m, fr, gprune, n, books=None):
    """One call on an all-tied model against the oracle: state scores and the MIXCACHE of every (used) codebook."""
    code = CODES[gprune]
    gm = lib.Gmm(engine, m, code, n)
    got = gm.outprob_host(fr)
    want = oracle.gmm_outprob(m, fr, code, n)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{gprune} {n}: {len(bad)} scores differ, first at (t, s) = {bad[0]}"
    dev = gm.tmix_cache_host(fr)
    sizes = tiedref.book_sizes(m)
    cap = int(sizes.max()) if gprune == "none" else min(n, int(sizes.max()))
    assert lib.load().jamd_gmm_tmix_cap(gm.h) == cap and dev[0].shape[2] == cap
    for b in (range(m["nbook"]) if books is None else books):
        same_cache(dev, b, oracle.tmix_topn(m, b, fr, code, n), f"{gprune} {n}")
        if gprune in ("none", "safe"):
            assert np.all(dev[2][:, b] == min(int(sizes[b]), cap))    # a small codebook keeps all it has
    return got, dev


# ================================================================== 1. safe pruning on plain states (gmm_safe_kernel)
@functools.lru_cache(maxsize=None)
def wide_model():
    m = synth.make_gmm(S=20, M=70, D=39, seed=2, ragged=True, null_frac=0.05)
    assert maxmix(m) >= 64 and (m["ent_dens"] < 0).any()
    return m, synth.make_frames(m, T=130, seed=5)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64])
def test_safe_list_capacity_edges(engine, oracle, n):
    """gmm_safe_kernel<39, N> at both sides of every step of dispatch_topn (N = 2, 4, 8, 16, 32, 64): mixtures of up
    to 70 Gaussians, so that a list of n entries is full and keeps being pushed into."""
    m, fr = wide_model()
    want = oracle.gmm_outprob(m, fr, po.GPRUNE_SAFE, n)
    if n < 16:
        assert not np.array_equal(want, oracle.gmm_outprob(m, fr))       # pruning really happens
    check_safe(engine, oracle, m, fr, n, want)


def test_safe_list_larger_than_every_mixture(engine, oracle):
    """gprune_num 64 on a model whose largest mixture is 40: cap = the largest mixture, held in the 64-slot list;
    every Gaussian is kept, in descending order."""
    m = synth.make_gmm(S=20, M=40, D=39, seed=8, ragged=True, null_frac=0.05)
    assert 32 < maxmix(m) <= 40
    check_safe(engine, oracle, m, synth.make_frames(m, T=130, seed=6), 64)


@pytest.mark.parametrize("D", [26, 25, 38, 13])
@pytest.mark.parametrize("n", [17, 64])
def test_safe_wide_lists_at_other_vector_lengths(engine, oracle, D, n):
    """The 32- and 64-slot lists with the other compiled vector lengths and with the generic-D body (frames in LDS)."""
    m = synth.make_gmm(S=12, M=70, D=D, seed=6, ragged=True, null_frac=0.05)
    assert maxmix(m) >= 64
    check_safe(engine, oracle, m, synth.make_frames(m, T=130, seed=D + 1), n)


@functools.lru_cache(maxsize=None)
def long_call(po_oracle):
    m = synth.make_gmm(S=20, M=6, D=39, seed=12, ragged=True, null_frac=0.05)
    fr = synth.make_frames(m, T=1025, seed=13)
    return m, fr, po_oracle.gmm_outprob(m, fr, po.GPRUNE_SAFE, 3)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025])
def test_safe_frame_counts(engine, oracle, T):
    """A wave owns 128 frames (lane l: frames l and 64 + l, clamped to T - 1), a block 512: calls that end at, before
    and after those edges, up to three frame-blocks.  (Plain states: a frame's scores do not depend on its
    neighbours, so the first T rows of the oracle's long call are the expected value of the T-frame call.)"""
    m, fr, want = long_call(oracle)
    got = check_safe(engine, oracle, m, fr[:T], 3, want[:T])
    if T == 1025:
        gm = lib.Gmm(engine, m, lib.GPRUNE_SAFE, 3)
        for t in (0, 511, 512, 1024):
            assert np.array_equal(gm.outprob_host(fr[t:t + 1])[0], got[t]), t


@pytest.mark.parametrize("S", [1, 15, 16, 17, 33])
def test_safe_state_counts_around_the_output_tile(engine, oracle, S):
    m = synth.make_gmm(S=S, M=6, D=39, seed=40 + S, ragged=True, null_frac=0.05)
    check_safe(engine, oracle, m, synth.make_frames(m, T=70, seed=S), 3)


def test_safe_states_without_entries(engine, oracle):
    """Three states with no mixture entry (first, in the middle, last): the log-sum of nothing is LOG_ZERO."""
    m = synth.make_gmm(S=9, M=6, D=39, seed=14, ragged=True)
    off = m["st_off"]
    m = dict(m, st_off=np.concatenate([[0], off[:5], off[4:], off[-1:]]).astype(np.int32))
    empty = np.nonzero(np.diff(m["st_off"]) == 0)[0]
    assert len(m["st_off"]) == 13 and list(empty) == [0, 5, 11]
    got = check_safe(engine, oracle, m, synth.make_frames(m, T=130, seed=15), 3)
    assert np.all(got[:, empty] == LZ) and np.all(got[:, [1, 6, 10]] > LZ)


@pytest.mark.parametrize("n", [1, 3, 8])
def test_safe_state_of_null_densities(engine, oracle, n):
    """A state whose entries are NULL densities except the first (missing <Mixture> entries: no density, weight
    LOG_ZERO), beside ordinary states."""
    m = synth.make_gmm(S=6, M=5, D=39, seed=16)
    m["ent_dens"] = m["ent_dens"].copy()
    m["ent_logw"] = m["ent_logw"].copy()
    e0, e1 = int(m["st_off"][2]), int(m["st_off"][3])
    m["ent_dens"][e0 + 1:e1] = -1
    m["ent_logw"][e0 + 1:e1] = LZ
    check_safe(engine, oracle, m, synth.make_frames(m, T=70, seed=17), n)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_safe_exact_ties_inside_states(engine, oracle, ref, n):
    """Entries 1 and 3 of every state share entry 0's density, with weights of their own: three equal scores in every
    list.  Plain states have no history, so device, oracle and compiled reference visit in the same order and
    cache_push()'s tie rule (an equal score goes behind its equals) must come out bit for bit."""
    m = tiedref.triplicate(synth.make_gmm(S=20, M=6, D=39, seed=31, ragged=True, null_frac=0.05))
    fr = synth.make_frames(m, T=70, seed=32)
    got = check_safe(engine, oracle, m, fr, n)
    assert np.array_equal(got, ref.am_from_flat(m, gprune="safe", gprune_num=n).outprob(fr))


@pytest.mark.parametrize("n", [3, 8])
def test_safe_far_frames(engine, oracle, n):
    """Every second frame 50 times, every fourth 400 times too far out: terms below the LOG_ADDMIN cutoff, and
    log-sums that end as LOG_ZERO."""
    m = synth.make_gmm(S=20, M=9, D=39, seed=18, ragged=True, null_frac=0.05)
    fr = tiedref.far_frames(synth.make_frames(m, T=130, seed=19))
    want = oracle.gmm_outprob(m, fr, po.GPRUNE_SAFE, n)
    assert (want == LZ).any() and np.isfinite(want).all()
    check_safe(engine, oracle, m, fr, n, want)


# ============================================ 2. tied-mixture, safe and none (tmix_book_kernel + tmix_state_kernel)
@pytest.mark.parametrize("gprune,n", [("safe", n) for n in (2, 4, 5, 8, 9, 16, 17, 32, 33, 64)] + [("none", 0)])
def test_tied_list_capacity_edges(engine, oracle, gprune, n):
    """tmix_book_kernel<39, N> at both sides of every step of dispatch_topn, on codebooks of 70 and 64 Gaussians."""
    m = tiedref.make_tied((70, 64), S=21, D=39, seed=20)
    check_tied(engine, oracle, m, synth.make_frames(m, T=75, seed=21, noise=2.0), gprune, n)


@pytest.mark.parametrize("sizes,gprune,n", [((3, 70, 64, 1, 129), "safe", 2), ((3, 70, 64, 1, 129), "safe", 4),
                                            ((3, 70, 64, 1, 129), "safe", 64), ((3, 70, 64, 1, 129), "none", 0),
                                            ((65, 8), "safe", 64)])
def test_tied_codebooks_of_unequal_size(engine, oracle, sizes, gprune, n):
    """The list size is one number for the model (min(n, largest codebook)); codebooks smaller than it, one of a single
    Gaussian included, sit beside larger ones: their cache rows are partly filled and the state kernel stops at num."""
    m = tiedref.make_tied(sizes, S=21, D=39, seed=22)
    check_tied(engine, oracle, m, synth.make_frames(m, T=75, seed=23, noise=2.0), gprune, n)


@pytest.mark.parametrize("gprune,n", [("safe", 4), ("none", 0), ("heu", 4), ("beam", 4)])
def test_tied_codebook_no_state_uses(engine, oracle, gprune, n):
    """nbook = 3 with only codebooks 0 and 2 referenced: the unused one is an empty codebook (num = 0 on every frame),
    and the scores are those of the same states over two codebooks."""
    m = tiedref.make_tied((16, 5, 24), S=21, D=39, seed=24, books=(0, 2))
    assert set(m["st_book"]) == {0, 2}
    fr = synth.make_frames(m, T=75, seed=25, noise=2.0)
    got, dev = check_tied(engine, oracle, m, fr, gprune, n, books=(0, 2))
    assert np.all(dev[2][:, 1] == 0)
    two = dict(m, st_book=np.where(m["st_book"] == 2, 1, 0).astype(np.int32), nbook=2)
    assert np.array_equal(lib.Gmm(engine, two, CODES[gprune], n).outprob_host(fr), got)


@pytest.mark.parametrize("T", [1, 64, 65, 128, 129, 512, 513])
def test_tied_frame_counts(engine, oracle, T):
    m = tiedref.make_tied((16, 24), S=21, D=39, seed=26)
    check_tied(engine, oracle, m, synth.make_frames(m, T=T, seed=27, noise=2.0), "safe", 4)


@pytest.mark.parametrize("ntied", [255, 256, 257])
def test_tied_state_counts_around_the_state_kernels_block(engine, oracle, ntied):
    """tmix_state_kernel gives a thread to every tied state, 256 to a block."""
    m = tiedref.make_tied((8, 8), S=258, D=39, seed=28)
    e = int(m["st_off"][ntied])
    m = dict(m, st_off=m["st_off"][:ntied + 1], st_book=m["st_book"][:ntied], ent_dens=m["ent_dens"][:e], ent_logw=m["ent_logw"][:e])
    fr = synth.make_frames(m, T=5, seed=29, noise=2.0)
    for gprune, n in (("safe", 3), ("none", 0)):
        check_tied(engine, oracle, m, fr, gprune, n)


@pytest.mark.parametrize("gprune,n", [("none", 0), ("safe", 3), ("safe", 12), ("heu", 3), ("heu", 12), ("beam", 3), ("beam", 12)])
def test_tied_null_densities_in_a_codebook(engine, oracle, gprune, n):
    """NULL densities inside codebooks (no hmmdefs file can say that: oracle only): they score LOG_ZERO and are pushed
    like any other Gaussian, with and without history."""
    K = 12
    m = tiedref.make_tied((K, K), S=21, D=39, seed=30, null=((0, 1), (1, K - 1)))
    assert (m["ent_dens"] < 0).sum() == 21
    check_tied(engine, oracle, m, synth.make_frames(m, T=75, seed=31, noise=2.0), gprune, n)


@functools.lru_cache(maxsize=None)
def tied_far_case():
    m = tiedref.make_tied((16, 24), S=21, D=39, seed=32)
    return m, tiedref.far_frames(synth.make_frames(m, T=75, seed=33, noise=2.0))


@pytest.mark.parametrize("gprune,n", [("none", 0), ("safe", 3), ("safe", 16)])
def test_tied_far_frames(engine, oracle, gprune, n):
    """Every second frame 50 times, every fourth 400 times too far out, against the oracle over the whole utterance
    (= the compiled reference, test_oracle_vs_ref.py::test_tied_gmm_far_frames).  On the 400-fold frames a full list's
    last score lies below LOG_ZERO, compute_g_safe() (gprune_safe.c:76-97) answers LOG_ZERO for every Gaussian below
    that entry and the LOG_ZERO enters the list, so WHICH Gaussians end up in the list depends on the order they are
    visited in -- without any tied score.  The reference starts from frame t - 1's winners; in index order 274 (list of
    3) and 137 (list of 16) of the 378 state scores of those 18 frames come out different (measured on an MI355X with
    the index-order kernel alone), so these frames go through tmix_book_safe_order_kernel."""
    m, fr = tied_far_case()
    want = oracle.gmm_outprob(m, fr, CODES[gprune], n)
    assert (want == LZ).any() and np.isfinite(want).all()
    if gprune == "safe":
        by_frame = tiedref.frame_by_frame(oracle, m, fr, po.GPRUNE_SAFE, n)
        far = np.arange(len(fr)) % 4 == 3
        assert np.array_equal(by_frame[~far], want[~far]) and not np.array_equal(by_frame[far], want[far])
    got, dev = check_tied(engine, oracle, m, fr, gprune, n)
    if gprune == "safe":
        assert (dev[0][far] == LZ).any()                               # the LOG_ZERO entries are really there


@functools.lru_cache(maxsize=None)
def tie_case():
    """Gaussians 2 and K - 1 of both 16-Gaussian codebooks are copies of Gaussian 0; list of 2; one 75-frame utterance."""
    m = tiedref.make_tied((16, 16), S=21, D=39, seed=7, dup=True)
    return m, synth.make_frames(m, T=75, seed=8, noise=2.0)


def test_tied_safe_exact_ties_vs_compiled_reference(engine, oracle, ref, tmp_path):
    """Tied-mixture SAFE pruning under exactly tied scores (HISTORY.md section 4): the reference visits frame t - 1's
    winners first, so which copy of a duplicated Gaussian survives (hence which weight is added) follows the history.
    Frame 0 has none; in index order 7 of the 75 rows come out different.  The frame-parallel kernel marks the frames
    with a tied score and tmix_book_safe_order_kernel does them again in the reference's order: the whole matrix and
    the MIXCACHE are the compiled reference's."""
    m, fr = tie_case()
    am, ex = tiedref.load_tied(ref, tmp_path, m, "safe", 2)
    gm = lib.Gmm(engine, ex, lib.GPRUNE_SAFE, 2)
    got = gm.outprob_host(fr)
    want = am.outprob(fr)
    by_frame = tiedref.frame_by_frame(oracle, ex, fr, po.GPRUNE_SAFE, 2)
    assert np.array_equal(by_frame[0], want[0]) and (by_frame != want).any(axis=1).sum() >= 1     # the order shows here
    assert np.array_equal(got[0], want[0])
    print("rows of the tie case that differ from the compiled reference:", int((got != want).any(axis=1).sum()), "of", len(fr))
    assert np.array_equal(got, want)
    dev = gm.tmix_cache_host(fr)
    for b in range(2):
        same_cache(dev, b, am.tmix_cache(fr, b, 2), "tie case")
    am.close()


@pytest.mark.parametrize("sizes,n", [((16, 16), 2), ((16, 16), 4), ((16, 16), 16), ((65, 8), 2), ((65, 8), 4), ((65, 8), 64)])
def test_tied_safe_exact_ties_more_shapes(engine, oracle, ref, tmp_path, sizes, n):
    """Duplicated Gaussians at more list sizes, in one utterance and in a call of several (the history restarts at every
    utterance's first frame; empty and one-frame utterances among them): compiled reference == oracle == device."""
    m = tiedref.make_tied(sizes, S=21, D=39, seed=7, dup=True)
    fr = synth.make_frames(m, T=75, seed=8, noise=2.0)
    am, ex = tiedref.load_tied(ref, tmp_path, m, "safe", n)
    want = am.outprob(fr)
    assert np.array_equal(oracle.gmm_outprob(ex, fr, po.GPRUNE_SAFE, n), want)
    gm = lib.Gmm(engine, ex, lib.GPRUNE_SAFE, n)
    assert np.array_equal(gm.outprob_host(fr), want)
    dev = gm.tmix_cache_host(fr)
    for b in range(2):
        same_cache(dev, b, am.tmix_cache(fr, b, n), f"safe {n}")
    off = [0, 0, 1, 1, 2, 40, 40, 75]
    cut = np.concatenate([am.outprob(fr[a:b]) for a, b in zip(off[:-1], off[1:]) if b > a])
    am.close()
    assert np.array_equal(utts_dev(engine, gm, fr, off), cut)
    assert np.array_equal(gm.outprob_host(fr), want)                    # and one utterance again on the same object


# ================================================================ 3. heu / beam with history (tmix_book_hist_kernel)
def check_hist(engine, oracle, ref, tmp_path, m, fr, method, n):
    """One utterance under gprune heu / beam: compiled reference == oracle == device, state scores and the MIXCACHE
    of every codebook."""
    am, ex = tiedref.load_tied(ref, tmp_path, m, method, n)
    want = am.outprob(fr)
    assert np.array_equal(oracle.gmm_outprob(ex, fr, CODES[method], n), want)
    gm = lib.Gmm(engine, ex, CODES[method], n)
    got = gm.outprob_host(fr)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{method} {n}: {len(bad)} scores differ, first at (t, s) = {bad[0]}"
    dev = gm.tmix_cache_host(fr)
    for b in range(ex["nbook"]):
        same_cache(dev, b, am.tmix_cache(fr, b, n), f"{method} {n}")
    am.close()
    return ex, want


@HIST
@pytest.mark.parametrize("sizes,n", [((129, 64), 16), ((129, 64), 33), ((129, 64), 63), ((129, 64), 64),
                                     ((65, 8), 8), ((65, 8), 9), ((65, 8), 64), ((63, 64, 128), 64),
                                     ((3, 70, 64, 1, 129), 1), ((3, 70, 64, 1, 129), 4), ((3, 70, 64, 1, 129), 64)])
def test_hist_list_sizes_and_unequal_codebooks(engine, oracle, ref, tmp_path, method, sizes, n):
    """The one-entry-per-lane list up to its last legal size (64), full while a codebook of more than 64 Gaussians is
    walked in a second chunk of lanes; codebooks at, below and above the list size side by side."""
    m = tiedref.make_tied(sizes, S=21, D=39, seed=sum(sizes) + n)
    check_hist(engine, oracle, ref, tmp_path, m, synth.make_frames(m, T=75, seed=n, noise=2.0), method, n)


@HIST
@pytest.mark.parametrize("D,n", [(13, 4), (13, 64), (60, 16), (60, 64)])
def test_hist_other_vector_lengths(engine, oracle, ref, tmp_path, method, D, n):
    """The kernel's LDS request grows as list size x vector length."""
    m = tiedref.make_tied((129, 64), S=21, D=D, seed=D + n)
    check_hist(engine, oracle, ref, tmp_path, m, synth.make_frames(m, T=75, seed=D, noise=2.0), method, n)


@HIST
@pytest.mark.parametrize("sizes,n", [((16, 16), 2), ((16, 16), 4), ((65, 8), 2), ((65, 8), 4)])
def test_hist_exact_ties(engine, oracle, ref, tmp_path, method, sizes, n):
    """Duplicated Gaussians under heu / beam: device and reference both push frame t - 1's winners first and the rest
    in index order, so here exact ties must come out bit for bit."""
    m = tiedref.make_tied(sizes, S=21, D=39, seed=7, dup=True)
    check_hist(engine, oracle, ref, tmp_path, m, synth.make_frames(m, T=75, seed=8, noise=2.0), method, n)


@HIST
@pytest.mark.parametrize("n", [4, 16])
def test_hist_far_frames_in_mid_utterance(engine, oracle, ref, tmp_path, method, n):
    """Four consecutive frames 60 times too far out: the thresholds of the frames behind them come from far frames."""
    m = tiedref.make_tied((70, 16), S=21, D=39, seed=34)
    fr = synth.make_frames(m, T=75, seed=35, noise=2.0)
    fr[40:44] *= np.float32(60.0)
    check_hist(engine, oracle, ref, tmp_path, m, fr, method, n)


@HIST
@pytest.mark.parametrize("n", [4, 16])
def test_hist_utterance_begins_far_out(engine, oracle, ref, tmp_path, method, n):
    """The first frame (no history: the safe-pruning branch) 400 times too far out: every score lies below LOG_ZERO,
    and compute_g_safe()'s LOG_ZERO enters the list (topn_push_safe(), csrc/gmm_dev.h); frame 1 starts from those."""
    m = tiedref.make_tied((70, 16), S=21, D=39, seed=34)
    fr = synth.make_frames(m, T=20, seed=36, noise=2.0)
    fr[0] *= np.float32(400.0)
    ex, want = check_hist(engine, oracle, ref, tmp_path, m, fr, method, n)
    assert any((oracle.tmix_topn(ex, b, fr[:1], CODES[method], n)[0] == LZ).any() for b in range(2))


def utts_dev(engine, gm, fr, utt_off):
    d_fr = lib.DevBuf(engine, fr.nbytes).upload(fr)
    d_out = lib.DevBuf(engine, 4 * len(fr) * gm.S)
    gm.outprob_utts_dev(d_fr.ptr, utt_off, d_out.ptr)
    engine.sync()
    return d_out.download((len(fr), gm.S), np.float32)


@HIST
def test_hist_empty_and_one_frame_utterances(engine, oracle, ref, tmp_path, method):
    """The history restarts at every utterance boundary; empty and one-frame utterances between ordinary ones."""
    m = tiedref.make_tied((70, 16), S=21, D=39, seed=36)
    am, ex = tiedref.load_tied(ref, tmp_path, m, method, 4)
    fr = synth.make_frames(m, T=75, seed=37, noise=2.0)
    off = [0, 0, 1, 1, 2, 40, 40, 75]
    want = np.concatenate([am.outprob(fr[a:b]) for a, b in zip(off[:-1], off[1:]) if b > a])
    assert not np.array_equal(want, am.outprob(fr))                     # the boundaries matter
    am.close()
    assert np.array_equal(utts_dev(engine, lib.Gmm(engine, ex, CODES[method], 4), fr, off), want)


@functools.lru_cache(maxsize=None)
def many_utterances(po_oracle, method):
    """1500 utterances of 0 .. 3 frames cut from one frame array, and the oracle's scores utterance by utterance."""
    m = tiedref.make_tied((20, 9), S=12, D=39, seed=38)
    rng = np.random.default_rng(39)
    lens = rng.choice(4, size=1500, p=[0.3, 0.3, 0.25, 0.15])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert off[-1] <= 2000 and (lens == 0).sum() >= 100 and (lens == 1).sum() >= 100
    fr = synth.make_frames(m, T=2000, seed=40, noise=2.0)[:off[-1]]
    want = np.concatenate([po_oracle.gmm_outprob(m, fr[a:b], CODES[method], 4) for a, b in zip(off[:-1], off[1:]) if b > a])
    return m, fr, off, want


@HIST
def test_hist_more_than_1024_utterances(engine, oracle, method):
    """More utterances in a call than the pinned boundary staging holds at first (it regrows beyond 1024)."""
    m, fr, off, want = many_utterances(oracle, method)
    assert not np.array_equal(want, oracle.gmm_outprob(m, fr, CODES[method], 4))
    assert np.array_equal(utts_dev(engine, lib.Gmm(engine, m, CODES[method], 4), fr, off), want)


@HIST
def test_hist_one_model_object_over_calls_of_different_utterance_counts(engine, oracle, method):
    """One jamd_gmm for calls of 1, 1500 and 3 utterances and then the cache entry point (which goes back to one
    utterance): every call gives what a fresh object gives."""
    m, fr, off, want = many_utterances(oracle, method)
    code = CODES[method]
    gm = lib.Gmm(engine, m, code, 4)
    one = oracle.gmm_outprob(m, fr[:60], code, 4)
    assert np.array_equal(gm.outprob_host(fr[:60]), one)
    assert np.array_equal(utts_dev(engine, gm, fr, off), want)
    off3 = [0, 20, 21, 60]
    got3 = utts_dev(engine, gm, fr[:60], off3)
    assert np.array_equal(got3, utts_dev(engine, lib.Gmm(engine, m, code, 4), fr[:60], off3))
    assert np.array_equal(got3, np.concatenate([oracle.gmm_outprob(m, fr[a:b], code, 4) for a, b in zip(off3[:-1], off3[1:])]))
    assert not np.array_equal(got3, one)
    dev = gm.tmix_cache_host(fr[:60])
    fresh = lib.Gmm(engine, m, code, 4).tmix_cache_host(fr[:60])
    for b in range(2):
        same_cache(dev, b, oracle.tmix_topn(m, b, fr[:60], code, 4), "reused")
        same_cache(fresh, b, oracle.tmix_topn(m, b, fr[:60], code, 4), "fresh")


@HIST
@pytest.mark.parametrize("n", [2, 8])
def test_hist_compound_model(engine, oracle, method, n):
    """Tied-mixture states under heu / beam beside plain states (calc_compound_mix): the tied half goes through the
    history kernel, the plain half through the safe kernel with the same list size."""
    tied = tiedref.make_tied((32, 32), S=18, D=39, seed=41)
    plain = synth.make_gmm(S=12, M=6, D=39, seed=42, ragged=True, null_frac=0.1)
    assert (plain["ent_dens"] < 0).any()
    mix = tiedref.compound(tied, plain)
    fr = synth.make_frames(tied, T=150, seed=43, noise=2.0)
    gm = lib.Gmm(engine, mix, CODES[method], n)
    got = gm.outprob_host(fr)
    assert gm.last_kernel() == f"gmm_safe<DT=39> cap={min(n, maxmix(plain))}"
    want_tied = oracle.gmm_outprob(tied, fr, CODES[method], n)
    assert np.array_equal(got[:, :18], want_tied)
    assert np.array_equal(got[:, 18:], oracle.gmm_outprob(plain, fr, po.GPRUNE_SAFE, n))
    assert np.array_equal(got, oracle.gmm_outprob(mix, fr, CODES[method], n))
    assert not np.array_equal(want_tied, oracle.gmm_outprob(tied, fr, po.GPRUNE_SAFE, n))     # hist_method is in effect
