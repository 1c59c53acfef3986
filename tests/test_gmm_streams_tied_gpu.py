"""GPU: multi-stream GMM scoring with tied-mixture codebooks and -gprune safe (jamd_gmm_ms_create_opt(), kernels K1mt)
bit for bit against the compiled reference's scores and codebook caches in tests/golden/gmm_streams_tied.npz."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import streamstied as st  # noqa: E402
from beamutil import load_beam_golden  # noqa: E402
from julius_amd import lexblob, lib  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def _case(name):
    """A fixture case, loaded once and left unchanged."""
    if name not in _cache:
        _cache[name] = st.load_case(name)
    return _cache[name]


def _dev(engine, g, frames, utt_off):
    """outprob_utts_dev() with device buffers of the caller."""
    d_fr = lib.DevBuf(engine, frames.nbytes).upload(frames)
    d_out = lib.DevBuf(engine, 4 * len(frames) * g.S)
    g.outprob_utts_dev(d_fr.ptr, utt_off, d_out.ptr)
    engine.sync()
    return d_out.download((len(frames), g.S), np.float32)


MODES = [(name, gprune, n) for name in st.CASES for gprune, n in st.modes(_case(name))]


@pytest.mark.parametrize("name,gprune,n", MODES, ids=[f"{a}-{st.key(b, c)}" for a, b, c in MODES])
def test_case_is_bit_exact(engine, name, gprune, n):
    """Every case under -gprune none and under safe at its gprune_nums, through _host and through _dev."""
    c = _case(name)
    want = c["scores"][st.key(gprune, n)]
    g = lib.GmmStreamsTied(engine, c["model"], gprune=gprune, gprune_num=n)
    assert (g.S, g.D, g.nstream, g.nbook) == (want.shape[1], c["frames"].shape[1], len(c["model"]["vsize"]), st.nbook(c["model"]))
    got = g.outprob_host(c["frames"], c["utt_off"])
    assert g.last_kernel().startswith(f"gmm_ms_tied<{gprune}>")
    assert np.array_equal(got, want)
    assert np.array_equal(_dev(engine, g, c["frames"], c["utt_off"]), want)
    g.close()


CACHES = [(name, n) for name in st.CASES for n in _case(name)["cache"]]


@pytest.mark.parametrize("name,n", CACHES, ids=[f"{a}-safe{b}" for a, b in CACHES])
def test_codebook_cache_equals_the_references(engine, name, n):
    """score, id and num of every (frame, codebook) against jref_am_tmix_cache()'s recorded rows: the ties case and
    the codebook sizes round the 64 members the order pass takes at a time."""
    c = _case(name)
    w_sc, w_id, w_num = c["caches"][f"safe{n}"]
    g = lib.GmmStreamsTied(engine, c["model"], gprune="safe", gprune_num=n)
    sc, ids, num = g.tmix_cache_host(c["frames"])
    assert np.array_equal(num, w_num) and g.tmix_cap <= n
    live = np.arange(g.tmix_cap)[None, None, :] < num[:, :, None]
    assert np.array_equal(ids[live], w_id[:, :, :g.tmix_cap][live]) and np.array_equal(sc[live], w_sc[:, :, :g.tmix_cap][live])
    g.close()


@pytest.mark.parametrize("n", [3])
def test_chunks_do_not_show(engine, n):
    """300 frames with tied pairs leading on frames 128 and 256: chunk_frames 128 (both are first frames of a chunk),
    129 and the default give the reference's scores."""
    c = _case("chunks")
    want = c["scores"][f"safe{n}"]
    for chunk in (128, 129, 0):
        g = lib.GmmStreamsTied(engine, c["model"], gprune="safe", gprune_num=n, chunk_frames=chunk)
        assert np.array_equal(g.outprob_host(c["frames"]), want), chunk
        assert f"chunk={chunk or 2048} " in g.last_kernel()
        g.close()
    g = lib.GmmStreamsTied(engine, c["model"], gprune="none", chunk_frames=128)
    assert np.array_equal(g.outprob_host(c["frames"]), c["scores"]["none"])


def test_utterance_boundaries_cut_the_history(engine):
    """7 | 1 | 9 frames and the same 17 as one utterance: each as the reference scores it, and they differ."""
    a, b = _case("ties"), _case("ties_one_utt")
    g = lib.GmmStreamsTied(engine, a["model"], gprune="safe", gprune_num=3)
    three, one = g.outprob_host(a["frames"], a["utt_off"]), g.outprob_host(a["frames"])
    assert np.array_equal(three, a["scores"]["safe3"]) and np.array_equal(one, b["scores"]["safe3"])
    assert not np.array_equal(three, one)
    # ... also where a chunk ends inside an utterance and where one begins with a chunk
    for chunk in (3, 7, 8):
        h = lib.GmmStreamsTied(engine, a["model"], gprune="safe", gprune_num=3, chunk_frames=chunk)
        assert np.array_equal(h.outprob_host(a["frames"], a["utt_off"]), three), chunk
        assert np.array_equal(h.outprob_host(a["frames"]), one), chunk
        h.close()


def test_back_to_back_calls_do_not_leak_cache_rows(engine):
    """The three-utterance ties, then a shorter call with other frames on the same object: the second is what a fresh
    object gives (and the reference: a prefix of the chunks case, the same model)."""
    a, c = _case("ties"), _case("chunks")
    g = lib.GmmStreamsTied(engine, a["model"], gprune="safe", gprune_num=3)
    assert np.array_equal(g.outprob_host(a["frames"], a["utt_off"]), a["scores"]["safe3"])
    assert np.array_equal(g.outprob_host(c["frames"][:11]), c["scores"]["safe3"][:11])
    assert np.array_equal(g.outprob_host(a["frames"], a["utt_off"]), a["scores"]["safe3"])


@pytest.mark.parametrize("name", ["branches", "compound"])
def test_from_binhmm_equals_descriptor(engine, tmp_path, name):
    """mkbinhmm's file of the model (the reference's write_binhmm(), committed) read by the library itself scores as the
    descriptor route under every mode."""
    c = _case(name)
    path = st.load_binhmm(name, tmp_path / "committed.binhmm")
    for gprune, n in st.modes(c):
        g = lib.GmmStreamsTied.from_binhmm(engine, path, gprune=gprune, gprune_num=n)
        assert (g.S, g.D, g.nstream, g.nbook) == (c["model"]["st_pdf"].shape[0], c["frames"].shape[1], len(c["model"]["vsize"]),
                                                  st.nbook(c["model"]))
        assert np.array_equal(g.outprob_host(c["frames"]), c["scores"][st.key(gprune, n)]), (gprune, n)
        g.close()
    with pytest.raises(lib.JamdError, match="is a tied-mixture pdf"):      # the entry without options keeps its refusal
        lib.GmmStreamsTied.from_binhmm(engine, path)


def test_one_stream_all_tied_equals_gmm(engine):
    """nstream = 1, every pdf tied: the same bits as lib.Gmm on the same model under both modes."""
    c = _case("one_stream")
    m = c["model"]
    assert np.array_equal(m["st_pdf"][:, 0], np.arange(m["st_pdf"].shape[0]))          # pdf p is state p's
    flat = dict(mean=m["mean"].reshape(-1, 39), ivar=m["ivar"].reshape(-1, 39), gconst=m["gconst"], st_off=m["pdf_off"],
                ent_dens=m["ent_dens"], ent_logw=m["ent_logw"], st_book=m["pdf_book"], nbook=st.nbook(m), nstream=1)
    for gprune, n, code in (("none", 0, lib.GPRUNE_NONE), ("safe", 2, lib.GPRUNE_SAFE)):
        k1 = lib.Gmm(engine, flat, code, n).outprob_host(c["frames"])
        assert np.array_equal(k1, c["scores"][st.key(gprune, n)])
        assert np.array_equal(lib.GmmStreamsTied(engine, m, gprune=gprune, gprune_num=n).outprob_host(c["frames"]), k1)


def test_all_plain_model_under_none_is_the_old_object(engine):
    """No tied pdf, -gprune none: jamd_gmm_ms_create_opt() makes what jamd_gmm_ms_create() makes -- K1m, the same bits --
    and under safe the plain pdfs go through the cache, as the reference scores them."""
    import streamsref
    model, frames, want = streamsref.load_case("ragged4")
    old = lib.GmmStreams(engine, model)
    new = lib.GmmStreamsTied(engine, model, gprune="none")
    assert np.array_equal(new.outprob_host(frames), old.outprob_host(frames)) and np.array_equal(new.outprob_host(frames), want)
    assert new.last_kernel() == old.last_kernel() and new.last_kernel().startswith("gmm_ms<")
    assert (new.nbook, new.tmix_cap) == (0, 0)
    assert np.array_equal(lib.GmmStreamsTied(engine, model).outprob_host(frames), want)      # gprune=None: the old entry
    with pytest.raises(lib.JamdError, match="jamd_gmm_ms_create: pdf 0 is a tied-mixture pdf"):
        lib.GmmStreamsTied(engine, _case("lay_26_13")["model"])
    with pytest.raises(lib.JamdError, match="gprune heu is not served"):
        lib.GmmStreamsTied(engine, model, gprune="heu", gprune_num=2)


def test_two_stream_tied_model_feeds_the_first_pass(engine):
    """A 26 + 13 tied model over the golden lexicon's 120 states: its device matrix goes straight into
    lib.Beam.pass1_dev, and the result is what pass1_dev gives on the reference's scores uploaded as they are."""
    c = _case("e2e")
    frames, want = c["frames"], c["scores"]["none"]
    g = load_beam_golden("beam_rank.npz")
    assert want.shape[1] == len(g["am"]["st_off"]) - 1
    ms = lib.GmmStreamsTied(engine, c["model"], gprune="none")
    lx = lib.Lexicon(engine, g["lex"])
    off = np.array([0, len(frames)], np.int32)

    def pass1(d_scores):
        bm = lib.Beam(engine, lx, g["beam_width"], g["score_pruning_width"], max_utts=1)
        bm.pass1_dev(d_scores.ptr, ms.S, off)
        r = bm.results()[0]
        return r.status, list(r.wseq[:r.wnum]), r.score, r.natom, lexblob.canonical_trellis(bm.trellis(0))

    d_fr = lib.DevBuf(engine, frames.nbytes).upload(frames)
    d_sc = lib.DevBuf(engine, want.nbytes)
    ms.outprob_dev(d_fr.ptr, len(frames), d_sc.ptr)
    got = pass1(d_sc)
    assert np.array_equal(d_sc.download(want.shape, np.float32), want)
    ref = pass1(lib.DevBuf(engine, want.nbytes).upload(want))
    assert got[:4] == ref[:4] and got[3] > 0
    assert all(np.array_equal(got[4][k], ref[4][k]) for k in ref[4])
