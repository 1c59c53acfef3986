"""GPU: multi-stream GMM scoring (jamd_gmm_ms, kernel K1m) bit for bit against the compiled reference's scores in
tests/golden/gmm_streams.npz -- and against the live reference where oracle/_ref is present."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import streamsref  # noqa: E402
from beamutil import assert_trellis_equal_modulo_ties, load_beam_golden  # noqa: E402
from julius_amd import lexblob, lib, synth  # noqa: E402
from oracle import pyoracle  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def _case(name):
    """(model, frames, the reference's scores) of a fixture case, loaded once and left unchanged."""
    if name not in _cache:
        _cache[name] = streamsref.load_case(name)
    return _cache[name]


def _live(tmp_path, model, frames):
    """The live reference's scores, or None where oracle/_ref is not present."""
    if not pyoracle.REF_SO.exists():
        return None
    path = tmp_path / "hmmdefs"
    streamsref.write_streams_hmmdefs(path, model)
    return streamsref.ref_scores(pyoracle.Ref(), path, frames)


@pytest.mark.parametrize("name", [n for n in streamsref.CASES if n != "e2e"])
def test_case_is_bit_exact(engine, tmp_path, name):
    """Layouts at D = 39 and D = 30, ragged mixtures over four streams, state counts round the 16-state tile, 513
    frames, one stream, and every branch of calc_mix() (case `branches`)."""
    model, frames, want = _case(name)
    g = lib.GmmStreams(engine, model)
    assert (g.S, g.D, g.nstream) == (want.shape[1], frames.shape[1], len(model["vsize"]))
    got = g.outprob_host(frames)
    assert g.last_kernel().startswith("gmm_ms<")
    assert np.array_equal(got, want)
    live = _live(tmp_path, model, frames)
    assert live is None or np.array_equal(got, live)
    g.close()


@pytest.mark.parametrize("T", [1, 127, 128, 129, 513])
def test_wave_and_block_edges(engine, T):
    """128 frames a wave, 512 a block: calls that end one short of, on and one past those."""
    model, frames, want = _case("S17_T513")
    g = lib.GmmStreams(engine, model)
    assert np.array_equal(g.outprob_host(frames[:T]), want[:T])
    g.close()


def test_branches_of_calc_mix(engine):
    """What the fixture's `branches` case holds arrives: LOG_ZERO where every stream is skipped and where all
    weights are 0, a finite score where one stream is skipped -- equal to the reference's (above), spelt out here."""
    model, frames, want = _case("branches")
    got = lib.GmmStreams(engine, model).outprob_host(frames)
    assert (got[5] == lib.LOG_ZERO).all() and (got[:, 5] == lib.LOG_ZERO).all()
    assert (got[4, :5] > lib.LOG_ZERO).all() and np.array_equal(got, want)


def test_one_stream_equals_k1(engine):
    """nstream = 1 through the new entry: the same bits as lib.Gmm on the same model."""
    model, frames, want = _case("one_stream")
    assert np.array_equal(model["st_pdf"][:, 0], np.arange(len(want[0])))          # pdf p is state p's
    flat = dict(mean=model["mean"].reshape(-1, 39), ivar=model["ivar"].reshape(-1, 39), gconst=model["gconst"],
                st_off=model["pdf_off"], ent_dens=model["ent_dens"], ent_logw=model["ent_logw"], st_book=None,
                nbook=0, nstream=1)
    k1 = lib.Gmm(engine, flat).outprob_host(frames)
    assert np.array_equal(lib.GmmStreams(engine, model).outprob_host(frames), k1)
    # ... and at a length where lib.Gmm runs K1 itself, not its narrow form
    m = synth.make_gmm(S=20, M=3, D=39, seed=3, ragged=True, null_frac=0.1)
    fr = synth.make_frames(m, T=300, seed=4)
    S, E = len(m["st_off"]) - 1, len(m["ent_dens"])
    ms = dict(vsize=[39], pdf_stream=np.zeros(S, np.int32), pdf_off=m["st_off"], ent_dens=m["ent_dens"],
              ent_logw=m["ent_logw"], st_pdf=np.arange(S, dtype=np.int32).reshape(S, 1), st_weight=None,
              dens_off=39 * np.arange(E + 1, dtype=np.int32), mean=m["mean"], ivar=m["ivar"], gconst=m["gconst"])
    gm = lib.Gmm(engine, m)
    k1 = gm.outprob_host(fr)
    assert "gmm_tile<" in gm.last_kernel()
    assert np.array_equal(lib.GmmStreams(engine, ms).outprob_host(fr), k1)


def test_dev_on_a_side_stream_equals_host(engine):
    model, frames, want = _case("S33")
    g = lib.GmmStreams(engine, model)
    s = C.c_void_p()
    assert lib.load().jamd_stream_create(engine.h, C.byref(s)) == 0
    try:
        d_fr = lib.DevBuf(engine, frames.nbytes).upload(frames)
        d_out = lib.DevBuf(engine, want.nbytes)
        g.outprob_dev(d_fr.ptr, len(frames), d_out.ptr, stream=s.value)
        assert lib.load().jamd_stream_sync(engine.h, s) == 0
        got = d_out.download(want.shape, np.float32)
    finally:
        lib.load().jamd_stream_destroy(engine.h, s)
    assert np.array_equal(got, want) and np.array_equal(g.outprob_host(frames), want)


@pytest.mark.parametrize("name", streamsref.BINHMM_CASES)
def test_from_binhmm_equals_descriptor(engine, tmp_path, name):
    """mkbinhmm's file (the reference's write_binhmm(): committed, and written afresh where oracle/_ref is present)
    read by the library itself scores as the descriptor path."""
    model, frames, want = _case(name)
    g = lib.GmmStreams.from_binhmm(engine, streamsref.load_binhmm(name, tmp_path / "committed.binhmm"))
    assert (g.S, g.D, g.nstream) == (want.shape[1], frames.shape[1], len(model["vsize"]))
    assert np.array_equal(g.outprob_host(frames), want)
    if pyoracle.REF_SO.exists():
        streamsref.write_streams_hmmdefs(tmp_path / "hmmdefs", model)
        fresh = streamsref.write_binhmm(pyoracle.Ref(), tmp_path / "hmmdefs", tmp_path / "fresh.binhmm")
        assert np.array_equal(lib.GmmStreams.from_binhmm(engine, fresh).outprob_host(frames), want)


def test_damaged_files_are_refused(engine, tmp_path):
    raw = streamsref.load_binhmm("branches", tmp_path / "binhmm").read_bytes()
    for k in range(1, 7):
        (tmp_path / "cut").write_bytes(raw[:len(raw) * k // 8])
        with pytest.raises(lib.JamdError):
            lib.GmmStreams.from_binhmm(engine, tmp_path / "cut")
    (tmp_path / "junk").write_bytes(b"JBINHMMV2\0_Q\0" + b"\0" * 64)
    with pytest.raises(lib.JamdError, match="unknown header qualifier"):
        lib.GmmStreams.from_binhmm(engine, tmp_path / "junk")
    with pytest.raises(lib.JamdError, match="3 streams"):         # the single-stream entry keeps its refusal
        lib.Gmm.from_binhmm(engine, tmp_path / "binhmm")


@pytest.mark.parametrize("name", list(streamsref.REFUSALS))
def test_create_refusals(engine, name):
    change, pattern = streamsref.REFUSALS[name]
    with pytest.raises(lib.JamdError, match=r"jamd_gmm_ms_create: .*" + pattern):
        lib.GmmStreams(engine, change(streamsref.refusal_model()))


def test_single_stream_entry_still_refuses_two_streams(engine):
    m = dict(synth.make_gmm(S=6, M=2, D=39, seed=1))
    m["nstream"] = 2
    with pytest.raises(lib.JamdError, match=re.escape("jamd_gmm_create: nstream=2; only single-stream models are supported")):
        lib.Gmm(engine, m)


def test_two_stream_model_feeds_the_first_pass(engine, oracle):
    """A 26 + 13 model over the golden lexicon's 120 states: its device matrix goes straight into lib.Beam.pass1_dev,
    and the result is the oracle's first pass over the reference's scores for the same model and frames."""
    model, frames, want = _case("e2e")
    g = load_beam_golden("beam_rank.npz")
    assert np.array_equal(frames, g["utts"][0]["frames"]) and want.shape[1] == len(g["am"]["st_off"]) - 1
    ms = lib.GmmStreams(engine, model)
    lx = lib.Lexicon(engine, g["lex"])
    bm = lib.Beam(engine, lx, g["beam_width"], g["score_pruning_width"], max_utts=1)
    d_fr = lib.DevBuf(engine, frames.nbytes).upload(frames)
    d_sc = lib.DevBuf(engine, want.nbytes)
    ms.outprob_dev(d_fr.ptr, len(frames), d_sc.ptr)
    bm.pass1_dev(d_sc.ptr, ms.S, np.array([0, len(frames)], np.int32))
    r = bm.results()[0]
    assert np.array_equal(d_sc.download(want.shape, np.float32), want)
    oatoms, owseq, oscore, rc, died = oracle.beam_pass1(g["lex"], want, g["beam_width"], g["score_pruning_width"])
    assert r.status == rc == 0
    assert list(r.wseq[:r.wnum]) == list(owseq) and r.score == oscore
    assert_trellis_equal_modulo_ties(bm.trellis(0), lexblob.canonical_trellis(oatoms), r.ties)
