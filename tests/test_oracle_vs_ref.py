"""CPU: oracle restatement vs the compiled reference on fresh seeded inputs
(more shapes than the committed fixtures).  Needs oracle/_ref/libjref.so, which
the dev container builds from /root/reference (oracle/Makefile)."""
import numpy as np
import pytest

import tiedref
from densref import dens_ref, gmax_winners, visiting_order_covered
from julius_amd import synth
from oracle import pyoracle as po


@pytest.mark.parametrize("S,M,D,ragged,nullf", [(30, 16, 39, False, 0.0), (27, 5, 26, True, 0.0),
                                                (12, 9, 13, True, 0.15), (9, 1, 39, False, 0.0)])
@pytest.mark.parametrize("gprune,n", [("none", 0), ("safe", 2), ("safe", 64)])
def test_plain_gmm(ref, oracle, tmp_path, S, M, D, ragged, nullf, gprune, n):
    m = synth.make_gmm(S=S, M=M, D=D, seed=S * 7 + M, ragged=ragged, null_frac=nullf)
    kind = "MFCC_E_D_A" if D == 39 else "USER"
    synth.write_hmmdefs(tmp_path / "h", m, kind=kind)
    am = ref.am_load(tmp_path / "h", gprune=gprune, gprune_num=n)
    ex = am.export()
    # the product-side flattening reproduces the loader's arrays
    for k in ("mean", "ivar", "gconst"):
        ok = ex["ent_dens"] >= 0
        assert np.array_equal(ex[k][ex["ent_dens"][ok]], m[k][m["ent_dens"][m["ent_dens"] >= 0]])
    assert np.array_equal(ex["st_off"], m["st_off"])
    assert np.array_equal(ex["ent_logw"], m["ent_logw"])
    fr = synth.make_frames(m, T=37, seed=3)
    want = am.outprob(fr)
    got = oracle.gmm_outprob(ex, fr, po.GPRUNE_NONE if gprune == "none" else po.GPRUNE_SAFE, n)
    assert np.array_equal(got, want)
    am.close()


@pytest.mark.parametrize("gprune,n", [("none", 64), ("safe", 1), ("safe", 2), ("safe", 8)])
def test_tied_gmm(ref, oracle, tmp_path, gprune, n):
    m = synth.make_tied_gmm(S=21, nbook=4, K=64, D=39, seed=5)
    synth.write_hmmdefs(tmp_path / "h", m)
    am = ref.am_load(tmp_path / "h", gprune=gprune, gprune_num=n)
    assert am.is_tied and am.nbook == 4
    ex = am.export()
    fr = synth.make_frames(m, T=45, seed=9, noise=2.0)
    got = oracle.gmm_outprob(ex, fr, po.GPRUNE_NONE if gprune == "none" else po.GPRUNE_SAFE, n)
    assert np.array_equal(got, am.outprob(fr))
    am.close()


@pytest.mark.parametrize("gprune", ["heu", "beam"])
@pytest.mark.parametrize("n,nbook,K,noise", [(1, 3, 64, 2.0), (2, 4, 64, 2.0), (4, 2, 129, 1.0), (10, 1, 40, 3.0), (64, 2, 24, 2.0)])
def test_tied_gmm_history_pruning(ref, oracle, tmp_path, gprune, n, nbook, K, noise):
    """SURVEY 8a A7, the tied-mixture half: gprune_heu() / gprune_beam() with a live last_id (`gprune_heu.c:305-335`,
    `gprune_beam.c:301-336`): the thresholds of frame t come from the codebook's cached winners of frame t-1
    (`calc_tied_mix.c:203-215`).  Under eager scoring (the batch loop `outprob.c:230-242`: every state of every frame)
    that history is deterministic, and the restatement must give the compiled reference's numbers and cache."""
    m = synth.make_tied_gmm(S=21, nbook=nbook, K=K, D=39, seed=K + n)
    synth.write_hmmdefs(tmp_path / "h", m)
    am = ref.am_load(tmp_path / "h", gprune=gprune, gprune_num=n)
    assert am.is_tied and am.nbook == nbook
    ex = am.export()
    fr = synth.make_frames(m, T=60, seed=9 + n, noise=noise)
    code = po.GPRUNE_HEU if gprune == "heu" else po.GPRUNE_BEAM
    want = am.outprob(fr)
    assert np.array_equal(oracle.gmm_outprob(ex, fr, code, n), want)
    safe = oracle.gmm_outprob(ex, fr, po.GPRUNE_SAFE, n)
    if n < 10:
        assert not np.array_equal(safe, want)              # these methods really prune differently from safe
    cap = n                                                 # the reference's cache rows are OP_gprune_num wide
    for b in range(nbook):
        sc, ids, num = am.tmix_cache(fr, b, cap)
        osc, oids, onum = oracle.tmix_topn(ex, b, fr, code, n)
        assert np.array_equal(num, onum)
        for t in range(len(fr)):
            assert np.array_equal(ids[t, :num[t]], oids[t, :num[t]]) and np.array_equal(sc[t, :num[t]], osc[t, :num[t]])
    am.close()


def test_lazy_equals_eager(ref, tmp_path):
    """outprob.c:245-247 (lazy cache fill) and :230-242 (batch) give the same values."""
    m = synth.make_gmm(S=15, M=4, D=39, seed=2)
    synth.write_hmmdefs(tmp_path / "h", m)
    am = ref.am_load(tmp_path / "h")
    fr = synth.make_frames(m, T=20, seed=4)
    full = am.outprob(fr)
    rng = np.random.default_rng(0)
    tt = np.sort(rng.integers(0, 20, 100)).astype(np.int32)
    ss = rng.integers(0, 15, 100).astype(np.int32)
    assert np.array_equal(am.outprob_list(fr, tt, ss), full[tt, ss])
    am.close()


@pytest.mark.parametrize("dims", [(48, 64, 64, 40), (40, 128, 128, 128, 128, 61), (528, 256, 256, 100)])
def test_dnn(ref, oracle, tmp_path, dims):
    if "FMA" not in ref.lib.jref_simd_string().decode():
        pytest.skip("host without FMA: the reference picks another SIMD kernel")
    dnn = synth.make_dnn(dims=dims, seed=dims[0])
    r = ref.dnn_load(dnn, tmp_path)
    fr = np.random.default_rng(1).normal(0, 1.5, (15, dims[0])).astype(np.float32)
    assert np.array_equal(oracle.dnn_outprob(dnn, fr, po.DNN_FMA), r.outprob(fr))


def test_gmm_blob_roundtrip(ref, tmp_path):
    """jamd_gmm_save() (reference-side shim) -> lexblob.load_gmm(): the same arrays the
    in-memory export gives, for a plain and a tied-mixture model."""
    from julius_amd import lexblob
    for name, m in (("plain", synth.make_gmm(S=12, M=3, D=39, seed=5, ragged=True)),
                    ("tied", synth.make_tied_gmm(S=12, nbook=2, K=8, D=39, seed=6))):
        synth.write_hmmdefs(tmp_path / name, m)
        am = ref.am_load(tmp_path / name)
        am.save_blob(tmp_path / f"{name}.blob")
        a, b = am.export(), lexblob.load_gmm(tmp_path / f"{name}.blob")
        for k in ("mean", "ivar", "gconst", "st_off", "ent_dens", "ent_logw"):
            assert np.array_equal(a[k], b[k]), (name, k)
        assert (a["st_book"] is None) == (b["st_book"] is None) and a["nbook"] == b["nbook"]
        if a["st_book"] is not None:
            assert np.array_equal(a["st_book"], b["st_book"])


def _gms_case(oracle, ref, tmp_path, nbest, **gs_args):
    """One selection model against the compiled reference on three utterances; returns what the caller needs to
    judge the inputs: the exported selection data, the utterances and their frame offsets."""
    task = synth.make_triphone_task(tmp_path, seed=5, nword=60)
    gpath, _ = synth.make_gs_model(task, seed=5, **gs_args)
    am = ref.am_load(task["hmmdefs"], task["hmmlist"], gshmm=gpath, gms_num=nbest)
    gs = am.gms()
    assert gs["nbest"] == nbest and len(gs["model"]["st_off"]) - 1 == 78
    full_model = ref.am_load(task["hmmdefs"], task["hmmlist"]).export()
    frames = []
    for u in range(3):
        fr, _ = synth.make_utterance(task, nwords=2 + u, seed=50 + u)
        want = am.outprob(fr)
        got = oracle.gms_apply(gs, fr, oracle.gmm_outprob(full_model, fr))
        used = gs["state2gs"] >= 0              # states outside every model: the reference reads out of bounds
        assert np.array_equal(got[:, used], want[:, used])
        assert 0.0 < (got[:, used] != oracle.gmm_outprob(full_model, fr)[:, used]).mean() < 1.0
        frames.append(fr)
    return gs, np.concatenate(frames), np.cumsum([0] + [len(f) for f in frames])


@pytest.mark.parametrize("nbest", [4, 8, 24])
def test_gaussian_mixture_selection(oracle, ref, tmp_path, nbest):
    """-gshmm / -gsnum: gms_state() (gms.c:394) returns the real score for states whose selection
    state is among the nbest of the frame and the selection state's score otherwise."""
    _gms_case(oracle, ref, tmp_path, nbest)


@pytest.mark.parametrize("nbest", [4, 24])
@pytest.mark.parametrize("M,ragged,null_frac", [(16, False, 0.0), (9, True, 0.0), (9, True, 0.15)])
def test_gaussian_mixture_selection_many_mixtures(oracle, ref, tmp_path, nbest, M, ragged, null_frac):
    """The same at the mixture counts of a real selection model, where compute_g_max()'s visiting order
    (gms_gprune.c:151-174: last frame's winner, then mix_num-1 .. 0 under a strict >) spans several groups of the
    device's four-wide loop -- the three-Gaussian model above never enters it.  The last case holds NULL densities:
    the reference reads them back from missing <Mixture> entries and calc_contprob_with_safe_pruning() scores them
    LOG_ZERO before it looks at anything else (gms_gprune.c:104), so they are deterministic and compared here too.
    The inputs must exercise the order: the winners of one state fall in all four classes of (n - 1 - k) % 4, inside
    four-wide groups and in the scalar tail, and a winner changes from one frame to the next."""
    gs, fr, utt_off = _gms_case(oracle, ref, tmp_path, nbest, M=M, ragged=ragged, null_frac=null_frac)
    m = gs["model"]
    assert int(np.diff(m["st_off"]).max()) == M and ((m["ent_dens"] < 0).any() == (null_frac > 0))
    win, _ = gmax_winners(m["st_off"], dens_ref(m, fr), utt_off)
    residues, changed, in_body, in_tail = visiting_order_covered(m["st_off"], win, utt_off)
    assert residues == {0, 1, 2, 3} and changed and in_body
    assert in_tail or M % 4 == 0 and not ragged


@pytest.mark.parametrize("num,null_frac", [(1, 0.0), (3, 0.2), (10, 0.0), (64, 0.1)])
def test_verification_gmm(oracle, ref, tmp_path, num, null_frac):
    """-gmm / -gmmnum: gmm_proceed() (libjulius/src/gmm.c:574-600) through the reference's own entry
    points, frame by frame, and gc->gmm_score[] / the winner after a whole input."""
    task = synth.make_triphone_task(tmp_path, seed=12, nword=60)
    gpath, _, names = synth.make_rejection_gmm(tmp_path, task["model"]["centre"], seed=12 + num, M=20, null_frac=null_frac)
    eng = po.RefEngine(ref, ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-nlr", task["arpa"],
                             "-input", "htkparam", "-gprune", "none", "-b", "120", "-gmm", str(gpath), "-gmmnum", str(num)])
    info = eng.gmm_info()
    assert info["nmodel"] == len(names) and info["gprune_num"] == num
    for u in range(2):
        fr, _ = synth.make_utterance(task, nwords=2 + u, seed=70 + u)
        want = eng.gmm_frame_scores(fr)
        got = oracle.rejgmm_frame_scores(info, fr)
        assert np.array_equal(got, want)
        synth.write_htk_param(tmp_path / "u.mfc", fr)
        eng.recognize(tmp_path / "u.mfc")
        sums, winner, cm, valid, nframe = eng.gmm_result()
        assert nframe == len(fr) and valid
        assert np.array_equal(oracle.rejgmm_accumulate(got), sums) and int(np.argmax(sums)) == winner


# ------------------------------------------------- shapes of tests/test_gmm_pruned_edges_gpu.py: the oracle's licence
CODES = {"safe": po.GPRUNE_SAFE, "heu": po.GPRUNE_HEU, "beam": po.GPRUNE_BEAM}


@pytest.mark.parametrize("sizes", [(3, 70, 64, 1, 129), (65, 8)])
@pytest.mark.parametrize("dup", [False, True])
def test_tied_gmm_unequal_codebooks(ref, oracle, tmp_path, sizes, dup):
    """Codebooks of unequal size (one of a single Gaussian, one smaller than the list) under safe / heu / beam at list
    sizes below, between and above the codebook sizes, with and without exactly tied Gaussians: state scores and the
    MIXCACHE of every codebook, oracle == compiled reference."""
    m = tiedref.make_tied(sizes, S=21, D=39, seed=len(sizes) + dup, dup=dup)
    fr = synth.make_frames(m, T=30, seed=11, noise=2.0)
    for gprune in ("safe", "heu", "beam"):
        for n in (1, 4, 17, 64):
            am, ex = tiedref.load_tied(ref, tmp_path, m, gprune, n)
            assert np.array_equal(oracle.gmm_outprob(ex, fr, CODES[gprune], n), am.outprob(fr)), (gprune, n)
            for b in range(len(sizes)):
                sc, ids, num = am.tmix_cache(fr, b, n)
                osc, oids, onum = oracle.tmix_topn(ex, b, fr, CODES[gprune], n)
                assert np.array_equal(num, onum), (gprune, n, b)
                for t in range(len(fr)):
                    k = num[t]
                    assert np.array_equal(ids[t, :k], oids[t, :k]) and np.array_equal(sc[t, :k], osc[t, :k]), (gprune, n, b, t)
            am.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_plain_safe_with_triplicated_densities(ref, oracle, n):
    """Exact score ties inside plain states under safe pruning: entries 1 and 3 share entry 0's density."""
    m = tiedref.triplicate(synth.make_gmm(S=20, M=6, D=39, seed=31, ragged=True, null_frac=0.05))
    fr = synth.make_frames(m, T=40, seed=32)
    want = ref.am_from_flat(m, gprune="safe", gprune_num=n).outprob(fr)
    assert np.array_equal(oracle.gmm_outprob(m, fr, po.GPRUNE_SAFE, n), want)
    assert np.array_equal(oracle.gmm_outprob(m, tiedref.far_frames(fr), po.GPRUNE_SAFE, n),
                          ref.am_from_flat(m, gprune="safe", gprune_num=n).outprob(tiedref.far_frames(fr)))


@pytest.mark.parametrize("num", [8, 32])
def test_verification_gmm_with_identical_mixtures(oracle, ref, tmp_path, num):
    """-gmmnum 8 and 32 (list sizes of their own on the device) with a model file in which two mixtures of one GMM
    are the same Gaussian: gmm.c's private pruning under exact ties, through the reference's own entry points."""
    task = synth.make_triphone_task(tmp_path, seed=12, nword=60)
    gpath, model, names = synth.make_rejection_gmm(tmp_path, task["model"]["centre"], seed=40 + num, M=40, ragged=False)
    for s in range(len(names)):
        e0 = int(model["st_off"][s])
        for k in (2, 39):
            model["mean"][model["ent_dens"][e0 + k]] = model["mean"][model["ent_dens"][e0]]
            model["var"][model["ent_dens"][e0 + k]] = model["var"][model["ent_dens"][e0]]
    tiedref.write_rejection_gmm(gpath, model, names)
    eng = po.RefEngine(ref, ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-nlr", task["arpa"],
                             "-input", "htkparam", "-gprune", "none", "-b", "120", "-gmm", str(gpath), "-gmmnum", str(num)])
    info = eng.gmm_info()
    assert info["nmodel"] == len(names) and info["gprune_num"] == num
    g = info["model"]
    e0 = int(g["st_off"][info["model_state"][0]])
    d0, d2 = g["ent_dens"][e0], g["ent_dens"][e0 + 2]
    assert np.array_equal(g["mean"][d0], g["mean"][d2]) and np.array_equal(g["ivar"][d0], g["ivar"][d2])
    fr, _ = synth.make_utterance(task, nwords=3, seed=71)
    assert np.array_equal(oracle.rejgmm_frame_scores(info, fr), eng.gmm_frame_scores(fr))


@pytest.mark.parametrize("sizes,n", [((16, 16), 2), ((16, 16), 16), ((65, 8), 2), ((65, 8), 4)])
def test_tied_safe_visiting_order_shows_under_exact_ties(oracle, sizes, n):
    """The premise of the GPU suite's tie case: with duplicated Gaussians in a codebook, tied-mixture safe pruning
    that starts from frame t - 1's winners (the reference, and the oracle over a whole utterance) gives other state
    scores than the same frames visited in index order (the oracle frame by frame)."""
    m = tiedref.make_tied(sizes, S=21, D=39, seed=7, dup=True)
    fr = synth.make_frames(m, T=75, seed=8, noise=2.0)
    full = oracle.gmm_outprob(m, fr, po.GPRUNE_SAFE, n)
    single = tiedref.frame_by_frame(oracle, m, fr, po.GPRUNE_SAFE, n)
    assert np.array_equal(full[0], single[0])
    rows = int((full != single).any(axis=1).sum())
    print(f"tie case {sizes} N={n}: {rows} of {len(fr)} rows differ")
    assert rows >= 1


@pytest.mark.parametrize("gprune", ["safe", "heu", "beam"])
@pytest.mark.parametrize("n", [3, 16])
def test_tied_gmm_far_frames(ref, oracle, tmp_path, gprune, n):
    """Frames 50 and 400 times too far out, the first frame of the utterance among them: where the kept scores lie below
    LOG_ZERO, compute_g_safe()'s LOG_ZERO for a pruned Gaussian is above the list's last entry and enters the list."""
    m = tiedref.make_tied((16, 24), S=21, D=39, seed=32)
    fr = tiedref.far_frames(synth.make_frames(m, T=40, seed=33, noise=2.0))
    fr[0] *= np.float32(400.0)
    am, ex = tiedref.load_tied(ref, tmp_path, m, gprune, n)
    want = am.outprob(fr)
    assert np.array_equal(oracle.gmm_outprob(ex, fr, CODES[gprune], n), want)
    assert (want == np.float32(-1000000.0)).any()
    lz = 0
    for b in range(2):
        sc, ids, num = am.tmix_cache(fr, b, n)
        osc, oids, onum = oracle.tmix_topn(ex, b, fr, CODES[gprune], n)
        assert np.array_equal(num, onum)
        for t in range(len(fr)):
            k = num[t]
            assert np.array_equal(ids[t, :k], oids[t, :k]) and np.array_equal(sc[t, :k], osc[t, :k]), (b, t)
            lz += int((sc[t, :k] == np.float32(-1000000.0)).sum())
    assert lz > 0
    am.close()
