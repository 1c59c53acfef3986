"""Multi-stream GMM acoustic models for the tests of jamd_gmm_ms: the model as a dict of the arrays of
jamd_gmm_ms_desc, its HTK ascii form, the compiled reference's scores for it, and the cases of the committed fixture
tests/golden/gmm_streams.npz (written by tests/make_golden_streams.py).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from julius_amd import synth

GOLDEN = Path(__file__).resolve().parent / "golden" / "gmm_streams.npz"
LOG_ZERO = np.float32(-1000000.0)
MODEL_KEYS = ("vsize", "pdf_stream", "pdf_off", "pdf_named", "ent_dens", "weight", "st_pdf", "st_weight", "has_sw",
              "dens_off", "mean", "var")


def _finish(m):
    """The arrays the reference derives on loading: ivar (htk_hmm_inverse_variances(): 1.0 / v in double), gconst
    (update_gconst(), rdhmmdef_dens.c:39-48, per density over ITS length) and ln w (rdhmmdef_mpdf.c:189; LOG_ZERO for
    a <Mixture> the file leaves out, :174)."""
    m = dict(m)
    m["ivar"] = (1.0 / m["var"].astype(np.float64)).astype(np.float32)
    off = m["dens_off"]
    m["gconst"] = np.array([synth.gconst_of(m["var"][off[g]:off[g + 1]]) for g in range(len(off) - 1)], np.float32)
    with np.errstate(divide="ignore"):
        lw = np.log(m["weight"]).astype(np.float32)
    lw[m["ent_dens"] < 0] = LOG_ZERO
    m["ent_logw"] = lw
    m["nstream"] = len(m["vsize"])
    m["veclen"] = int(np.sum(m["vsize"]))
    return m


def make_streams_model(vsize, S, mix_range=(1, 3), seed=0, no_sweights=(), zero_weight=(), all_zero=(), null=(),
                       share=(), unit_weights=False):
    """S states over streams of the lengths `vsize`; every stream of every state has its own mixture pdf of
    mix_range[0] .. mix_range[1] Gaussians (drawn per pdf) and every state its own stream weights in [0.2, 1.5).
      no_sweights   states written without <SWeights> (weights 1.0)
      zero_weight   (state, stream) pairs whose weight is 0
      all_zero      states whose weights are all 0
      null          (state, stream, mixture) triples left without a density (a NULL density, ln w = LOG_ZERO)
      share         (from, to, stream): state `to` uses state `from`'s pdf of that stream (a `~p` macro)
      unit_weights  every weight 1.0 and no <SWeights> anywhere"""
    rng = np.random.default_rng(seed)
    vsize = np.asarray(vsize, np.int32)
    ns, D = len(vsize), int(vsize.sum())
    soff = np.concatenate([[0], np.cumsum(vsize)])
    centre = rng.normal(0.0, 1.0, size=(S, D)).astype(np.float32)
    pdf_stream, pdf_off, ent_dens, weight, dens_off, mean, var = [], [0], [], [], [0], [], []
    st_pdf = np.zeros((S, ns), np.int32)
    shared = {(to, k): frm for frm, to, k in share}
    nullset = set(null)
    for s in range(S):
        for k in range(ns):
            if (s, k) in shared:
                st_pdf[s, k] = st_pdf[shared[(s, k)], k]
                continue
            n = int(rng.integers(mix_range[0], mix_range[1] + 1))
            w = rng.dirichlet(np.full(n, 2.0)) if n > 1 else np.ones(1)
            st_pdf[s, k] = len(pdf_stream)
            pdf_stream.append(k)
            for i in range(n):
                weight.append(float(f"{max(w[i], 1e-5):.6e}"))     # as parsed back from 6 significant digits
                if (s, k, i) in nullset:
                    ent_dens.append(-1)
                    continue
                ent_dens.append(len(dens_off) - 1)
                mean.append((centre[s, soff[k]:soff[k + 1]] + rng.normal(0.0, 0.5, vsize[k])).astype(np.float32))
                var.append(rng.uniform(0.5, 2.0, vsize[k]).astype(np.float32))
                dens_off.append(dens_off[-1] + int(vsize[k]))
            pdf_off.append(len(ent_dens))
    st_weight = rng.uniform(0.2, 1.5, size=(S, ns)).astype(np.float32)
    has_sw = np.ones(S, bool)
    if unit_weights:
        no_sweights = range(S)
    for s in no_sweights:
        st_weight[s], has_sw[s] = 1.0, False
    for s, k in zero_weight:
        st_weight[s, k] = 0.0
    for s in all_zero:
        st_weight[s] = 0.0
    named = np.zeros(len(pdf_stream), bool)
    for (to, k), frm in shared.items():
        named[st_pdf[frm, k]] = True
    m = dict(vsize=vsize, pdf_stream=np.array(pdf_stream, np.int32), pdf_off=np.array(pdf_off, np.int32),
             pdf_named=named, ent_dens=np.array(ent_dens, np.int32), weight=np.array(weight, np.float64),
             st_pdf=st_pdf, st_weight=st_weight, has_sw=has_sw, dens_off=np.array(dens_off, np.int32),
             mean=np.concatenate(mean), var=np.concatenate(var))
    m = _finish(m)
    m["centre"] = centre
    return m


def make_streams_frames(model, T, seed=1, noise=1.0):
    """Frames that wander over the states' centres (synth.make_frames)."""
    return synth.make_frames(dict(mean=np.zeros((1, model["veclen"]), np.float32), centre=model["centre"]), T=T,
                             seed=seed, noise=noise)


def _vec(v):
    return " ".join(f"{float(x):.9e}" for x in v)


def _pdf_lines(model, p, with_nummixes):
    e0, e1 = int(model["pdf_off"][p]), int(model["pdf_off"][p + 1])
    L = [f"<NUMMIXES> {e1 - e0}"] if with_nummixes else []
    for i, e in enumerate(range(e0, e1)):
        g = int(model["ent_dens"][e])
        if g < 0:
            continue                       # a missing <MIXTURE> leaves a NULL density in the reference
        a, b = int(model["dens_off"][g]), int(model["dens_off"][g + 1])
        L.append(f"<MIXTURE> {i + 1} {model['weight'][e]:.6e}")
        L.append(f"<MEAN> {b - a}\n {_vec(model['mean'][a:b])}")
        L.append(f"<VARIANCE> {b - a}\n {_vec(model['var'][a:b])}")
    return L


def write_streams_hmmdefs(path, model, kind="MFCC_E_D_A"):
    """HTK ascii hmmdefs of the model: `~o <STREAMINFO> n v1 .. vn`, shared pdfs as `~p` macros, every state an `~s`
    macro (state id = order of appearance) written as <NUMMIXES> m1 .. mn [<SWEIGHTS> n ..] <STREAM> k <MIXTURE> ..,
    and one single-state `~h` per state, so that any state count loads."""
    vs = [int(v) for v in model["vsize"]]
    ns, S = len(vs), model["st_pdf"].shape[0]
    L = [f"~o <STREAMINFO> {ns} " + " ".join(map(str, vs)) + f" <VECSIZE> {sum(vs)} <NULLD> <{kind}> <DIAGC>"]
    for p in np.nonzero(model["pdf_named"])[0]:
        L.append(f'~p "pdf{p}"\n<STREAM> {int(model["pdf_stream"][p]) + 1}')
        L += _pdf_lines(model, p, with_nummixes=True)
    for s in range(S):
        pdfs = [int(p) for p in model["st_pdf"][s]]
        L.append(f'~s "s{s}"')
        L.append("<NUMMIXES> " + " ".join(str(int(model["pdf_off"][p + 1] - model["pdf_off"][p])) for p in pdfs))
        if model["has_sw"][s]:
            L.append(f"<SWEIGHTS> {ns}\n {_vec(model['st_weight'][s])}")
        for k, p in enumerate(pdfs):
            if ns > 1:
                L.append(f"<STREAM> {k + 1}")
            if model["pdf_named"][p]:
                L.append(f'~p "pdf{p}"')
            else:
                L += _pdf_lines(model, p, with_nummixes=False)
    L.append('~t "t0"\n<TRANSP> 3\n 0.000000e+00 1.000000e+00 0.000000e+00\n 0.000000e+00 6.000000e-01 4.000000e-01\n'
             ' 0.000000e+00 0.000000e+00 0.000000e+00')
    for s in range(S):
        L.append(f'~h "p{s}"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n~s "s{s}"\n~t "t0"\n<ENDHMM>')
    Path(path).write_text("\n".join(L) + "\n")


def ref_scores(ref, hmmdefs, frames, nstate=None):
    """[T][S] log10 scores of the UNMODIFIED reference for an hmmdefs (ascii or binary): init_hmminfo() /
    outprob_init() under -gprune none, then outprob_state() for every state of every frame.  Straight through
    ref.lib: pyoracle.RefAM flattens the model on construction, which a multi-stream model does not survive.
    nstate: the row length, which no tap tells without flattening; by default the `~s` macros of the ascii file."""
    lib = ref.lib
    if nstate is None:
        nstate = len({line for line in Path(hmmdefs).read_text().splitlines() if line.startswith('~s "')})
    h = lib.jref_am_load(str(hmmdefs).encode(), None, 1, 0, 1, 3)      # GPRUNE_SEL_NONE, IWCD max
    if not h:
        raise RuntimeError(f"reference failed to load {hmmdefs}")
    fr = np.ascontiguousarray(frames, np.float32)
    out = np.full((fr.shape[0], nstate), np.nan, np.float32)
    lib.jref_am_outprob(C.c_void_p(h), fr.ctypes.data_as(C.c_void_p), fr.shape[0], out.ctypes.data_as(C.c_void_p))
    lib.jref_am_free(C.c_void_p(h))
    return out


def write_binhmm(ref, hmmdefs, binhmm):
    """mkbinhmm's work through the reference's own write_binhmm() (oracle/ref_driver.c)."""
    ref.lib.jref_write_binhmm.argtypes = [C.c_char_p, C.c_char_p]
    rc = ref.lib.jref_write_binhmm(str(hmmdefs).encode(), str(binhmm).encode())
    if rc != 0:
        raise RuntimeError(f"jref_write_binhmm failed ({rc})")
    return binhmm


# ---- the cases of the fixture -------------------------------------------------------------------------------
def _far(frames, model, t, streams):
    """Frame t moved so far from every Gaussian of `streams` that those streams fall below LOG_ZERO."""
    soff = np.concatenate([[0], np.cumsum(model["vsize"])])
    for k in streams:
        frames[t, soff[k]:soff[k + 1]] = 1.0e4
    return frames


def _case_branches():
    """Every branch of calc_mix() in one model of six states over (26, 10, 3):
    state 2 has no <SWeights>, state 4 a weight of 0, state 5 all weights 0, state 3 a NULL density in stream 2,
    state 1 shares state 0's pdf of stream 1 (a `~p` macro); frame 4 drives stream 1 of every state below LOG_ZERO
    (skipped), frame 5 every stream (LOG_ZERO out)."""
    m = make_streams_model((26, 10, 3), 6, (2, 3), seed=11, no_sweights=(2,), zero_weight=((4, 1),), all_zero=(5,),
                           null=((3, 2, 0),), share=((0, 1, 1), (2, 4, 0)))
    fr = make_streams_frames(m, 7, seed=12)
    _far(fr, m, 4, (1,))
    _far(fr, m, 5, (0, 1, 2))
    return m, fr


def _case_e2e():
    """A two-stream (26 + 13) model over the 120 states of the golden lexicon beam_rank.npz: every state's two
    streams are the two halves of its first Gaussian, so that the scores still follow the golden utterance."""
    z = np.load(GOLDEN.parent / "beam_rank.npz")
    S = len(z["am_st_off"]) - 1
    g = z["am_ent_dens"][z["am_st_off"][:-1]]
    mean, ivar = z["am_mean"][g], z["am_ivar"][g]
    var = (1.0 / ivar.astype(np.float64)).astype(np.float32)
    vs = np.array([26, 13], np.int32)
    rng = np.random.default_rng(5)
    m = dict(vsize=vs, pdf_stream=np.tile(np.array([0, 1], np.int32), S), pdf_off=np.arange(2 * S + 1, dtype=np.int32),
             pdf_named=np.zeros(2 * S, bool), ent_dens=np.arange(2 * S, dtype=np.int32), weight=np.ones(2 * S),
             st_pdf=np.arange(2 * S, dtype=np.int32).reshape(S, 2),
             st_weight=rng.uniform(0.7, 1.3, size=(S, 2)).astype(np.float32), has_sw=np.ones(S, bool),
             dens_off=np.concatenate([[0], np.cumsum(np.tile(vs, S))]).astype(np.int32),
             mean=mean.reshape(-1).copy(), var=var.reshape(-1).copy())
    return _finish(m), z["u0_frames"].astype(np.float32)


def _simple(vsize, S, T, seed, mix_range=(1, 2), **kw):
    m = make_streams_model(vsize, S, mix_range, seed=seed, **kw)
    return m, make_streams_frames(m, T, seed=seed + 1000)


# name -> (model, frames).  Layouts at D = 39 and one at D = 30, ragged mixture counts over four streams, the state
# counts around the 16-state tile (130 frames: a full wave and two frames of the next), 513 frames over 17 states
# (the kernel takes 128 frames a wave and 512 a block; the shorter calls of the GPU test are prefixes of it), a
# single-stream model, calc_mix()'s branches and the model of the first-pass case.  The tile-edge cases use short
# vectors (what they probe does not depend on the layout) to keep the fixture small.
CASES = {
    "lay_26_13": lambda: _simple((26, 13), 5, 40, 1),
    "lay_13_13_13": lambda: _simple((13, 13, 13), 5, 40, 2),
    "lay_12_12_12_3": lambda: _simple((12, 12, 12, 3), 5, 40, 3),
    "lay_38_1": lambda: _simple((38, 1), 5, 40, 4),
    "lay_10_20": lambda: _simple((10, 20), 5, 40, 5),
    "ragged4": lambda: _simple((20, 9, 7, 3), 7, 40, 6, mix_range=(1, 5)),
    "S1": lambda: _simple((9, 4), 1, 130, 21),
    "S15": lambda: _simple((9, 4), 15, 130, 22),
    "S16": lambda: _simple((9, 4), 16, 130, 23),
    "S33": lambda: _simple((9, 4), 33, 130, 24),
    "S17_T513": lambda: _simple((7, 5), 17, 513, 25),
    "one_stream": lambda: _simple((39,), 9, 40, 26, mix_range=(1, 4), unit_weights=True),
    "branches": _case_branches,
    "e2e": _case_e2e,
}


BINHMM_CASES = ("branches", "ragged4", "one_stream")      # the fixture also holds these models' binary HMM files


def load_binhmm(name, path):
    """The committed binary HMM file of a case, written out to `path`."""
    Path(path).write_bytes(np.load(GOLDEN)[f"{name}/binhmm"].tobytes())
    return path


def load_case(name):
    """(model, frames, the reference's scores) of a case from the committed fixture."""
    z = np.load(GOLDEN)
    m = _finish({k: z[f"{name}/{k}"] for k in MODEL_KEYS})
    frames = z[f"{name}/frames"] if f"{name}/frames" in z.files else CASES[name]()[1]   # (e2e: the golden utterance)
    return m, frames, z[f"{name}/scores"]


# ---- what jamd_gmm_ms_create() refuses, each with the field its message names ------------------------------
def _set(key, fn):
    def apply(m):
        m = dict(m)
        m[key] = fn(np.array(m[key], copy=True), m)
        return m
    return apply


def _put(a, idx, v):
    a[idx] = v
    return a


def _tied(m):
    m = dict(m)
    m["pdf_book"] = np.full(len(m["pdf_stream"]), -1, np.int32)
    m["pdf_book"][1] = 0
    return m


def _nstream(n):
    def apply(m):
        m = dict(m)
        m["nstream"] = n
        return m
    return apply


# id -> (change to a good two-stream model, what the message must say)
REFUSALS = {
    "nstream_0": (_nstream(0), r"nstream=0"),
    "nstream_51": (_nstream(51), r"nstream=51"),
    "vsize_sum": (_set("vsize", lambda a, m: _put(a, 1, a[1] + 1)), r"vsize sums to 40, veclen is 39"),
    "pdf_stream_slot": (_set("st_pdf", lambda a, m: _put(a, (2, 0), a[2, 1])), r"st_pdf\[2\]\[0\] names pdf \d+, whose pdf_stream is 1"),
    "st_pdf_range": (_set("st_pdf", lambda a, m: _put(a, (1, 1), len(m["pdf_stream"]))), r"st_pdf\[1\]\[1\]=\d+ out of range"),
    "st_pdf_negative": (_set("st_pdf", lambda a, m: _put(a, (0, 0), -1)), r"st_pdf\[0\]\[0\]=-1 out of range"),
    "ent_dens_range": (_set("ent_dens", lambda a, m: _put(a, 0, len(m["gconst"]))), r"ent_dens\[0\]=\d+ out of range"),
    "pdf_stream_range": (_set("pdf_stream", lambda a, m: _put(a, 0, 2)), r"pdf_stream\[0\]=2 out of range"),
    "dens_length": (_set("ent_dens", lambda a, m: _put(a, 0, a[m["pdf_off"][1]])), r"density \d+ has length 13, the vsize of stream 0 \(pdf 0\) is 26"),
    "weight_nan": (_set("st_weight", lambda a, m: _put(a, (3, 1), np.nan)), r"st_weight\[3\]\[1\] is not finite"),
    "weight_inf": (_set("st_weight", lambda a, m: _put(a, (0, 0), np.inf)), r"st_weight\[0\]\[0\] is not finite"),
    "tied_mixture": (_tied, r"pdf 1 is a tied-mixture pdf"),
}


def refusal_model():
    """The good model the REFUSALS are applied to (the fixture's first layout case: 5 states over 26 + 13)."""
    return load_case("lay_26_13")[0]
