"""Tied-mixture models with codebooks of UNEQUAL size for the tests of the pruned / tied-mixture GMM kernels
(csrc/gmm_pruned.hip), their HTK text form for the compiled reference, and small helpers shared by
test_gmm_pruned_edges_gpu.py and test_oracle_vs_ref.py.  synth.make_tied_gmm / synth.write_hmmdefs know one
codebook size per model; everything here is plain numpy."""
from pathlib import Path

import numpy as np

from julius_amd import synth

LOG_ZERO = np.float32(-1000000.0)


def make_tied(sizes, S, D=39, seed=0, dup=False, null=(), books=None):
    """Flat all-tied model (jamd_gmm_desc keys plus `var`, `weight`, `sizes`): codebook b has sizes[b] Gaussians,
    every state is a weight vector over one codebook.  The states reference the codebooks in an order that is NOT
    ascending by id (the first states walk the ids downwards, the rest are random).  S % 3 == 0 (three-state HMMs).
      dup    copy Gaussian 0 of every codebook of size >= 4 into slots 2 and K - 1 (exact score ties; the weights differ)
      null   (book, slot) pairs that are NULL densities in every state of that book: ent_dens = -1, ent_logw = LOG_ZERO
      books  the codebook ids the states may reference (default: all); the others stay unused"""
    assert S % 3 == 0
    rng = np.random.default_rng(seed)
    sizes = [int(k) for k in sizes]
    nbook = len(sizes)
    boff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    G = int(boff[-1])
    mean = rng.normal(0.0, 1.5, size=(G, D)).astype(np.float32)
    var = rng.uniform(0.5, 2.0, size=(G, D)).astype(np.float32)
    if dup:
        for b, K in enumerate(sizes):
            if K >= 4:
                for k in (2, K - 1):
                    mean[boff[b] + k] = mean[boff[b]]
                    var[boff[b] + k] = var[boff[b]]
    used = list(range(nbook)) if books is None else [int(b) for b in books]
    assert S >= len(used)
    st_book = np.asarray(used, np.int32)[rng.integers(0, len(used), size=S)]
    st_book[:len(used)] = used[::-1]                       # every listed codebook used, ids descending
    st_off = np.concatenate([[0], np.cumsum([sizes[b] for b in st_book])]).astype(np.int32)
    ent_dens = np.concatenate([np.arange(boff[b], boff[b + 1]) for b in st_book]).astype(np.int32)
    weight = np.empty(int(st_off[-1]), dtype=np.float64)
    for s in range(S):
        K = sizes[st_book[s]]
        w = rng.dirichlet(np.full(K, 0.3)) if K > 1 else np.ones(1)
        weight[st_off[s]:st_off[s + 1]] = np.array([float(f"{x:.6e}") for x in np.maximum(w, 1e-7)])
    ent_logw = np.log(weight).astype(np.float32)
    for b, k in null:
        for s in np.nonzero(st_book == b)[0]:
            ent_dens[st_off[s] + k] = -1
            ent_logw[st_off[s] + k] = LOG_ZERO
    return dict(mean=mean, var=var, ivar=(1.0 / var.astype(np.float64)).astype(np.float32), gconst=synth.gconst_of(var),
                weight=weight, st_off=st_off, ent_dens=ent_dens, ent_logw=ent_logw, st_book=st_book, nbook=nbook,
                nstream=1, sizes=np.asarray(sizes, np.int32), has_null=len(tuple(null)) > 0)


def book_sizes(model):
    """Size of every codebook as the states tied to it give it (0 for a codebook no state uses)."""
    n = np.zeros(int(model["nbook"]), np.int32)
    for s, b in enumerate(np.asarray(model["st_book"])):
        if b >= 0:
            n[b] = model["st_off"][s + 1] - model["st_off"][s]
    return n


def write_hmmdefs_tied(path, model, kind="MFCC_E_D_A"):
    """HTK ascii hmmdefs of a make_tied() model: ~m "book{b}_{k}" macros (k from 1, as <TMIX> counts them) and
    <TMIX> book{b}_ states, so the compiled reference loads codebooks of unequal size.  NULL densities inside a
    codebook cannot be written this way."""
    assert not model.get("has_null"), "a <TMIX> codebook has no way to leave a density out"
    S = len(model["st_off"]) - 1
    D = model["mean"].shape[1]
    boff = np.concatenate([[0], np.cumsum(model["sizes"])])
    L = [f"~o <STREAMINFO> 1 {D} <VECSIZE> {D} <NULLD> <{kind}> <DIAGC>"]
    for b in range(model["nbook"]):
        for k in range(int(model["sizes"][b])):
            g = int(boff[b]) + k
            L.append(f'~m "book{b}_{k + 1}"')
            L.append(f"<MEAN> {D}\n {synth._vec(model['mean'][g])}")
            L.append(f"<VARIANCE> {D}\n {synth._vec(model['var'][g])}")
    for s in range(S):
        e0, e1 = int(model["st_off"][s]), int(model["st_off"][s + 1])
        L.append(f'~s "s{s}"\n<NUMMIXES> {e1 - e0}')
        L.append(f"<TMIX> book{int(model['st_book'][s])}_ " + " ".join(f"{w:.6e}" for w in model["weight"][e0:e1]))
    L.append('~t "t0"\n<TRANSP> 5')
    for row in ([0, 1, 0, 0, 0], [0, .6, .4, 0, 0], [0, 0, .6, .4, 0], [0, 0, 0, .7, .3], [0, 0, 0, 0, 0]):
        L.append(" " + " ".join(f"{x:.6e}" for x in row))
    for i in range(S // 3):
        L.append(f'~h "p{i}"\n<BEGINHMM>\n<NUMSTATES> 5')
        L.append(f'<STATE> 2\n~s "s{3 * i}"\n<STATE> 3\n~s "s{3 * i + 1}"\n<STATE> 4\n~s "s{3 * i + 2}"')
        L.append('~t "t0"\n<ENDHMM>')
    Path(path).write_text("\n".join(L) + "\n")


def load_tied(ref, tmp_path, model, gprune, n):
    """The model written out and loaded by the compiled reference: (RefAM, its exported flat arrays).  The
    export is what device and oracle are given, so that codebook ids mean the same on every side."""
    kind = "MFCC_E_D_A" if model["mean"].shape[1] == 39 else "USER"
    path = Path(tmp_path) / "tied_hmmdefs"
    write_hmmdefs_tied(path, model, kind=kind)
    am = ref.am_load(path, gprune=gprune, gprune_num=n)
    assert am.is_tied and am.nbook == model["nbook"]
    ex = am.export()
    assert sorted(book_sizes(ex)) == sorted(int(k) for k in model["sizes"])
    return am, ex


def compound(tied, plain):
    """Tied-mixture states followed by plain states in one flat model (calc_compound_mix, calc_tied_mix.c:258)."""
    G0 = tied["mean"].shape[0]
    Sp = len(plain["st_off"]) - 1
    return dict(
        mean=np.concatenate([tied["mean"], plain["mean"]]), ivar=np.concatenate([tied["ivar"], plain["ivar"]]),
        gconst=np.concatenate([tied["gconst"], plain["gconst"]]),
        st_off=np.concatenate([tied["st_off"], tied["st_off"][-1] + plain["st_off"][1:]]).astype(np.int32),
        ent_dens=np.concatenate([tied["ent_dens"], np.where(plain["ent_dens"] >= 0, plain["ent_dens"] + G0, -1)]).astype(np.int32),
        ent_logw=np.concatenate([tied["ent_logw"], plain["ent_logw"]]),
        st_book=np.concatenate([tied["st_book"], -np.ones(Sp, np.int32)]).astype(np.int32),
        nbook=int(tied["nbook"]), nstream=1)


def triplicate(model):
    """A plain model in which entries 1 and 3 of every state that has them share entry 0's density (exact score
    ties inside a state); the weights stay distinct."""
    m = dict(model, ent_dens=model["ent_dens"].copy())
    for s in range(len(m["st_off"]) - 1):
        e0, e1 = int(m["st_off"][s]), int(m["st_off"][s + 1])
        for k in (1, 3):
            if e0 + k < e1 and m["ent_dens"][e0 + k] >= 0:
                m["ent_dens"][e0 + k] = m["ent_dens"][e0]
    return m


def far_frames(frames, every2=50.0, every4=400.0):
    """Every second frame scaled by 50 and every fourth by 400: far from every Gaussian (the LOG_ADDMIN cutoff,
    log-sums of exactly LOG_ZERO)."""
    fr = np.array(frames, np.float32, copy=True)
    fr[1::2] *= np.float32(every2)
    fr[3::4] *= np.float32(every4 / every2)
    return fr


def frame_by_frame(oracle, model, frames, gprune, n):
    """Every frame scored as an utterance of its own: no frame sees a predecessor's winners."""
    return np.concatenate([oracle.gmm_outprob(model, frames[t:t + 1], gprune, n) for t in range(len(frames))])


def write_rejection_gmm(path, model, names, kind="MFCC_E_D_A"):
    """The -gmm file of synth.make_rejection_gmm() written again from a (changed) flat model."""
    D = model["mean"].shape[1]
    L = [f"~o <STREAMINFO> 1 {D} <VECSIZE> {D} <NULLD> <{kind}> <DIAGC>"]
    for s, name in enumerate(names):
        e0, e1 = int(model["st_off"][s]), int(model["st_off"][s + 1])
        L.append(f'~h "{name}"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n<NUMMIXES> {e1 - e0}')
        for m, e in enumerate(range(e0, e1)):
            if model["ent_dens"][e] < 0:
                continue
            L.append(f"<MIXTURE> {m + 1} {model['weight'][e]:.6e}")
            L.append(f"<MEAN> {D}\n {synth._vec(model['mean'][model['ent_dens'][e]])}")
            L.append(f"<VARIANCE> {D}\n {synth._vec(model['var'][model['ent_dens'][e]])}")
        L.append("<TRANSP> 3\n 0.0 1.0 0.0\n 0.0 0.6 0.4\n 0.0 0.0 0.0\n<ENDHMM>")
    Path(path).write_text("\n".join(L) + "\n")
