"""Multi-stream GMM acoustic models with tied-mixture codebooks for the tests of jamd_gmm_ms_create_opt(): the model as
a dict of the arrays of jamd_gmm_ms_desc (streamsref's, plus pdf_book), its HTK ascii form, the compiled reference's
scores and codebook caches for it under -gprune none and safe, and the cases of the committed fixture
tests/golden/gmm_streams_tied.npz (written by tests/make_golden_streams_tied.py).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import streamsref
from streamsref import LOG_ZERO, write_binhmm  # noqa: F401  (re-exported)

GOLDEN = Path(__file__).resolve().parent / "golden" / "gmm_streams_tied.npz"
MODEL_KEYS = streamsref.MODEL_KEYS + ("pdf_book",)
REF_GPRUNE = {"none": 1, "safe": 2}        # GPRUNE_SEL_*, hmm_calc.h:45


def _finish(m):
    """streamsref._finish(), and bweight of a tied-mixture pdf: ln w of EVERY member, an undefined one included
    (tmix_read(), rdhmmdef_tiedmix.c:170-196)."""
    m = streamsref._finish(m)
    tied = np.repeat(m["pdf_book"] >= 0, np.diff(m["pdf_off"]))
    m["ent_logw"][tied] = np.log(m["weight"][tied]).astype(np.float32)
    return m


def make_tied_model(vsize, S, books, seed=0, plain=None, null_members=(), twins=(), no_sweights=(), zero_weight=(),
                    all_zero=()):
    """S states over streams of the lengths `vsize`.
      books         [(stream, K), ..] codebooks of K Gaussians.  A state's pdf of stream k is a weight vector over one
                    of that stream's books, taken in turn over the states, so that every book is used; the books are
                    numbered in the order the states first name them (GCODEBOOK.id, rdhmmdef_tiedmix.c:155)
      plain         {(state, stream): n}: that pdf is a plain mixture of n Gaussians of its own
      null_members  (book, member) pairs left undefined (no `~m` macro: a NULL density); `book` indexes `books`
      twins         (book, i, j): member j has member i's mean and variance (exactly tied scores)
      no_sweights, zero_weight, all_zero   as streamsref.make_streams_model()"""
    rng = np.random.default_rng(seed)
    vsize = np.asarray(vsize, np.int32)
    ns = len(vsize)
    plain = dict(plain or {})
    of_stream = [[b for b, (k, _) in enumerate(books) if k == s] for s in range(ns)]
    choice = {(s, k): of_stream[k][s % len(of_stream[k])] for s in range(S) for k in range(ns)
              if (s, k) not in plain}
    order = list(dict.fromkeys(choice[(s, k)] for s in range(S) for k in range(ns) if (s, k) in choice))
    assert sorted(order) == list(range(len(books))), "a book is not used"
    book_id = {b: i for i, b in enumerate(order)}
    dens_off, mean, var = [0], [], []

    def add_dens(mu, v):
        mean.append(np.asarray(mu, np.float32)); var.append(np.asarray(v, np.float32))
        dens_off.append(dens_off[-1] + len(mu))
        return len(dens_off) - 2

    members = {}
    for b in order:                              # densities in book-id order
        k, K = books[b]
        ids = []
        for i in range(K):
            if (b, i) in set(null_members):
                ids.append(-1)
                continue
            mu, v = rng.normal(0.0, 1.5, vsize[k]), rng.uniform(0.5, 2.0, vsize[k])
            for bb, a, j in twins:
                if bb == b and j == i:
                    mu, v = mean[ids[a]], var[ids[a]]
            ids.append(add_dens(mu, v))
        members[b] = ids
    pdf_stream, pdf_book, pdf_off, ent_dens, weight = [], [], [0], [], []
    st_pdf = np.zeros((S, ns), np.int32)
    for s in range(S):
        for k in range(ns):
            st_pdf[s, k] = len(pdf_stream)
            pdf_stream.append(k)
            if (s, k) in plain:
                n = plain[(s, k)]
                pdf_book.append(-1)
                ent_dens += [add_dens(rng.normal(0.0, 1.5, vsize[k]), rng.uniform(0.5, 2.0, vsize[k])) for _ in range(n)]
                w = rng.dirichlet(np.full(n, 2.0)) if n > 1 else np.ones(1)
            else:
                b = choice[(s, k)]
                pdf_book.append(book_id[b])
                ent_dens += members[b]
                w = rng.dirichlet(np.full(len(members[b]), 0.5))
            weight += [float(f"{max(x, 1e-5):.6e}") for x in w]
            pdf_off.append(len(ent_dens))
    st_weight = rng.uniform(0.2, 1.5, size=(S, ns)).astype(np.float32)
    has_sw = np.ones(S, bool)
    for s in no_sweights:
        st_weight[s], has_sw[s] = 1.0, False
    for s, k in zero_weight:
        st_weight[s, k] = 0.0
    for s in all_zero:
        st_weight[s] = 0.0
    m = dict(vsize=vsize, pdf_stream=np.array(pdf_stream, np.int32), pdf_off=np.array(pdf_off, np.int32),
             pdf_named=np.zeros(len(pdf_stream), bool), pdf_book=np.array(pdf_book, np.int32),
             ent_dens=np.array(ent_dens, np.int32), weight=np.array(weight, np.float64), st_pdf=st_pdf,
             st_weight=st_weight, has_sw=has_sw, dens_off=np.array(dens_off, np.int32),
             mean=np.concatenate(mean), var=np.concatenate(var))
    return _finish(m)


def make_tied_frames(model, T, seed=1, noise=1.0):
    """Frames whose stream slices wander over the means of the model's densities of that stream."""
    rng = np.random.default_rng(seed)
    soff = np.concatenate([[0], np.cumsum(model["vsize"])])
    out = np.empty((T, int(soff[-1])), np.float32)
    lens = np.diff(model["dens_off"])
    for k, n in enumerate(model["vsize"]):
        cand = np.nonzero(lens == n)[0]
        cand = np.array([g for g in cand if _stream_of_dens(model, g) == k])
        pick = np.repeat(rng.choice(cand, size=(T + 9) // 10), 10)[:T]
        base = np.stack([model["mean"][model["dens_off"][g]:model["dens_off"][g + 1]] for g in pick])
        out[:, soff[k]:soff[k + 1]] = base + rng.normal(0.0, noise, size=(T, n))
    return out


def _stream_of_dens(model, g):
    e = int(np.nonzero(model["ent_dens"] == g)[0][0])
    return int(model["pdf_stream"][np.searchsorted(model["pdf_off"], e, side="right") - 1])


def nbook(model):
    return int(model["pdf_book"].max()) + 1


def book_sizes(model):
    """members of every codebook, by id"""
    out = {}
    for p, b in enumerate(model["pdf_book"]):
        if b >= 0:
            out[int(b)] = int(model["pdf_off"][p + 1] - model["pdf_off"][p])
    return [out[b] for b in range(len(out))]


def write_tied_hmmdefs(path, model, kind="MFCC_E_D_A"):
    """HTK ascii hmmdefs of the model: `~o <STREAMINFO>`, the codebooks' members as `~m "bk<b>_<i>"` macros (an
    undefined member has none), every state an `~s` macro written as <NUMMIXES> m1 .. mn [<SWEIGHTS> n ..] <STREAM> k
    <TMIX> bk<b>_ w .. (or <MIXTURE> .. for a plain pdf), and one single-state `~h` per state."""
    vs = [int(v) for v in model["vsize"]]
    ns, S = len(vs), model["st_pdf"].shape[0]
    L = [f"~o <STREAMINFO> {ns} " + " ".join(map(str, vs)) + f" <VECSIZE> {sum(vs)} <NULLD> <{kind}> <DIAGC>"]
    done = set()
    for p, b in enumerate(model["pdf_book"]):
        if b < 0 or int(b) in done:
            continue
        done.add(int(b))
        for i, e in enumerate(range(int(model["pdf_off"][p]), int(model["pdf_off"][p + 1]))):
            g = int(model["ent_dens"][e])
            if g < 0:
                continue
            a, z = int(model["dens_off"][g]), int(model["dens_off"][g + 1])
            L.append(f'~m "bk{b}_{i + 1}"')
            L.append(f"<MEAN> {z - a}\n {streamsref._vec(model['mean'][a:z])}")
            L.append(f"<VARIANCE> {z - a}\n {streamsref._vec(model['var'][a:z])}")
    for s in range(S):
        pdfs = [int(p) for p in model["st_pdf"][s]]
        L.append(f'~s "s{s}"')
        L.append("<NUMMIXES> " + " ".join(str(int(model["pdf_off"][p + 1] - model["pdf_off"][p])) for p in pdfs))
        if model["has_sw"][s]:
            L.append(f"<SWEIGHTS> {ns}\n {streamsref._vec(model['st_weight'][s])}")
        for k, p in enumerate(pdfs):
            if ns > 1:
                L.append(f"<STREAM> {k + 1}")
            b = int(model["pdf_book"][p])
            if b >= 0:
                e0, e1 = int(model["pdf_off"][p]), int(model["pdf_off"][p + 1])
                L.append(f"<TMIX> bk{b}_ " + " ".join(f"{w:.6e}" for w in model["weight"][e0:e1]))
            else:
                L += streamsref._pdf_lines(model, p, with_nummixes=False)
    L.append('~t "t0"\n<TRANSP> 3\n 0.000000e+00 1.000000e+00 0.000000e+00\n 0.000000e+00 6.000000e-01 4.000000e-01\n'
             ' 0.000000e+00 0.000000e+00 0.000000e+00')
    for s in range(S):
        L.append(f'~h "p{s}"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n~s "s{s}"\n~t "t0"\n<ENDHMM>')
    Path(path).write_text("\n".join(L) + "\n")


# ---- the compiled reference ------------------------------------------------------------------------------------
class RefModel:
    """The UNMODIFIED reference with an hmmdefs (ascii or binary) loaded under one pruning mode: jref_am_load(path,
    NULL, gprune, gprune_num, 1, 3).  Straight through ref.lib, as streamsref.ref_scores()."""

    def __init__(self, ref, hmmdefs, nstate, gprune="none", gprune_num=0):
        self.lib, self.S = ref.lib, nstate
        self.h = self.lib.jref_am_load(str(hmmdefs).encode(), None, REF_GPRUNE[gprune], gprune_num, 1, 3)
        if not self.h:
            raise RuntimeError(f"reference failed to load {hmmdefs}")

    def scores(self, frames, utt_off=None):
        """[T][S]: one jref_am_outprob() per utterance (outprob_prepare() clears the codebook cache)."""
        fr = np.ascontiguousarray(frames, np.float32)
        off = [0, len(fr)] if utt_off is None else [int(x) for x in utt_off]
        out = np.full((len(fr), self.S), np.nan, np.float32)
        for a, b in zip(off[:-1], off[1:]):
            if b > a:
                f, o = np.ascontiguousarray(fr[a:b]), np.empty((b - a, self.S), np.float32)
                self.lib.jref_am_outprob(C.c_void_p(self.h), f.ctypes.data_as(C.c_void_p), b - a, o.ctypes.data_as(C.c_void_p))
                out[a:b] = o
        return out

    def cache(self, frames, nbook):
        """mixture_cache of one utterance: score / id [T][nbook][cap] (id -1, score 0 past num) and num [T][nbook]."""
        fr = np.ascontiguousarray(frames, np.float32)
        T, room = len(fr), 512
        sc, ids, num = [], [], []
        for b in range(nbook):
            s, i, n = np.zeros(T * room, np.float32), np.full(T * room, -1, np.int32), np.zeros(T, np.int32)
            cap = self.lib.jref_am_tmix_cache(C.c_void_p(self.h), fr.ctypes.data_as(C.c_void_p), T, b,
                                              s.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p),
                                              n.ctypes.data_as(C.c_void_p))
            assert 0 < cap <= room
            sc.append(s[:T * cap].reshape(T, cap)); ids.append(i[:T * cap].reshape(T, cap)); num.append(n)
        return np.stack(sc, 1), np.stack(ids, 1), np.stack(num, 1)

    def close(self):
        if self.h:
            self.lib.jref_am_free(C.c_void_p(self.h))
            self.h = None


# ---- the cases of the fixture ------------------------------------------------------------------------------------
def _far(frames, model, t, streams):
    return streamsref._far(frames, model, t, streams)


def _case(model, frames, nums, utt_off=None, cache=(), binhmm=False):
    """cache: the gprune_nums at which the reference's codebook caches are recorded too"""
    return dict(model=model, frames=frames, nums=tuple(nums), cache=tuple(cache), binhmm=binhmm,
                utt_off=np.array([0, len(frames)] if utt_off is None else utt_off, np.int32))


def _layout(vsize, books, seed, S=5, T=40, nums=(2,)):
    m = make_tied_model(vsize, S, books, seed=seed)
    return _case(m, make_tied_frames(m, T, seed=seed + 1000), nums)


def _booksize(K, nums, seed, cache=None):
    """One book of K Gaussians on stream 0 of (5, 3), a small one on stream 1; 6 states, 20 frames."""
    m = make_tied_model((5, 3), 6, [(0, K), (1, 3)], seed=seed)
    return _case(m, make_tied_frames(m, 20, seed=seed + 1000), nums, cache=nums if cache is None else cache)


def _tile(S, T, seed):
    m = make_tied_model((3, 2), S, [(0, 5), (1, 4)], seed=seed)
    return _case(m, make_tied_frames(m, T, seed=seed + 1000), (2,))


def _case_branches():
    """Every branch of the stream loop in one model of six states over (4, 3, 2) with two books on stream 0 and one
    each on streams 1 and 2, shared by every state that uses the stream: state 2 has no <SWeights>, state 4 a weight of
    0, state 5 all weights 0, member 1 of stream 0's second book (the odd states') is undefined (a NULL density);
    frame 4 drives stream 1 below LOG_ZERO (skipped), frame 5 every stream (LOG_ZERO out -- but for the odd states: a
    NULL member's LOG_ZERO + bweight joins addlog_array()'s own LOG_ZERO start to a value just above it)."""
    m = make_tied_model((4, 3, 2), 6, [(0, 4), (0, 3), (1, 4), (2, 3)], seed=31, no_sweights=(2,),
                        zero_weight=((4, 1),), all_zero=(5,), null_members=((1, 1),))
    fr = make_tied_frames(m, 7, seed=32)
    _far(fr, m, 4, (1,))
    _far(fr, m, 5, (0, 1, 2))
    return _case(m, fr, (1, 2), binhmm=True)


def _case_compound():
    """calc_compound_mix(): over (4, 3), states 0 .. 3 have a plain pdf on stream 1 of 1, 2, 3 and 5 Gaussians (below,
    at and above gprune_num 2), state 4 a plain pdf on stream 0, state 5 is all tied; state 6 is all plain."""
    m = make_tied_model((4, 3), 7, [(0, 5), (1, 4)], seed=41,
                        plain={(0, 1): 1, (1, 1): 2, (2, 1): 3, (3, 1): 5, (4, 0): 4, (6, 0): 3, (6, 1): 2})
    return _case(m, make_tied_frames(m, 24, seed=42), (2, 3), binhmm=True)


def _ties_model():
    """(4, 3) with two books on stream 0; book 0 has members 1 and 3 with one mean and variance, and 0 and 2 another:
    their scores tie exactly on every frame."""
    return make_tied_model((4, 3), 6, [(0, 6), (0, 4), (1, 4)], seed=51, twins=((0, 1, 3), (0, 0, 2)))


def _twin_frame(m, fr, t, member):
    """Frame t sits on the twins' mean in stream 0: the tied pair leads the list there."""
    p = int(np.nonzero(m["pdf_book"] == 0)[0][0])
    g = int(m["ent_dens"][m["pdf_off"][p] + member])
    fr[t, :m["vsize"][0]] = m["mean"][m["dens_off"][g]:m["dens_off"][g + 1]]
    return fr


TIES_SEED = 52          # frames for which the reference's one-utterance scores differ from the three-utterance ones


def _case_ties(utt_off=(0, 7, 8, 17)):
    """Exactly tied scores, far frames that put scores below LOG_ZERO (3 and 12), a tie on the first frame of the
    third utterance (8): history must not cross the boundaries 7 | 1 | 9."""
    m = _ties_model()
    fr = make_tied_frames(m, 17, seed=TIES_SEED, noise=0.7)
    _far(fr, m, 3, (0,))
    _far(fr, m, 12, (0, 1))
    _twin_frame(m, fr, 8, 1)
    return _case(m, fr, (1, 2, 3), utt_off=utt_off, cache=(1, 2, 3) if len(utt_off) == 2 else ())


def _case_chunks():
    """The ties model over 300 frames of one utterance; tied pairs lead on frames 128 and 256, the first frames of the
    second and third chunk at chunk_frames = 128."""
    m = _ties_model()
    fr = make_tied_frames(m, 300, seed=61, noise=0.7)
    _far(fr, m, 127, (0,))
    _twin_frame(m, fr, 128, 1)
    _twin_frame(m, fr, 256, 0)
    return _case(m, fr, (3,))


def _case_one_stream():
    """One stream of 39, all tied over three books: what lib.Gmm serves too."""
    m = make_tied_model((39,), 9, [(0, 6), (0, 5), (0, 7)], seed=71, no_sweights=range(9))
    return _case(m, make_tied_frames(m, 24, seed=72), (2,))


def _case_e2e():
    """A two-stream (26 + 13) tied model over the 120 states of the golden lexicon beam_rank.npz, scored on its
    utterance's first 40 frames (not stored twice)."""
    z = np.load(GOLDEN.parent / "beam_rank.npz")
    S = len(z["am_st_off"]) - 1
    m = make_tied_model((26, 13), S, [(0, 6), (0, 5), (1, 4)], seed=81)
    return _case(m, z["u0_frames"][:40].astype(np.float32), ())


# name -> case.  Layouts with 2, 3 and 4 books and one with two books on a stream; codebook sizes round the 64 members
# the order pass takes at a time, gprune_num 1, 2, 4, 8 and one larger than the book (at most 64); the state counts
# round the 16-state tile, 130 frames (a wave and two frames) and 513 (a block and one); the branches of the stream
# loop; compound states; ties and chunks (above).  Short vectors wherever the layout is not what the case probes.
CASES = {
    "lay_26_13": lambda: _layout((26, 13), [(0, 6), (1, 5)], 1),
    "lay_13_13_13": lambda: _layout((13, 13, 13), [(0, 5), (1, 6), (2, 4)], 2),
    "lay_12_12_12_3": lambda: _layout((12, 12, 12, 3), [(0, 5), (1, 4), (2, 6), (3, 3)], 3),
    "lay_4_3_two_books": lambda: _layout((4, 3), [(0, 5), (0, 7), (1, 4)], 4),
    "K1": lambda: _booksize(1, (1, 2), 11),
    "K2": lambda: _booksize(2, (1, 2, 3), 12),
    "K63": lambda: _booksize(63, (1, 2, 4, 8, 64), 13, cache=(2, 8)),
    "K64": lambda: _booksize(64, (1, 2, 4, 8, 64), 14),
    "K65": lambda: _booksize(65, (1, 2, 4, 8, 64), 15, cache=(1, 4)),
    "K130": lambda: _booksize(130, (1, 2, 4, 8, 64), 16),
    "S1": lambda: _tile(1, 20, 21),
    "S15": lambda: _tile(15, 20, 22),
    "S16": lambda: _tile(16, 20, 23),
    "S17_T130": lambda: _tile(17, 130, 24),
    "S33": lambda: _tile(33, 20, 25),
    "S3_T513": lambda: _tile(3, 513, 26),
    "branches": _case_branches,
    "compound": _case_compound,
    "ties": _case_ties,
    "ties_one_utt": lambda: _case_ties(utt_off=(0, 17)),
    "chunks": _case_chunks,
    "one_stream": _case_one_stream,
    "e2e": _case_e2e,
}


def modes(case):
    """("none", 0) and ("safe", n) for the case's gprune_nums."""
    return [("none", 0)] + [("safe", n) for n in case["nums"]]


def key(gprune, n):
    return "none" if gprune == "none" else f"safe{n}"


def load_binhmm(name, path):
    Path(path).write_bytes(np.load(GOLDEN)[f"{name}/binhmm"].tobytes())
    return path


def load_case(name):
    """The case from the committed fixture: as CASES[name]() gives it, with `scores` {key: [T][S]} and, where the case
    records them, `caches` {key: (score, id, num)}."""
    z = np.load(GOLDEN)
    c = dict(model=_finish({k: z[f"{name}/{k}"] for k in MODEL_KEYS}), utt_off=z[f"{name}/utt_off"],
             nums=tuple(int(n) for n in z[f"{name}/nums"]), binhmm=f"{name}/binhmm" in z.files)
    c["frames"] = z[f"{name}/frames"] if f"{name}/frames" in z.files else CASES[name]()["frames"]
    c["scores"] = {key(g, n): z[f"{name}/{key(g, n)}"] for g, n in modes(c)}
    c["caches"] = {f"safe{n}": tuple(z[f"{name}/cache{n}/{f}"] for f in ("score", "id", "num"))
                   for n in c["nums"] if f"{name}/cache{n}/num" in z.files}
    c["cache"] = tuple(n for n in c["nums"] if f"safe{n}" in c["caches"])
    return c
