"""Inputs of the first-pass state-set tests (test_iwcd_first_pass.py, test_iwcd_first_pass_gpu.py).

A token on a word-boundary node takes its output probability from a pseudo-phone state set (outprob_cd(), `-iwcd1
max | avg | best N`).  Inside the first pass that reduction is implemented three more times beside the stand-alone
kernel: the exact-order kernel's step C (4, 2 or 1 lanes per set, chosen per frame from the number of reductions
against NT/4 and NT/2), the canonical-tie kernel's drain (always 4 lanes) and the one-lane cd_reduce() of the
multipath frame and of strict order.  This module builds the small task on which every one of these paths, every
method and both sides of every round of the member loops is reached:

  A  a 600-word cross-word triphone lexicon built by the compiled reference (12 phones, nvar = 64: 969 sets of 1 and
     7..14 members plus 36 of 42..53 that no beam reduces), checked against the compiled reference;
  B  the same lexicon with its sets resized to SIZES (both sides of a round at 1, 2 and 4 lanes of the exact-order
     kernel -- 8 / 16 / 32 members -- of the canonical-tie kernel -- 16 -- and of two rounds), which the reference
     cannot load; checked against the CPU oracle, which A pins to the reference bit for bit.

The streams are 30 frames of state scores fed as they are (`-input outprob`): `flat`, `gmm`, and `holes(frac)` = flat
with a random share of the columns dead on every frame.  No set is ever ENTIRELY dead: an all-dead set gives 0/0 = NaN
under avg and best N in the reference, and what becomes of a NaN token there depends on comparison order."""
import numpy as np

from julius_amd import lexblob, synth
from oracle import pyoracle

S = 1500
T = 30
LOG_ZERO = -1000000.0
BELOW_LOG_ZERO = -2000000.0           # a score under LOG_ZERO, which `-input outprob` passes through as it is
BEAMS = (40, 400, 900, 2000)
WIDE_BEAM_B = 4000                    # case B: the beam at which the one-lane class has its frames in the full shape
METHODS = {"max": ["max"], "avg": ["avg"], "best1": ["best", "1"], "best2": ["best", "2"], "best3": ["best", "3"],
           "best4": ["best", "4"], "best5": ["best", "5"], "best16": ["best", "16"]}
# (cdset_method, cdmax_num) of jamd_lexicon_desc for each of them
METHOD_DESC = {"max": (0, None), "avg": (1, None), "best1": (2, 1), "best2": (2, 2), "best3": (2, 3), "best4": (2, 4),
               "best5": (2, 5), "best16": (2, 16)}
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 70]
NT = {"full": 1024, "half": 512}      # threads of the exact-order kernel's workgroup shapes
TASK_KW = dict(nphone=12, S=S, M=1, nword=600, nvar=64, seed=1, maxlen=8, nbigram_per_word=10)


def device_frames(calls):
    """The oracle's per-frame reduction counts as the exact-order kernel numbers its frames.  Under an N-gram the
    oracle's frame 0 is get_back_trellis_init(): it scores the one initial token (one reduction: the head silence
    stands on a set node).  The kernel does the same on one thread BEFORE its frame loop, through cd_reduce(), so that
    frame is no turn of the loop: its counters ([11] frames, [13..15]) cover the oracle's frames 1..T-1."""
    return np.asarray(calls)[1:]


def lane_classes(calls, nt):
    """(frames on two lanes per set, frames on one lane per set) of the exact-order kernel for a workgroup of nt
    threads, from the per-frame reduction counts of its frame loop (device_frames()): four lanes up to nt/4 reductions,
    two up to nt/2, one beyond."""
    c = np.asarray(calls)
    return int(((c > nt // 4) & (c <= nt // 2)).sum()), int((c > nt // 2).sum())


def assert_no_dead_set(lex, stream):
    """The condition on every stream: each set keeps a member above LOG_ZERO on each frame (no 0/0), no NaN."""
    assert np.isfinite(stream).all()
    live = stream[:, lex["set_states"]] > LOG_ZERO
    assert np.logical_or.reduceat(live, lex["set_off"][:-1], axis=1).all()


def holes(lex, flat, frac, seed):
    """flat with a random `frac` of the columns dead on each frame, half of them at LOG_ZERO and half below it; the
    first member of every set that would be all dead is revived."""
    rng = np.random.default_rng(seed)
    out = flat.copy()
    ndead = int(round(frac * flat.shape[1]))
    for t in range(flat.shape[0]):
        dead = rng.permutation(flat.shape[1])[:ndead]
        out[t, dead[:ndead // 2]] = LOG_ZERO
        out[t, dead[ndead // 2:]] = BELOW_LOG_ZERO
    live = out[:, lex["set_states"]] > LOG_ZERO
    alive = np.logical_or.reduceat(live, lex["set_off"][:-1], axis=1)
    first = lex["set_states"][lex["set_off"][:-1]]
    for t, i in zip(*np.nonzero(~alive)):
        out[t, first[i]] = flat[t, first[i]]
    assert_no_dead_set(lex, out)
    return out


def resized(lex, seed=11):
    """Case B: set i gets SIZES[i % len(SIZES)] members -- the original ones first, then distinct random states."""
    rng = np.random.default_rng(seed)
    off, st = lex["set_off"], lex["set_states"]
    new = []
    for i in range(lex["nset"]):
        orig, n = st[off[i]:off[i + 1]], SIZES[i % len(SIZES)]
        if n > len(orig):
            pool = np.setdiff1d(np.arange(S, dtype=np.int32), orig)
            orig = np.concatenate([orig, rng.choice(pool, n - len(orig), replace=False).astype(np.int32)])
        new.append(orig[:n])
        assert len(set(new[-1].tolist())) == n
    out = dict(lex)
    out["set_off"] = np.concatenate([[0], np.cumsum([len(x) for x in new])]).astype(np.int32)
    out["set_states"] = np.concatenate(new).astype(np.int32)
    return out


def with_method(lex, method):
    out = dict(lex)
    out["cdset_method"] = METHOD_DESC[method][0]
    if METHOD_DESC[method][1] is not None:
        out["cdmax_num"] = METHOD_DESC[method][1]
    return out


class Task:
    """The task as the compiled reference loads it, its streams, the reference and the oracle at any method and beam
    (cached: every result is computed once and shared by the tests that need it)."""

    def __init__(self, ref, oracle, wd, extra=()):
        self.ref, self.oracle, self.wd, self.extra = ref, oracle, wd, list(extra)
        self.task = synth.make_triphone_task(wd, **TASK_KW)
        t = self.task
        self.args = ["-h", t["hmmdefs"], "-hlist", t["hmmlist"], "-v", t["dict"], "-nlr", t["arpa"], "-input", "outprob",
                     "-1pass"] + self.extra
        self._eng, self._lex, self._want, self._orc = {}, {}, {}, {}
        lex = self.lex("max")
        self.lex_b = resized(lex)
        am = ref.am_load(t["hmmdefs"], t["hmmlist"]).export()
        assert len(am["st_off"]) - 1 == S
        flat = np.random.default_rng(7).normal(-8.0, 0.33, (T, S)).astype(np.float32)
        gmm = oracle.gmm_outprob(am, synth.make_utterance(t, nwords=3, seed=9042)[0])[:T]
        assert gmm.shape == (T, S)
        self.streams = {"flat": flat, "gmm": gmm, "holes50": holes(lex, flat, 0.5, 50), "holes90": holes(lex, flat, 0.9, 90)}
        self.streams_b = {"flat": flat, "holes50": holes(self.lex_b, flat, 0.5, 50)}
        for v in self.streams.values():
            assert_no_dead_set(lex, v)
        for v in self.streams_b.values():
            assert_no_dead_set(self.lex_b, v)

    def engine(self, method, beam):
        key = (method, beam)
        if key not in self._eng:
            self._eng[key] = pyoracle.RefEngine(self.ref, self.args + ["-iwcd1"] + METHODS[method] + ["-b", str(beam)])
            assert self._eng[key].beam_width == beam
        return self._eng[key]

    def lex(self, method):
        """The lexicon as the reference exports it under this method."""
        if method not in self._lex:
            self.engine(method, 400).save_lexicon(self.wd / "lex.blob")
            self._lex[method] = lexblob.load(self.wd / "lex.blob")
            kind, num = METHOD_DESC[method]
            assert self._lex[method]["cdset_method"] == kind and (num is None or self._lex[method]["cdmax_num"] == num)
        return self._lex[method]

    def lex_resized(self, method):
        return with_method(self.lex_b, method)

    def want(self, method, beam, kind, nframes=T):
        """The compiled reference's (trellis, (wseq, score)) on a stream of case A."""
        key = (method, beam, kind, nframes)
        if key not in self._want:
            synth.write_htk_param(self.wd / "u.prob", self.streams[kind][:nframes], parmkind=synth.PARM_USER)
            self._want[key] = self.engine(method, beam).recognize(self.wd / "u.prob")
        return self._want[key]

    def oracle_run(self, case, method, beam, kind, nframes=T):
        """The oracle's (canonical trellis, wseq, score, rc, calls, big) on a stream of case 'A' or 'B'."""
        key = (case, method, beam, kind, nframes)
        if key not in self._orc:
            lex = self.lex(method) if case == "A" else self.lex_resized(method)
            sc = (self.streams if case == "A" else self.streams_b)[kind][:nframes]
            atoms, wseq, score, rc, died, calls, big = self.oracle.beam_pass1(lex, sc, beam, counts=True)
            assert rc in (0, 1) and died == -1
            self._orc[key] = (lexblob.canonical_trellis(atoms), wseq, score, rc, calls, big)
        return self._orc[key]
