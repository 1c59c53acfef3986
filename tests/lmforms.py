"""Language-model forms of the first pass that the synthetic tasks do not write by themselves: word classes
(`ENTRY @logprob WORD [out] phones`, libsent/src/voca/voca_load_htkdict.c:418-437), pronunciation variants (several
dictionary words on one N-gram entry), a backward N-gram alone (-nrl without -nlr: bi_prob_compute(),
libsent/src/ngram/ngram_access.c:383) and in-category word probabilities under a grammar.  The dictionaries written by
julius_amd.synth are rewritten in place here; synth itself stays as it is (bench.py and the golden fixtures depend on
its bytes)."""
import numpy as np

from julius_amd import lexblob, synth

NENT = 20
FORMS = ("class", "variants", "class_unk", "class_transp", "rlonly", "rlonly_class")
GRAMMAR_FORMS = ("grammar_wrap", "grammar_free")

# what each form adds to the task and to the reference's options
_FORM_TASK = {"class_unk": dict(nunk=10), "class_transp": dict(ntransparent=12), "rlonly": dict(with_rl3=True),
              "rlonly_class": dict(with_rl3=True)}
_FORM_EXTRA = {"class_transp": ["-transp", "-1.5"]}


def classed_dict(path, nent, seed, at=True, grammar=False, nunk=0):
    """Rewrite a dictionary written by synth in place.  N-gram dictionary: word number k (of the lines that begin with
    `W`) gets the LM entry W{k % nent:04d} and keeps its own name as the word field; at=True adds `@p`,
    p = -U(0.05, 2.0) printed with four decimals, at=False writes plain variants (no `@`: cprob stays 0, wton is
    shared).  The output field keeps its brackets ({out}: transparent), and the last `nunk` words keep their line: they
    have no LM entry and stay with <unk>.  grammar=True: the category field stays, `@p xK` goes in after it (every
    line, <s> and </s> included).  Returns the number of lines rewritten."""
    rng = np.random.default_rng(seed)
    lines = open(path).read().splitlines()
    if grammar:
        out = []
        for k, ln in enumerate(lines):
            cat, rest = ln.split(None, 1)
            out.append(f"{cat} @{-rng.uniform(0.05, 2.0):.4f} x{k} {rest}")
        open(path, "w").write("\n".join(out) + "\n")
        return len(out)
    idx = [i for i, ln in enumerate(lines) if ln.startswith("W")]
    idx = idx[:len(idx) - nunk] if nunk > 0 else idx
    for k, i in enumerate(idx):
        name, rest = lines[i].split(None, 1)
        assert rest[0] in "[{", lines[i]
        if at:
            lines[i] = f"W{k % nent:04d} @{-rng.uniform(0.05, 2.0):.4f} {name} {rest}"
        else:
            lines[i] = f"W{k % nent:04d} {rest}"
    open(path, "w").write("\n".join(lines) + "\n")
    return len(idx)


def ref_lm_task(ref, tmpdir, seed, beam, extra, form, **task_kw):
    """beamutil.ref_task for one of FORMS (or "plain": the task as synth writes it):
    (RefEngine, lex dict, flat AM, task); the descriptor conditions of the form are asserted (assert_form)."""
    from oracle import pyoracle
    assert form == "plain" or form in FORMS, form
    kw = dict(_FORM_TASK.get(form, {}))
    kw.update(task_kw)
    task = synth.make_triphone_task(tmpdir, seed=seed, **kw)
    if form in ("class", "class_unk", "class_transp", "rlonly_class"):
        classed_dict(task["dict"], NENT, seed, nunk=kw.get("nunk", 0))
    elif form == "variants":
        classed_dict(task["dict"], NENT, seed, at=False)
    if form.startswith("rlonly"):
        lm = ["-nrl", task["arpa_rl"]]                       # no -nlr: no forward 2-gram at all
    else:
        lm = ["-nlr", task["arpa"]] + (["-nrl", task["arpa_rl"]] if task.get("arpa_rl") else [])
    eng = pyoracle.RefEngine(ref, ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"]] + lm +
                             ["-input", "htkparam", "-1pass", "-gprune", "none", "-b", str(beam)] + list(extra) +
                             _FORM_EXTRA.get(form, []))
    eng.save_lexicon(tmpdir / "lex.blob")
    lex = lexblob.load(tmpdir / "lex.blob")
    am = ref.am_load(task["hmmdefs"], task["hmmlist"]).export()
    assert_form(lex, form)
    return eng, lex, am, task


def ref_lm_grammar_task(ref, tmpdir, seed, beam, extra=(), wrap=True, **task_kw):
    """beamutil.ref_grammar_task with in-category word probabilities on every dictionary line
    (classed_dict(grammar=True)): the delayed per-word value of beam.c:2448-2451 and, with wrap=False, one initial
    token per word, each with its own init_lscore (beam.c:1729)."""
    from oracle import pyoracle
    task = synth.make_triphone_grammar(synth.make_triphone_task(tmpdir, seed=seed, **task_kw), ncat=3, seed=seed, wrap=wrap)
    classed_dict(task["gdict"], NENT, seed, grammar=True)
    eng = pyoracle.RefEngine(ref, ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-dfa", task["dfa"], "-v", task["gdict"],
                                   "-input", "htkparam", "-1pass", "-gprune", "none", "-b", str(beam)] + list(extra))
    eng.save_lexicon(tmpdir / "lex.blob")
    lex = lexblob.load(tmpdir / "lex.blob")
    am = ref.am_load(task["hmmdefs"], task["hmmlist"]).export()
    assert_form(lex, "grammar_wrap" if wrap else "grammar_free")
    return eng, lex, am, task


# form -> seed of the task (and of its utterances); chosen on the CPU so that every utterance ends with a sentence
# (rc == 0) and the trellises hold at least 20 word pairs on either branch of the 2-gram lookup (test_lm_forms.py)
SEEDS = {"plain": 50, "class": 51, "variants": 52, "class_unk": 53, "class_transp": 54, "rlonly": 55, "rlonly_class": 56,
         "grammar_wrap": 61, "grammar_free": 62, "class-mp": 57, "rlonly-mp": 58, "class-wide": 59, "rlonly-wide": 60}
WIDE = dict(nword=600, nphone=14, S=260, M=2)            # with -b 5000: the exact-order kernel's wide layout


class LmCase:
    """One form loaded by the compiled reference, its utterances, and both references' results for them:
    .ref[u] = (trellis, wseq, score) of the compiled reference, .orc[u] = (canonical trellis, wseq, score, rc) of
    oracle.beam_pass1.  Nothing in it is changed after it is built."""

    def __init__(self, ref, oracle, wd, form, nwords, multipath=False, wide=False, sepnum=4, seed=None):
        self.form, self.oracle, self.wd = form, oracle, wd
        self.seed = seed if seed is not None else SEEDS[form + ("-mp" if multipath else "-wide" if wide else "")]
        if form in GRAMMAR_FORMS:
            self.beam = 120
            self.eng, self.lex, self.am, self.task = ref_lm_grammar_task(
                ref, wd, self.seed, self.beam, ["-penalty1", "-2.0"], wrap=form == "grammar_wrap", nword=70)
            make = synth.make_triphone_grammar_utterance
        else:
            self.beam = 5000 if wide else 150
            extra = ["-sepnum", str(20 if wide else sepnum)] + (["-multipath"] if multipath else [])
            self.eng, self.lex, self.am, self.task = ref_lm_task(ref, wd, self.seed, self.beam, extra, form, **(WIDE if wide else {}))
            make = synth.make_utterance
        assert bool(self.lex["lm_type"] & 0x100) == multipath
        self.frames = [make(self.task, nwords=n, seed=100 * self.seed + u)[0] for u, n in enumerate(nwords)]
        self.scores = [oracle.gmm_outprob(self.am, fr) for fr in self.frames]
        self.ref, self.orc = [], []
        for fr, sc in zip(self.frames, self.scores):
            synth.write_htk_param(wd / "u.mfc", fr)
            tr, (wseq, score) = self.eng.recognize(wd / "u.mfc")
            self.ref.append((tr, wseq, score))
            self.orc.append(self.run_oracle(self.lex, sc))

    def run_oracle(self, lex, sc):
        atoms, wseq, score, rc, died = self.oracle.beam_pass1(lex, sc, self.eng.beam_width, -1.0)
        return lexblob.canonical_trellis(atoms), wseq, score, rc


def same_trellis(a, b):
    """Two canonical trellises, field by field."""
    return len(a["wid"]) == len(b["wid"]) and all(np.array_equal(a[k], b[k]) for k in a)


def assert_form(lex, form):
    """The properties of the flattened lexicon that make a form what it is; a change of synth that quietly removes one
    fails here instead of hollowing the tests out."""
    nword = lex["nword"]
    wton, cprob = np.asarray(lex["wton"]), np.asarray(lex["cprob"])
    if form in GRAMMAR_FORMS:
        assert lex["lm_type"] & 0xff == 1
        assert (lex["ninit"] == 1) == (form == "grammar_wrap")
        assert np.all(cprob != 0) and len(cprob) == nword
        if form == "grammar_free":
            assert lex["ninit"] > 10 and len(np.unique(lex["init_lscore"][:lex["ninit"]])) > 10
        return
    assert lex["lm_type"] & 0xff == 0
    if form == "plain":
        assert len(np.unique(wton)) == nword and np.all(cprob == 0) and lex["ng_mode"] == 0
        return
    nunk = 10 if form == "class_unk" else 0
    if form in ("class", "variants", "class_unk", "class_transp", "rlonly_class"):
        assert len(np.unique(wton)) < nword / 2, (len(np.unique(wton)), nword)
        assert np.all(np.bincount(wton[2:nword - nunk]) != 1)          # every rewritten word shares its entry
    if form in ("class", "class_unk", "class_transp", "rlonly_class"):
        assert np.all(cprob[2:nword - nunk] != 0) and np.all(cprob[:2] == 0) and np.all(cprob[nword - nunk:] == 0)
    else:
        assert np.all(cprob == 0)
    if form == "class_unk":
        assert lex["ng_unk_id"] < lex["ng_nword"] and lex["ng_unk_num_log"] > 0
        assert np.all(wton[nword - nunk:] == lex["ng_unk_id"])
    if form == "class_transp":
        tr = np.asarray(lex["is_transparent"]) != 0
        assert int(tr.sum()) == 12 and np.all(cprob[tr] != 0) and lex["lm_penalty_trans"] == -1.5
    assert lex["ng_mode"] == (3 if form.startswith("rlonly") else 0)
    if form == "rlonly":
        assert len(np.unique(wton)) == nword


def form_counts(lex):
    """(ng_mode, distinct wton, non-zero cprob) of a lexicon."""
    return int(lex["ng_mode"]), int(len(np.unique(lex["wton"]))), int(np.count_nonzero(lex["cprob"]))


def search_bigram(lex, w_context, w):
    """search_bigram(), ngram_access.c:225-247, over the descriptor's tables: the tuple's index or -1."""
    left = int(lex["ng_bi_bgn"][w_context])
    if left < 0:
        return -1
    right = left + int(lex["ng_bi_num"][w_context])
    i = left + int(np.searchsorted(lex["ng_bi_wid"][left:right], w))
    return i if i < right and lex["ng_bi_wid"][i] == w else -1


def bigram_branches(lex, trellises):
    """Over the (predecessor word, word) pairs of canonical trellises: how many distinct pairs the 2-gram lookup of the
    lexicon's ng_mode finds (search_bigram) and how many back off.  (hits, backoffs)."""
    wton = lex["wton"]
    pairs = set()
    for tr in trellises:
        ok = tr["pwid"] >= 0
        pairs |= set(zip(tr["pwid"][ok].tolist(), tr["wid"][ok].tolist()))
    hit = 0
    for pw, w in pairs:
        c1, c2 = int(wton[pw]), int(wton[w])
        n2 = search_bigram(lex, c1, c2) if lex["ng_mode"] in (0, 1) else search_bigram(lex, c2, c1)
        hit += n2 >= 0
    return hit, len(pairs) - hit


def shared_context_atoms(lex, tr):
    """Atoms of a canonical trellis whose word's N-gram entry (the key of the kernels' LM memo and of the cross-word
    table) belongs to at least two dictionary words."""
    wton = np.asarray(lex["wton"])
    return int(np.sum(np.bincount(wton)[wton[tr["wid"]]] >= 2))


def with_fields(lex, **fields):
    """A copy of a lexicon dict with some fields replaced."""
    out = dict(lex)
    out.update(fields)
    return out
