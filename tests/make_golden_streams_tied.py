"""Writes tests/golden/gmm_streams_tied.npz: for every case of tests/streamstied.py the model arrays, the frames, the
utterance offsets and the scores of the compiled, unmodified reference (oracle/_ref/libjref.so) under -gprune none
and under -gprune safe at the case's gprune_nums; for some the codebook caches and the model's binary HMM file.
Data only.  Run where the reference is built:

    python tests/make_golden_streams_tied.py
"""
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import streamstied as st  # noqa: E402
from oracle import pyoracle  # noqa: E402


def main():
    ref = pyoracle.Ref()
    out, kept = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, make in st.CASES.items():
            c = make()
            model, frames, S = c["model"], c["frames"], c["model"]["st_pdf"].shape[0]
            path = Path(tmp) / f"{name}.hmmdefs"
            st.write_tied_hmmdefs(path, model)
            for k in st.MODEL_KEYS:
                out[f"{name}/{k}"] = model[k]
            if name != "e2e":              # (its frames are beam_rank.npz's utterance, not stored twice)
                out[f"{name}/frames"] = frames
            out[f"{name}/utt_off"] = c["utt_off"]
            out[f"{name}/nums"] = np.array(c["nums"], np.int32)
            bpath = st.write_binhmm(ref, path, Path(tmp) / f"{name}.binhmm") if c["binhmm"] else None
            for gprune, n in st.modes(c):
                r = st.RefModel(ref, path, S, gprune, n)
                scores = r.scores(frames, c["utt_off"])
                assert not np.isnan(scores).any()
                out[f"{name}/{st.key(gprune, n)}"] = kept[name, gprune, n] = scores
                if gprune == "safe" and n in c["cache"]:
                    sc, ids, num = r.cache(frames, st.nbook(model))
                    assert sc.shape[2] == n
                    out[f"{name}/cache{n}/score"], out[f"{name}/cache{n}/id"], out[f"{name}/cache{n}/num"] = sc, ids, num
                r.close()
                if bpath:                  # mkbinhmm's file of the model scores the same under this mode
                    rb = st.RefModel(ref, bpath, S, gprune, n)
                    assert np.array_equal(rb.scores(frames, c["utt_off"]), scores)
                    rb.close()
            if bpath:
                out[f"{name}/binhmm"] = np.frombuffer(bpath.read_bytes(), np.uint8)
            differ = [n for n in c["nums"] if not np.array_equal(kept[name, "safe", n], kept[name, "none", 0])]
            print(f"{name}: S={S} T={len(frames)} streams={list(model['vsize'])} books={st.book_sizes(model)} "
                  f"utts={len(c['utt_off']) - 1} safe differs from none at gprune_num {differ} of {list(c['nums'])}")
    # the history must show: the same frames as one utterance score differently somewhere
    for n in st.CASES["ties"]()["nums"]:
        a, b = kept["ties", "safe", n], kept["ties_one_utt", "safe", n]
        print(f"ties: gprune_num {n}: {(a != b).sum()} scores differ between three utterances and one")
    assert any((kept["ties", "safe", n] != kept["ties_one_utt", "safe", n]).any() for n in st.CASES["ties"]()["nums"]), \
        "choose another TIES_SEED: the reference alone must show the difference"
    np.savez_compressed(st.GOLDEN, **out)
    print(f"wrote {st.GOLDEN} ({st.GOLDEN.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
