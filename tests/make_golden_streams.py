"""Writes tests/golden/gmm_streams.npz: for every case of tests/streamsref.py the model arrays, the frames and the
scores of the compiled, unmodified reference (oracle/_ref/libjref.so: init_hmminfo() / outprob_init() /
outprob_state() on the case's ascii hmmdefs).  Data only.  Run where the reference is built:

    python tests/make_golden_streams.py
"""
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import streamsref  # noqa: E402
from oracle import pyoracle  # noqa: E402


def main():
    ref = pyoracle.Ref()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, make in streamsref.CASES.items():
            model, frames = make()
            path = Path(tmp) / f"{name}.hmmdefs"
            streamsref.write_streams_hmmdefs(path, model)
            scores = streamsref.ref_scores(ref, path, frames)
            assert not np.isnan(scores).any()
            for k in streamsref.MODEL_KEYS:
                out[f"{name}/{k}"] = model[k]
            if name != "e2e":              # (its frames are beam_rank.npz's utterance, not stored twice)
                out[f"{name}/frames"] = frames
            out[f"{name}/scores"] = scores
            if name in streamsref.BINHMM_CASES:     # mkbinhmm's file of the model, as the reference's write_binhmm() made it
                bpath = streamsref.write_binhmm(ref, path, Path(tmp) / f"{name}.binhmm")
                assert np.array_equal(streamsref.ref_scores(ref, bpath, frames, nstate=scores.shape[1]), scores)
                out[f"{name}/binhmm"] = np.frombuffer(bpath.read_bytes(), np.uint8)
            print(f"{name}: S={scores.shape[1]} T={scores.shape[0]} streams={list(model['vsize'])} "
                  f"LOG_ZERO={int((scores <= streamsref.LOG_ZERO).sum())}")
    np.savez_compressed(streamsref.GOLDEN, **out)
    print(f"wrote {streamsref.GOLDEN} ({streamsref.GOLDEN.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
