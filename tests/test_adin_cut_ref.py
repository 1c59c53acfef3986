"""tests/adincutref.py held to the real program.  The helper restates the block control flow of adin_cut() in Python around
the reference's own count_zc_e(); here the unmodified `julius` (oracle/_ref/bin/julius) reads one 16 kHz file with
-cutsilence (-nostrip -norealtime), and the same program reads, with -nocutsilence, the helper's segments as separate
files.  Both must see the same number of inputs, report the same frame counts (read off the word alignment, -walign)
and print the same first-pass word sequences, scores and alignments -- with the default parameters and with
-lv 500 -zc 40 -headmargin 200 -tailmargin 250 -chunksize 800.  The streams end inside a segment: behind a stream that
ends in silence the program reports one more, empty input.  No GPU."""
import numpy as np
import pytest

import adincutref as K
from julius_amd import synth
from oracle import pyoracle
from test_adin_ref import BIN, _results, _run, _write_wavs

OTHER = dict(level_thres=500, zero_cross_num=40, head_margin_msec=200, tail_margin_msec=250, chunk_size=800)
OTHER_ARGS = ["-lv", "500", "-zc", "40", "-headmargin", "200", "-tailmargin", "250", "-chunksize", "800"]


@pytest.fixture(scope="module")
def task(tmp_path_factory):
    return synth.make_triphone_task(tmp_path_factory.mktemp("cuttask"), seed=43, nword=80, nphone=8, S=120, M=2)


@pytest.mark.parametrize("seed,desc,args,nseg", [(2, {}, [], 4), (3, {}, [], 4), (2, OTHER, OTHER_ARGS, None)])
def test_helper_segments_decode_as_the_program_with_cutsilence(ref, task, tmp_path, seed, desc, args, nseg):
    if not BIN.exists():
        pytest.skip("oracle/_ref/bin/julius not built")
    w = K.bursts(seed)
    common = ["-h", task["hmmdefs"], "-hlist", task["hmmlist"], "-v", task["dict"], "-nlr", task["arpa"],
              "-b", "300", "-1pass", "-gprune", "none", "-sepnum", "5", "-walign", "-input", "rawfile", "-norealtime",
              "-nostrip"]
    prog = _run(common + ["-filelist", _write_wavs(tmp_path, "a", [w], 16000), "-cutsilence"] + args)

    r = K.RefCut(ref, 1, **desc)
    parts = r.push([w], [1])[0]
    r.close()
    assert all(p.final for p in parts) and r.events["end_eos"] == 1      # the stream ends inside a segment
    segs = [p.data() for p in parts]
    fed = _run(common + ["-filelist", _write_wavs(tmp_path, "b", segs, 16000), "-nocutsilence"])

    pframes, pres = _results(prog)
    fframes, fres = _results(fed)
    print("-cutsilence:", pframes, [ln for ln in pres if ln.startswith("pass1_best")])
    print("helper fed :", fframes, [ln for ln in fres if ln.startswith("pass1_best")])
    assert nseg is None or len(segs) == nseg
    assert len(segs) >= 3 and len(pframes) == len(segs) and pframes == fframes
    assert pframes == [(len(s) - 400) // 160 + 1 for s in segs]
    assert len([ln for ln in pres if ln.startswith("pass1_best_score:")]) == len(segs), prog[-3000:]
    assert pres == fres                                      # word sequences, scores and alignments as printed
    assert len(set(ln for ln in pres if ln.startswith("pass1_best:"))) > 1    # not one constant answer
