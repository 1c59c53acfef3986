"""GPU: a streaming session of the exact-order kernels (csrc/beam_exact.hip, csrc/beam_exact_mp.h) in which one
utterance ENDS EARLY.  The kernels share their end (csrc/beam_exact_dev.h): a push in which an utterance stops -- the
beam dies, the trellis atoms run out -- parks it with StreamState::active = 0, and every later launch of the session
returns at once for it and leaves its result alone.  The session must end with the one-shot results all the same:
for the utterance that stopped and for its neighbour that went on, in both workgroup shapes, for an ordinary (K6x)
and a multipath (K6m) lexicon."""
import numpy as np
import pytest

from beamutil import assert_trellis_equal, load_beam_golden
from julius_amd import lexblob, lib

pytestmark = pytest.mark.gpu

BEAM, WIDTH = 50, -1.0
CHUNKS = [3, 4, 0, 100000]          # rows per push (+ the utterance number), 0 = an empty push; the last one is final


_CASES = {}


def _case(oracle, name):
    """(golden, the two score arrays, the oracle's first pass of each): computed once, read by every test."""
    if name not in _CASES:
        g = load_beam_golden(name)
        S = len(g["am"]["st_off"]) - 1
        scores = [np.full((12, S), -1000000.0, np.float32), oracle.gmm_outprob(g["am"], g["utts"][0]["frames"])]
        _CASES[name] = (g, scores, [oracle.beam_pass1(g["lex"], sc, BEAM, WIDTH) for sc in scores])
    return _CASES[name]


def _shape(bm, shape):
    try:
        bm.set_workgroup_shape(shape)
    except lib.JamdError:
        pytest.skip(f"the {shape} shape is not available for this work area")
    assert bm.workgroup_shape(1) == shape
    return bm


def _stream(bm, scores):
    S = scores[0].shape[1]
    bm.stream_begin(len(scores))
    pos = [0] * len(scores)
    for ci, c in enumerate(CHUNKS):
        part, off = [], [0]
        for u, sc in enumerate(scores):
            n = min(len(sc) - pos[u], (c + u) if c else 0)
            part.append(sc[pos[u]:pos[u] + n]); pos[u] += n; off.append(off[-1] + n)
        rows = np.concatenate(part) if off[-1] else np.zeros((1, S), np.float32)
        d = lib.DevBuf(bm.eng, rows.nbytes).upload(rows)
        bm.stream_push_dev(d.ptr, S, np.array(off, np.int32), final=ci == len(CHUNKS) - 1)
        bm.results(len(scores))
        d.free()
    assert all(p == len(sc) for p, sc in zip(pos, scores))
    return bm.results(len(scores)), [bm.trellis(u) for u in range(len(scores))]


def _assert_same_trellis(atoms, other):
    """Two trellises of the device, field by field and BIT for bit (hopeless scores leave a NaN backscore behind, which
    no value comparison calls equal to itself)."""
    got, want = lexblob.canonical_trellis(atoms), lexblob.canonical_trellis(other)
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), f"trellis field {k} differs"


def _figures(r):
    return dict(status=r.status, died_at=r.died_at, natom=r.natom, frames=r.frames, wseq=list(r.wseq[:r.wnum]), score=r.score)


@pytest.mark.parametrize("shape", ["full", "half"])
@pytest.mark.parametrize("name", ["beam_score.npz", "beam_multipath.npz"])
def test_stream_with_an_utterance_that_dies(engine, oracle, name, shape):
    """Utterance 0 is hopeless (all scores -1e6), utterance 1 is the golden's first; pushes of 3, 4, 0 and the remaining
    rows (+ the utterance number).  Under the ordinary lexicon no token of utterance 0 survives frame 1: it stops in the
    first push and sits out the others.  The multipath frame carries it to the end without a sentence (status 1, as in
    the oracle); there the utterance that stops early is the one of the overflow test below."""
    g, scores, want = _case(oracle, name)
    lx = lib.Lexicon(engine, g["lex"])
    one = _shape(lib.Beam(engine, lx, BEAM, WIDTH, max_utts=2), shape)
    ores, otre = one.pass1_host(scores)
    bm = _shape(lib.Beam(engine, lx, BEAM, WIDTH, max_utts=2), shape)
    assert bm.order_mode() == "exact"
    sres, stre = _stream(bm, scores)
    for u in range(2):
        print(name, shape, u, "one-shot", _figures(ores[u]), "streamed", _figures(sres[u]), "oracle rc/died", want[u][3], want[u][4])
    for u in range(2):
        got, one_shot = _figures(sres[u]), _figures(ores[u])
        if u == 0 and sres[0].status == 2:
            # `frames` of an utterance whose beam died in an earlier push is left out: the kernel's end
            # (csrc/beam_exact_dev.h, XBEAM_END) writes res->frames = the rows seen up to the push in which it stopped
            # (3 here), the later launches return before they touch the result, and the one-shot call reports all 12
            # rows.  The figures are printed above.
            got.pop("frames"); one_shot.pop("frames")
        assert got == one_shot, u
        _assert_same_trellis(stre[u], otre[u])
    # the utterance that dies: no sentence (1) or the beam dies (2), as in the oracle
    rc, died = want[0][3], want[0][4]
    assert sres[0].status == rc and rc in (1, 2) and (rc != 2 or sres[0].died_at == died)
    if name == "beam_score.npz":
        assert rc == 2 and died == 1
    # its neighbour: the oracle's first pass
    oatoms, wseq, score, rc, died = want[1]
    assert rc == 0 and sres[1].status == 0
    assert_trellis_equal(stre[1], lexblob.canonical_trellis(oatoms))
    assert list(sres[1].wseq[:sres[1].wnum]) == list(wseq) and sres[1].score == score
    one.close(); bm.close()


def test_stream_with_an_utterance_that_overflows(engine, oracle):
    """The same session with room for 50 trellis atoms per utterance: utterance 1 runs out of them while it streams (status
    3, JAMD_PASS1_OVERFLOW) and keeps the atom count of the one-shot call."""
    for name in ("beam_score.npz", "beam_multipath.npz"):
        g, scores, want = _case(oracle, name)
        lx = lib.Lexicon(engine, g["lex"])
        one = lib.Beam(engine, lx, BEAM, WIDTH, max_utts=2, atoms_per_utt=50)
        ores, _ = one.pass1_host(scores)
        bm = lib.Beam(engine, lx, BEAM, WIDTH, max_utts=2, atoms_per_utt=50)
        sres, _ = _stream(bm, scores)
        for u in range(2):
            print(name, u, "one-shot", _figures(ores[u]), "streamed", _figures(sres[u]))
        assert ores[1].status == 3 and sres[1].status == 3
        assert sres[1].natom == ores[1].natom
        one.close(); bm.close()
