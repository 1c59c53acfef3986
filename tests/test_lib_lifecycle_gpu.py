"""GPU: every object of julius_amd.lib through its whole life on the smallest shapes there are -- created, used for
one trivial call, closed, closed again and dropped -- and what a create the library refuses leaves behind: a JamdError
and an object whose close() and collection say nothing.  The refusals are argument checks of the create entries; nothing
here reaches a kernel with them, and nothing but close() is called on a closed object."""
import gc
from types import SimpleNamespace

import numpy as np
import pytest

from beamutil import load_beam_golden
from conftest import GOLDEN
from julius_amd import lexblob, lib, synth

pytestmark = pytest.mark.gpu

KIND = "MFCC_E_D_A_Z"
CHUNK = np.arange(160, dtype=np.int16) * 37


def _gmm():
    return synth.make_gmm(S=2, M=2, D=13, seed=7)


def _streams(nstream=1):
    """_gmm() as a one-stream model of the multi-stream entry."""
    m = _gmm()
    S, E = len(m["st_off"]) - 1, len(m["ent_dens"])
    return dict(vsize=[13], pdf_stream=np.zeros(S, np.int32), pdf_off=m["st_off"], ent_dens=m["ent_dens"],
                ent_logw=m["ent_logw"], st_pdf=np.arange(S, dtype=np.int32).reshape(S, 1), st_weight=None,
                dens_off=13 * np.arange(E + 1, dtype=np.int32), mean=m["mean"], ivar=m["ivar"], gconst=m["gconst"],
                nstream=nstream)


def _frames():
    return synth.make_frames(_gmm(), T=2, seed=8)


def _dnn(dims=(16, 8, 5)):
    return synth.make_dnn(dims=dims, seed=1)


@pytest.fixture(scope="module")
def lex():
    return load_beam_golden("beam_rank.npz")["lex"]


@pytest.fixture()
def ctx(engine, lex):
    """What the creates below draw on: the engine, the lexicon dict, the detector's model, and the two objects others
    are made over -- made on first use and closed after the test that made children of them."""
    made = {}

    def parent(what):
        if what not in made:
            made[what] = lib.Lexicon(engine, lex) if what == "lexicon" else lib.Frontend.from_kind(engine, KIND, 39)
        return made[what]
    yield SimpleNamespace(e=engine, lex=lex, model=lib.FvadModel.read(GOLDEN / "fvad_model.txt"), parent=parent)
    for obj in made.values():
        obj.close()


# class -> (create, one trivial use that says whether it went well)
LIVES = {
    "Engine": (lambda c: lib.Engine(0), lambda o: o.sync() is None),
    "DevBuf": (lambda c: lib.DevBuf(c.e, 8),
               lambda o: list(o.upload(np.arange(2, dtype=np.int32)).download(2, np.int32)) == [0, 1]),
    "Gmm": (lambda c: lib.Gmm(c.e, _gmm()), lambda o: o.outprob_host(_frames()).shape == (2, 2)),
    "GmmStreams": (lambda c: lib.GmmStreams(c.e, _streams()), lambda o: o.outprob_host(_frames()).shape == (2, 2)),
    "Gms": (lambda c: lib.Gms(c.e, _gmm(), [0, 1], 1),
            lambda o: o.apply_host(_frames(), np.zeros((2, 2), np.float32)).shape == (2, 2)),
    "RejGmm": (lambda c: lib.RejGmm(c.e, _gmm(), [0], 5), lambda o: o.scores_host(_frames())[1].shape == (1, 1)),
    "CdSet": (lambda c: lib.CdSet(c.e, [0, 2], [0, 1]),
              lambda o: o.outprob_host(np.zeros((2, 2), np.float32)).shape == (2, 1)),
    "Dnn": (lambda c: lib.Dnn(c.e, _dnn()), lambda o: o.outprob_host(np.zeros((2, 16), np.float32)).shape == (2, 5)),
    "Lexicon": (lambda c: lib.Lexicon(c.e, c.lex), lambda o: o.lm_table() in (0, 1)),
    "Beam": (lambda c: lib.Beam(c.e, c.parent("lexicon"), 100), lambda o: o.order_mode() in lib.Beam.ORDER_MODES),
    "Frontend": (lambda c: lib.Frontend.from_kind(c.e, KIND, 39), lambda o: o.veclen == 39 and o.frames(16000) > 0),
    "LiveFrontend": (lambda c: lib.LiveFrontend(c.parent("frontend"), 1), lambda o: o.push_host([CHUNK])[1][0] == 0),
    "Adin": (lambda c: lib.Adin(c.e, 1), lambda o: 0 <= o.push_host([CHUNK])[1][1] <= 160),
    "AdinCut": (lambda c: lib.AdinCut(c.e, 1), lambda o: len(o.push_host([CHUNK])) == 4),
    "Fvad": (lambda c: lib.Fvad(c.e, 1, c.model), lambda o: list(o.push_host([CHUNK])[1]) == [0, 1]),
}


def _handle(obj):
    return obj.ptr if isinstance(obj, lib.DevBuf) else obj.h


@pytest.mark.parametrize("name", list(LIVES))
def test_whole_life(ctx, capfd, name):
    create, use = LIVES[name]
    obj = create(ctx)
    assert type(obj).__name__ == name and _handle(obj)
    assert use(obj)
    close = obj.free if name == "DevBuf" else obj.close
    close()
    assert not _handle(obj)
    close()                                      # idempotent
    assert not _handle(obj)
    del obj, close
    gc.collect()
    ctx.e.sync()                                 # the engine still serves
    assert "Exception ignored" not in capfd.readouterr().err


# class -> (class, arguments) of a create the library refuses on its argument checks
REFUSED = {
    "Engine": lambda c: (lib.Engine, (lib.load().jamd_device_count(),)),
    "Gmm": lambda c: (lib.Gmm, (c.e, dict(_gmm(), nstream=2))),
    "GmmStreams": lambda c: (lib.GmmStreams, (c.e, _streams(nstream=0))),
    "Gms": lambda c: (lib.Gms, (c.e, _gmm(), [0, 1], 0)),
    "RejGmm": lambda c: (lib.RejGmm, (c.e, _gmm(), [0], 0)),
    "CdSet": lambda c: (lib.CdSet, (c.e, [0, 2], [0, 1], 99)),
    "Dnn": lambda c: (lib.Dnn, (c.e, _dnn(dims=(12, 8, 5)))),
    "Lexicon": lambda c: (lib.Lexicon, (c.e, dict(c.lex, lm_type=0x200))),
    "Beam": lambda c: (lib.Beam, (c.e, c.parent("lexicon"), 0)),
    "Frontend": lambda c: (lib.Frontend, (c.e, lib.Frontend.desc_for(KIND, 39, realtime=1))),
    "LiveFrontend": lambda c: (lib.LiveFrontend, (c.parent("frontend"), 0)),
    "Adin": lambda c: (lib.Adin, (c.e, 0)),
    "AdinCut": lambda c: (lib.AdinCut, (c.e, 0)),
    "Fvad": lambda c: (lib.Fvad, (c.e, 0, None)),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_create_leaves_a_quiet_object(ctx, capfd, name):
    cls, args = REFUSED[name](ctx)
    obj = cls.__new__(cls)
    with pytest.raises(lib.JamdError, match=r"^jamd_\w+_create failed \(-?\d+\): jamd_\w+_create: "):
        obj.__init__(*args)
    assert not obj.h
    obj.close()
    obj.close()
    del obj
    gc.collect()
    ctx.e.sync()
    assert "Exception ignored" not in capfd.readouterr().err


def test_loaders_set_what_the_dict_constructors_set(engine, lex, tmp_path):
    """from_file / from_dnnconf on files written from the same models: the same attributes, one handle each."""
    m = _gmm()
    lexblob.save_gmm(m, tmp_path / "am.blob")
    lexblob.save_gmm(m, tmp_path / "m.gms", state2gs=np.array([0, 1], np.int32), nbest=1)
    lexblob.save(lex, tmp_path / "lex.blob")
    dnn = _dnn()
    conf = synth.write_dnnconf(tmp_path, dnn)
    pairs = [(lib.Gmm(engine, m, lib.GPRUNE_SAFE, 2), lib.Gmm.from_file(engine, tmp_path / "am.blob", lib.GPRUNE_SAFE, 2),
              ("S", "D", "nbook", "gprune_num")),
             (lib.Gms(engine, m, [0, 1], 1), lib.Gms.from_file(engine, tmp_path / "m.gms", veclen=13), ("S", "D")),
             (lib.Dnn(engine, dnn), lib.Dnn.from_dnnconf(engine, conf), ("S", "D"))]
    for made, loaded, attrs in pairs:
        assert type(loaded) is type(made) and loaded.h and loaded.eng is engine
        assert {a: getattr(loaded, a) for a in attrs} == {a: getattr(made, a) for a in attrs}
        assert all(isinstance(getattr(loaded, a), int) for a in attrs)
        for obj in (made, loaded):
            obj.close()
            assert not obj.h
    plain = lib.Gmm.from_file(engine, tmp_path / "am.blob")
    assert plain._keep == {} and plain.gprune_num == 0
    made, loaded = lib.Lexicon(engine, lex), lib.Lexicon.from_file(engine, tmp_path / "lex.blob")
    assert loaded.h and loaded.eng is engine and loaded.lex is None and made.lex is lex
    assert loaded.lm_table() == made.lm_table()
    with pytest.raises(lib.JamdError, match=r"^jamd_gmm_load failed \(-?\d+\): "):
        lib.Gmm.from_file(engine, tmp_path / "none.blob")


def test_pack_chunks_is_the_frontends_pack():
    assert lib.Frontend._pack is lib.pack_chunks
    samples, off = lib.pack_chunks([])
    assert samples.dtype == np.int16 and len(samples) == 0 and off.dtype == np.int64 and list(off) == [0]
    samples, off = lib.pack_chunks([[1, 2, 3], np.zeros(0, np.int16), np.array([7], np.int32)])
    assert samples.dtype == np.int16 and list(samples) == [1, 2, 3, 7]
    assert off.dtype == np.int64 and list(off) == [0, 3, 3, 4]
