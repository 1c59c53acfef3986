"""GPU: GMM-based input verification / rejection (-gmm / -gmmnum / -gmmreject).
jamd_rejgmm_* stands where gmm_proceed()'s scoring stands (libjulius/src/gmm.c:574-600 with its
private pruning, gmm.c:177-370): per-frame model scores and the per-input sums, bit for bit against
the committed outputs of the compiled reference and against the oracle on fresh inputs."""
import numpy as np
import pytest

from conftest import GOLDEN
from julius_amd import lib, synth

pytestmark = pytest.mark.gpu

KEYS = ("mean", "ivar", "gconst", "st_off", "ent_dens", "ent_logw")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN / "rejgmm.npz")


@pytest.mark.parametrize("num", [5, 20])
def test_golden(engine, z, num):
    m = lib.RejGmm(engine, {k: z[k] for k in KEYS}, z["model_state"], num)
    fs, us = m.scores_host(z["frames"], z["utt_off"])
    assert np.array_equal(fs, z["frame_scores_%d" % num])
    assert np.array_equal(us, z["utt_scores_%d" % num])
    assert np.array_equal(np.argmax(us, axis=1), z["winner_%d" % num])


@pytest.mark.parametrize("num,M,D,null_frac", [(1, 6, 39, 0.0), (3, 20, 39, 0.2), (10, 40, 26, 0.0), (64, 70, 13, 0.1),
                                                (16, 16, 39, 0.0)])
def test_against_oracle(engine, oracle, num, M, D, null_frac):
    """Mixture counts below, at and above -gmmnum; NULL densities; other vector lengths."""
    model = synth.make_gmm(S=5, M=M, D=D, seed=num + M, ragged=True, null_frac=null_frac)
    order = np.array([4, 0, 3, 1, 2], np.int32)       # the model list is not in state order (gmm->start)
    fr = synth.make_frames(model, T=257, seed=3)
    gm = dict(model=model, model_state=order, gprune_num=num)
    want = oracle.rejgmm_frame_scores(gm, fr)
    off = np.array([0, 100, 101, 257], np.int32)
    fs, us = lib.RejGmm(engine, model, order, num).scores_host(fr, off)
    assert np.array_equal(fs, want)
    for u in range(3):
        assert np.array_equal(us[u], oracle.rejgmm_accumulate(want[off[u]:off[u + 1]]))


def test_bad_arguments(engine, z):
    model = {k: z[k] for k in KEYS}
    with pytest.raises(lib.JamdError):
        lib.RejGmm(engine, model, z["model_state"], 0)
    with pytest.raises(lib.JamdError):
        lib.RejGmm(engine, model, [0, 99], 5)
    m = lib.RejGmm(engine, model, z["model_state"], 5)
    with pytest.raises(lib.JamdError):
        m.scores_host(z["frames"][:10], [0, 5])


def tied_model(nmodel, M, seed):
    """nmodel one-state GMMs of M mixtures each; in the first and the last, mixtures 2 and M - 1 are mixture 0's density
    once more under weights of their own (exactly tied scores)."""
    model = synth.make_gmm(S=nmodel, M=M, D=39, seed=seed, null_frac=0.05 if M > 6 else 0.0)
    model["ent_dens"] = model["ent_dens"].copy()
    for s in {0, nmodel - 1}:
        e0 = int(model["st_off"][s])
        model["ent_dens"][[e0 + 2, e0 + M - 1]] = model["ent_dens"][e0]
        model["ent_logw"][[e0 + 2, e0 + M - 1]] = np.log(model["weight"][[e0 + 2, e0 + M - 1]]).astype(np.float32)
    return model


def check(engine, oracle, model, order, num, fr, off):
    want = oracle.rejgmm_frame_scores(dict(model=model, model_state=order, gprune_num=num), fr)
    fs, us = lib.RejGmm(engine, model, order, num).scores_host(fr, off)
    assert np.array_equal(fs, want)
    for u in range(len(off) - 1):
        assert np.array_equal(us[u], oracle.rejgmm_accumulate(want[off[u]:off[u + 1]]))
    return us


@pytest.mark.parametrize("num,M", [(4, 9), (5, 9), (8, 20), (9, 20), (17, 40), (32, 40), (33, 40), (64, 64), (100, 6)])
def test_list_sizes_with_tied_mixtures(engine, oracle, num, M):
    """Both sides of every list size the frame kernel is instantiated with (4, 8, 16, 32, 64 slots for min(-gmmnum,
    largest mixture) entries), each with exactly tied Gaussians in a model; an empty utterance sums to 0."""
    model = tied_model(5, M, 100 + num)
    fr = synth.make_frames(model, T=70, seed=num)
    us = check(engine, oracle, model, np.array([4, 0, 3, 1, 2], np.int32), num, fr, np.array([0, 30, 30, 70], np.int32))
    assert np.all(us[1] == 0.0) and np.all(us[0] != 0.0)


@pytest.mark.parametrize("nmodel,T", [(5, 51), (4, 64), (1, 257), (1, 1)])
def test_frames_times_models_around_the_block(engine, oracle, nmodel, T):
    """One thread per (frame, model), 256 to a block: 255, 256 and 257 of them, and a single one."""
    model = tied_model(nmodel, 9, 7 * nmodel)
    fr = synth.make_frames(model, T=T, seed=T)
    check(engine, oracle, model, np.arange(nmodel, dtype=np.int32)[::-1].copy(), 4, fr, np.array([0, T], np.int32))


def test_more_than_64_kept_gaussians_are_refused(engine):
    model = synth.make_gmm(S=2, M=70, D=39, seed=1)
    with pytest.raises(lib.JamdError, match="64"):
        lib.RejGmm(engine, model, [0, 1], 70)
