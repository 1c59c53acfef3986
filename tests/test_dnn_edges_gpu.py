"""DNN-HMM scoring (csrc/dnn.hip) where tests/test_dnn_gpu.py does not reach: the chunked path of calls of
131 072 frames and more, the grid-stride loops of the packing and normalisation kernels, both clamp branches and the
table ends of the logistic, the cut-off of the output log-sum, and shapes no other test builds.

One comparison throughout: np.array_equal with oracle.dnn_outprob(dnn, frames, po.DNN_FMA), the C restatement of
calc_dnn.c:774-868 / calc_dnn_fma.c:19-80 that test_dnn_gpu.py::test_full_size_envr_shape pins to the compiled
reference.  No tolerance anywhere.

The conditions on the inputs (shares of saturated units, of terms below the cut-off) are computed by a float64 numpy
forward pass before any device call; the shares measured when the cases were written stand beside them.

Oracle seconds on one CPU core (whole parametrised test, all cases): test_chunked_call_equals_oracle 19 s,
test_strided_tails 1.5 s, test_shapes_the_suite_never_built 3 s, every other test well under 1 s."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from julius_amd import lib, synth
from oracle import pyoracle as po

gpu = pytest.mark.gpu

LOG_ADDMIN = -13.815510558          # stddefs.h:176, a double constant
LOG_ZERO = -1000000.0               # stddefs.h:171
F32 = np.float32


def fl_up_addmin():
    """engine.hip:90-91: `tmp < LOG_ADDMIN` (addlog.c:114) for a float tmp is `tmp < a`, a the smallest float >= the
    double constant."""
    a = F32(LOG_ADDMIN)
    if float(a) < LOG_ADDMIN:
        a = np.nextafter(a, F32(np.inf))
    assert float(a) >= LOG_ADDMIN > float(np.nextafter(a, F32(-np.inf)))
    return a


def chunk_plan(T):
    """nchunk / per of jamd_dnn_outprob_dev (dnn.hip, the chunking of long calls) restated."""
    nchunk = (T + 32767) // 32768 if T >= 131072 else 1
    nchunk = min(nchunk, 8)
    per = ((T + nchunk - 1) // nchunk + 127) // 128 * 128
    return nchunk, per


def first_diff(got, want, per=None):
    """As tests/test_frontend_gpu.py::first_diff; for chunked calls also the chunk the first differing row is in."""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad) == 0:
        return "none"
    t, s = (int(v) for v in bad[0])
    msg = f"{len(bad)} values differ, first at frame {t} state {s}: device {got[t, s]!r} oracle {want[t, s]!r}"
    if per:
        rows = np.unique(bad[:, 0])
        msg += f"; frame {t} is in chunk {t // per} (chunks of {per}); chunks with differences {sorted(set((rows // per).tolist()))}"
    return msg


def check(engine, oracle, dnn, fr, what=""):
    net = lib.Dnn(engine, dnn)
    try:
        got = net.outprob_host(fr)
    finally:
        net.close()
    want = oracle.dnn_outprob(dnn, fr, po.DNN_FMA)
    assert not np.isnan(want).any(), f"{what}: the oracle returns NaN: not a contract"
    assert np.array_equal(got, want), f"{what}: {first_diff(got, want, chunk_plan(len(fr))[1] if len(fr) >= 131072 else None)}"
    return got


def noise(seed, T, D, sd=1.0):
    return np.random.default_rng(seed).normal(0.0, sd, (T, D)).astype(np.float32)


# ------------------------------------------------------------------------------------------ float64 conditions
def forward64(dnn, fr):
    """dnn_calc_outprob() in float64 numpy (the pattern of synth._dnn_hidden): the hidden layers' pre-activations
    and the output layer's values."""
    h = np.asarray(fr, dtype=np.float64)
    pre = []
    for w, b in zip(dnn["w"][:-1], dnn["b"][:-1]):
        v = h @ w.astype(np.float64).T + b.astype(np.float64)
        pre.append(v)
        h = 1.0 / (1.0 + np.exp(-np.clip(v, -8.0, 8.0)))
    return pre, h @ dnn["w"][-1].astype(np.float64).T + dnn["b"][-1].astype(np.float64)


def clamp_shares(dnn, fr):
    """Per hidden layer: (share of pre-activations <= -8, share >= 8)."""
    return [(float(np.mean(v <= -8.0)), float(np.mean(v >= 8.0))) for v in forward64(dnn, fr)[0]]


def far_share(dnn, fr):
    """Share of (frame, output) pairs more than 13.8155 below their row's maximum: such a term can only meet the
    cut-off branch of addlog_array() once the maximum has been scanned."""
    o = forward64(dnn, fr)[1]
    return float(np.mean(o.max(axis=1, keepdims=True) - o > 13.8155))


# ------------------------------------------------------------------------------------------------ host only
def test_make_dnn_default_arrays_unchanged():
    """gain = out_gain = 1.0 must leave make_dnn()'s arrays byte for byte what they were before the two arguments
    existed (every other DNN test and the benchmark draw their networks from it).  The digest was computed from the
    generator as it was before the arguments were added."""
    want = "f2fad23201e74dd92abe770e7e79e821de831040132768d1a7188bc64e098a8e"
    for d in (synth.make_dnn(dims=(48, 64, 64, 40), seed=3), synth.make_dnn(dims=(48, 64, 64, 40), seed=3, gain=1.0, out_gain=1.0)):
        h = hashlib.sha256()
        for a in d["w"] + d["b"] + [d["prior"]]:
            assert a.dtype == np.float32
            h.update(np.ascontiguousarray(a).tobytes())
        assert h.hexdigest() == want
    g = synth.make_dnn(dims=(48, 64, 64, 40), seed=3, gain=8.0, out_gain=4.0)
    d = synth.make_dnn(dims=(48, 64, 64, 40), seed=3)
    assert np.array_equal(g["w"][0], d["w"][0] * F32(8)) and np.array_equal(g["w"][1], d["w"][1] * F32(8))
    assert np.array_equal(g["w"][2], d["w"][2] * F32(4))
    assert all(np.array_equal(x, y) for x, y in zip(g["b"], d["b"])) and np.array_equal(g["prior_lin"], d["prior_lin"])


CHUNK_T = (131071, 131072, 131073, 200001, 262221, 300000)


def test_chunk_plan():
    """The T list of test_chunked_call_equals_oracle is chosen against these constants: one frame below the
    threshold, exactly on it (whole chunks), one past it (a fifth chunk, its last tile holding one frame), seven
    ragged chunks, and two lengths at which the chunk count is capped at eight.  If this fails because the constants
    of jamd_dnn_outprob_dev were retuned, restate them in chunk_plan() AND move CHUNK_T so that it again covers:
    below / on / just past the threshold, a ragged last chunk, and the cap."""
    def plan(T):
        nchunk, per = chunk_plan(T)
        used = (T + per - 1) // per                  # chunks the loop `for (t0 = 0; t0 < T; t0 += per)` runs
        return nchunk, per, used, T - (used - 1) * per
    assert plan(131071) == (1, 131072, 1, 131071)
    assert plan(131072) == (4, 32768, 4, 32768)
    assert plan(131073) == (5, 26240, 5, 26113) and 26113 % 128 == 1
    assert plan(200001) == (7, 28672, 7, 27969)
    assert (200001 + 32767) // 32768 == 7
    assert (262221 + 32767) // 32768 == 9 and plan(262221)[:3] == (8, 32896, 8)
    assert plan(300000) == (8, 37504, 8, 37472)
    for T in CHUNK_T:                                # never more chunks than events, every chunk non-empty
        nchunk, per, used, last = plan(T)
        assert used <= nchunk <= 8 and 0 < last <= per and per % 128 == 0


# ------------------------------------------------------------------------------- A. probe networks (exact values)
def logistic_edge_inputs():
    up, dn = F32(np.inf), F32(-np.inf)
    v = []
    for e in (F32(-8.0), F32(8.0)):
        v += [np.nextafter(e, dn), e, np.nextafter(e, up)]
    fi = np.finfo(np.float32)
    v += [F32(0.0), F32(-0.0), F32(1e30), F32(-1e30), fi.max, -fi.max, fi.tiny, F32(1e-41)]   # 1e-41: subnormal
    ks = [0, 1, 2, 159999, 160000, 160001, 319998, 319999, 320000]
    ks += [int(k) for k in np.random.default_rng(2024).integers(0, 320001, 200)]
    for k in ks:                                     # the rounding boundary between table slots k and k + 1
        c = F32((k + 0.5) / 20000.0 - 8.0)
        v += [np.nextafter(c, dn), c, np.nextafter(c, up)]
    v = np.array(v, dtype=np.float32)
    assert np.isfinite(v).all() and len(v) == 14 + 3 * 209
    return v


@gpu
@pytest.mark.parametrize("layout", ["packed", "isolated"])
def test_logistic_edges(engine, oracle, layout):
    """The hidden probe's pre-activations ARE its inputs, so the inputs sit on the clamp compares (v <= -8, v >= 8,
    calc_dnn.c:813-818), far outside them, and on the rounding boundary of the table index (float add, float
    multiply, double + 0.5, truncation) at both ends, the middle and 200 random slots of the table.
    packed: eight values per frame, unit output weights.  isolated: one value per frame, the seven other units at
    -9 (clamped), output weights 65536 -- the log-softmax of the packed form rounds the activations to the ulp of the
    row's log-sum (about 2.6), which hides a neighbouring table entry; scaled and alone, every bit of the activation
    reaches the other seven outputs."""
    v = logistic_edge_inputs()
    if layout == "packed":
        dnn = synth.make_probe_dnn(S=8, hidden=True)
        fr = np.concatenate([v, np.zeros(-len(v) % 8, np.float32)]).reshape(-1, 8)
        # and every value once in every column (the eight chains are eight different accumulator passes)
        fr = np.concatenate([np.roll(fr, j, axis=1) for j in range(8)])
    else:
        dnn = synth.make_probe_dnn(S=8, hidden=True, scales=np.full(8, 65536.0, np.float32))
        fr = np.full((len(v), 8), -9.0, np.float32)
        fr[np.arange(len(v)), np.arange(len(v)) % 8] = v
    got = check(engine, oracle, dnn, fr, layout)
    assert np.isfinite(got).all()


def logsum_rows(P, a):
    """Rows of P <= 8 output values (see test_logsum_edges)."""
    rows = [np.full(P, c, np.float32) for c in (0.0, 1.5, -3.25, 700.0)]
    for step in (0.01, 1.0, 20.0):
        r = (F32(-2.0) + F32(step) * np.arange(P, dtype=np.float32)).astype(np.float32)
        rows += [r, r[::-1].copy()]
    up, dn = F32(np.inf), F32(-np.inf)
    near = [a, np.nextafter(a, up), np.nextafter(a, dn), F32(-13.8154), F32(-13.8156), F32(-14.0)]
    for dom in sorted({0, P - 1}):                   # the scan runs from the last column to the first
        for other in sorted({(dom + 1) % P, (dom - 1) % P, (dom + P // 2) % P} - {dom}):
            for x in near:
                r = np.full(P, -50.0, np.float32)
                r[other] = x
                r[dom] = 0.0
                rows.append(r)
    for base in (1e4, -1e4):
        rows.append((F32(base) + F32(0.37) * np.arange(P, dtype=np.float32)).astype(np.float32))
        rows.append(np.full(P, base, np.float32))
    rows += [np.full(P, LOG_ZERO, np.float32), np.full(P, 2 * LOG_ZERO, np.float32)]
    for dom in sorted({0, P - 1}):
        for c in (LOG_ZERO, 2 * LOG_ZERO):
            r = np.full(P, c, np.float32)
            r[dom] = 0.0
            rows.append(r)
            r = np.where(np.arange(P) % 2 == 0, F32(LOG_ZERO), F32(2 * LOG_ZERO)).astype(np.float32)
            rows.append(r)
    rng = np.random.default_rng(99)
    for sd in (0.1, 3.0, 10.0, 30.0):
        rows += list(rng.normal(0.0, sd, (40, P)).astype(np.float32))
    return np.array(rows, dtype=np.float32)


@gpu
@pytest.mark.parametrize("S,with_prior", [(S, False) for S in (1, 3, 8, 15, 16, 17, 33, 64)] + [(8, True), (17, True)])
def test_logsum_edges(engine, oracle, S, with_prior):
    """Output probe: output i is scales[i] * x_(i mod 8) exactly (scales are powers of two, cycled with period 4, so
    outputs i and i + 8 are equal), which puts the difference of two terms of addlog_array() (addlog.c:103-123) ON
    the cut-off `tmp < LOG_ADDMIN`: the dominant output is exactly 0.0f and another is a = fl_up(LOG_ADDMIN), each
    float32 neighbour of a, -13.8154, -13.8156, -14; the rest at -50.  With the dominant term 0 the table term at
    the cut-off (1e-6) is the whole sum and shows in every output of the row."""
    a = fl_up_addmin()
    scales = np.array([(1.0, 0.5, 2.0, -1.0)[i % 4] for i in range(S)], dtype=np.float32)
    prior = None
    if with_prior:
        p = np.random.default_rng(S).dirichlet(np.full(S, 5.0)).astype(np.float32)
        prior = np.log10(p.astype(np.float64)).astype(np.float32)
    dnn = synth.make_probe_dnn(S=S, hidden=False, scales=scales, prior=prior)
    P = min(S, 8)
    z = logsum_rows(P, a)
    fr = np.zeros((len(z), 8), np.float32)
    fr[:, :P] = z / scales[:P]                       # exact: powers of two, no overflow or underflow in these rows
    assert np.array_equal((fr[:, :P] * scales[:P]).astype(np.float32), z)
    if P >= 2:                                       # the rows do put a difference of exactly a, and its neighbours, before the compare
        d = z[:, None, :] - z[:, :, None]
        for x in (a, np.nextafter(a, F32(np.inf)), np.nextafter(a, F32(-np.inf))):
            assert (d == x).any()
    check(engine, oracle, dnn, fr, f"S={S}")


# ------------------------------------------------------------------------- B. saturating and peaked random networks
SAT_DIMS = [(48, 64, 64, 40), (528, 256, 256, 100), (24, 136, 200, 129)]


@gpu
@pytest.mark.parametrize("dims", SAT_DIMS)
def test_saturated_hidden_units(engine, oracle, dims):
    """gain = 8: both clamp branches of the logistic are taken by a large share of the units of every hidden layer.
    Measured (seed 1, T = 300, float64 forward pass), share <= -8 / share >= 8:
      (48, 64, 64, 40)      layer 1 0.243 / 0.251, layer 2 0.065 / 0.064
      (528, 256, 256, 100)  layer 1 0.252 / 0.253, layer 2 0.068 / 0.058
      (24, 136, 200, 129)   layer 1 0.241 / 0.249, layer 2 0.076 / 0.054
    (at gain 6 the second layer holds 0.017 - 0.025 per clamp: too few)"""
    dnn = synth.make_dnn(dims=dims, seed=1, gain=8.0)
    fr = noise(1, 300, dims[0], 1.5)
    for l, (lo, hi) in enumerate(clamp_shares(dnn, fr)):
        need = 0.10 if l == 0 else 0.03
        assert lo >= need and hi >= need, f"hidden layer {l + 1}: shares {lo:.3f} / {hi:.3f} below {need}: the case is empty"
    check(engine, oracle, dnn, fr, str(dims))


# out_gain per shape, found with far_share() on the CPU; measured share of (frame, output) pairs more than 13.8155
# below their row's maximum (seed 1, T = 300, gain 1)
# (out_gain 6 leaves 0.010 / 0.007 / 0.054 far, out_gain 24 gives 0.898 / 0.868 / 0.956)
PEAKED = [((48, 64, 64, 40), 13.0, 0.527), ((528, 256, 256, 100), 13.0, 0.535), ((24, 136, 200, 129), 9.0, 0.479)]


@gpu
@pytest.mark.parametrize("dims,out_gain,measured", PEAKED)
def test_peaked_outputs_pass_the_addlog_cutoff(engine, oracle, dims, out_gain, measured):
    """Rows whose terms lie on both sides of the log-sum's cut-off: at least 10 % of the (frame, output) pairs more
    than 13.8155 below their row's maximum (dnn_lse_kernel skips the table for them once the maximum is in the
    running sum), at least 10 % within it."""
    dnn = synth.make_dnn(dims=dims, seed=1, out_gain=out_gain)
    fr = noise(1, 300, dims[0], 1.5)
    far = far_share(dnn, fr)
    assert 0.10 <= far <= 0.90, f"share of far pairs {far:.3f} (was {measured}): the case is one-sided"
    check(engine, oracle, dnn, fr, str(dims))


@gpu
def test_saturated_network_vs_compiled_reference(engine, oracle, ref, tmp_path):
    """The clamp branches against calc_dnn.c:813-818 itself (the compiled reference's dnn_calc_outprob() on the same
    .npy files), not only against the restatement.  Equal hidden widths: a limitation of the reference's loader."""
    dims = (48, 64, 64, 40)
    dnn = synth.make_dnn(dims=dims, seed=1, gain=8.0)
    fr = noise(7, 200, dims[0], 1.5)
    for l, (lo, hi) in enumerate(clamp_shares(dnn, fr)):         # measured: 0.251 / 0.248, 0.064 / 0.060
        need = 0.10 if l == 0 else 0.03
        assert lo >= need and hi >= need, f"hidden layer {l + 1}: shares {lo:.3f} / {hi:.3f} below {need}"
    got = check(engine, oracle, dnn, fr, "restatement")
    if b"FMA" in ref.lib.jref_simd_string():         # the reference picks the best SIMD kernel of the host CPU
        want_ref = ref.dnn_load(dnn, tmp_path, num_threads=1).outprob(fr)
        assert np.array_equal(got, want_ref), f"vs compiled reference: {first_diff(got, want_ref)}"


# ------------------------------------------------------------------------------------------------ C. long calls
@gpu
@pytest.mark.parametrize("T", [4095, 4096, 4097, 16384, 16385, 40000])
@pytest.mark.parametrize("dims", [(16, 8, 8, 5), (24, 136, 8, 36)])
def test_strided_tails(engine, oracle, dims, T):
    """dnn_pack_rm_kernel walks the frames with gridDim.y capped at 16 384, dnn_norm_kernel at 4 096; T on, one
    below and one past each cap, and several strides long.  S = 5 takes dnn_norm_kernel's scalar branch, S = 36 its
    float4 branch; the second shape has a straddling first layer and a 136-wide layer of two output tiles."""
    dnn = synth.make_dnn(dims=dims, seed=11)
    check(engine, oracle, dnn, noise(T, T, dims[0], 1.5), f"{dims} T={T}")


def _dev_call(engine, net, fr, S):
    """jamd_dnn_outprob_dev on a stream and buffers of the caller's."""
    T = len(fr)
    d_in = lib.DevBuf(engine, fr.nbytes).upload(fr)
    d_out = lib.DevBuf(engine, 4 * T * S).upload(np.full((T, S), np.nan, np.float32))   # nothing stale can pass
    s = C.c_void_p()
    assert lib.load().jamd_stream_create(engine.h, C.byref(s)) == 0
    try:
        net.outprob_dev(d_in.ptr, T, d_out.ptr, stream=s.value)
        assert lib.load().jamd_stream_sync(engine.h, s) == 0
    finally:
        lib.load().jamd_stream_destroy(engine.h, s)
    out = d_out.download((T, S), np.float32)
    d_in.free(); d_out.free()
    return out


@gpu
@pytest.mark.parametrize("T", CHUNK_T)
@pytest.mark.parametrize("dims", [(16, 8, 8, 5), (16, 8, 12), (24, 136, 8, 36)])
def test_chunked_call_equals_oracle(engine, oracle, dims, T):
    """Calls of 131 072 frames and more are cut into up to eight chunks whose log-sum and normalisation run on a side
    stream (test_chunk_plan says what each T does to the plan).  The frames are seeded noise, every row different: a
    chunk that reads or writes another chunk's rows cannot pass.  For T = 200 001 on the first shape the same object
    then serves a 1-frame and a 257-frame call (buffers re-used at a smaller size), the long call again through
    jamd_dnn_outprob_dev on a stream and buffers of the caller's (the events and the side stream were created by a
    call on the engine's stream), and once more through the host entry.  Calls are sequential."""
    dnn = synth.make_dnn(dims=dims, seed=13)
    fr = noise(T, T, dims[0], 1.5)
    per = chunk_plan(T)[1]
    want = oracle.dnn_outprob(dnn, fr, po.DNN_FMA)
    net = lib.Dnn(engine, dnn)
    try:
        got = net.outprob_host(fr)
        assert np.array_equal(got, want), f"{dims} T={T}: {first_diff(got, want, per)}"
        if T == 200001 and dims == (16, 8, 8, 5):
            for lo, n in ((150000, 1), (28672 - 100, 257)):
                short = net.outprob_host(fr[lo:lo + n])
                assert np.array_equal(short, want[lo:lo + n]), f"{n}-frame call after the long one: {first_diff(short, want[lo:lo + n])}"
            again = _dev_call(engine, net, fr, dims[-1])
            assert np.array_equal(again, want), f"outprob_dev on the caller's stream: {first_diff(again, want, per)}"
            again = net.outprob_host(fr)
            assert np.array_equal(again, want), f"host entry after the device entry: {first_diff(again, want, per)}"
    finally:
        net.close()


# ---------------------------------------------------------------------------------------------------- D. shapes
@gpu
@pytest.mark.parametrize("T", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("dims", [
    (64, 40), (528, 129),                  # no hidden layer: (straddling) chains and the output epilogue in one kernel
    (512, 512, 512, 64), (768, 256, 24),   # non-straddle chains of two and three slabs (kmp 64 and 96)
    (40, 8, 1040, 8, 3),                   # an 8-wide layer (the epilogue writes its zero padding) feeding nine output tiles, and back
    (8, 8, 1),                             # one output: the log-softmax of a single term
])
def test_shapes_the_suite_never_built(engine, oracle, dims, T):
    dnn = synth.make_dnn(dims=dims, seed=17)
    check(engine, oracle, dnn, noise(1000 + T, T, dims[0], 1.5), f"{dims} T={T}")
