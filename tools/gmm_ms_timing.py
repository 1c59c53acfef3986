"""K1m (jamd_gmm_ms_outprob_dev) beside K1 (jamd_gmm_outprob_dev) at the benchmark's shape: 3000 states x 16 Gaussians,
64 000 frames.  The two-stream model is the single-stream one cut in two -- every Gaussian's dimensions 0..25 are
stream 1, 26..38 stream 2 -- so both kernels do the same Gaussian x dimension count.  Frames already on the device,
warm, HIP work timed by a host clock round a device synchronise; the two alternate, `--rounds` times."""
import argparse
import json
import time

import numpy as np

from julius_amd import lib, synth


def split_model(m, vsize=(26, 13)):
    """The multi-stream dict (lib.GmmStreams) of a plain single-stream model cut at the stream boundaries."""
    S, E, ns = len(m["st_off"]) - 1, len(m["ent_dens"]), len(vsize)
    soff = np.concatenate([[0], np.cumsum(vsize)])
    n = np.diff(m["st_off"])
    # pdf s * ns + k: state s, stream k; its entries are the state's in order; density e * ns + k: entry e's slice k
    pdf_off = np.concatenate([[0], np.cumsum(np.repeat(n, ns))]).astype(np.int32)
    ent = np.concatenate([np.arange(m["st_off"][s], m["st_off"][s + 1]) for s in range(S) for k in range(ns)])
    k_of = np.concatenate([np.full(n[s], k) for s in range(S) for k in range(ns)])
    # density e * ns + k is entry e's slice k: back to back they are the entry's own row
    var = m["var"].astype(np.float32)
    gconst = np.stack([synth.gconst_of(var[:, soff[k]:soff[k + 1]]) for k in range(ns)], axis=1).reshape(-1)
    return dict(vsize=np.asarray(vsize, np.int32), pdf_stream=np.tile(np.arange(ns, dtype=np.int32), S), pdf_off=pdf_off,
                ent_dens=(ent * ns + k_of).astype(np.int32), ent_logw=m["ent_logw"][ent],
                st_pdf=np.arange(S * ns, dtype=np.int32).reshape(S, ns),
                st_weight=np.random.default_rng(7).uniform(0.5, 1.5, (S, ns)).astype(np.float32),
                dens_off=np.concatenate([[0], np.cumsum(np.tile(np.asarray(vsize), E))]).astype(np.int32),
                mean=m["mean"].reshape(-1), ivar=(1.0 / var.astype(np.float64)).astype(np.float32).reshape(-1),
                gconst=gconst.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=3000)
    ap.add_argument("--mix", type=int, default=16)
    ap.add_argument("--frames", type=int, default=64000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    eng = lib.Engine(0)
    m = synth.make_gmm(S=a.states, M=a.mix, D=39, seed=1)
    fr = synth.make_frames(m, T=a.frames, seed=2)
    k1, k1m = lib.Gmm(eng, m), lib.GmmStreams(eng, split_model(m))
    d_fr = lib.DevBuf(eng, fr.nbytes).upload(fr)
    d_sc = lib.DevBuf(eng, 4 * a.frames * a.states)
    runs = {"k1": lambda: k1.outprob_dev(d_fr.ptr, a.frames, d_sc.ptr),
            "k1m": lambda: k1m.outprob_dev(d_fr.ptr, a.frames, d_sc.ptr)}
    ms = {k: [] for k in runs}
    for fn in runs.values():
        fn()
    eng.sync()
    for _ in range(a.rounds):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            eng.sync()
            ms[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(states=a.states, mix_per_stream=a.mix, frames=a.frames, vsize=[26, 13], iters=a.iters,
                          k1_kernel=k1.last_kernel(), k1m_kernel=k1m.last_kernel(), k1_ms=ms["k1"], k1m_ms=ms["k1m"],
                          k1_ms_median=med["k1"], k1m_ms_median=med["k1m"], ratio_k1m_over_k1=med["k1m"] / med["k1"],
                          gauss_dims_per_frame=a.states * a.mix * 39)))


if __name__ == "__main__":
    main()
