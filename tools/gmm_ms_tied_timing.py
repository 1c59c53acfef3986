"""K1mt (jamd_gmm_ms_create_opt) beside the single-stream tied-mixture path (jamd_gmm_create) at the tied-mixture shape
of tools/gmm_modes_timing.py: 3000 states over 129 codebooks of 64 Gaussians, 16 000 frames.  The two-stream model is
the single-stream one cut in two -- every codebook Gaussian's dimensions 0..25 are a member of a stream-1 book, 26..38
of a stream-2 book, and a state keeps its weight vector on both -- so both objects do the same Gaussian x dimension
count.  Both under -gprune none and under -gprune safe with gprune_num 2.  Frames already on the device, warm, HIP work
timed by a host clock round a device synchronise; the four alternate, `--rounds` times.  A record, not a gate."""
import argparse
import json
import time

import numpy as np

from julius_amd import lib, synth


def split_tied_model(m, vsize=(26, 13)):
    """The multi-stream dict (lib.GmmStreamsTied) of an all-tied single-stream model cut at the stream boundaries: book
    b of stream k is book b * ns + k, its member i the slice k of codebook Gaussian b * K + i."""
    S, K, ns = len(m["st_off"]) - 1, int(m["book_size"]), len(vsize)
    G = m["mean"].shape[0]
    soff = np.concatenate([[0], np.cumsum(vsize)])
    var = m["var"].astype(np.float32)
    gconst = np.stack([synth.gconst_of(var[:, soff[k]:soff[k + 1]]) for k in range(ns)], axis=1).reshape(-1)
    book = m["st_book"].astype(np.int64)
    members = (book[:, None, None] * K + np.arange(K)[None, None, :]) * ns + np.arange(ns)[None, :, None]   # [S][ns][K]
    logw = np.repeat(m["ent_logw"].reshape(S, 1, K), ns, axis=1)
    return dict(vsize=np.asarray(vsize, np.int32), pdf_stream=np.tile(np.arange(ns, dtype=np.int32), S),
                pdf_off=(np.arange(S * ns + 1) * K).astype(np.int32),
                pdf_book=(book[:, None] * ns + np.arange(ns)[None, :]).reshape(-1).astype(np.int32),
                ent_dens=members.reshape(-1).astype(np.int32), ent_logw=logw.reshape(-1).astype(np.float32),
                st_pdf=np.arange(S * ns, dtype=np.int32).reshape(S, ns), st_weight=None,
                dens_off=np.concatenate([[0], np.cumsum(np.tile(np.asarray(vsize), G))]).astype(np.int32),
                mean=m["mean"].reshape(-1), ivar=(1.0 / var.astype(np.float64)).astype(np.float32).reshape(-1),
                gconst=gconst.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=3000)
    ap.add_argument("--books", type=int, default=129)
    ap.add_argument("--book-size", type=int, default=64)
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    eng = lib.Engine(0)
    m = synth.make_tied_gmm(S=a.states, nbook=a.books, K=a.book_size, D=39, seed=1)
    fr = np.random.default_rng(3).normal(0, 1.5, (a.frames, 39)).astype(np.float32)
    ms_model = split_tied_model(m)
    objs = {"k1_none": lib.Gmm(eng, m, lib.GPRUNE_NONE, 0), "k1_safe2": lib.Gmm(eng, m, lib.GPRUNE_SAFE, 2),
            "k1mt_none": lib.GmmStreamsTied(eng, ms_model, gprune="none"),
            "k1mt_safe2": lib.GmmStreamsTied(eng, ms_model, gprune="safe", gprune_num=2)}
    d_fr = lib.DevBuf(eng, fr.nbytes).upload(fr)
    d_sc = lib.DevBuf(eng, 4 * a.frames * a.states)
    ms = {k: [] for k in objs}
    for o in objs.values():
        o.outprob_dev(d_fr.ptr, a.frames, d_sc.ptr)
    eng.sync()
    for _ in range(a.rounds):
        for name, o in objs.items():
            t0 = time.perf_counter()
            for _ in range(a.iters):
                o.outprob_dev(d_fr.ptr, a.frames, d_sc.ptr)
            eng.sync()
            ms[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(states=a.states, books=a.books, book_size=a.book_size, frames=a.frames, vsize=[26, 13], iters=a.iters,
                          kernels={k: o.last_kernel() for k, o in objs.items()}, ms=ms, ms_median=med,
                          ratio_k1mt_over_k1_none=med["k1mt_none"] / med["k1_none"],
                          ratio_k1mt_over_k1_safe2=med["k1mt_safe2"] / med["k1_safe2"],
                          gauss_dims_per_frame=a.books * a.book_size * 39)))


if __name__ == "__main__":
    main()
