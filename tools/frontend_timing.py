"""Device audio front end (jamd_frontend_run_dev) on the C3 batch shape -- 512 ragged utterances, 727 200
frames at 16 kHz / 10 ms -- beside the compiled reference's Wav2MFCC() on one host core of the same machine.

  python tools/frontend_timing.py [--reps 10] [--ref-frames 30000] [--ss off|calc|load] [--json out.json]
  python tools/frontend_timing.py --live [--reps 10] [--json out.json]

Device time: wall clock of run_dev + stream sync (median of --reps, after a warm-up), samples already on the
device.  Reference: the Wav2MFCC() call alone of oracle/_ref/libjref.so over utterances of the same length distribution
(--ref-frames frames in all), per frame, scaled to the batch.  Both kinds of the issue: MFCC_E_D_A_Z (39) and
MFCC_E_D_N_Z (25).

--ss calc runs the batch under -sscalc (a 300 ms head per utterance: two more kernels in front of the frame kernel),
--ss load under -ssload with one spectrum for all (taken from the first utterance); alpha 2.0, floor 0.5.  The default,
off, is the run without spectral subtraction.  The reference is not timed under --ss calc / load.

--live times the live-input front end (jamd_frontend_live_run_dev) on the same audio: 512 channels, one segment each,
MFCC_E_D_A_Z, the channels warm (two committed runs first, so that the MAP branch of the mean runs).  The live window is
one sample longer, so every channel yields one frame fewer than its utterance does in the buffered front end.  Three
figures come from one process, alternating: the buffered run, the live run, the live run plus commit -- each between
two HIP events recorded on the launch stream (through torch.cuda.ExternalStream), median and minimum of --reps."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from julius_amd import lib, synth  # noqa: E402

NUTT, FRAMES = 512, 727200


def batch(seed=0):
    """512 utterances, 727 200 frames in all, lengths spread 0.5x .. 1.5x the mean, cut from synthetic speech."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, NUTT)
    T = np.floor(w / w.sum() * FRAMES).astype(np.int64)
    T[: FRAMES - T.sum()] += 1
    src = synth.make_audio(16000 * 120, seed=seed + 1)
    utts = []
    for t in T:
        n = 400 + 160 * (int(t) - 1)
        reps = -(-n // len(src))
        a = int(rng.integers(0, len(src)))
        utts.append(np.roll(np.tile(src, reps), -a)[:n])
    return utts


def live_main(a):
    import ctypes as C

    import torch
    eng = lib.Engine(0)
    sp = C.c_void_p()
    assert lib.load().jamd_stream_create(eng.h, C.byref(sp)) == 0
    st = torch.cuda.ExternalStream(sp.value)
    utts = batch()
    samples, off = lib.Frontend._pack(utts)
    d_in = lib.DevBuf(eng, samples.nbytes).upload(samples)
    kind, vs = "MFCC_E_D_A_Z", 39
    fe = lib.Frontend.from_kind(eng, kind, vs)
    lv = lib.LiveFrontend(fe, NUTT)
    d_out = lib.DevBuf(eng, 4 * FRAMES * fe.veclen)
    steps = {"buffered_run": lambda: fe.run_dev(d_in.ptr, off, d_out.ptr, stream=sp.value),
             "live_run": lambda: lv.run_dev(d_in.ptr, off, d_out.ptr, stream=sp.value),
             "live_run_commit": lambda: (lv.run_dev(d_in.ptr, off, d_out.ptr, stream=sp.value), lv.commit(stream=sp.value))}
    for _ in range(2):                           # warm-up of every shape; the channels get their initial mean
        lfoff = steps["live_run_commit"]()[0]
        bfoff = steps["buffered_run"]()
    st.synchronize()
    assert bfoff[-1] == FRAMES and lfoff[-1] == FRAMES - NUTT, (bfoff[-1], lfoff[-1])
    ms = {k: [] for k in steps}
    for _ in range(a.reps):
        for k, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            st.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    out = {"channels": NUTT, "kind": kind, "frames_buffered": FRAMES, "frames_live": int(lfoff[-1]), "reps": a.reps,
           "timer": "HIP events on the launch stream", "ms": {}}
    for k, v in ms.items():
        out["ms"][k] = {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["live_over_buffered"] = round(out["ms"]["live_run"]["median"] / out["ms"]["buffered_run"]["median"], 3)
    out["live_commit_over_buffered"] = round(out["ms"]["live_run_commit"]["median"] / out["ms"]["buffered_run"]["median"], 3)
    line = json.dumps({"frontend_live_timing": out})
    print(line)
    if a.json:
        Path(a.json).write_text(line + "\n")
    lv.close()
    fe.close()
    lib.load().jamd_stream_destroy(eng.h, sp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-frames", type=int, default=30000)
    ap.add_argument("--ss", choices=("off", "calc", "load"), default="off")
    ap.add_argument("--json")
    ap.add_argument("--live", action="store_true")
    a = ap.parse_args()
    if a.live:
        return live_main(a)
    eng = lib.Engine(0)
    utts = batch()
    samples, off = lib.Frontend._pack(utts)
    d_in = lib.DevBuf(eng, samples.nbytes).upload(samples)
    out = {"utterances": NUTT, "frames": FRAMES, "samples": int(off[-1]), "ss": a.ss, "kinds": {}}
    for kind, vs in (("MFCC_E_D_A_Z", 39), ("MFCC_E_D_N_Z", 25)):
        fe = lib.Frontend.from_kind(eng, kind, vs)
        if a.ss == "calc":
            fe.set_ss(lib.SS_CALC)
        elif a.ss == "load":
            fe.set_ss(lib.SS_LOAD, noise=fe.noise_host(utts[:1])[0])
        d_out = lib.DevBuf(eng, 4 * FRAMES * fe.veclen)
        foff = fe.run_dev(d_in.ptr, off, d_out.ptr)
        eng.sync()
        assert foff[-1] == FRAMES, foff[-1]
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fe.run_dev(d_in.ptr, off, d_out.ptr)
            eng.sync()
            ts.append(time.perf_counter() - t0)
        dev_ms = 1e3 * float(np.median(ts))
        rec = {"device_ms_per_batch": round(dev_ms, 3), "device_ms_min": round(1e3 * min(ts), 3),
               "device_rtf_inv": round(FRAMES * 0.01 / (dev_ms / 1e3), 1)}
        try:
            if a.ss != "off":
                raise FileNotFoundError("the reference is timed without spectral subtraction only")
            from oracle import pyoracle
            from frontendref import RefFrontend
            rf = RefFrontend(pyoracle.Ref())
            v = rf.para(lib.param_kind(kind), vs)
            nref, tref, k = 0, 0.0, 0
            while nref < a.ref_frames:
                f = rf.wav2mfcc(utts[k], v)
                tref += rf.last_s
                nref += len(f)
                k += 1
            us = 1e6 * tref / nref
            rec.update(ref_us_per_frame_1core=round(us, 3), ref_rtf_inv_1core=round(1e4 / us, 1),
                       ref_ms_per_batch_1core=round(us * FRAMES / 1e3, 1),
                       ref_ms_per_batch_16core_ideal=round(us * FRAMES / 1e3 / 16, 1),
                       speedup_vs_1core=round(us * FRAMES / 1e3 / dev_ms, 1))
        except FileNotFoundError as e:
            rec["ref"] = f"not measured: {e}"
        out["kinds"][kind] = rec
        fe.close()
    line = json.dumps({"frontend_timing": out})
    print(line)
    if a.json:
        Path(a.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
