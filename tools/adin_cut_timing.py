"""The silence cutting stage (jamd_adin_cut_push_dev) timed beside the stage before it and the one behind it.

  python tools/adin_cut_timing.py [--reps 10] [--json out.json]

Samples already on the device; every figure lies between two HIP events recorded on the launch stream (through
torch.cuda.ExternalStream), after a warm-up, median / min / max of --reps.  The audio is 16 kHz: synthetic speech of
0.6 s between 0.9 s of N(0, 30) noise, every channel at another offset, default parameters (-lv 2000 -zc 60
-headmargin 300 -tailmargin 400 -chunksize 1000).
  push_4000    one push of 4 000 samples per channel (a quarter of a second) for 1 / 64 / 512 channels, in the middle of
               a stream
  batch        512 channels of about 227 000 samples (1 420 frames), one push with end of stream
Beside each: jamd_adin_push_dev() (zero stripping + -zmean at 16 kHz) over the same samples, and
jamd_frontend_live_push_dev() over what the cutting delivered, one call per part, taken in the same run.
A push waits once for its part tables (the part count is data), and the event pair spans that wait: `cut` is the device
work plus the host's turn-around in the middle.  `host_ms` is the wall clock of the call, `wait_us` one blocking copy of
64 KiB (the tables of 512 channels and 4 parts) to the host on an idle device, measured alone: what the design pays for the count being
data.  `floor_us` is 2 B read + 2 B written per sample over 8 TB/s.  A per-kernel trace is a run of its own
(rocprofv3 --kernel-trace -- python tools/adin_cut_timing.py --reps 3)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

from julius_amd import lib, synth  # noqa: E402

KIND, VS = "MFCC_E_D_A_Z", 39
FRAMES, NCHAN = 1420, 512
N16 = 401 + 160 * (FRAMES - 1)
PUSH = 4000
HBM = 8e12


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def source(seconds, seed=1):
    rng = np.random.default_rng(seed)
    out, n = [], 0
    while n < 16000 * seconds:
        out.append(np.round(rng.normal(0, 30, 14400)).astype(np.int16))
        out.append(synth.make_audio(9600, seed=seed + len(out), dc=0.0, zero_runs=0, silent_frac=0, clip=False))
        n += 24000
    return np.concatenate(out)


def windows(src, nchan, n, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([np.roll(src, -int(rng.integers(0, len(src))))[:n] for _ in range(nchan)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    eng = lib.Engine(0)
    sp = C.c_void_p()
    assert lib.load().jamd_stream_create(eng.h, C.byref(sp)) == 0
    st = torch.cuda.ExternalStream(sp.value)

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        r = fn()
        e1.record(st)
        st.synchronize()
        return r, e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

    out = {"kind": KIND, "reps": a.reps, "timer": "HIP events on the launch stream", "device": torch.cuda.get_device_name(0),
           "runs": 1}
    fe = lib.Frontend.from_kind(eng, KIND, VS)
    src = source(60)

    # ---- the wait alone: tables of the size 512 channels and 4 parts have, to the host, blocking
    probe = lib.DevBuf(eng, 64 * 1024)
    waits = []
    for i in range(a.reps + 2):
        st.synchronize()
        t0 = time.perf_counter()
        probe.download((64 * 1024,), np.uint8)
        if i >= 2:
            waits.append(1e6 * (time.perf_counter() - t0))
    out["wait_us"] = stats(waits)
    probe.free()

    # ---- one push in a stream
    out["push_4000"] = {}
    for nchan in (1, 64, 512):
        npush = 16
        seg = windows(src, nchan, npush * PUSH, seed=3)
        bufs = [lib.DevBuf(eng, 2 * nchan * PUSH).upload(np.ascontiguousarray(seg[:, j * PUSH:(j + 1) * PUSH]))
                for j in range(npush)]
        ioff = np.arange(nchan + 1, dtype=np.int64) * PUSH
        ad = lib.Adin(eng, nchan, lib.Adin.desc_for(zmean=True))
        cut = lib.AdinCut(eng, nchan)
        lv = lib.LiveFrontend(fe, nchan)
        d_mid = lib.DevBuf(eng, 2 * nchan * PUSH)
        d_cut = lib.DevBuf(eng, 2 * nchan * cut.push_cap(PUSH))
        d_out = lib.DevBuf(eng, 4 * nchan * (cut.push_cap(PUSH) // 160 + 64) * lv.veclen)
        t_ad, t_cut, t_host, t_lv, delivered, parts = [], [], [], [], 0, 0
        for rep in range(a.reps + 1):
            ad.reset(stream=sp.value)
            cut.reset(stream=sp.value)
            for j in range(npush):
                off, ms_ad, _ = span(lambda: ad.push_dev(bufs[j].ptr, ioff, d_mid.ptr, stream=sp.value))
                (poff, pfin, _), ms_cut, ms_host = span(lambda: cut.push_dev(d_mid.ptr, off, d_cut.ptr, max_parts=4,
                                                                            stream=sp.value))

                def live():
                    for row in range(len(poff)):
                        lv.push_dev(d_cut.ptr, poff[row], d_out.ptr, final=pfin[row], stream=sp.value)
                _, ms_lv, _ = span(live)
                if rep and j:
                    t_ad.append(1e3 * ms_ad); t_cut.append(1e3 * ms_cut); t_host.append(1e3 * ms_host); t_lv.append(1e3 * ms_lv)
                    delivered += int(poff[-1, -1]) if len(poff) else 0
                    parts += len(poff)
        n = len(t_cut)
        out["push_4000"][str(nchan)] = {
            "adin_strip_zmean_us": stats(t_ad), "cut_us": stats(t_cut), "cut_host_us": stats(t_host),
            "frontend_live_push_dev_us": stats(t_lv), "samples_delivered_per_push": round(delivered / n, 1),
            "parts_per_push": round(parts / n, 2),
            "floor_us": round(1e6 * nchan * PUSH * 4 / HBM, 3)}
        for o in (lv, cut, ad):
            o.close()
        for b in bufs + [d_mid, d_cut, d_out]:
            b.free()

    # ---- the batch
    seg = windows(src, NCHAN, N16, seed=5)
    ioff = np.arange(NCHAN + 1, dtype=np.int64) * N16
    d_in = lib.DevBuf(eng, seg.nbytes).upload(seg)
    ad = lib.Adin(eng, NCHAN, lib.Adin.desc_for(zmean=True))
    cut = lib.AdinCut(eng, NCHAN)
    lv = lib.LiveFrontend(fe, NCHAN)
    d_mid = lib.DevBuf(eng, 2 * NCHAN * N16)
    d_cut = lib.DevBuf(eng, 2 * NCHAN * cut.push_cap(N16))
    maxp = cut.parts_cap(N16)
    t_ad, t_cut, t_host, t_lv = [], [], [], []
    eos = np.ones(NCHAN, bool)
    d_out = None
    for rep in range(a.reps + 2):
        ad.reset(stream=sp.value)
        off, ms_ad, _ = span(lambda: ad.push_dev(d_in.ptr, ioff, d_mid.ptr, stream=sp.value))
        (poff, pfin, _), ms_cut, ms_host = span(lambda: cut.push_dev(d_mid.ptr, off, d_cut.ptr, eos, max_parts=maxp,
                                                                    stream=sp.value))
        if d_out is None:
            d_out = lib.DevBuf(eng, 4 * (int(np.diff(poff, axis=1).max(initial=0)) // 160 + 64) * NCHAN * lv.veclen)

        def live():
            for row in range(len(poff)):
                lv.push_dev(d_cut.ptr, poff[row], d_out.ptr, final=pfin[row], stream=sp.value)
        _, ms_lv, _ = span(live)
        if rep >= 2:
            t_ad.append(ms_ad); t_cut.append(ms_cut); t_host.append(ms_host); t_lv.append(ms_lv)
    out["batch"] = {"channels": NCHAN, "samples_in_per_channel": N16, "samples_behind_adin": int(off[-1]),
                    "samples_delivered": int(poff[-1, -1]), "parts": len(poff), "max_parts": int(maxp),
                    "adin_strip_zmean_ms": stats(t_ad), "cut_ms": stats(t_cut), "cut_host_ms": stats(t_host),
                    "frontend_live_push_dev_ms": stats(t_lv), "floor_ms": round(1e3 * int(off[-1]) * 4 / HBM, 4)}
    for o in (lv, cut, ad, fe):
        o.close()
    for b in (d_in, d_mid, d_cut, d_out):
        b.free()
    line = json.dumps({"adin_cut_timing": out})
    print(line)
    if a.json:
        Path(a.json).write_text(line + "\n")
    lib.load().jamd_stream_destroy(eng.h, sp)


if __name__ == "__main__":
    main()
