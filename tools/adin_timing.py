"""The audio conditioning stage (jamd_adin_push_dev) timed beside the front end that takes its output.

  python tools/adin_timing.py [--reps 10] [--json out.json] [--fir-3to4 FILE --fir-2to1 FILE]

Samples already on the device; every figure lies between two HIP events recorded on the launch stream (through
torch.cuda.ExternalStream), after a warm-up, median / min / max of --reps.
  batch_48k_all_steps   512 channels of about 1 420 frames as 48 kHz input, one chunk each (a file shorter than 20 s),
                        -48 + -lvscale 1.5 + zero stripping + -zmean; beside jamd_frontend_run_dev() over its output
  batch_16k_strip_zmean the same audio at 16 kHz, stripping and -zmean alone
  push_25_frames        one push of 12 000 samples at 48 kHz (25 frames at 10 ms) for 1 / 64 / 512 channels, all steps on, in
                        the middle of a stream: while sub_zmean() still estimates (first 48 000 samples of the stream) and
                        after; beside jamd_frontend_live_push_dev() over its output
With stripping on a push waits for its counts (one wait on the stream), so the host sees the device time of every push;
the event pairs hold the device work alone.  The two coefficient tables are the caller's: files in the text format of the
reference's load_filter() (one number per line), or -- without the two options -- a windowed-sinc low-pass of the
reference's lengths (217 and 401 taps) made here: the cost depends on the lengths only.  A per-kernel trace is a run of
its own (rocprofv3 --kernel-trace -- python tools/adin_timing.py --reps 3)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

from julius_amd import lib, synth  # noqa: E402

KIND, VS = "MFCC_E_D_A_Z", 39
FRAMES, NCHAN = 1420, 512
N16 = 401 + 160 * (FRAMES - 1)
PUSH48 = 12000


def lowpass(ntaps, cutoff, gain):
    """Hamming-windowed sinc, `cutoff` as a fraction of the sampling rate."""
    n = np.arange(ntaps) - (ntaps - 1) / 2
    return gain * 2 * cutoff * np.sinc(2 * cutoff * n) * np.hamming(ntaps)


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def windows(src, nchan, n, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([np.roll(src, -int(rng.integers(0, len(src))))[:n] for _ in range(nchan)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fir-3to4")
    ap.add_argument("--fir-2to1")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    if a.fir_3to4 and a.fir_2to1:
        tabs, src_tabs = (lib.adin_fir_read(a.fir_3to4), lib.adin_fir_read(a.fir_2to1)), "files"
    else:
        tabs, src_tabs = (lowpass(217, 1 / 8 * 0.9, 4.0), lowpass(401, 1 / 4 * 0.9, 1.0)), "windowed sinc made by the tool"
    eng = lib.Engine(0)
    sp = C.c_void_p()
    assert lib.load().jamd_stream_create(eng.h, C.byref(sp)) == 0
    st = torch.cuda.ExternalStream(sp.value)

    def timed_ms(fn, reps):
        for _ in range(2):
            fn()
        st.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            st.synchronize()
            ms.append(e0.elapsed_time(e1))
        return stats(ms)

    out = {"kind": KIND, "channels": NCHAN, "frames": FRAMES, "reps": a.reps, "timer": "HIP events on the launch stream",
           "device": torch.cuda.get_device_name(0), "tables": {"from": src_tabs, "n_3to4": len(tabs[0]), "n_2to1": len(tabs[1])}}
    try:
        out["clock_mhz"] = torch.cuda.clock_rate()
    except Exception as e:                       # (needs the SMI bindings)
        out["clock_mhz"] = f"not read: {type(e).__name__}"
    fe = lib.Frontend.from_kind(eng, KIND, VS)

    # ---- the batch
    src48 = synth.make_audio(48000 * 40, seed=1, sfreq=48000, zero_runs=40)
    src16 = synth.make_audio(16000 * 40, seed=2, zero_runs=40)
    for name, src, n, kw in (("batch_48k_all_steps", src48, 3 * N16 + 2400, dict(fir_3to4=tabs[0], fir_2to1=tabs[1], level_coef=1.5, zmean=True)),
                             ("batch_16k_strip_zmean", src16, N16, dict(zmean=True))):
        seg = windows(src, NCHAN, n)
        ioff = np.arange(NCHAN + 1, dtype=np.int64) * n
        d_in = lib.DevBuf(eng, seg.nbytes).upload(seg)
        ad = lib.Adin(eng, NCHAN, lib.Adin.desc_for(**kw))
        cap = NCHAN * ad.push_cap(0, n)
        d_mid = lib.DevBuf(eng, 2 * cap)
        d_out = lib.DevBuf(eng, 4 * NCHAN * (FRAMES + 40) * fe.veclen)
        state = {}

        def push():
            ad.reset(stream=sp.value)            # every repetition a fresh stream: the whole chunk goes into the mean
            state["off"] = ad.push_dev(d_in.ptr, ioff, d_mid.ptr, stream=sp.value)

        rec = {"samples_in_per_channel": n, "adin_ms": timed_ms(push, a.reps)}
        off = state["off"]
        rec["samples_out"] = int(off[-1])
        rec["frames_out"] = int(sum(fe.frames(int(k)) for k in np.diff(off)))
        rec["frontend_run_dev_ms"] = timed_ms(lambda: fe.run_dev(d_mid.ptr, off, d_out.ptr, stream=sp.value), a.reps)
        rec["adin_over_frontend"] = round(rec["adin_ms"]["median"] / rec["frontend_run_dev_ms"]["median"], 3)
        out[name] = rec
        ad.close()
        for b in (d_in, d_mid, d_out):
            b.free()

    # ---- one push in a stream
    out["push_25_frames"] = {}
    for nchan in (1, 64, 512):
        npush = 24                               # 288 000 samples: sub_zmean() estimates during the first four pushes
        seg = windows(src48, nchan, npush * PUSH48, seed=3)
        bufs = [lib.DevBuf(eng, 2 * nchan * PUSH48).upload(np.ascontiguousarray(seg[:, j * PUSH48:(j + 1) * PUSH48]))
                for j in range(npush)]
        ioff = np.arange(nchan + 1, dtype=np.int64) * PUSH48
        ad = lib.Adin(eng, nchan, lib.Adin.desc_for(fir_3to4=tabs[0], fir_2to1=tabs[1], level_coef=1.5, zmean=True))
        lv = lib.LiveFrontend(fe, nchan)
        d_mid = lib.DevBuf(eng, 2 * nchan * PUSH48)
        d_out = lib.DevBuf(eng, 4 * nchan * 64 * lv.veclen)
        est, frozen, live = [], [], []
        for rep in range(a.reps + 1):
            ad.reset(stream=sp.value)
            for j in range(npush):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record(st)
                off = ad.push_dev(bufs[j].ptr, ioff, d_mid.ptr, stream=sp.value)
                ev[1].record(st)
                lv.push_dev(d_mid.ptr, off, d_out.ptr, final=np.full(nchan, j == npush - 1), stream=sp.value)
                ev[2].record(st)
                st.synchronize()
                if rep and 0 < j < npush - 1:    # (rep 0 warms up; the first push has nothing to emit, the last ends the segment)
                    (est if j < 4 else frozen).append(1e3 * ev[0].elapsed_time(ev[1]))
                    live.append(1e3 * ev[1].elapsed_time(ev[2]))
        out["push_25_frames"][str(nchan)] = {"adin_us_estimating": stats(est), "adin_us_after_48000": stats(frozen),
                                             "frontend_live_push_dev_us": stats(live)}
        lv.close()
        ad.close()
        for b in bufs + [d_mid, d_out]:
            b.free()
    fe.close()
    line = json.dumps({"adin_timing": out})
    print(line)
    if a.json:
        Path(a.json).write_text(line + "\n")
    lib.load().jamd_stream_destroy(eng.h, sp)


if __name__ == "__main__":
    main()
