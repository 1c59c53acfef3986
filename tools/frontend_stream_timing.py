"""Chunked live input (jamd_frontend_live_push_dev) timed: pushes of 25 frames (4 000 samples at 16 kHz / 10 ms) for
1, 64 and 512 channels, and a 1 420-frame segment of 512 channels fed as 57 pushes beside the same segment in one
jamd_frontend_live_run_dev().

  python tools/frontend_stream_timing.py [--reps 10] [--parent-lib /path/to/libjulius_amd.so] [--json out.json]

MFCC_E_D_A_Z, samples already on the device, channels warm (two committed segments first, so that the MAP branch of the
mean runs).  Every figure lies between two HIP events recorded on the launch stream (through torch.cuda.ExternalStream).
Per channel count:
  push_us            events around one push in the middle of a segment (no channel opens or ends): median / min / max
                     over every such push of --reps segments
  segment_us_per_push  events around the 57 pushes of one segment, over 57: this holds the host's share between pushes
                     (a push waits for the previous call's offset upload before it rewrites the pinned tables)
  host_us_per_push   host clock around the push calls of a segment alone (enqueue), over 57
For 512 channels the segment as pushes, as one run_dev of this library and -- with --parent-lib, the library built from
the parent commit, loaded beside this one -- as one run_dev of the parent alternate in one process.
launches_per_push is what the code enqueues for a push that completes frames (csrc/frontend_live_api.hip); a kernel trace
of this tool counts the same."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

from julius_amd import lib, synth  # noqa: E402

KIND, VS = "MFCC_E_D_A_Z", 39
FRAMES, CHUNK = 1420, 4000
NSAMP = 401 + 160 * (FRAMES - 1)
LAUNCHES = {"kernels": ["lv_pack_kernel", "fe_frame_kernel", "lv_feat_kernel", "lv_keep_kernel", "lv_cmn_kernel"],
            "h2d_copies": ["live tables (coff, soff, rlen, newr)", "frame-kernel offsets and tables"]}


def segments(nchan, seed=0):
    """[nchan][NSAMP] int16: every channel another stretch of the same synthetic speech."""
    rng = np.random.default_rng(seed)
    src = synth.make_audio(16000 * 120, seed=seed + 1)
    reps = -(-NSAMP // len(src))
    return np.stack([np.roll(np.tile(src, reps), -int(rng.integers(0, len(src))))[:NSAMP] for _ in range(nchan)])


class Parent:
    """The live front end of another build of the library, through its C ABI (same ABI version)."""

    def __init__(self, path, nchan):
        self.l = pl = C.CDLL(str(path), mode=os.RTLD_LOCAL | os.RTLD_NOW | os.RTLD_DEEPBIND)
        mine = lib.load()
        for name in ("jamd_engine_create", "jamd_engine_destroy", "jamd_frontend_create", "jamd_frontend_destroy",
                     "jamd_frontend_live_create", "jamd_frontend_live_destroy", "jamd_frontend_live_run_dev",
                     "jamd_frontend_live_commit", "jamd_last_error", "jamd_abi_version"):
            getattr(pl, name).restype = getattr(mine, name).restype
            getattr(pl, name).argtypes = getattr(mine, name).argtypes
        assert pl.jamd_abi_version() == mine.jamd_abi_version()
        self.has_push = hasattr(pl, "jamd_frontend_live_push_dev")
        self.eng, self.fe, self.lv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ok(pl.jamd_engine_create(0, C.byref(self.eng)))
        d = lib.Frontend.desc_for(KIND, VS)
        self.ok(pl.jamd_frontend_create(self.eng, C.byref(d), C.byref(self.fe)))
        ld = lib.FrontendLiveDesc(1, 100.0, None, None)
        self.ok(pl.jamd_frontend_live_create(self.fe, C.byref(ld), nchan, C.byref(self.lv)))
        self.foff = np.zeros(nchan + 1, np.int32)

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"parent library: {rc}: {self.l.jamd_last_error().decode()}")

    def run_commit(self, d_in, off, d_out, stream):
        self.ok(self.l.jamd_frontend_live_run_dev(self.lv, d_in, off.ctypes.data, d_out, self.foff.ctypes.data, stream))
        self.ok(self.l.jamd_frontend_live_commit(self.lv, None, stream))

    def close(self):
        self.l.jamd_frontend_live_destroy(self.lv)
        self.l.jamd_frontend_destroy(self.fe)
        self.l.jamd_engine_destroy(self.eng)


def stats(v):
    return {"median": round(float(np.median(v)), 2), "min": round(float(min(v)), 2), "max": round(float(max(v)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    eng = lib.Engine(0)
    sp = C.c_void_p()
    assert lib.load().jamd_stream_create(eng.h, C.byref(sp)) == 0
    st = torch.cuda.ExternalStream(sp.value)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        return e0, e1

    npush = -(-NSAMP // CHUNK)
    out = {"kind": KIND, "frames_per_segment": FRAMES, "samples_per_push": CHUNK, "pushes_per_segment": npush,
           "reps": a.reps, "timer": "HIP events on the launch stream", "launches_per_push": LAUNCHES, "channels": {}}
    for nchan in (1, 64, 512):
        seg = segments(nchan)
        # one buffer per push, the channels' chunks back to back
        pushes = []
        for j in range(npush):
            part = np.ascontiguousarray(seg[:, j * CHUNK:(j + 1) * CHUNK])
            off = np.arange(nchan + 1, dtype=np.int64) * part.shape[1]
            pushes.append((lib.DevBuf(eng, part.nbytes).upload(part), off))
        fe = lib.Frontend.from_kind(eng, KIND, VS)
        lv = lib.LiveFrontend(fe, nchan)
        d_out = lib.DevBuf(eng, 4 * nchan * (FRAMES + 8) * fe.veclen)
        last = np.ones(nchan, bool)

        def segment_pushes(events=None, host=None):
            rows = 0
            for j, (buf, off) in enumerate(pushes):
                fin = last if j == npush - 1 else None
                ev = events is not None and 0 < j < npush - 1
                t0 = time.perf_counter()
                if ev:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                foff = lv.push_dev(buf.ptr, off, d_out.ptr, final=fin, stream=sp.value)
                if ev:
                    e1.record(st)
                    events.append((e0, e1))
                if host is not None:
                    host.append(time.perf_counter() - t0)
                rows += int(foff[-1])
            lv.commit(stream=sp.value)
            return rows

        for _ in range(2):                       # warm-up; the channels get their initial mean
            rows = segment_pushes()
        st.synchronize()
        assert rows == nchan * FRAMES, (rows, nchan * FRAMES)
        push_us, seg_us, host_us = [], [], []
        for _ in range(a.reps):
            ev, host = [], []
            segment_pushes(events=ev)
            st.synchronize()
            push_us += [1e3 * e0.elapsed_time(e1) for e0, e1 in ev]
            e0, e1 = timed(lambda: segment_pushes(host=host))
            st.synchronize()
            host_us.append(1e6 * sum(host) / npush)
            seg_us.append(1e3 * e0.elapsed_time(e1) / npush)
        rec = {"push_us": stats(push_us), "segment_us_per_push": stats(seg_us), "host_us_per_push": stats(host_us)}
        if nchan == 512:
            samples = np.ascontiguousarray(seg.reshape(-1))
            woff = np.arange(nchan + 1, dtype=np.int64) * NSAMP
            d_in = lib.DevBuf(eng, samples.nbytes).upload(samples)
            steps = {"segment_as_pushes": segment_pushes,
                     "segment_one_run_dev": lambda: (lv.run_dev(d_in.ptr, woff, d_out.ptr, stream=sp.value), lv.commit(stream=sp.value))}
            parent = None
            if a.parent_lib:
                parent = Parent(a.parent_lib, nchan)
                assert not parent.has_push, "--parent-lib is not the parent commit's build: it has the push entry"
                steps["parent_one_run_dev"] = lambda: parent.run_commit(d_in.ptr, woff, d_out.ptr, sp.value)
            for fn in steps.values():            # warm-up of every shape
                fn(); fn()
            st.synchronize()
            ms = {k: [] for k in steps}
            for _ in range(a.reps):
                for k, fn in steps.items():
                    e0, e1 = timed(fn)
                    st.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
            rec["segment_ms"] = {k: stats(v) for k, v in ms.items()}
            if parent is None:
                rec["segment_ms"]["parent_one_run_dev"] = "not measured: no --parent-lib"
            else:
                rec["pushes_over_parent_run"] = round(float(np.median(ms["segment_as_pushes"]) / np.median(ms["parent_one_run_dev"])), 3)
                rec["run_over_parent_run"] = round(float(np.median(ms["segment_one_run_dev"]) / np.median(ms["parent_one_run_dev"])), 3)
                parent.close()
            d_in.free()
        out["channels"][str(nchan)] = rec
        lv.close()
        fe.close()
        d_out.free()
        for buf, _ in pushes:
            buf.free()
    line = json.dumps({"frontend_live_stream_timing": out})
    print(line)
    if a.json:
        Path(a.json).write_text(line + "\n")
    lib.load().jamd_stream_destroy(eng.h, sp)


if __name__ == "__main__":
    main()
