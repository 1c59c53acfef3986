"""The silence cutting stage (jamd_adin_cut_push_dev) timed with and without the -fvad gate.

  python tools/fvad_timing.py [--reps 10] [--json out.json] [--ungated-only] [--model tests/golden/fvad_model.txt]

The cases, the audio and the timer are those of tools/adin_cut_timing.py (16 kHz synthetic speech between noise, every
channel at another offset, default cutting parameters; samples already on the device; HIP events on the launch stream
around the call, which spans the wait for the part tables; warm; median / min / max of --reps):
  push_4000    one push of 4 000 samples per channel for 1 / 64 / 512 channels, in the middle of a stream
  batch        512 channels of 227 441 samples, one push with end of stream
each for an object made by jamd_adin_cut_create() (`ungated`) and one made by jamd_adin_cut_create_fvad() with
-fvad 1 -fvad_param 5 0.5 (`gated`).  --ungated-only takes the first alone and uses nothing this stage added, so the
same file runs on the commit before it: that is how the `parent_run1` and `parent_run2` entries of
profiles/fvad_timing.json were taken."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tools")]

import adin_cut_timing as T  # noqa: E402
from julius_amd import lib  # noqa: E402

PUSH, NCHAN, N16 = T.PUSH, T.NCHAN, 227441


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    ap.add_argument("--ungated-only", action="store_true")
    ap.add_argument("--model", default=str(ROOT / "tests" / "golden" / "fvad_model.txt"))
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

    kinds = {"ungated": lambda n: lib.AdinCut(eng, n)}
    if not a.ungated_only:
        model = lib.FvadModel.read(a.model)
        kinds["gated"] = lambda n: lib.AdinCut(eng, n, fvad=lib.AdinCut.fvad_for(model, 1, 5, 0.5))
    out = {"reps": a.reps, "timer": "HIP events on the launch stream", "device": torch.cuda.get_device_name(0), "runs": 1,
           "gate": None if a.ungated_only else "-fvad 1 -fvad_param 5 0.5", "push_4000": {}, "batch": {}}
    src = T.source(60)

    for nchan in (1, 64, 512):
        npush = 16
        seg = T.windows(src, nchan, npush * PUSH, seed=3)
        bufs = [lib.DevBuf(eng, 2 * nchan * PUSH).upload(np.ascontiguousarray(seg[:, j * PUSH:(j + 1) * PUSH]))
                for j in range(npush)]
        ioff = np.arange(nchan + 1, dtype=np.int64) * PUSH
        row = {}
        for kind, make in kinds.items():
            cut = make(nchan)
            d_cut = lib.DevBuf(eng, 2 * nchan * cut.push_cap(PUSH))
            t_cut, t_host, delivered = [], [], 0
            for rep in range(a.reps + 1):
                cut.reset(stream=sp.value)
                for j in range(npush):
                    (poff, _, _), ms, ms_host = span(lambda: cut.push_dev(bufs[j].ptr, ioff, d_cut.ptr, max_parts=4,
                                                                         stream=sp.value))
                    if rep and j:
                        t_cut.append(1e3 * ms); t_host.append(1e3 * ms_host)
                        delivered += int(poff[-1, -1]) if len(poff) else 0
            row[kind] = {"cut_us": T.stats(t_cut), "cut_host_us": T.stats(t_host),
                         "samples_delivered_per_push": round(delivered / len(t_cut), 1)}
            cut.close()
            d_cut.free()
        out["push_4000"][str(nchan)] = row
        for b in bufs:
            b.free()

    seg = T.windows(src, NCHAN, N16, seed=5)
    ioff = np.arange(NCHAN + 1, dtype=np.int64) * N16
    d_in = lib.DevBuf(eng, seg.nbytes).upload(seg)
    eos = np.ones(NCHAN, bool)
    for kind, make in kinds.items():
        cut = make(NCHAN)
        d_cut = lib.DevBuf(eng, 2 * NCHAN * cut.push_cap(N16))
        maxp = cut.parts_cap(N16)
        t_cut, t_host = [], []
        for rep in range(a.reps + 2):
            (poff, _, _), ms, ms_host = span(lambda: cut.push_dev(d_in.ptr, ioff, d_cut.ptr, eos, max_parts=maxp, stream=sp.value))
            if rep >= 2:
                t_cut.append(ms); t_host.append(ms_host)
        out["batch"][kind] = {"channels": NCHAN, "samples_in_per_channel": N16, "samples_delivered": int(poff[-1, -1]),
                              "parts": len(poff), "cut_ms": T.stats(t_cut), "cut_host_ms": T.stats(t_host)}
        cut.close()
        d_cut.free()
    d_in.free()
    line = json.dumps({"fvad_timing": out})
    print(line)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(line + "\n")
    lib.load().jamd_stream_destroy(eng.h, sp)


if __name__ == "__main__":
    main()
