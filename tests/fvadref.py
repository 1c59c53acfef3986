"""The reference's voice-activity detector (libfvad, -fvad) for the tests: the twelve libfvad sources compiled into a
pytest temp directory with a small tap of the project's own that returns a core's state as integers, the restated
fvad_proceed() (libjulius/src/adin-cut.c:264-311), and the streams, the recording and the fixture names shared by
tests/make_golden_fvad.py and the tests; and a second tap that takes the reference's adin-cut.c in with HAVE_LIBFVAD
defined, so that its static fvad_proceed() and adin_cut() can be run (CUT_TAP, below).  Nothing compiled is written into
the tree; where the reference tree or a compiler is missing, build() and build_cut_tap() skip."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
MODEL = GOLDEN / "fvad_model.txt"
REFERENCE = Path(os.environ.get("JULIUS_REF", "/root/reference"))
FVAD_SRC = REFERENCE / "libjulius" / "libfvad" / "libfvad" / "src"
STATE_INTS = 266
MAX_SPEECH_FRAMES = 6
# stream name -> (adincutref.bursts() seed, sample rate)
STREAMS = {"fvad_b2_16k": (2, 16000), "fvad_b3_16k": (3, 16000), "fvad_b2_8k": (2, 8000)}

# VadInstT in the order of jamd_fvad_state_get() (include/julius_amd.h), without the waiting samples
TAP = r"""
#include "vad/vad_core.h"
int jamd_fvad_tap_state(void *fvad, int *out)
{
  const VadInstT *v = (const VadInstT *)fvad;          /* (the core is struct Fvad's first member) */
  int n = 0, i;
  out[n++] = v->downsampling_filter_states[0]; out[n++] = v->downsampling_filter_states[1];
  for (i = 0; i < kTableSize; i++) out[n++] = v->noise_means[i];
  for (i = 0; i < kTableSize; i++) out[n++] = v->speech_means[i];
  for (i = 0; i < kTableSize; i++) out[n++] = v->noise_stds[i];
  for (i = 0; i < kTableSize; i++) out[n++] = v->speech_stds[i];
  out[n++] = v->frame_counter; out[n++] = v->over_hang; out[n++] = v->num_of_speech;
  for (i = 0; i < 16 * kNumChannels; i++) out[n++] = v->index_vector[i];
  for (i = 0; i < 16 * kNumChannels; i++) out[n++] = v->low_value_vector[i];
  for (i = 0; i < kNumChannels; i++) out[n++] = v->mean_value[i];
  for (i = 0; i < 5; i++) out[n++] = v->upper_state[i];
  for (i = 0; i < 5; i++) out[n++] = v->lower_state[i];
  for (i = 0; i < 4; i++) out[n++] = v->hp_filter_state[i];
  return n;
}
int jamd_fvad_tap_raw(void *fvad) { return ((const VadInstT *)fvad)->vad; }
"""

_lib = None


def sources():
    return sorted(list((FVAD_SRC / "vad").glob("*.c")) + list((FVAD_SRC / "signal_processing").glob("*.c"))
                  + [FVAD_SRC / "fvad.c"])


def build(tmp: Path):
    """libfvad + the tap as a shared library under `tmp` (once per process); skips where it cannot be built."""
    global _lib
    if _lib is not None:
        return _lib
    import pytest
    cc = shutil.which("cc") or shutil.which("gcc")
    if not FVAD_SRC.is_dir() or cc is None:
        pytest.skip("no reference tree or no C compiler: libfvad cannot be built")
    tmp.mkdir(parents=True, exist_ok=True)
    (tmp / "tap.c").write_text(TAP)
    so = tmp / "libfvadref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-I", str(FVAD_SRC), "-o", str(so), str(tmp / "tap.c")]
                   + [str(s) for s in sources()], check=True)
    lib = C.CDLL(str(so))
    lib.fvad_new.restype = C.c_void_p
    lib.fvad_free.argtypes = [C.c_void_p]
    lib.fvad_set_mode.argtypes = [C.c_void_p, C.c_int]
    lib.fvad_set_sample_rate.argtypes = [C.c_void_p, C.c_int]
    lib.fvad_process.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.jamd_fvad_tap_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.jamd_fvad_tap_raw.argtypes = [C.c_void_p]
    _lib = lib
    return lib


class RefFvad:
    """One libfvad instance as adin_setup_param() makes it (adin-cut.c:215-233): fvad_new(), rate, mode, no reset after."""

    def __init__(self, lib, sfreq, mode):
        self.lib, self.fs = lib, sfreq // 100
        self.h = lib.fvad_new()
        assert lib.fvad_set_sample_rate(self.h, sfreq) == 0 and lib.fvad_set_mode(self.h, mode) == 0

    def frame(self, x):
        """fvad_process() on one frame -> (its 0 / 1, the core's raw value)."""
        x = np.ascontiguousarray(x, np.int16)
        assert len(x) == self.fs
        r = self.lib.fvad_process(self.h, x.ctypes.data, len(x))
        raw = self.lib.jamd_fvad_tap_raw(self.h)
        assert r == (1 if raw > 0 else 0)
        return r, raw

    def raw(self, samples):
        """The raw value of every whole frame of `samples` (uint8)."""
        n = len(samples) // self.fs
        return np.array([self.frame(samples[f * self.fs:(f + 1) * self.fs])[1] for f in range(n)], np.uint8)

    def state(self):
        out = np.zeros(STATE_INTS, np.int32)
        assert self.lib.jamd_fvad_tap_state(self.h, out.ctypes.data) == STATE_INTS - 1
        return out

    def close(self):
        if self.h:
            self.lib.fvad_free(self.h)
            self.h = None


def gate_frames(e, fs):
    """Frames fvad_proceed() has processed once its blocks end at sample e: max(0, ceil(e / fs) - 1)."""
    return max(0, -(-e // fs) - 1)


def cmin(N, thres):
    """The smallest count c of speech frames among the last N with float(c) / float(N) >= thres, N + 1 if none."""
    for c in range(N + 1):
        if np.float32(c) / np.float32(N) >= np.float32(thres):
            return c
    return N + 1


class Proceed:
    """fvad_proceed() restated: the pending samples, the ring of the last `smoothnum` results, the float comparison.
    `process(frame) -> 0 / 1` is the detector behind it."""

    def __init__(self, process, fs, smoothnum, thres):
        self.process, self.fs, self.n, self.thres = process, fs, int(smoothnum), np.float32(thres)
        self.init()

    def init(self):
        """need_init (adin-cut.c:424-430): the pending samples and the ring go, the detector stays."""
        self.pend = np.zeros(0, np.int16)
        self.ring, self.at = [0] * self.n, 0

    def __call__(self, block):
        buf = np.concatenate([self.pend, np.asarray(block, np.int16)])
        i = 0
        while i + self.fs < len(buf):
            self.ring[self.at] = int(self.process(buf[i:i + self.fs]))
            self.at = (self.at + 1) % self.n
            i += self.fs
        s = np.float32(0)
        for r in self.ring:
            s = np.float32(s + np.float32(r))
        s = np.float32(s / np.float32(self.n))
        self.pend = buf[i:]
        return 1 if s >= self.thres else 0


class Replay:
    """Recorded decisions (the raw values of a stream's frames) in place of the detector: process() hands them out in
    order; finish(n) asserts that exactly n were asked for."""

    def __init__(self, raw):
        self.raw, self.at = np.asarray(raw), 0

    def __call__(self, frame):
        assert self.at < len(self.raw), "asked for more frames than were recorded"
        self.at += 1
        return 1 if self.raw[self.at - 1] > 0 else 0

    def finish(self, n):
        assert self.at == n, (self.at, n)


def ref_cut_fvad(K):
    """RefCut (tests/adincutref.py, module K) with the gate of adin-cut.c:662-668, made without copying the helper."""

    class RefCutFvad(K.RefCut):
        def __init__(self, ref, process, smoothnum, thres, nchan=1, **desc):
            """process: one callable per channel, frame -> 0 / 1."""
            self._mk = lambda i: Proceed(process[i], desc.get("sfreq", 16000) // 100, smoothnum, thres)
            self._n = 0
            self.gates = [[] for _ in range(nchan)]      # per channel: (zero-cross count over the threshold, gate) per block
            super().__init__(ref, nchan, **desc)

        def _init(self, c):
            super()._init(c)
            if not hasattr(c, "proceed"):
                c.index = self._n
                c.proceed = self._mk(self._n)
                self._n += 1
            c.proceed.init()

        def _block(self, c, blk, parts):
            gate = c.proceed(blk)
            keep = self.noise_zerocross
            if not gate:
                self.noise_zerocross = 1 << 30               # out of reach: count_zc_e() still runs, nothing triggers
            try:
                super()._block(c, blk, parts)
            finally:
                self.noise_zerocross = keep
            self.gates[c.index].append((c.zc.zero_cross > keep, gate))

    return RefCutFvad


def rails():
    """1 600 samples at the rails: the detector's wrap-arounds."""
    return np.concatenate([np.full(400, 32767), np.tile([32767, -32768], 400), np.full(400, -32768)]).astype(np.int16)


def make_stream(name):
    """adincutref.bursts() with 1 600 zeros in front (from a fresh core: frames of power 0, which update nothing and
    leave frame_counter behind) and the rails in the middle."""
    import adincutref as K
    seed, sfreq = STREAMS[name]
    s = K.bursts(seed, sfreq=sfreq)
    half = len(s) // 2
    return np.concatenate([np.zeros(1600, np.int16), s[:half], rails(), s[half:]]).astype(np.int16)


TWO_FIRST = 48000                                # the first stream of the two-stream scenarios: a multiple of 160


def record_from(lib, x, sfreq):
    """What a fixture holds beside its stream x, per mode m:
      raw<m>, state<m>    the raw value of every whole frame from a fresh core, and the core behind them
      gstate<m>           the core behind the frames fvad_proceed() has processed at the end of x: one fewer where the
                          length is a multiple of the frame
      twoA<m>, twoB<m>    two streams on one core as adin_cut() runs them: x[:TWO_FIRST] and x[:TWO_FIRST + 1], each to
                          its end (where the last whole frame of the first never reaches the detector, the pending
                          samples go and the core stays), then x: the raw values of both streams' frames
      twoAstate<m>, ...   the core behind them"""
    fs = sfreq // 100
    out = {"samples": x, "sfreq": np.int32(sfreq)}

    def gated(r, w):
        n = gate_frames(len(w), fs)
        return [r.frame(w[f * fs:(f + 1) * fs])[1] for f in range(n)]

    for mode in range(4):
        r = RefFvad(lib, sfreq, mode)
        out[f"raw{mode}"] = r.raw(x)
        out[f"state{mode}"] = r.state()
        out[f"state{mode}"][STATE_INTS - 1] = len(x) % fs                    # what waits for its frame
        r.close()
        r = RefFvad(lib, sfreq, mode)
        gated(r, x)
        out[f"gstate{mode}"] = r.state()
        r.close()
        for tag, first in (("A", TWO_FIRST), ("B", TWO_FIRST + 1)):
            r = RefFvad(lib, sfreq, mode)
            out[f"two{tag}{mode}"] = np.array(gated(r, x[:first]) + gated(r, x), np.uint8)
            out[f"two{tag}state{mode}"] = r.state()
            r.close()
    return out


def record(lib, name):
    return record_from(lib, make_stream(name), STREAMS[name][1])


def load(name):
    z = np.load(GOLDEN / f"{name}.npz")
    return {k: z[k] for k in z.files}


def model_ints(path=MODEL):
    """The integers of a model file, as jamd_fvad_model_read() takes them."""
    return [int(t) for t in Path(path).read_text().splitlines() if t.strip() and not t.lstrip().startswith("#")]


# ---- the reference's own adin-cut.c with HAVE_LIBFVAD, for tests/test_fvad_ref.py

# A translation unit of the project's own that takes adin-cut.c in with HAVE_LIBFVAD defined, so that its static
# fvad_proceed() and adin_cut() can be called on an ADIn of the tap's own.  The compiled reference in oracle/_ref was
# built without that define: its ADIn and Jconf are laid out differently, so neither is ever handed to it; what the
# tap takes from libjref.so (count_zc_e() on &adin->zc, jlog(), mymalloc(), the callbacks of a zeroed Recog, whose
# layout does not depend on the define) does not look at them.
CUT_TAP = r"""
#define HAVE_LIBFVAD 1
#include "adin-cut.c"

typedef struct {
  Recog recog;
  Jconf jconf;
  ADIn adin;
  const SP16 *src; int nsrc, at, read_max;    /* what ad_read() hands out */
  SP16 *out; int nout, cap;                    /* what ad_process() was given */
} Tap;
static Tap *cur;

static int tap_read(SP16 *buf, int max)
{
  int n = cur->nsrc - cur->at;
  if (n <= 0) return -1;                        /* end of stream */
  if (n > max) n = max;
  if (n > cur->read_max) n = cur->read_max;
  memcpy(buf, cur->src + cur->at, sizeof(SP16) * n);
  cur->at += n;
  return n;
}
static int tap_process(SP16 *s, int n, Recog *r)
{
  if (cur->nout + n > cur->cap) return -1;
  memcpy(cur->out + cur->nout, s, sizeof(SP16) * n);
  cur->nout += n;
  return 0;
}

/* an ADIn as adin_setup_param() makes it for -cutsilence -fvad mode -fvad_param smoothnum thres */
void *jamd_cut_tap_new(int sfreq, int lv, int zc, int head, int tail, int chunk, int mode, int smoothnum, float thres)
{
  Tap *t = (Tap *)calloc(1, sizeof(Tap));
  Jconf *j = &t->jconf;
  j->input.sfreq = sfreq;
  j->detect.silence_cut = 1; j->detect.level_thres = lv; j->detect.zero_cross_num = zc;
  j->detect.head_margin_msec = head; j->detect.tail_margin_msec = tail; j->detect.chunk_size = chunk;
  j->detect.fvad_mode = mode; j->detect.fvad_smoothnum = smoothnum; j->detect.fvad_thres = thres;
  j->preprocess.strip_zero_sample = FALSE; j->preprocess.use_zmean = FALSE; j->preprocess.level_coef = 1.0;
  j->reject.rejectlonglen = -1;
  t->recog.adin = &t->adin; t->recog.jconf = j;
  t->adin.ad_read = tap_read;
  if (!adin_setup_param(&t->adin, j)) { free(t); return NULL; }
  return t;
}

/* fvad_proceed() on one block -> its result; *pending: the samples it keeps, *ring_sum: the results it holds */
int jamd_cut_tap_proceed(void *p, const SP16 *blk, int n, int *pending, int *ring_sum)
{
  Tap *t = (Tap *)p;
  int i, r = fvad_proceed(&t->adin, (SP16 *)blk, n);
  *pending = t->adin.fvad_speechlen;
  for (*ring_sum = 0, i = 0; i < t->adin.fvad_lastresultnum; i++) *ring_sum += t->adin.fvad_lastresult[i];
  return r;
}

/* adin_cut() over a whole stream given in reads of at most read_max samples, called again after every segment end:
   the samples it passed on -> out (cap samples of room), the length of each segment -> seg; returns the segments,
   -1 on an error.  need_init is whatever the call before left: TRUE after adin_setup_param() and after a stream's end. */
int jamd_cut_tap_stream(void *p, const SP16 *src, int n, int read_max, SP16 *out, int cap, int *seg, int segcap)
{
  Tap *t = (Tap *)p;
  int rc, nseg = 0, before;
  cur = t;
  t->src = src; t->nsrc = n; t->at = 0; t->read_max = read_max; t->out = out; t->nout = 0; t->cap = cap;
  do {
    before = t->nout;
    rc = adin_cut(tap_process, NULL, &t->recog);
    if (rc < 0) return -1;
    if (t->nout > before || rc == 1) {
      if (nseg >= segcap) return -1;
      seg[nseg++] = t->nout - before;
    }
  } while (rc == 1);
  return nseg;
}

int jamd_cut_tap_need_init(void *p) { return ((Tap *)p)->adin.need_init; }
void *jamd_cut_tap_fvad(void *p) { return ((Tap *)p)->adin.fvad; }
"""

_cut_tap = None


def build_cut_tap(tmp: Path):
    """The tap above + libfvad as a shared library under `tmp`, linked with oracle/_ref/libjref.so for the rest of the
    reference.  Skips where the reference tree, a compiler or the compiled reference is missing; a build or link
    failure is an error."""
    global _cut_tap
    if _cut_tap is not None:
        return _cut_tap
    import pytest
    cc = shutil.which("cc") or shutil.which("gcc")
    ref_dir = ROOT / "oracle" / "_ref"
    if not FVAD_SRC.is_dir() or cc is None or not (ref_dir / "libjref.so").exists():
        pytest.skip("no reference tree, no C compiler or no oracle/_ref/libjref.so: the adin-cut.c tap cannot be built")
    tmp.mkdir(parents=True, exist_ok=True)
    (tmp / "cut_tap.c").write_text(CUT_TAP)
    so = tmp / "libcuttap.so"
    jul, sent = REFERENCE / "libjulius", REFERENCE / "libsent"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-fopenmp", "-w", "-DHAVE_CONFIG_H", "-I", str(ROOT / "oracle" / "refcfg"),
                    "-I", str(sent / "include"), "-I", str(jul / "include"), "-I", str(jul / "src"), "-o", str(so),
                    str(tmp / "cut_tap.c")] + [str(s) for s in sources()]
                   + ["-L", str(ref_dir), "-ljref", f"-Wl,-rpath,{ref_dir}", "-lm", "-lpthread"], check=True)
    lib = C.CDLL(str(so))
    lib.jamd_cut_tap_new.restype = C.c_void_p
    lib.jamd_cut_tap_new.argtypes = [C.c_int] * 8 + [C.c_float]
    lib.jamd_cut_tap_proceed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.jamd_cut_tap_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.jamd_cut_tap_need_init.argtypes = [C.c_void_p]
    lib.jamd_cut_tap_fvad.restype = C.c_void_p
    lib.jamd_cut_tap_fvad.argtypes = [C.c_void_p]
    _cut_tap = lib
    return lib


class CutTap:
    """One ADIn of the reference's adin-cut.c built with HAVE_LIBFVAD."""

    def __init__(self, lib, mode, smoothnum, thres, sfreq=16000, level_thres=2000, zero_cross_num=60, head_margin_msec=300,
                 tail_margin_msec=400, chunk_size=1000):
        self.lib = lib
        self.h = lib.jamd_cut_tap_new(sfreq, level_thres, zero_cross_num, head_margin_msec, tail_margin_msec, chunk_size,
                                      mode, smoothnum, thres)
        assert self.h

    def proceed(self, blk):
        """The static fvad_proceed() on one block -> (gate, samples it keeps, sum of the results it holds)."""
        blk = np.ascontiguousarray(blk, np.int16)
        pend, ring = C.c_int(0), C.c_int(0)
        g = self.lib.jamd_cut_tap_proceed(self.h, blk.ctypes.data, len(blk), C.addressof(pend), C.addressof(ring))
        return g, pend.value, ring.value

    def stream(self, x, read_max=1 << 30):
        """The static adin_cut() over one whole stream -> the list of segments it passed on; ends with need_init set."""
        x = np.ascontiguousarray(x, np.int16)
        out, seg = np.zeros(2 * len(x) + 1000000, np.int16), np.zeros(4096, np.int32)
        n = self.lib.jamd_cut_tap_stream(self.h, x.ctypes.data, len(x), int(read_max), out.ctypes.data, len(out),
                                         seg.ctypes.data, len(seg))
        assert n >= 0
        assert self.lib.jamd_cut_tap_need_init(self.h) == 1
        ends = np.cumsum(seg[:n])
        return [out[e - l:e].copy() for e, l in zip(ends, seg[:n])]

    def raw_state(self):
        """The state of the detector inside (libfvad's core through the tap of build(): same struct)."""
        out = np.zeros(STATE_INTS, np.int32)
        build(Path("unused")).jamd_fvad_tap_state(self.lib.jamd_cut_tap_fvad(self.h), out.ctypes.data)
        return out
