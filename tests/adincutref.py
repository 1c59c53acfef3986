"""The reference's silence cutting (libjulius/src/adin-cut.c:600-984) for the tests.  Every zero-cross count comes out of
the compiled reference in oracle/_ref/libjref.so -- init_count_zc_e() / reset_count_zc_e() / count_zc_e() /
zc_copy_buffer() on one ZEROCROSS structure per channel (the state is in the structure) -- and the head margin is what
zc_copy_buffer() hands back, the swap buffer a real copy of the blocks stored.  Python restates the parameters of
adin_setup_param() (:171-185, np.float32 where the reference computes in float) and the block control flow only.

What a push hands back is what the reference has passed to ad_process() once it has seen the samples so far: the stream
is walked in blocks of chunk_size however it arrives, a remainder waits, and only end of stream makes it a short block.
Per channel the deliveries are cut into parts at segment ends, as jamd_adin_cut_push_*() reports them.

One thing is not the reference's: need_init does not touch rest_tail there (it is set before it is read); here a reset
clears it with everything else, as the product's state does."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

ci, vp = C.c_int, C.c_void_p
P = C.POINTER

EVENTS = ("trigger_head", "trigger_at_start", "tail_delivered", "swapped", "retrigger_swap", "retrigger_empty",
          "end_silence", "end_eos", "eos_idle", "eos_empty_carry", "short_last_block", "short_stream")


class ZeroCross(C.Structure):      # adin.h:116-128
    _fields_ = [("trigger", ci), ("length", ci), ("offset", ci), ("zero_cross", ci), ("is_trig", ci), ("sign", ci),
                ("top", ci), ("valid_len", ci), ("data", P(C.c_int16)), ("is_zc", P(ci)), ("level", ci)]


def _bind(lib):
    if getattr(lib, "_adin_cut_bound", False):
        return
    lib.init_count_zc_e.argtypes = [P(ZeroCross), ci]
    lib.init_count_zc_e.restype = None
    lib.reset_count_zc_e.argtypes = [P(ZeroCross), ci, ci, ci]
    lib.reset_count_zc_e.restype = None
    lib.free_count_zc_e.argtypes = [P(ZeroCross)]
    lib.free_count_zc_e.restype = None
    lib.count_zc_e.argtypes = [P(ZeroCross), vp, ci]
    lib.count_zc_e.restype = ci
    lib.zc_copy_buffer.argtypes = [P(ZeroCross), vp, P(ci)]
    lib.zc_copy_buffer.restype = None
    lib._adin_cut_bound = True


def params(sfreq=16000, level_thres=2000, zero_cross_num=60, head_margin_msec=300, tail_margin_msec=400, chunk_size=1000):
    """(c_length, noise_zerocross, nc_max, sbsize) of adin_setup_param(), C's int and float arithmetic restated."""
    f32 = np.float32
    sim = f32(sfreq) / f32(1000.0)
    c_length = int(f32(head_margin_msec) * sim)
    noise_zerocross = zero_cross_num * c_length // sfreq
    nc_max = int(f32(f32(tail_margin_msec) * sim / f32(chunk_size))) + 2
    sbsize = int(f32(tail_margin_msec) * sim + f32(c_length * zero_cross_num // 200))
    return c_length, noise_zerocross, nc_max, sbsize


def overflows(c_length, nc_max, sbsize, chunk_size):
    """The descriptors with which the reference writes past swapbuf[]."""
    return (nc_max - -(-(sbsize - c_length) // chunk_size)) * chunk_size > sbsize


class Part:
    def __init__(self):
        self.samples, self.final, self.start = [], False, -1

    def data(self):
        return np.concatenate(self.samples) if self.samples else np.zeros(0, np.int16)


class _Chan:
    pass


class RefCut:
    """nchan independent channels of the reference's cutting, one chunk per channel and push."""

    def __init__(self, ref, nchan=1, **desc):
        self.lib = lib = ref.lib
        _bind(lib)
        self.nchan = int(nchan)
        d = dict(sfreq=16000, level_thres=2000, zero_cross_num=60, head_margin_msec=300, tail_margin_msec=400,
                 chunk_size=1000)
        d.update(desc)
        self.desc = d
        self.thres, self.chunk = d["level_thres"], d["chunk_size"]
        self.c_length, self.noise_zerocross, self.nc_max, self.sbsize = params(**d)
        assert 1 <= self.chunk <= self.c_length and not overflows(self.c_length, self.nc_max, self.sbsize, self.chunk)
        self.events = collections.Counter()
        self.ch = []
        for _ in range(self.nchan):
            c = _Chan()
            c.zc = ZeroCross()
            lib.init_count_zc_e(C.byref(c.zc), self.c_length)
            self.ch.append(c)
            self._init(c)

    def close(self):
        for c in self.ch:
            self.lib.free_count_zc_e(C.byref(c.zc))
        self.ch = []

    def _init(self, c):
        """need_init (adin-cut.c:412-431)"""
        self.lib.reset_count_zc_e(C.byref(c.zc), self.thres, self.c_length, 0)
        c.buffer = np.zeros(0, np.int16)
        c.is_valid, c.nc, c.rest_tail, c.sblen = False, 0, 0, 0
        c.swap = []
        c.pos = 0                                    # samples given since the reset
        c.done = 0                                   # samples the blocks have covered

    def reset(self, mask=None):
        for i, c in enumerate(self.ch):
            if mask is None or mask[i]:
                self._init(c)

    def state(self, i):
        c = self.ch[i]
        return (int(c.is_valid), c.nc, c.rest_tail, c.sblen, c.zc.zero_cross, len(c.buffer), c.pos)

    def _block(self, c, blk, parts):
        """One pass of the loop at adin-cut.c:647-984 over buffer[i .. i + wstep)."""
        ev, lib, wstep = self.events, self.lib, len(blk)
        cur = parts[-1]
        c.done += wstep
        zc = lib.count_zc_e(C.byref(c.zc), blk.ctypes.data, wstep)
        if zc > self.noise_zerocross:
            if not c.is_valid:
                c.is_valid, c.nc = True, 0
                cbuf = np.zeros(self.c_length, np.int16)
                n = ci(0)
                lib.zc_copy_buffer(C.byref(c.zc), cbuf.ctypes.data, C.byref(n))
                cur.start = c.done - n.value
                if n.value - wstep > 0:
                    cur.samples.append(cbuf[:n.value - wstep].copy())
                    ev["trigger_head"] += 1
                elif n.value < self.c_length:
                    ev["trigger_at_start"] += 1
            elif c.nc > 0:
                c.nc = 0
                if c.sblen > 0:
                    cur.samples.append(np.concatenate(c.swap))
                    c.swap, c.sblen = [], 0
                    ev["retrigger_swap"] += 1
                else:
                    ev["retrigger_empty"] += 1
        elif c.is_valid:
            if c.nc == 0:
                c.rest_tail = self.sbsize - self.c_length
                c.sblen, c.swap = 0, []
            c.nc += 1
        if c.is_valid and c.nc > 0 and c.rest_tail == 0:
            assert c.sblen + wstep <= self.sbsize
            c.swap.append(blk.copy())
            c.sblen += wstep
            ev["swapped"] += 1
        elif c.is_valid:
            if c.nc > 0:
                c.rest_tail = 0 if c.rest_tail < wstep else c.rest_tail - wstep
                ev["tail_delivered"] += 1
            cur.samples.append(blk.copy())
        if c.is_valid and c.nc >= self.nc_max:
            c.is_valid, c.sblen, c.swap = False, 0, []
            cur.final = True
            parts.append(Part())
            ev["end_silence"] += 1

    def push(self, chunks, eos=None):
        """One int16 array per channel (empty = none) -> per channel the list of its parts (Part: samples, final,
        start), as many as the channel needs."""
        assert len(chunks) == self.nchan
        out = []
        for i, w in enumerate(chunks):
            c = self.ch[i]
            w = np.ascontiguousarray(w, np.int16)
            end = bool(eos is not None and eos[i])
            parts = [Part()]
            c.buffer = np.concatenate([c.buffer, w])
            c.pos += len(w)
            at = 0
            while at + self.chunk <= len(c.buffer):
                self._block(c, np.ascontiguousarray(c.buffer[at:at + self.chunk]), parts)
                at += self.chunk
            c.buffer = c.buffer[at:].copy()
            if end:
                if len(c.buffer):
                    self.events["short_last_block"] += 1
                    if c.pos < self.chunk:
                        self.events["short_stream"] += 1
                    self._block(c, np.ascontiguousarray(c.buffer), parts)
                else:
                    self.events["eos_empty_carry"] += 1
                if c.is_valid:
                    parts[-1].final = True
                    parts.append(Part())
                    self.events["end_eos"] += 1
                else:
                    self.events["eos_idle"] += 1
                self._init(c)
            last = parts[-1]
            if not last.samples and last.start < 0 and not last.final:
                parts.pop()
            out.append(parts)
        return out


BURSTS = (0.5, 0.3, 0.12, 0.4, 0.3, 0.2, 0.35)    # seconds of synthetic speech ...
GAPS = (0.25, 0.08, 1.1, 0.03, 1.3, 0.62, 1.0)     # ... each behind this much N(0, 30) noise


def bursts(seed, scale=1.0, sfreq=16000, tail=0.0):
    """A stream that ends inside its last burst (or `tail` seconds of noise behind it)."""
    from julius_amd import synth
    rng = np.random.default_rng(1000 + seed)
    out = []
    for i, (g, b) in enumerate(zip(GAPS, BURSTS)):
        out.append(np.round(rng.normal(0, 30, int(g * scale * sfreq))).astype(np.int16))
        out.append(synth.make_audio(int(b * scale * sfreq), seed=100 * seed + i, sfreq=sfreq, dc=0.0, zero_runs=0,
                                    silent_frac=0, clip=False))
    if tail > 0:
        out.append(np.round(rng.normal(0, 30, int(tail * scale * sfreq))).astype(np.int16))
    return np.concatenate(out)


def layout(parts, nchan):
    """What jamd_adin_cut_push_*() returns for the per-channel parts of RefCut.push(): (samples, part_off
    [nparts][nchan + 1], part_final [nparts][nchan], part_start [nparts][nchan])."""
    nparts = max(len(p) for p in parts)
    off = np.zeros((nparts, nchan + 1), np.int64)
    fin = np.zeros((nparts, nchan), np.uint8)
    start = np.full((nparts, nchan), -1, np.int64)
    rows, at = [], 0
    for p in range(nparts):
        for c in range(nchan):
            off[p, c] = at
            if p < len(parts[c]):
                d = parts[c][p].data()
                rows.append(d)
                at += len(d)
                fin[p, c] = parts[c][p].final
                start[p, c] = parts[c][p].start
        off[p, nchan] = at
    samples = np.concatenate(rows) if rows else np.zeros(0, np.int16)
    return samples.astype(np.int16), off, fin, start
