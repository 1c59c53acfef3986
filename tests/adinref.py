"""The reference's sample stage of adin_cut() (libjulius/src/adin-cut.c:470-545) for the tests: every number comes out
of the compiled reference in oracle/_ref/libjref.so -- ds48to16_new() / ds48to16(), strip_zero(), zmean_reset() /
sub_zmean(), and the coefficient tables lpfcoef_3to4[] / lpfcoef_2to1[] it exports -- and Python restates only the
control flow around them: per chunk (one ad_read()) down-sampling, level, stripping, DC removal, each under adin_cut()'s
own condition (`cnt > 0` before stripping decides whether sub_zmean() is called at all).

Two things are restated, because the reference has no function for them:
  * the level scaling is one expression inside adin_cut() (:514), `(SP16)((float)buffer[i] * level_coef)`: here
    float32 product -> int32 (truncating) -> int16 (wrapping), what gcc makes of it on x86-64;
  * sub_zmean() keeps (zlen, zmean) in two file-static variables, one stream per process.  A channel's state is a
    function of the chunks it has been shown, so for many channels the helper resets and shows a channel's earlier
    chunks again (copies; only while zlen < ZMEANSAMPLES, after which the state no longer moves) whenever another channel
    has used the library in between.  zlen is followed along (an integer count); the float mean stays inside the library.

ds48to16_new() takes its filter history rb[] from malloc() and never clears it: samples before the stream start are
undefined in the reference.  The product defines them as 0.0, and so does this helper: it zeroes rb[] of the three
DS_FILTERs after ds48to16_new()."""
from __future__ import annotations

import ctypes as C

import numpy as np

ci, cd, vp = C.c_int, C.c_double, C.c_void_p
P = C.POINTER
ZMEANSAMPLES = 48000               # libsent/include/sent/adin.h:80
DS, ZMEAN = 1, 2


class DSFilter(C.Structure):       # adin.h:89-101
    _fields_ = [("decrate", ci), ("intrate", ci), ("hdn", cd * 513), ("hdn_len", ci), ("delay", ci), ("x", cd * 256),
                ("y", cd * 512), ("rb", cd * 512), ("indx", ci), ("bp", ci), ("count", ci)]


class DSBuffer(C.Structure):       # adin.h:106-110
    _fields_ = [("fir", P(DSFilter) * 3), ("buf", P(cd) * 4), ("buflen", ci)]


def _bind(lib):
    if getattr(lib, "_adin_bound", False):
        return
    lib.ds48to16_new.argtypes = []
    lib.ds48to16_new.restype = P(DSBuffer)
    lib.ds48to16_free.argtypes = [P(DSBuffer)]
    lib.ds48to16_free.restype = None
    lib.ds48to16.argtypes = [vp, vp, ci, ci, P(DSBuffer)]
    lib.ds48to16.restype = ci
    lib.strip_zero.argtypes = [vp, ci]
    lib.strip_zero.restype = ci
    lib.zmean_reset.argtypes = []
    lib.zmean_reset.restype = None
    lib.sub_zmean.argtypes = [vp, ci]
    lib.sub_zmean.restype = None
    lib._adin_bound = True


def tables(ref):
    """(lpfcoef_3to4 [217], lpfcoef_2to1 [401]) as the compiled reference holds them."""
    lib = ref.lib
    out = []
    for name in ("lpfcoef_3to4", "lpfcoef_2to1"):
        n = ci.in_dll(lib, name + "_num").value
        out.append(np.array((cd * n).in_dll(lib, name), np.float64))
    return tuple(out)


_libc = C.CDLL(None)
_libc.malloc.argtypes = [C.c_size_t]
_libc.malloc.restype = vp
_ROOM = 2048                       # doubles per work buffer of a DS_BUFFER to begin with: a block's outputs and more

_zowner = None                     # (helper, channel) whose DC state the library holds


class RefAdin:
    """nchan independent channels of the reference's sample stage, one chunk per channel and push."""

    def __init__(self, ref, nchan=1, down48=False, level_coef=1.0, strip_zero=True, zmean=False, tabs=None):
        """tabs: other coefficients than the reference's own, (3to4, 2to1), no longer than those: ds48to16_new() copies
        lpfcoef_*[] (writable data of the library) into each filter, so they are swapped in around that call alone."""
        self.lib = lib = ref.lib
        _bind(lib)
        self.tabs = tabs
        self.nchan, self.down48, self.coef = int(nchan), bool(down48), np.float32(level_coef)
        self.strip, self.zmean = bool(strip_zero), bool(zmean)
        self.ds = [self._new_ds() if self.down48 else None for _ in range(self.nchan)]
        self.ds_out = [0] * self.nchan           # 16 kHz samples ds48to16() has returned since the last DS reset
        self.ds_in = [0] * self.nchan
        self.zlen = [0] * self.nchan
        self.shown = [[] for _ in range(self.nchan)]   # the chunks sub_zmean() saw while it was still estimating

    def _new_ds(self):
        saved = []
        for name, t in zip(("lpfcoef_3to4", "lpfcoef_2to1"), self.tabs or ()):
            num = ci.in_dll(self.lib, name + "_num")
            arr = (cd * num.value).in_dll(self.lib, name)
            assert len(t) <= num.value
            saved.append((num, arr, num.value, list(arr)))
            arr[:len(t)] = list(map(float, t))
            num.value = len(t)
        ds = self.lib.ds48to16_new()
        for num, arr, n, vals in saved:
            num.value = n
            arr[:n] = vals
        for s in range(3):
            C.memset(ds.contents.fir[s].contents.rb, 0, C.sizeof(cd) * 512)
        # ds48to16() sizes its work buffers at twice the first call's length and grows them only by a later call's own
        # length, so a short read behind pending samples overflows them ("buffer overflow in down sampling") -- the
        # program always reads alike.  Give them room for one block's outputs up front (malloc()ed: ds48to16() grows
        # them for longer reads, ds48to16_free() frees them).
        ds.contents.buflen = _ROOM
        for n in range(4):
            ds.contents.buf[n] = C.cast(_libc.malloc(C.sizeof(cd) * _ROOM), P(cd))
        return ds

    def close(self):
        for ds in self.ds:
            if ds is not None:
                self.lib.ds48to16_free(ds)
        self.ds = []

    def reset(self, mask=None, what=DS | ZMEAN):
        global _zowner
        for c in range(self.nchan):
            if mask is not None and not mask[c]:
                continue
            if (what & DS) and self.down48:
                self.lib.ds48to16_free(self.ds[c])
                self.ds[c] = self._new_ds()
                self.ds_out[c] = self.ds_in[c] = 0
            if what & ZMEAN:
                self.zlen[c] = 0
                self.shown[c] = []
                if _zowner == (id(self), c):
                    _zowner = None

    def _own_zmean(self, c):
        global _zowner
        if _zowner == (id(self), c):
            return
        self.lib.zmean_reset()
        for a in self.shown[c]:
            b = a.copy()
            self.lib.sub_zmean(b.ctypes.data, len(a))
        _zowner = (id(self), c)

    def ds_state(self, c):
        """Per stage (pending inputs bp, delay still to drop), and the totals in and out."""
        f = [self.ds[c].contents.fir[s].contents for s in range(3)]
        return [(x.bp, x.delay) for x in f], self.ds_in[c], self.ds_out[c]

    def push(self, chunks):
        """One int16 array per channel (empty = idle) -> the conditioned samples per channel."""
        assert len(chunks) == self.nchan
        out = []
        for c, w in enumerate(chunks):
            w = np.ascontiguousarray(w, np.int16)
            cnt = len(w)
            buf = w.copy()
            if self.down48 and cnt:
                buf = np.zeros(cnt + 512, np.int16)      # (a short read can complete a pending block)
                cnt = self.lib.ds48to16(buf.ctypes.data, w.ctypes.data, len(w), len(buf), self.ds[c])
                assert cnt >= 0
                self.ds_in[c] += len(w)
                self.ds_out[c] += cnt
                buf = buf[:cnt].copy()
            if cnt > 0 and self.coef != np.float32(1.0):
                buf = (buf.astype(np.float32) * self.coef).astype(np.int32).astype(np.int16)
            if cnt > 0:
                if self.strip:
                    buf = np.ascontiguousarray(buf)
                    cnt = self.lib.strip_zero(buf.ctypes.data, cnt)
                    buf = buf[:cnt].copy()
                if self.zmean:
                    self._own_zmean(c)
                    if self.zlen[c] < ZMEANSAMPLES:
                        self.shown[c].append(buf.copy())
                        self.zlen[c] += cnt
                    room = np.zeros(cnt + 1, np.int16)       # (a valid address for an empty chunk)
                    room[:cnt] = buf
                    self.lib.sub_zmean(room.ctypes.data, cnt)
                    buf = room[:cnt].copy()
            out.append(buf)
        return out
