"""The reference's live-input (pipelined) front end for the tests, on top of frontendref.RefFrontend: every number
comes out of the compiled reference in oracle/_ref/libjref.so -- WMP_calc(), energy_max_init / _prepare / _normalize(),
WMP_deltabuf_new / _prepare / _proceed / _flush(), CMN_realtime_new / _prepare / CMN_realtime / _update(),
CMN_load_from_file / CMN_save_to_file() -- and Python restates only the control flow and the memcpy()s around them:
the window loop of RealTimePipeLine() (libjulius/src/realtime-1stpass.c:842-930), RealTimeMFCC() (:496-602), the flush
loop of RealTimeParam() (:1188-1375) and splice_mfcc() (:446-461).  No arithmetic lives here.

One thing in the flush loop is kept apart.  When a flushed delta vector meets an acceleration buffer that is still in
its delay (:1249-1257), or a spliced vector is not complete yet (:1292-1294), the loop `continue`s with mfcc->valid
still TRUE, and the reference advances mfcc->f without having stored a vector: param->samplenum then counts rows that
hold nothing defined.  `rows` here are the vectors the reference does store, in order; `f_ref` is its counter, and it
is what CMN_realtime_update() is shown as samplenum, so that its own consistency check (wav2mfcc-pipe.c:420) decides as
it does in the program.

A second thing the restated memcpy()s bring out: the flush loop takes the last block of an _A vector from
ab->vec[veclen - baselen] (:1252, :1276), which for [base][delta][acc] is index 2 * baselen -- the acceleration
buffer's delta of the BASE coefficients (window accWin) -- where RealTimeMFCC() takes ab->vec[3 * baselen], its delta
of the deltas (:574).  So the frames the flush loop emits (the last delWin + accWin of a segment) carry that in their
third block.  That is what the program stores and decodes, and what this helper returns."""
from __future__ import annotations

import ctypes as C

import numpy as np

from frontendref import CMNWork, MFCCWork, RefFrontend, Value

ci, cf, vp, ub = C.c_int, C.c_float, C.c_void_p, C.c_ubyte
P = C.POINTER


class DeltaBuf(C.Structure):       # libsent/include/sent/mfcc.h:132-141
    _fields_ = [("mfcc", P(P(cf))), ("veclen", ci), ("vec", P(cf)), ("win", ci), ("len", ci), ("store", ci),
                ("is_on", P(ub)), ("B", ci)]


class ENERGYWork(C.Structure):     # mfcc.h:209-213
    _fields_ = [("max_last", cf), ("min_last", cf), ("max", cf)]


class HTKParamHeader(C.Structure):
    _fields_ = [("samplenum", C.c_uint), ("wshift", C.c_uint), ("sampsize", C.c_ushort), ("samptype", C.c_short)]


class HTKParam(C.Structure):       # libsent/include/sent/htk_param.h:76-85
    _fields_ = [("header", HTKParamHeader), ("samplenum", C.c_uint), ("veclen", C.c_short), ("parvec", P(P(cf))),
                ("veclen_alloc", C.c_short), ("samplenum_alloc", C.c_uint), ("mroot", vp), ("is_outprob", ub)]


def _bind(lib):
    if getattr(lib, "_live_bound", False):
        return
    lib.WMP_calc.argtypes = [P(MFCCWork), vp, P(Value)]
    lib.WMP_calc.restype = None
    lib.energy_max_init.argtypes = [P(ENERGYWork)]
    lib.energy_max_prepare.argtypes = [P(ENERGYWork), P(Value)]
    lib.energy_max_normalize.argtypes = [P(ENERGYWork), cf, P(Value)]
    lib.energy_max_normalize.restype = cf
    lib.WMP_deltabuf_new.argtypes = [ci, ci]
    lib.WMP_deltabuf_new.restype = P(DeltaBuf)
    lib.WMP_deltabuf_free.argtypes = [P(DeltaBuf)]
    lib.WMP_deltabuf_prepare.argtypes = [P(DeltaBuf)]
    lib.WMP_deltabuf_proceed.argtypes = [P(DeltaBuf), vp]
    lib.WMP_deltabuf_proceed.restype = ub
    lib.WMP_deltabuf_flush.argtypes = [P(DeltaBuf)]
    lib.WMP_deltabuf_flush.restype = ub
    lib.CMN_realtime_new.argtypes = [P(Value), cf, ub]
    lib.CMN_realtime_new.restype = P(CMNWork)
    lib.CMN_realtime_free.argtypes = [P(CMNWork)]
    lib.CMN_realtime_prepare.argtypes = [P(CMNWork)]
    lib.CMN_realtime.argtypes = [P(CMNWork), vp]
    lib.CMN_realtime.restype = None
    lib.CMN_realtime_update.argtypes = [P(CMNWork), P(HTKParam)]
    lib.CMN_realtime_update.restype = None
    lib.CMN_load_from_file.argtypes = [P(CMNWork), C.c_char_p]
    lib.CMN_load_from_file.restype = ub
    lib.CMN_save_to_file.argtypes = [P(CMNWork), C.c_char_p]
    lib.CMN_save_to_file.restype = ub
    lib._live_bound = True


def _vec(ptr, n):
    """A copy of n floats at a reference pointer (memcpy)."""
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(np.float32, copy=True)


class RefLiveChannel:
    """One MFCCCalc of the reference fed whole segments: RealTimeInit()'s work areas, then per segment reset_mfcc() +
    CMN_realtime_prepare(), the window loop, the flush loop; commit() is RealTimeCMNUpdate()'s CMN_realtime_update()."""

    def __init__(self, ref, v: Value, splice=1, map_cmn=True, map_weight=100.0, cmean=None, cvar=None, ss=None):
        self.lib = lib = ref.lib
        _bind(lib)
        self.fe = RefFrontend(ref)
        self.v, self.splice = v, int(splice)
        self.w = self.fe.work(v)
        # WMP_work_new() sizes bf at fftN floats; RealTimeMFCC() writes bf[1 .. framesize + 1] (:508-510): lend it a
        # buffer with room, exactly as RefFrontend.wav2mfcc() does (WMP_calc() reads bf[1 .. framesize] only)
        self._own_bf = C.cast(self.w.contents.bf, vp).value
        self._room = np.zeros(self.w.contents.fb.fftN + 2, np.float32)
        self.w.contents.bf = self._room.ctypes.data_as(P(cf))
        if ss is not None:                       # RealTimeInit() :246-249
            noise, alpha, floor = ss
            self._noise = np.ascontiguousarray(noise, np.float32)
            self.w.contents.ssbuf = self._noise.ctypes.data_as(P(cf))
            self.w.contents.ssbuflen = len(self._noise)
            self.w.contents.ss_alpha = alpha
            self.w.contents.ss_floor = floor
        self.ewrk = ENERGYWork()
        if v.energy and v.enormal:
            lib.energy_max_init(C.byref(self.ewrk))
        self.db = lib.WMP_deltabuf_new(v.baselen, v.delWin) if v.delta else None
        self.ab = lib.WMP_deltabuf_new(v.baselen * 2, v.accWin) if v.acc else None
        self.cmn = None
        if v.cmn or v.cvn:
            self.cmn = lib.CMN_realtime_new(C.byref(v), map_weight, 1 if map_cmn else 0)
            if cmean is not None:
                self.load(cmean, cvar)
        self.tmp = np.zeros(max(v.vecbuflen, v.veclen) + 4, np.float32)
        self.spliced = np.zeros(v.veclen * self.splice, np.float32)
        self.rows = np.zeros((0, v.veclen * self.splice), np.float32)
        self.f_ref = 0

    def load(self, cmean, cvar=None):
        """The state CMN_load_from_file() leaves (:628-648), without the file."""
        c = self.cmn.contents
        cm = np.ascontiguousarray(cmean, np.float32)
        C.memmove(c.cmean_init, cm.ctypes.data, 4 * self.v.veclen)
        if c.var and cvar is not None:
            cv = np.ascontiguousarray(cvar, np.float32)
            C.memmove(c.cvar_init, cv.ctypes.data, 4 * self.v.veclen)
        c.cmean_init_set = 1
        c.loaded_from_file = 1

    def close(self):
        if self.w is not None:
            self.w.contents.bf = C.cast(self._own_bf, P(cf))
            self.w.contents.ssbuf = None
            self.lib.WMP_free(self.w)
            self.w = None

    # ---- control flow of the reference
    def _tmp_p(self):
        return self.tmp.ctypes.data

    def _splice(self):                           # splice_mfcc()
        V = self.v.veclen
        if self.splicedlen >= self.splice:
            self.spliced[:V * (self.splice - 1)] = self.spliced[V:V * self.splice].copy()
            self.splicedlen -= 1
        self.spliced[V * self.splicedlen:V * (self.splicedlen + 1)] = self.tmp[:V]
        self.splicedlen += 1
        return self.splicedlen >= self.splice

    def _realtime_mfcc(self, window, calc):      # RealTimeMFCC()
        v, lib, tmp = self.v, self.lib, self.tmp
        bl = v.baselen
        if calc:
            self._room[1:1 + len(window)] = window
            lib.WMP_calc(self.w, self._tmp_p(), C.byref(v))
        if v.energy and v.enormal:
            tmp[bl - 1] = lib.energy_max_normalize(C.byref(self.ewrk), cf(tmp[bl - 1]), C.byref(v))
        if v.delta:
            if not lib.WMP_deltabuf_proceed(self.db, self._tmp_p()):
                return False
            tmp[:bl * 2] = _vec(self.db.contents.vec, bl * 2)
        if v.acc:
            if not lib.WMP_deltabuf_proceed(self.ab, self._tmp_p()):
                return False
            vec = _vec(self.ab.contents.vec, bl * 4)
            tmp[:bl * 2] = vec[:bl * 2]
            tmp[bl * 2:bl * 3] = vec[bl * 3:bl * 4]
        if v.delta and (v.energy or v.c0) and v.absesup:
            tmp[bl - 1:v.vecbuflen - 1] = tmp[bl:v.vecbuflen].copy()
        if v.cmn or v.cvn:
            lib.CMN_realtime(self.cmn, self._tmp_p())
        if self.splice > 1:
            return self._splice()
        return True

    def _store(self, rows):
        rows.append((self.spliced if self.splice > 1 else self.tmp[:self.v.veclen]).copy())

    def segment(self, wave, calc=True):
        """One whole segment -> the rows the reference stores ([T][veclen * splice]).  calc=False skips WMP_calc() (the
        buffers then carry zeros): for frame counts alone."""
        v, lib = self.v, self.lib
        wave = np.ascontiguousarray(wave, np.int16)
        # reset_mfcc() (:336-341) and CMN_realtime_prepare()
        if v.energy and v.enormal:
            lib.energy_max_prepare(C.byref(self.ewrk), C.byref(v))
        if v.delta:
            lib.WMP_deltabuf_prepare(self.db)
        if v.acc:
            lib.WMP_deltabuf_prepare(self.ab)
        self.splicedlen = 0
        if self.cmn is not None:
            lib.CMN_realtime_prepare(self.cmn)
        rows, f = [], 0
        # RealTimePipeLine(): fill the window of framesize + 1 samples, compute, shift by frameshift
        windowlen, now, n = v.framesize + 1, 0, len(wave)
        window = np.zeros(windowlen, np.float32)
        windownum = 0
        while now < n:
            i = min(windowlen - windownum, n - now)
            window[windownum:windownum + i] = wave[now:now + i]
            windownum += i
            now += i
            if windownum < windowlen:
                break
            if self._realtime_mfcc(window, calc):
                self._store(rows)
                f += 1
            window[:windowlen - v.frameshift] = window[v.frameshift:].copy()
            windownum -= v.frameshift
        # RealTimeParam(): the flush loop
        bl = v.baselen
        valid = bool(v.delta or v.acc)
        while valid:
            got = False
            if lib.WMP_deltabuf_flush(self.db):
                vec = _vec(self.db.contents.vec, bl * 2)
                if v.energy and v.absesup:
                    self.tmp[:bl - 1] = vec[:bl - 1]
                    self.tmp[bl - 1:2 * bl - 1] = vec[bl:2 * bl]
                else:
                    self.tmp[:bl * 2] = vec
                got = True
                if v.acc:
                    got = bool(lib.WMP_deltabuf_proceed(self.ab, self._tmp_p()))
                    if got:
                        a = _vec(self.ab.contents.vec, bl * 4)
                        k = v.veclen - bl
                        self.tmp[:k] = a[:k]
                        self.tmp[k:k + bl] = a[k:k + bl]      # (:1252 reads ab->vec[veclen - baselen], not [3 * baselen])
            else:
                if v.acc and lib.WMP_deltabuf_flush(self.ab):
                    a = _vec(self.ab.contents.vec, bl * 4)
                    k = v.veclen - bl
                    self.tmp[:k] = a[:k]
                    self.tmp[k:k + bl] = a[k:k + bl]          # (:1276, the same)
                    got = True
                else:
                    valid = False
            if got:
                if self.cmn is not None:
                    lib.CMN_realtime(self.cmn, self._tmp_p())
                if self.splice == 1 or self._splice():
                    self._store(rows)
            if valid:
                f += 1                           # (:1371-1374, also after a `continue` that stored nothing)
        self.f_ref = f
        self.rows = np.array(rows, np.float32).reshape(len(rows), v.veclen * self.splice)
        return self.rows

    def commit(self):
        """CMN_realtime_update(wrk, param) over the rows of the last segment."""
        if self.cmn is None:
            return
        T = len(self.rows)
        prm = HTKParam()
        prm.samplenum = prm.header.samplenum = self.f_ref
        prm.veclen = self.v.veclen * self.splice
        ptrs = (P(cf) * max(T, 1))(*[r.ctypes.data_as(P(cf)) for r in self.rows])
        prm.parvec = C.cast(ptrs, P(P(cf)))
        # (the rows are read only when samplenum == now.framenum and veclen matches: then f_ref == T)
        assert not (self.f_ref == self.cmn.contents.now.framenum and self.splice == 1) or self.f_ref == T
        self.lib.CMN_realtime_update(self.cmn, C.byref(prm))

    def state(self):
        """(cmean_init, cvar_init or zeros, ENERGYWork.max, cmean_init_set)."""
        V = self.v.veclen
        if self.cmn is None:
            return np.zeros(V, np.float32), np.zeros(V, np.float32), np.float32(self.ewrk.max), 0
        c = self.cmn.contents
        cm = _vec(c.cmean_init, V)
        cv = _vec(c.cvar_init, V) if c.var else np.zeros(V, np.float32)
        return cm, cv, np.float32(self.ewrk.max), int(c.cmean_init_set)

    def history(self):
        """(clist_num, clist_max) of the CMN work area."""
        c = self.cmn.contents
        return int(c.clist_num), int(c.clist_max)


def live_frames(ref, v: Value, splice, nsamples):
    """Rows a first segment of nsamples samples yields: the helper's own loops over the reference's buffers, without
    WMP_calc().  The window loop is walked for every n; what follows depends on the number of windows only."""
    windowlen, windownum, now, nwin = v.framesize + 1, 0, 0, 0
    while now < nsamples:                        # RealTimePipeLine() :842-930, counting
        i = min(windowlen - windownum, nsamples - now)
        windownum += i
        now += i
        if windownum < windowlen:
            break
        nwin += 1
        windownum -= v.frameshift
    key = (v.framesize, v.frameshift, v.delta, v.acc, v.delWin, v.accWin, v.absesup, v.energy, v.c0, v.baselen,
           v.veclen, v.vecbuflen, int(splice), nwin)
    return _rows_of_windows(ref, key, v, splice, nwin)


_ROWS = {}


def _rows_of_windows(ref, key, v, splice, nwin):
    if key not in _ROWS:
        vv = Value.from_buffer_copy(v)
        vv.cmn = vv.cvn = vv.enormal = 0
        ch = RefLiveChannel(ref, vv, splice=splice)
        n = 0 if nwin == 0 else v.framesize + 1 + (nwin - 1) * v.frameshift
        _ROWS[key] = len(ch.segment(np.zeros(n, np.int16), calc=False))
        ch.close()
    return _ROWS[key]
