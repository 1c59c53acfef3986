"""ctypes view of the reference's front end in oracle/_ref/libjref.so (Value, MFCCWork, CMNWork of
libsent/include/sent/mfcc.h; make_default_para / calc_para_from_header / htk_config_file_parse of
para.c; WMP_work_new of mfcc-core.c; Wav2MFCC of wav2mfcc-buffer.c) for the front-end tests."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

ci, cf, vp = C.c_int, C.c_float, C.c_void_p
P = C.POINTER


class Value(C.Structure):
    _fields_ = [("basetype", C.c_short)] + [(n, ci) for n in ("smp_period", "smp_freq", "framesize", "frameshift")] + [
        ("preEmph", cf)] + [(n, ci) for n in ("lifter", "fbank_num", "delWin", "accWin")] + [
        ("silFloor", cf), ("escale", cf)] + [(n, ci) for n in ("hipass", "lopass", "enormal", "raw_e", "zmeanframe",
                                                             "usepower")] + [
        (n, cf) for n in ("vtln_alpha", "vtln_upper", "vtln_lower")] + [
        (n, ci) for n in ("delta", "acc", "energy", "c0", "absesup", "cmn", "cvn", "mfcc_dim", "baselen", "vecbuflen",
                          "veclen", "loaded")]


class FBankInfo(C.Structure):
    _fields_ = [("fftN", ci), ("n", ci), ("klo", ci), ("khi", ci), ("fres", cf), ("cf", P(cf)), ("loChan", P(C.c_short)),
                ("loWt", P(cf)), ("Re", P(cf)), ("Im", P(cf))]


class MFCCWork(C.Structure):   # MFCC_SINCOS_TABLE layout (oracle/refcfg/sent/config.h)
    _fields_ = [("bf", P(cf)), ("fbank", P(C.c_double)), ("fb", FBankInfo), ("bflen", ci), ("fbank_only", C.c_ubyte),
                ("log_fbank", C.c_ubyte), ("costbl_hamming", P(C.c_double)), ("costbl_hamming_len", ci),
                ("costbl_fft", P(C.c_double)), ("sintbl_fft", P(C.c_double)), ("tbllen", ci),
                ("costbl_makemfcc", P(C.c_double)), ("costbl_makemfcc_len", ci), ("sintbl_wcep", P(C.c_double)),
                ("sintbl_wcep_len", ci), ("sqrt2var", cf), ("ssbuf", P(cf)), ("ssbuflen", ci), ("ss_floor", cf),
                ("ss_alpha", cf)]


class CMEAN(C.Structure):
    _fields_ = [("mfcc_sum", P(cf)), ("mfcc_var", P(cf)), ("framenum", ci)]


class CMNWork(C.Structure):
    _fields_ = [("clist", vp), ("clist_max", ci), ("clist_num", ci), ("cweight", cf), ("cmean_init", P(cf)),
                ("cvar_init", P(cf)), ("mfcc_dim", ci), ("veclen", ci), ("mean", C.c_ubyte), ("var", C.c_ubyte),
                ("cmean_init_set", C.c_ubyte), ("now", CMEAN), ("all", CMEAN), ("loaded_from_file", C.c_ubyte),
                ("do_map", C.c_ubyte), ("static_cvn_only", C.c_ubyte)]


def same(a, b):
    """Bits for numbers, NaN for NaN (the payload differs by architecture)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_diff(a, b):
    bad = np.argwhere(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    if len(bad) == 0:
        return "shape" if a.shape != b.shape else "none"
    t, d = bad[0]
    return f"{len(bad)} values differ, first at frame {t} dim {d}: device {a[t, d]!r} reference {b[t, d]!r}"


# Geometries away from the speech defaults, where the frame kernel's 64-lane loops and the tables change
# path (tests/test_frontend_edges_gpu.py; the ones that change a table also in tests/test_frontend_host.py):
# name -> (kind, vecsize, fields on top of the defaults)
EDGE_GEOMETRY = {
    "fs512": ("MFCC_E_D_A_Z", 39, dict(framesize=512, frameshift=160)),          # window == fftN: no zero padding
    "fs256": ("MFCC_E_D_A_Z", 39, dict(framesize=256, frameshift=100)),
    "fs257": ("MFCC_E_D_A_Z", 39, dict(framesize=257, frameshift=100)),          # fftN / 2 + 1: maximal padding
    "fs2049": ("MFCC_E_D_N_Z", 25, dict(framesize=2049, frameshift=512)),        # two frames per workgroup
    "fs4096": ("MFCC_E_D_N_Z", 25, dict(framesize=4096, frameshift=1024)),       # the limit
    "fs16": ("MFCC_E_D_A_Z", 39, dict(framesize=16, frameshift=8)),              # fftN 16, nv2 8: lanes without work
    "fs16_fb4": ("MFCC_E_D_A", 9, dict(framesize=16, frameshift=8, fbank_num=4)),
    "fs33": ("MFCC_E_D_A_Z", 39, dict(framesize=33, frameshift=16)),             # fftN 64, nv2 32
    "fs64": ("MFCC_E_D_A_Z", 39, dict(framesize=64, frameshift=32)),             # fftN == 64
    "fs128_fb12": ("MFCC_E_D_A_Z", 39, dict(framesize=128, frameshift=64, fbank_num=12)),   # nv2 == 64
    "gap": ("MFCC_E_D_A_Z", 39, dict(framesize=400, frameshift=640)),            # samples between frames unread
    "fbank65": ("FBANK_D_A_Z", 195, dict(fbank_num=65)),                         # second trip of the bin loop
    "fbank80": ("FBANK_D_A", 240, dict(fbank_num=80)),
    "melspec128": ("MELSPEC", 128, dict(fbank_num=128, usepower=1)),
    "mfcc100ch": ("MFCC_E_D_A_Z", 39, dict(fbank_num=100)),                      # DCT over > 64 channels
    "mfcc20": ("MFCC_E_D_A_Z", 63, dict(fbank_num=40)),                          # 20 cepstra
    "mfcc_plain": ("MFCC", 12, {}),
    "mfcc_0_only": ("MFCC_0", 13, {}),
    "mfcc_e_0_n": ("MFCC_E_0_D_N_Z", 27, {}),
    "band_clamps": ("MFCC_E_D_A_Z", 39, dict(lopass=0, hipass=9000)),            # klo < 2 -> 2, khi > nv2 -> nv2
    "narrow_band": ("MFCC_E_D_A_Z", 39, dict(lopass=1000, hipass=2000)),         # channels with one FFT bin or none
    "vtln_lt1": ("MFCC_E_D_A_Z", 39, dict(vtln_alpha=0.9, vtln_lower=300.0, vtln_upper=6000.0)),
    "fbank_power": ("FBANK_D_A_Z", 72, dict(usepower=1, zmeanframe=1)),
    "zmean_rawe": ("MFCC_E_D_A_Z", 39, dict(zmeanframe=1, raw_e=1, enormal=1)),
}
# the ones whose tables differ from what tests/test_frontend_host.py already holds to WMP_work_new()
EDGE_TABLES = ("fs16", "fs16_fb4", "fs33", "fs64", "fs512", "fs4096", "fbank80", "melspec128", "mfcc100ch", "mfcc20",
               "band_clamps", "narrow_band")


# the Value fields make_default_para() and calc_para_from_header() set, by jamd_frontend_desc name
DESC_FIELDS = ("smp_period", "smp_freq", "framesize", "frameshift", "preEmph", "lifter", "fbank_num", "delWin",
               "accWin", "silFloor", "escale", "hipass", "lopass", "enormal", "raw_e", "zmeanframe", "usepower", "cvn",
               "vtln_alpha", "basetype", "delta", "acc", "energy", "c0", "absesup", "cmn", "mfcc_dim", "baselen",
               "vecbuflen", "veclen")


class RefFrontend:
    def __init__(self, ref):
        self.lib = lib = ref.lib
        lib.make_default_para.argtypes = [P(Value)]
        lib.calc_para_from_header.argtypes = [P(Value), C.c_short, C.c_short]
        lib.htk_config_file_parse.argtypes = [C.c_char_p, P(Value)]
        lib.htk_config_file_parse.restype = C.c_ubyte
        lib.WMP_work_new.argtypes = [P(Value)]
        lib.WMP_work_new.restype = P(MFCCWork)
        lib.WMP_free.argtypes = [P(MFCCWork)]
        lib.Wav2MFCC.argtypes = [vp, P(P(cf)), P(Value), ci, P(MFCCWork), vp]
        lib.Wav2MFCC.restype = ci

    def para(self, code, vecsize, htkconf=None, **fields):
        """make_default_para() [+ htk_config_file_parse()] + calc_para_from_header(), then `fields`."""
        v = Value()
        self.lib.make_default_para(C.byref(v))
        if htkconf is not None:
            assert self.lib.htk_config_file_parse(str(htkconf).encode(), C.byref(v))
        self.lib.calc_para_from_header(C.byref(v), code, vecsize)
        for k, x in fields.items():
            setattr(v, k, x)
        return v

    def work(self, v):
        w = self.lib.WMP_work_new(C.byref(v))
        assert w, "WMP_work_new failed"
        return w

    def wav2mfcc(self, wave, v, splice=1, cmean=None, cvar=None, static_cvn_only=False):
        """Wav2MFCC() over one utterance, then libjulius' splicing: [T - splice + 1][veclen * splice]."""
        wave = np.ascontiguousarray(wave, np.int16)
        n = len(wave)
        buf = np.zeros(n + 8, np.int16)        # the reference copies framesize + 1 samples per frame
        buf[:n] = wave
        T = (n - v.framesize) // v.frameshift + 1
        rows = np.zeros((T, max(v.vecbuflen, v.veclen) + 4), np.float32)
        ptrs = (P(cf) * T)(*[r.ctypes.data_as(P(cf)) for r in rows])
        w = self.work(v)
        # Wav2MFCC() copies framesize + 1 samples into bf[1 .. framesize + 1] (wav2mfcc-buffer.c:78-80), but
        # WMP_work_new() sizes bf at fftN floats (mfcc-core.c:665): at framesize >= fftN - 1 the reference writes
        # past its own buffer.  It reads bf[1 .. framesize] only, so lending it a buffer with room changes no
        # value; keep this swap, or the windows that are a power of two are undefined behaviour
        own = C.cast(w.contents.bf, vp).value
        room = np.zeros(w.contents.fb.fftN + 2, np.float32)
        w.contents.bf = room.ctypes.data_as(P(cf))
        cw = None
        keep = []
        if cmean is not None:
            cw = CMNWork()
            cm = np.ascontiguousarray(cmean, np.float32); keep.append(cm)
            cw.cmean_init = cm.ctypes.data_as(P(cf))
            if cvar is not None:
                cv = np.ascontiguousarray(cvar, np.float32); keep.append(cv)
                cw.cvar_init = cv.ctypes.data_as(P(cf))
            cw.cmean_init_set = 1
            cw.static_cvn_only = 1 if static_cvn_only else 0
        t0 = time.perf_counter()
        got = self.lib.Wav2MFCC(buf.ctypes.data, ptrs, C.byref(v), n, w, C.addressof(cw) if cw is not None else None)
        self.last_s = time.perf_counter() - t0      # the reference's own call alone (tools/frontend_timing.py)
        w.contents.bf = C.cast(own, P(cf))
        self.lib.WMP_free(w)
        assert got == T
        feat = rows[:, :v.veclen]
        if splice > 1:
            feat = np.concatenate([feat[i:T - splice + 1 + i] for i in range(splice)], axis=1)
        return np.ascontiguousarray(feat)
