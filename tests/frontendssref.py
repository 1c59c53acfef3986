"""The reference's spectral subtraction for the front-end tests, on top of frontendref.RefFrontend: the noise
spectrum of new_SS_calculate() / new_SS_load_from_file() (libsent/src/wav2mfcc/ss.c) and Wav2MFCC() with
ssbuf / ss_alpha / ss_floor installed on its work area as libjulius/src/wav2mfcc.c:144-150 installs them."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from frontendref import MFCCWork, RefFrontend, Value

ci, cf, vp = C.c_int, C.c_float, C.c_void_p
P = C.POINTER
_libc = C.CDLL(None)
_libc.free.argtypes = [vp]
_libc.fopen.restype = vp
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [vp]


class RefFrontendSS(RefFrontend):
    def __init__(self, ref):
        super().__init__(ref)
        lib = self.lib
        lib.new_SS_calculate.argtypes = [vp, ci, P(ci), P(MFCCWork), P(Value)]
        lib.new_SS_calculate.restype = P(cf)
        lib.new_SS_load_from_file.argtypes = [C.c_char_p, P(ci)]
        lib.new_SS_load_from_file.restype = P(cf)
        lib.j_output_argument_help.argtypes = [vp]
        lib.j_output_argument_help.restype = None
        self._ss = None

    def work(self, v):
        """The work area of WMP_work_new(), with the noise spectrum of the running wav2mfcc_ss() call on it
        (WMP_free() leaves ssbuf alone: it belongs to the numpy array)."""
        w = super().work(v)
        if self._ss is not None:
            noise, alpha, floor = self._ss
            w.contents.ssbuf = noise.ctypes.data_as(P(cf))
            w.contents.ssbuflen = len(noise)
            w.contents.ss_alpha = alpha
            w.contents.ss_floor = floor
        return w

    def wav2mfcc_ss(self, wave, v, noise, alpha=2.0, floor=0.5, **kw):
        """Wav2MFCC() + splicing with spectral subtraction by `noise` ([fftN] float32)."""
        self._ss = (np.ascontiguousarray(noise, np.float32), float(alpha), float(floor))
        try:
            return self.wav2mfcc(wave, v, **kw)
        finally:
            self._ss = None

    def noise(self, wave, v, nsamples=None):
        """new_SS_calculate() over the first `nsamples` samples of `wave` -> float32 [fftN].

        Like Wav2MFCC() it copies framesize + 1 samples into bf[1 ..], which WMP_work_new() sizes at fftN floats,
        and so reads one sample past the given length: it is lent a roomy bf and a padded input, exactly as
        RefFrontend.wav2mfcc() does, or windows of fftN - 1 and fftN samples are undefined behaviour."""
        wave = np.ascontiguousarray(wave, np.int16)
        n = len(wave) if nsamples is None else int(nsamples)
        assert v.framesize <= n <= len(wave)
        buf = np.zeros(len(wave) + 8, np.int16)
        buf[:len(wave)] = wave
        w = RefFrontend.work(self, v)
        own = C.cast(w.contents.bf, vp).value
        room = np.zeros(w.contents.fb.fftN + 2, np.float32)
        w.contents.bf = room.ctypes.data_as(P(cf))
        slen = ci(0)
        spec = self.lib.new_SS_calculate(buf.ctypes.data, n, C.byref(slen), w, C.byref(v))
        fftN = w.contents.fb.fftN
        assert slen.value == fftN
        out = np.ctypeslib.as_array(spec, shape=(fftN,)).astype(np.float32, copy=True)
        _libc.free(C.cast(spec, vp))
        w.contents.bf = C.cast(own, P(cf))
        self.lib.WMP_free(w)
        return out

    def load(self, path):
        """new_SS_load_from_file() -> float32 [count], or None where the reference refuses the file."""
        n = ci(-1)
        buf = self.lib.new_SS_load_from_file(str(path).encode(), C.byref(n))
        if not buf:
            return None
        out = np.ctypeslib.as_array(buf, shape=(n.value,)).astype(np.float32, copy=True)
        _libc.free(C.cast(buf, vp))
        return out

    def defaults(self, tmp_path):
        """(-sscalclen, -ssalpha, -ssfloor) of a fresh configuration (default.c:158-162), as the reference's own
        usage text prints them (m_usage.c:203-206)."""
        path = tmp_path / "usage.txt"
        fp = _libc.fopen(str(path).encode(), b"w")
        assert fp
        self.lib.j_output_argument_help(fp)
        _libc.fclose(fp)
        txt = path.read_text(errors="replace")
        get = lambda opt: re.search(r"\[-%s \w+\].*\(([-0-9.]+)\)" % opt, txt).group(1)
        return int(get("sscalclen")), float(get("ssalpha")), float(get("ssfloor"))


def floor_share(spectra, noise, alpha, klo, khi):
    """Share of (frame, FFT index k - 1 in klo - 1 .. khi - 1) pairs with P^2 - alpha * NP^2 < 0: a plain numpy
    restatement over |X| of the frames (`spectra` [T][fftN] complex or magnitude) -- a property of the inputs."""
    Pm = np.abs(np.asarray(spectra))[:, klo - 1:khi].astype(np.float64)
    NP = np.asarray(noise, np.float64)[..., klo - 1:khi]
    return float((Pm * Pm - alpha * NP * NP < 0).mean())


def frame_spectra(wave, framesize=400, frameshift=160, fftN=512, preEmph=0.97):
    """|FFT| of the pre-emphasised, Hamming-windowed frames of `wave` in plain numpy (for floor_share())."""
    wave = np.asarray(wave, np.float64)
    T = (len(wave) - framesize) // frameshift + 1
    idx = np.arange(framesize)[None, :] + frameshift * np.arange(T)[:, None]
    fr = wave[idx]
    pe = np.empty_like(fr)
    pe[:, 1:] = fr[:, 1:] - preEmph * fr[:, :-1]
    pe[:, 0] = fr[:, 0] * (1.0 - preEmph)
    ham = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(framesize) / (framesize - 1))
    return np.abs(np.fft.fft(pe * ham, fftN, axis=1))
