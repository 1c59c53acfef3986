"""ctypes binding of the C ABI in include/julius_amd.h (libjulius_amd.so), in the header's order.

This module is plumbing for tests and bench.py; the product is the shared
library.  There is NO fallback: if the HIP library is missing, or no gfx950
device is present when an engine is created, it raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libjulius_amd.so"
if os.environ.get("JAMD_LIB"):          # development: a library variant built by tools/build_variant.sh
    LIB_PATH = Path(os.environ["JAMD_LIB"]).resolve()

# ---- constants and structs of include/julius_amd.h ------------------------------------------------------------------

LOG_ZERO = -1000000.0
GPRUNE_NONE, GPRUNE_SAFE, GPRUNE_HEU, GPRUNE_BEAM = 0, 1, 2, 3
IWCD_MAX, IWCD_AVG, IWCD_NBEST = 0, 1, 2
SS_OFF, SS_CALC, SS_LOAD = 0, 1, 2
LIVE_CMEAN_SET, LIVE_LOADED = 1, 2
ADIN_DS, ADIN_ZMEAN = 1, 2
FVAD_MODEL_INTS, FVAD_STATE_INTS = 130, 266


class JamdError(RuntimeError):
    pass


class GmmDesc(C.Structure):
    _fields_ = [
        ("nstate", C.c_int), ("veclen", C.c_int), ("ndens", C.c_int),
        ("nentry", C.c_int), ("nbook", C.c_int), ("nstream", C.c_int),
        ("mean", C.c_void_p), ("ivar", C.c_void_p), ("gconst", C.c_void_p),
        ("st_off", C.c_void_p), ("ent_dens", C.c_void_p), ("ent_logw", C.c_void_p),
        ("st_book", C.c_void_p),
    ]


class GmmStreamsDesc(C.Structure):
    """jamd_gmm_ms_desc (include/julius_amd.h): a multi-stream model's pdf pool, states and densities."""
    _fields_ = [(n, C.c_int) for n in ("nstate", "veclen", "nstream", "npdf", "nentry", "ndens")] + [
        (n, C.c_void_p) for n in ("vsize", "pdf_stream", "pdf_off", "pdf_book", "ent_dens", "ent_logw", "st_pdf",
                                  "st_weight", "dens_off", "mean", "ivar", "gconst")]


class DnnDesc(C.Structure):
    _fields_ = [
        ("nlayer", C.c_int), ("dims", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p),
        ("state_prior", C.c_void_p),
    ]


class Pass1Result(C.Structure):
    """jamd_pass1_result (include/julius_amd.h)."""
    _fields_ = [("status", C.c_int), ("natom", C.c_int), ("wnum", C.c_int), ("score", C.c_float),
                ("died_at", C.c_int), ("ties", C.c_int), ("frames", C.c_int), ("max_tokens", C.c_int),
                ("ties_node", C.c_int), ("ties_wordend", C.c_int), ("ties_cut", C.c_int),
                ("phase_us", C.c_int * 8),
                ("wseq", C.c_int * 150)]


class FrontendDesc(C.Structure):
    """jamd_frontend_desc (include/julius_amd.h): the reference's Value plus static CMN / splice."""
    _fields_ = [(n, C.c_int) for n in ("paramtype", "vecsize", "smp_period", "smp_freq", "framesize", "frameshift")] + [
        ("preEmph", C.c_float)] + [(n, C.c_int) for n in ("lifter", "fbank_num", "delWin", "accWin")] + [
        ("silFloor", C.c_float), ("escale", C.c_float)] + [
        (n, C.c_int) for n in ("hipass", "lopass", "enormal", "raw_e", "zmeanframe", "usepower", "cvn")] + [
        (n, C.c_float) for n in ("vtln_alpha", "vtln_upper", "vtln_lower")] + [
        (n, C.c_int) for n in ("basetype", "delta", "acc", "energy", "c0", "absesup", "cmn", "mfcc_dim", "baselen",
                               "vecbuflen", "veclen")] + [
        ("cmean_init", C.c_void_p), ("cvar_init", C.c_void_p), ("static_cvn_only", C.c_int), ("splice", C.c_int),
        ("ss", C.c_int), ("realtime", C.c_int)]


class FrontendSS(C.Structure):
    """jamd_frontend_ss (include/julius_amd.h): -sscalc / -sscalclen / -ssload / -ssalpha / -ssfloor."""
    _fields_ = [("mode", C.c_int), ("calc_len_ms", C.c_int), ("alpha", C.c_float), ("floor", C.c_float),
                ("noise", C.c_void_p), ("noise_len", C.c_int)]


class FrontendLiveDesc(C.Structure):
    """jamd_frontend_live_desc (include/julius_amd.h): -cmnstatic / -cmnmapweight / -cmnload of the live front end."""
    _fields_ = [("map_cmn", C.c_int), ("map_weight", C.c_float), ("cmean_init", C.c_void_p), ("cvar_init", C.c_void_p)]


class AdinDesc(C.Structure):
    """jamd_adin_desc (include/julius_amd.h): -48 with the caller's two FIR tables, -lvscale, -nostrip, -zmean."""
    _fields_ = [("down48", C.c_int), ("fir_3to4", C.c_void_p), ("n_3to4", C.c_int), ("fir_2to1", C.c_void_p),
                ("n_2to1", C.c_int), ("level_coef", C.c_float), ("strip_zero", C.c_int), ("zmean", C.c_int)]


class AdinCutDesc(C.Structure):
    """jamd_adin_cut_desc (include/julius_amd.h): -lv / -zc / -headmargin / -tailmargin / -chunksize of -cutsilence."""
    _fields_ = [("sfreq", C.c_int), ("level_thres", C.c_int), ("zero_cross_num", C.c_int), ("head_margin_msec", C.c_int),
                ("tail_margin_msec", C.c_int), ("chunk_size", C.c_int)]


class FvadModel(C.Structure):
    """jamd_fvad_model (include/julius_amd.h): libfvad's array constants, handed in by the caller."""
    _fields_ = [(n, C.c_int * k) for n, k in (
        ("allpass_q15", 2), ("allpass_q13", 2), ("hp_zero", 3), ("hp_pole", 3), ("offset", 6), ("spectrum_weight", 6),
        ("min_diff", 6), ("max_speech", 6), ("max_noise", 6), ("min_mean", 2), ("noise_weight", 12), ("speech_weight", 12),
        ("noise_mean", 12), ("speech_mean", 12), ("noise_std", 12), ("speech_std", 12), ("over_hang_1", 4),
        ("over_hang_2", 4), ("local_thres", 4), ("global_thres", 4))]

    @classmethod
    def read(cls, path) -> "FvadModel":
        """The model file that julius_amd/shim/jamd_fvad_export writes (jamd_fvad_model_read())."""
        m = cls()
        _call("jamd_fvad_model_read", str(path).encode(), C.byref(m))
        return m

    @classmethod
    def from_ints(cls, ints) -> "FvadModel":
        ints = [int(v) for v in ints]
        assert len(ints) == FVAD_MODEL_INTS
        return cls.from_buffer_copy((C.c_int * FVAD_MODEL_INTS)(*ints))

    def ints(self):
        return list((C.c_int * FVAD_MODEL_INTS).from_buffer_copy(self))


class FvadDesc(C.Structure):
    """jamd_fvad_desc (include/julius_amd.h): the rate, -fvad's mode and the model."""
    _fields_ = [("sfreq", C.c_int), ("mode", C.c_int), ("model", C.POINTER(FvadModel))]


class AdinCutFvad(C.Structure):
    """jamd_adin_cut_fvad (include/julius_amd.h): -fvad's detector and the two arguments of -fvad_param."""
    _fields_ = [("det", FvadDesc), ("smoothnum", C.c_int), ("thres", C.c_float)]


# ---- the kit: signatures, calls, handles, argument conversions ------------------------------------------------------

def _signatures():
    vp, ci, cf, i64, cs = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_char_p
    P = C.POINTER
    return {
        # engine
        "jamd_abi_version": (ci, []),
        "jamd_last_error": (cs, []),
        "jamd_device_count": (ci, []),
        "jamd_engine_create": (ci, [ci, P(vp)]),
        "jamd_engine_destroy": (None, [vp]),
        "jamd_engine_device": (ci, [vp]),
        "jamd_engine_sync": (ci, [vp]),
        "jamd_malloc": (ci, [vp, C.c_size_t, P(vp)]),
        "jamd_free": (ci, [vp, vp]),
        "jamd_host_alloc": (ci, [vp, C.c_size_t, P(vp)]),
        "jamd_host_free": (ci, [vp, vp]),
        "jamd_memcpy_h2d": (ci, [vp, vp, vp, C.c_size_t]),
        "jamd_memcpy_d2h": (ci, [vp, vp, vp, C.c_size_t]),
        "jamd_stream_create": (ci, [vp, vp]),
        "jamd_stream_destroy": (ci, [vp, vp]),
        "jamd_stream_wait": (ci, [vp, vp, vp]),
        "jamd_stream_sync": (ci, [vp, vp]),
        "jamd_memcpy_h2d_async": (ci, [vp, vp, vp, C.c_size_t, vp]),
        # GMM model
        "jamd_gmm_create": (ci, [vp, P(GmmDesc), ci, ci, P(vp)]),
        "jamd_gmm_load": (ci, [vp, cs, ci, ci, P(vp)]),
        "jamd_gmm_destroy": (None, [vp]),
        "jamd_gmm_nstate": (ci, [vp]),
        "jamd_gmm_veclen": (ci, [vp]),
        "jamd_gmm_outprob_dev": (ci, [vp, vp, ci, vp, vp]),
        "jamd_gmm_outprob_utts_dev": (ci, [vp, vp, vp, ci, vp, vp]),
        "jamd_gmm_outprob_host": (ci, [vp, vp, ci, vp]),
        "jamd_gmm_tmix_cache_dev": (ci, [vp, vp, ci, vp, vp, vp, vp]),
        "jamd_gmm_tmix_cap": (ci, [vp]),
        "jamd_gmm_nbook": (ci, [vp]),
        "jamd_gmm_last_kernel": (cs, [vp]),
        "jamd_gmm_nentry": (ci, [vp]),
        "jamd_gmm_book_offsets": (ci, [vp, vp, ci]),
        "jamd_gmm_dens_dev": (ci, [vp, vp, ci, vp, vp]),
        "jamd_gmm_dens_host": (ci, [vp, vp, ci, vp]),
        # multi-stream GMM model
        "jamd_gmm_ms_create": (ci, [vp, P(GmmStreamsDesc), P(vp)]),
        "jamd_gmm_ms_load_binhmm": (ci, [vp, cs, P(vp)]),
        "jamd_gmm_ms_destroy": (None, [vp]),
        "jamd_gmm_ms_nstate": (ci, [vp]),
        "jamd_gmm_ms_veclen": (ci, [vp]),
        "jamd_gmm_ms_nstream": (ci, [vp]),
        "jamd_gmm_ms_outprob_dev": (ci, [vp, vp, ci, vp, vp]),
        "jamd_gmm_ms_outprob_host": (ci, [vp, vp, ci, vp]),
        "jamd_gmm_ms_last_kernel": (cs, [vp]),
        "jamd_gmm_ms_create_opt": (ci, [vp, P(GmmStreamsDesc), vp, P(vp)]),
        "jamd_gmm_ms_load_binhmm_opt": (ci, [vp, cs, vp, P(vp)]),
        "jamd_gmm_ms_outprob_utts_dev": (ci, [vp, vp, vp, ci, vp, vp]),
        "jamd_gmm_ms_outprob_utts_host": (ci, [vp, vp, vp, ci, vp]),
        "jamd_gmm_ms_tmix_cap": (ci, [vp]),
        "jamd_gmm_ms_nbook": (ci, [vp]),
        "jamd_gmm_ms_tmix_cache_dev": (ci, [vp, vp, ci, vp, vp, vp, vp]),
        # Gaussian mixture selection
        "jamd_gms_create": (ci, [vp, P(GmmDesc), vp, ci, ci, P(vp)]),
        "jamd_gms_load": (ci, [vp, cs, P(vp)]),
        "jamd_gms_set_strict_order": (ci, [vp, ci]),
        "jamd_gms_nstate": (ci, [vp]),
        "jamd_gms_destroy": (None, [vp]),
        "jamd_gms_apply_dev": (ci, [vp, vp, ci, vp, ci, vp, vp]),
        "jamd_gms_apply_host": (ci, [vp, vp, ci, vp, ci, vp]),
        # GMM-based input verification
        "jamd_rejgmm_create": (ci, [vp, P(GmmDesc), vp, ci, ci, P(vp)]),
        "jamd_rejgmm_destroy": (None, [vp]),
        "jamd_rejgmm_load": (ci, [vp, cs, P(vp)]),
        "jamd_rejgmm_set_models": (ci, [vp, P(cs), vp]),
        "jamd_rejgmm_model_name": (cs, [vp, ci]),
        "jamd_rejgmm_verdict": (ci, [vp, vp, P(ci), P(cf), P(ci)]),
        "jamd_rejgmm_nmodel": (ci, [vp]),
        "jamd_rejgmm_veclen": (ci, [vp]),
        "jamd_rejgmm_frame_scores_dev": (ci, [vp, vp, ci, vp, vp]),
        "jamd_rejgmm_utt_scores_dev": (ci, [vp, vp, ci, vp, ci, vp, vp]),
        "jamd_rejgmm_scores_host": (ci, [vp, vp, ci, vp, ci, vp, vp]),
        # pseudo-phone state sets
        "jamd_cdset_create": (ci, [vp, ci, vp, vp, ci, ci, P(vp)]),
        "jamd_cdset_destroy": (None, [vp]),
        "jamd_cdset_nset": (ci, [vp]),
        "jamd_cdset_outprob_dev": (ci, [vp, vp, ci, ci, vp, vp]),
        # DNN
        "jamd_dnn_create": (ci, [vp, P(DnnDesc), P(vp)]),
        "jamd_dnn_load": (ci, [vp, cs, P(vp)]),
        "jamd_dnn_destroy": (None, [vp]),
        "jamd_dnn_nstate": (ci, [vp]),
        "jamd_dnn_veclen": (ci, [vp]),
        "jamd_dnn_outprob_dev": (ci, [vp, vp, ci, vp, vp]),
        "jamd_dnn_outprob_host": (ci, [vp, vp, ci, vp]),
        # first pass: lexicon and the files the library reads itself
        "jamd_lexicon_create": (ci, [vp, vp, P(vp)]),
        "jamd_gmm_load_binhmm": (ci, [vp, cs, ci, ci, P(vp)]),
        "jamd_binhmm_to_blob": (ci, [cs, cs]),
        "jamd_lexicon_load": (ci, [vp, cs, P(vp)]),
        "jamd_lexicon_load_ngram": (ci, [vp, cs, cs, P(vp)]),
        "jamd_bingram_check": (ci, [cs, cs, P(ci)]),
        "jamd_bingram_fscore": (ci, [cs, cs, vp, ci, P(ci)]),
        "jamd_lexicon_lm_table": (ci, [vp]),
        "jamd_lexicon_destroy": (None, [vp]),
        # first pass: work area
        "jamd_beam_create": (ci, [vp, vp, ci, cf, ci, ci, P(vp)]),
        "jamd_beam_destroy": (None, [vp]),
        "jamd_beam_pass1_dev": (ci, [vp, vp, ci, vp, ci, vp]),
        "jamd_beam_stream_begin": (ci, [vp, ci]),
        "jamd_beam_stream_push_dev": (ci, [vp, vp, ci, vp, ci, ci, vp]),
        "jamd_beam_set_strict_order": (ci, [vp, ci]),
        "jamd_beam_set_order_mode": (ci, [vp, ci]),
        "jamd_beam_order_mode": (ci, [vp]),
        "jamd_beam_set_workgroup_shape": (ci, [vp, ci]),
        "jamd_beam_workgroup_shape": (ci, [vp, ci]),
        "jamd_beam_exact_layout": (ci, [vp]),
        "jamd_beam_wait_started": (ci, [vp]),
        "jamd_beam_stream_wait_resident": (ci, [vp, vp]),
        "jamd_beam_debug_preset_resident": (ci, [vp, C.c_uint]),
        "jamd_beam_debug_resident": (ci, [vp, P(C.c_uint), P(C.c_uint)]),
        "jamd_beam_prune_order": (ci, [vp, vp, ci, vp, P(ci)]),
        "jamd_beam_prune_arrange": (ci, [vp, vp, ci, vp, P(ci), vp]),
        "jamd_beam_prune_info": (ci, [vp, P(ci), P(ci), P(ci)]),
        "jamd_beam_prune_stats": (ci, [vp, ci, vp, ci]),
        "jamd_beam_results": (ci, [vp, vp, ci]),
        "jamd_beam_trellis": (ci, [vp, ci, vp, ci, P(ci)]),
        # audio front end
        "jamd_frontend_default_desc": (ci, [ci, ci, P(FrontendDesc)]),
        "jamd_frontend_set_kind": (ci, [P(FrontendDesc), ci, ci]),
        "jamd_frontend_htkconf": (ci, [cs, P(FrontendDesc)]),
        "jamd_frontend_table": (ci, [P(FrontendDesc), cs, vp, ci]),
        "jamd_frontend_create": (ci, [vp, P(FrontendDesc), P(vp)]),
        "jamd_frontend_destroy": (None, [vp]),
        "jamd_frontend_veclen": (ci, [vp]),
        "jamd_frontend_frames": (ci, [P(FrontendDesc), i64]),
        "jamd_frontend_run_dev": (ci, [vp, vp, vp, ci, vp, vp, vp]),
        "jamd_frontend_run_host": (ci, [vp, vp, vp, ci, vp, vp]),
        "jamd_frontend_ss_default": (ci, [P(FrontendSS)]),
        "jamd_frontend_set_ss": (ci, [vp, P(FrontendSS)]),
        "jamd_frontend_fftn": (ci, [vp]),
        "jamd_frontend_noise_dev": (ci, [vp, vp, vp, ci, i64, vp, vp]),
        "jamd_frontend_noise_host": (ci, [vp, vp, vp, ci, i64, vp]),
        "jamd_frontend_ss_read": (ci, [cs, vp, ci]),
        "jamd_frontend_ss_write": (ci, [cs, vp, ci]),
        # live-input front end
        "jamd_frontend_live_default": (ci, [P(FrontendLiveDesc)]),
        "jamd_frontend_live_create": (ci, [vp, P(FrontendLiveDesc), ci, P(vp)]),
        "jamd_frontend_live_destroy": (None, [vp]),
        "jamd_frontend_live_frames": (ci, [P(FrontendDesc), i64]),
        "jamd_frontend_live_run_dev": (ci, [vp, vp, vp, vp, vp, vp]),
        "jamd_frontend_live_run_host": (ci, [vp, vp, vp, vp, vp]),
        "jamd_frontend_live_push_dev": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "jamd_frontend_live_push_host": (ci, [vp, vp, vp, vp, vp, vp]),
        "jamd_frontend_live_push_frames": (ci, [P(FrontendDesc), i64, i64, ci]),
        "jamd_frontend_live_stream_cap": (ci, [vp, ci]),
        "jamd_frontend_live_commit": (ci, [vp, vp, vp]),
        "jamd_frontend_live_state_get": (ci, [vp, ci, vp, vp, vp, vp]),
        "jamd_frontend_live_state_set": (ci, [vp, ci, vp, vp]),
        "jamd_frontend_cmn_read": (ci, [cs, ci, ci, ci, vp, vp]),
        "jamd_frontend_cmn_write": (ci, [cs, ci, vp, vp]),
        # audio conditioning
        "jamd_adin_default": (ci, [P(AdinDesc)]),
        "jamd_adin_fir_read": (ci, [cs, vp, ci]),
        "jamd_adin_create": (ci, [vp, P(AdinDesc), ci, P(vp)]),
        "jamd_adin_destroy": (None, [vp]),
        "jamd_adin_reset": (ci, [vp, vp, ci, vp]),
        "jamd_adin_ds_count": (i64, [P(AdinDesc), i64, i64]),
        "jamd_adin_push_cap": (i64, [P(AdinDesc), i64, i64]),
        "jamd_adin_push_dev": (ci, [vp, vp, vp, vp, vp, vp]),
        "jamd_adin_push_host": (ci, [vp, vp, vp, vp, vp]),
        "jamd_adin_state_get": (ci, [vp, ci, vp, vp, vp, vp]),
        # silence cutting
        "jamd_adin_cut_default": (ci, [P(AdinCutDesc)]),
        "jamd_adin_cut_params": (ci, [P(AdinCutDesc), vp, vp, vp, vp]),
        "jamd_adin_cut_create": (ci, [vp, P(AdinCutDesc), ci, P(vp)]),
        "jamd_adin_cut_destroy": (None, [vp]),
        "jamd_adin_cut_reset": (ci, [vp, vp, vp]),
        "jamd_adin_cut_push_cap": (i64, [P(AdinCutDesc), i64]),
        "jamd_adin_cut_parts_cap": (i64, [P(AdinCutDesc), i64]),
        "jamd_adin_cut_push_dev": (ci, [vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]),
        "jamd_adin_cut_push_host": (ci, [vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]),
        "jamd_adin_cut_state_get": (ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp]),
        # voice-activity detector
        "jamd_fvad_model_read": (ci, [cs, P(FvadModel)]),
        "jamd_fvad_create": (ci, [vp, P(FvadDesc), ci, P(vp)]),
        "jamd_fvad_destroy": (None, [vp]),
        "jamd_fvad_reset": (ci, [vp, vp, vp]),
        "jamd_fvad_frames": (i64, [P(FvadDesc), i64, i64]),
        "jamd_fvad_push_dev": (ci, [vp, vp, vp, vp, vp, vp]),
        "jamd_fvad_push_host": (ci, [vp, vp, vp, vp, vp]),
        "jamd_fvad_state_get": (ci, [vp, ci, vp]),
        # the detector inside the silence cutting
        "jamd_adin_cut_create_fvad": (ci, [vp, P(AdinCutDesc), P(AdinCutFvad), ci, P(vp)]),
        "jamd_adin_cut_fvad_reset": (ci, [vp, vp, vp]),
        "jamd_adin_cut_fvad_state_get": (ci, [vp, ci, vp]),
    }


SIGNATURES = _signatures()     # name -> (restype, argtypes) of every function the header declares, in its order

_lib = None


def load():
    """Load libjulius_amd.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise JamdError(
            f"{LIB_PATH} not found: build the HIP engine first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C julius_amd/csrc)")
    lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def declared_symbols():
    """Every `jamd_*` function declared in include/julius_amd.h."""
    import re
    hdr = (_PKG.parent / "include" / "julius_amd.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(jamd_[a-z0-9_]+)\s*\(", hdr)))


def _fail(name, rc):
    return JamdError(f"{name} failed ({rc}): {load().jamd_last_error().decode()}")


def _call(name, *args):
    """An entry that returns 0 or an error code."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise _fail(name, rc)


def _count(name, *args):
    """An entry that returns a count or a negative error code."""
    n = getattr(load(), name)(*args)
    if n < 0:
        raise _fail(name, n)
    return n


class _Handle:
    """An object of the library behind `h`: made by one create entry, destroyed once by the entry `_destroy` names."""
    h = None
    _destroy = None

    def _create(self, name, *args):
        h = C.c_void_p()
        _call(name, *args, C.byref(h))
        self.h = h

    @classmethod
    def _load(cls, eng, name, paths, *args, **attrs):
        """The object a load entry reads from `paths` itself: no host arrays to keep; its attributes are what
        _query() asks the library, then `attrs`."""
        self = cls.__new__(cls)
        self.eng, self._keep = eng, {}
        self._create(name, eng.h, *[str(p).encode() for p in paths], *args)
        self._query()
        vars(self).update(attrs)
        return self

    def _query(self):
        pass

    def close(self):
        if self.h:
            getattr(load(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a):
    """The address of an optional array."""
    return a.ctypes.data if a is not None else None


def _mask(m, nchan):
    """An optional per-channel mask as uint8 [nchan]."""
    if m is None:
        return None
    m = np.ascontiguousarray(np.asarray(m).astype(bool), dtype=np.uint8)
    assert len(m) == nchan
    return m


def _off64(off, nchan=None):
    """A sample offset table as int64 [n + 1]; with nchan, one entry per channel."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    assert nchan is None or len(off) == nchan + 1
    return off


def pack_chunks(chunks):
    """list of int16 arrays -> (the samples back to back, offsets int64 [n + 1])."""
    chunks = [np.ascontiguousarray(u, dtype=np.int16) for u in chunks]
    off = np.zeros(len(chunks) + 1, np.int64)
    off[1:] = np.cumsum([len(u) for u in chunks])
    return (np.concatenate(chunks) if chunks else np.zeros(0, np.int16)), off


def _gmm_desc(model: dict, books: bool = False):
    """(GmmDesc, the arrays it points into); the codebook and stream fields of `model` count only with `books`."""
    keep = {k: (_i32 if k in ("st_off", "ent_dens") else _f32)(model[k])
            for k in ("mean", "ivar", "gconst", "st_off", "ent_dens", "ent_logw")}
    if books and model.get("st_book") is not None:
        keep["st_book"] = _i32(model["st_book"])
    d = GmmDesc()
    d.nstate = len(keep["st_off"]) - 1
    d.veclen = keep["mean"].shape[1]
    d.ndens = keep["mean"].shape[0]
    d.nentry = len(keep["ent_dens"])
    d.nbook = int(model.get("nbook", 0)) if books else 0
    d.nstream = int(model.get("nstream", 1)) if books else 1
    for k, a in keep.items():                # (st_book stays NULL without one)
        setattr(d, k, a.ctypes.data)
    return d, keep


# ---- engine and memory ----------------------------------------------------------------------------------------------

class Engine(_Handle):
    _destroy = "jamd_engine_destroy"

    def __init__(self, device: int = 0):
        self._create("jamd_engine_create", device)
        self.device = device

    def sync(self):
        _call("jamd_engine_sync", self.h)


class DevBuf(_Handle):
    """A raw device allocation through the C ABI (jamd_malloc / jamd_free)."""
    ptr = None

    def __init__(self, eng: "Engine", nbytes: int):
        self.eng, self.nbytes = eng, int(nbytes)
        self._create("jamd_malloc", eng.h, self.nbytes)
        self.ptr = self.h.value

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        _call("jamd_memcpy_h2d", self.eng.h, self.ptr, a.ctypes.data, a.nbytes)
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _call("jamd_memcpy_d2h", self.eng.h, out.ctypes.data, self.ptr, out.nbytes)
        return out

    def free(self):
        if self.ptr:
            load().jamd_free(self.eng.h, self.ptr)
            self.ptr = self.h = None

    close = free


# ---- acoustic models ------------------------------------------------------------------------------------------------

class Gmm(_Handle):
    """Device-resident flattened GMM acoustic model (jamd_gmm)."""
    _destroy = "jamd_gmm_destroy"

    def __init__(self, eng: Engine, model: dict, gprune: int = GPRUNE_NONE, gprune_num: int = 0):
        self.eng = eng
        d, self._keep = _gmm_desc(model, books=True)
        self._desc = d
        self._create("jamd_gmm_create", eng.h, C.byref(d), gprune, gprune_num)
        self.S, self.D = d.nstate, d.veclen
        self.nbook, self.gprune_num = d.nbook, gprune_num

    def _query(self):
        lib = load()
        self.S, self.D, self.nbook = lib.jamd_gmm_nstate(self.h), lib.jamd_gmm_veclen(self.h), lib.jamd_gmm_nbook(self.h)

    @classmethod
    def from_file(cls, eng: Engine, path, gprune: int = GPRUNE_NONE, gprune_num: int = 0):
        """jamd_gmm_load(): a JAMDGMM1 blob read by the library itself."""
        return cls._load(eng, "jamd_gmm_load", [path], gprune, gprune_num, gprune_num=gprune_num)

    @classmethod
    def from_binhmm(cls, eng: Engine, path, gprune: int = GPRUNE_NONE, gprune_num: int = 0):
        """jamd_gmm_load_binhmm(): Julius' binary HMM definition read by the library itself."""
        return cls._load(eng, "jamd_gmm_load_binhmm", [path], gprune, gprune_num, gprune_num=gprune_num)

    def outprob_host(self, frames: np.ndarray) -> np.ndarray:
        fr = _f32(frames)
        T = fr.shape[0]
        assert fr.ndim == 2 and fr.shape[1] == self.D
        out = np.empty((T, self.S), dtype=np.float32)
        _call("jamd_gmm_outprob_host", self.h, fr.ctypes.data, T, out.ctypes.data)
        return out

    def outprob_dev(self, dev_frames: int, T: int, dev_out: int, stream: int = 0):
        _call("jamd_gmm_outprob_dev", self.h, dev_frames, T, dev_out, stream or None)

    def outprob_utts_dev(self, dev_frames: int, utt_off, dev_out: int, stream: int = 0):
        """A batch of utterances back to back (the boundaries matter to gprune heu / beam over tied-mixture codebooks)."""
        off = _i32(utt_off)
        _call("jamd_gmm_outprob_utts_dev", self.h, dev_frames, off.ctypes.data, len(off) - 1, dev_out, stream or None)

    def dens_host(self, frames: np.ndarray) -> np.ndarray:
        """Per-Gaussian scores [T][nentry] (the plugin slot's compute_gaussset values)."""
        fr = _f32(frames)
        E = load().jamd_gmm_nentry(self.h)
        out = np.empty((fr.shape[0], E), dtype=np.float32)
        _call("jamd_gmm_dens_host", self.h, fr.ctypes.data, fr.shape[0], out.ctypes.data)
        return out

    def last_kernel(self) -> str:
        return load().jamd_gmm_last_kernel(self.h).decode()

    def tmix_cache_host(self, frames: np.ndarray):
        """Codebook top-N cache (MIXCACHE) for every (frame, book): score, id, num."""
        lib = load()
        fr = _f32(frames)
        T = fr.shape[0]
        cap, nbook = lib.jamd_gmm_tmix_cap(self.h), lib.jamd_gmm_nbook(self.h)
        d_fr = DevBuf(self.eng, fr.nbytes).upload(fr)
        d_sc = DevBuf(self.eng, 4 * T * nbook * cap)
        d_id = DevBuf(self.eng, 4 * T * nbook * cap)
        d_n = DevBuf(self.eng, 4 * T * nbook)
        _call("jamd_gmm_tmix_cache_dev", self.h, d_fr.ptr, T, d_sc.ptr, d_id.ptr, d_n.ptr, None)
        self.eng.sync()
        return (d_sc.download((T, nbook, cap), np.float32), d_id.download((T, nbook, cap), np.int32),
                d_n.download((T, nbook), np.int32))


class GmmStreams(_Handle):
    """Device-resident multi-stream GMM acoustic model (jamd_gmm_ms): per-state stream weights over a pool of
    mixture pdfs, `-gprune none` (tied-mixture pdfs and `-gprune safe`: GmmStreamsTied).  model: nstream, vsize[nstream], pdf_stream[npdf], pdf_off[npdf + 1],
    ent_dens / ent_logw[nentry], st_pdf[S][nstream], st_weight[S][nstream] or None, dens_off[ndens + 1],
    mean / ivar (flat, back to back), gconst[ndens]; pdf_book[npdf] optional."""
    _destroy = "jamd_gmm_ms_destroy"

    _INT = ("vsize", "pdf_stream", "pdf_off", "ent_dens", "st_pdf", "dens_off")
    _FLT = ("ent_logw", "mean", "ivar", "gconst")

    @classmethod
    def make_desc(cls, model: dict):
        """(GmmStreamsDesc, the arrays it points into)."""
        keep = {k: _i32(model[k]) for k in cls._INT}
        keep.update({k: _f32(model[k]).reshape(-1) for k in cls._FLT})
        keep["st_pdf"] = keep["st_pdf"].reshape(-1, len(keep["vsize"]))
        for k, conv in (("st_weight", _f32), ("pdf_book", _i32)):
            if model.get(k) is not None:
                keep[k] = conv(model[k])
        d = GmmStreamsDesc()
        d.nstate = keep["st_pdf"].shape[0]
        d.veclen = int(model["veclen"]) if "veclen" in model else int(keep["vsize"].sum())
        d.nstream = int(model.get("nstream", len(keep["vsize"])))
        d.npdf, d.nentry, d.ndens = len(keep["pdf_stream"]), len(keep["ent_dens"]), len(keep["gconst"])
        for k in cls._INT + cls._FLT + ("st_weight", "pdf_book"):
            setattr(d, k, keep[k].ctypes.data if k in keep else None)
        return d, keep

    def __init__(self, eng: Engine, model: dict):
        self.eng = eng
        d, self._keep = self.make_desc(model)
        self._create("jamd_gmm_ms_create", eng.h, C.byref(d))
        self._query()

    def _query(self):
        lib, h = load(), self.h
        self.S, self.D, self.nstream = lib.jamd_gmm_ms_nstate(h), lib.jamd_gmm_ms_veclen(h), lib.jamd_gmm_ms_nstream(h)

    @classmethod
    def from_binhmm(cls, eng: Engine, path):
        """jamd_gmm_ms_load_binhmm(): mkbinhmm's file of a model of any stream count, read by the library itself."""
        return cls._load(eng, "jamd_gmm_ms_load_binhmm", [path])

    def outprob_host(self, frames: np.ndarray) -> np.ndarray:
        fr = _f32(frames)
        T = fr.shape[0]
        assert fr.ndim == 2 and fr.shape[1] == self.D
        out = np.empty((T, self.S), dtype=np.float32)
        _call("jamd_gmm_ms_outprob_host", self.h, fr.ctypes.data, T, out.ctypes.data)
        return out

    def outprob_dev(self, dev_frames: int, T: int, dev_out: int, stream: int = 0):
        _call("jamd_gmm_ms_outprob_dev", self.h, dev_frames, T, dev_out, stream or None)

    def last_kernel(self) -> str:
        return load().jamd_gmm_ms_last_kernel(self.h).decode()

    def outprob_utts_dev(self, dev_frames: int, utt_off, dev_out: int, stream: int = 0):
        """A batch of utterances back to back (the boundaries matter to gprune safe over tied-mixture pdfs)."""
        off = _i32(utt_off)
        _call("jamd_gmm_ms_outprob_utts_dev", self.h, dev_frames, off.ctypes.data, len(off) - 1, dev_out, stream or None)


class GmmStreamsTied(GmmStreams):
    """jamd_gmm_ms through jamd_gmm_ms_create_opt(): tied-mixture codebooks (model["pdf_book"]) and `-gprune safe`.
    GmmStreams with the keyword arguments gprune = None | "none" | "safe", gprune_num (-tmix) and chunk_frames; None
    routes to the entries GmmStreams itself uses.  (A class of its own: GmmStreams' signatures are a kept surface.)"""

    class Opt(C.Structure):
        """jamd_gmm_ms_opt (include/julius_amd.h)."""
        _fields_ = [("gprune", C.c_int), ("gprune_num", C.c_int), ("chunk_frames", C.c_int)]

    _GPRUNE = {"none": GPRUNE_NONE, "safe": GPRUNE_SAFE, "heu": GPRUNE_HEU, "beam": GPRUNE_BEAM}

    @classmethod
    def _opt(cls, gprune, gprune_num, chunk_frames):
        return cls.Opt(cls._GPRUNE[gprune] if isinstance(gprune, str) else int(gprune), int(gprune_num), int(chunk_frames))

    def __init__(self, eng: Engine, model: dict, gprune=None, gprune_num: int = 0, chunk_frames: int = 0):
        if gprune is None:
            GmmStreams.__init__(self, eng, model)
            return
        self.eng = eng
        d, self._keep = self.make_desc(model)
        self._create("jamd_gmm_ms_create_opt", eng.h, C.byref(d), C.byref(self._opt(gprune, gprune_num, chunk_frames)))
        self._query()

    def _query(self):
        GmmStreams._query(self)
        lib = load()
        self.tmix_cap, self.nbook = lib.jamd_gmm_ms_tmix_cap(self.h), lib.jamd_gmm_ms_nbook(self.h)

    @classmethod
    def from_binhmm(cls, eng: Engine, path, gprune=None, gprune_num: int = 0, chunk_frames: int = 0):
        """jamd_gmm_ms_load_binhmm_opt(): the codebook section and tmix pdfs of mkbinhmm's file included."""
        if gprune is None:
            return cls._load(eng, "jamd_gmm_ms_load_binhmm", [path])
        return cls._load(eng, "jamd_gmm_ms_load_binhmm_opt", [path], C.byref(cls._opt(gprune, gprune_num, chunk_frames)))

    def outprob_host(self, frames: np.ndarray, utt_off=None) -> np.ndarray:
        if utt_off is None:
            return GmmStreams.outprob_host(self, frames)
        fr, off = _f32(frames), _i32(utt_off)
        assert fr.ndim == 2 and fr.shape[1] == self.D and off[-1] == fr.shape[0]
        out = np.empty((fr.shape[0], self.S), dtype=np.float32)
        _call("jamd_gmm_ms_outprob_utts_host", self.h, fr.ctypes.data, off.ctypes.data, len(off) - 1, out.ctypes.data)
        return out

    def tmix_cache_host(self, frames: np.ndarray):
        """Codebook cache (MIXCACHE) for every (frame, book) of one utterance: score, id, num."""
        fr = _f32(frames)
        T, cap, nbook = fr.shape[0], self.tmix_cap, self.nbook
        d_fr = DevBuf(self.eng, fr.nbytes).upload(fr)
        d_sc, d_id, d_n = (DevBuf(self.eng, 4 * T * nbook * c) for c in (cap, cap, 1))
        _call("jamd_gmm_ms_tmix_cache_dev", self.h, d_fr.ptr, T, d_sc.ptr, d_id.ptr, d_n.ptr, None)
        self.eng.sync()
        return (d_sc.download((T, nbook, cap), np.float32), d_id.download((T, nbook, cap), np.int32),
                d_n.download((T, nbook), np.int32))


class Gms(_Handle):
    """Gaussian mixture selection stage (jamd_gms): gms_state() of libsent/src/phmm/gms.c."""
    _destroy = "jamd_gms_destroy"

    def __init__(self, eng: Engine, gs_model: dict, state2gs, nbest: int):
        self.eng = eng
        d, self._keep = _gmm_desc(gs_model)
        self.state2gs = _i32(state2gs)
        self.S, self.D, self.nbest = len(self.state2gs), d.veclen, int(nbest)
        self._create("jamd_gms_create", eng.h, C.byref(d), self.state2gs.ctypes.data, self.S, self.nbest)

    def _query(self):
        self.S = load().jamd_gms_nstate(self.h)

    @classmethod
    def from_file(cls, eng: Engine, path, veclen: int):
        """jamd_gms_load(): the selection model file jamd_export writes next to PREFIX.am."""
        return cls._load(eng, "jamd_gms_load", [path], D=int(veclen))

    def set_strict_order(self, on: bool = True):
        _call("jamd_gms_set_strict_order", self.h, int(on))
        return self

    def apply_dev(self, dev_frames: int, T: int, dev_scores: int, utt_off=None, stream: int = 0):
        off = _i32(utt_off) if utt_off is not None else None
        _call("jamd_gms_apply_dev", self.h, dev_frames, T, _ptr(off), len(off) - 1 if off is not None else 0,
              dev_scores, stream or None)

    def apply_host(self, frames: np.ndarray, scores: np.ndarray, utt_off=None) -> np.ndarray:
        fr, sc = _f32(frames), _f32(scores)
        T = fr.shape[0]
        assert sc.shape == (T, self.S) and fr.shape[1] == self.D
        out = sc.copy()
        off = _i32(utt_off) if utt_off is not None else None
        _call("jamd_gms_apply_host", self.h, fr.ctypes.data, T, _ptr(off), len(off) - 1 if off is not None else 0,
              out.ctypes.data)
        return out


class RejGmm(_Handle):
    """GMM-based input verification scores (jamd_rejgmm): gmm_proceed() of libjulius/src/gmm.c."""
    _destroy = "jamd_rejgmm_destroy"

    def __init__(self, eng: Engine, model: dict, model_state, gprune_num: int = 10):
        self.eng = eng
        d, self._keep = _gmm_desc(model)
        ms = _i32(model_state)
        self.nmodel, self.D = len(ms), d.veclen
        self._create("jamd_rejgmm_create", eng.h, C.byref(d), ms.ctypes.data, self.nmodel, int(gprune_num))

    def scores_host(self, frames: np.ndarray, utt_off=None):
        """(frame scores [T][nmodel], utterance sums [nutt][nmodel]); one utterance by default."""
        fr = _f32(frames)
        T = fr.shape[0]
        assert fr.ndim == 2 and fr.shape[1] == self.D
        off = _i32(utt_off if utt_off is not None else [0, T])
        fs = np.empty((T, self.nmodel), np.float32)
        us = np.empty((len(off) - 1, self.nmodel), np.float32)
        _call("jamd_rejgmm_scores_host", self.h, fr.ctypes.data, T, off.ctypes.data, len(off) - 1, fs.ctypes.data,
              us.ctypes.data)
        return fs, us


class CdSet(_Handle):
    """Pseudo-phone state sets (jamd_cdset): outprob_cd() over a score matrix."""
    _destroy = "jamd_cdset_destroy"

    def __init__(self, eng: Engine, set_off, states, method=IWCD_MAX, nbest=3):
        self.eng = eng
        self.set_off, self.states = _i32(set_off), _i32(states)
        self.nset = len(self.set_off) - 1
        self._create("jamd_cdset_create", eng.h, self.nset, self.set_off.ctypes.data, self.states.ctypes.data, method,
                     nbest)

    def outprob_dev(self, dev_scores: int, T: int, nstate: int, dev_cd: int, stream: int = 0):
        _call("jamd_cdset_outprob_dev", self.h, dev_scores, T, nstate, dev_cd, stream or None)

    def outprob_host(self, scores: np.ndarray) -> np.ndarray:
        sc = _f32(scores)
        T, S = sc.shape
        d_sc = DevBuf(self.eng, sc.nbytes).upload(sc)
        d_cd = DevBuf(self.eng, 4 * T * max(self.nset, 1))
        self.outprob_dev(d_sc.ptr, T, S, d_cd.ptr)
        self.eng.sync()
        return d_cd.download((T, self.nset), np.float32)


class Dnn(_Handle):
    """Device-resident DNN acoustic model (jamd_dnn)."""
    _destroy = "jamd_dnn_destroy"

    def __init__(self, eng: Engine, dnn: dict):
        self.eng = eng
        self.dims = _i32(dnn["dims"])
        nl = len(self.dims) - 1
        self._w = [_f32(w) for w in dnn["w"]]
        self._b = [_f32(b) for b in dnn["b"]]
        for l in range(nl):
            assert self._w[l].shape == (self.dims[l + 1], self.dims[l]), "W[l] must be [out][in]"
        self._wp = (C.c_void_p * nl)(*[w.ctypes.data for w in self._w])
        self._bp = (C.c_void_p * nl)(*[b.ctypes.data for b in self._b])
        self._prior = _f32(dnn["prior"])
        d = DnnDesc()
        d.nlayer = nl
        d.dims = self.dims.ctypes.data
        d.w = C.cast(self._wp, C.c_void_p)
        d.b = C.cast(self._bp, C.c_void_p)
        d.state_prior = self._prior.ctypes.data
        self._create("jamd_dnn_create", eng.h, C.byref(d))
        self.S, self.D = int(self.dims[-1]), int(self.dims[0])

    def _query(self):
        self.S, self.D = load().jamd_dnn_nstate(self.h), load().jamd_dnn_veclen(self.h)

    @classmethod
    def from_dnnconf(cls, eng: Engine, path):
        """jamd_dnn_load(): Julius' dnnconf + .npy + prior files read by the library itself."""
        return cls._load(eng, "jamd_dnn_load", [path])

    def outprob_host(self, frames: np.ndarray) -> np.ndarray:
        fr = _f32(frames)
        T = fr.shape[0]
        assert fr.shape[1] == self.D
        out = np.empty((T, self.S), dtype=np.float32)
        _call("jamd_dnn_outprob_host", self.h, fr.ctypes.data, T, out.ctypes.data)
        return out

    def outprob_dev(self, dev_frames: int, T: int, dev_out: int, stream: int = 0):
        _call("jamd_dnn_outprob_dev", self.h, dev_frames, T, dev_out, stream or None)


# ---- first pass -----------------------------------------------------------------------------------------------------

class Lexicon(_Handle):
    """Device-resident first-pass tables (jamd_lexicon) from a lexicon dict
    (julius_amd.lexblob.load)."""
    _destroy = "jamd_lexicon_destroy"

    def __init__(self, eng: Engine, lex: dict):
        from . import lexblob
        self.eng, self.lex = eng, lex
        d, self._keep = lexblob.make_desc(lex)
        self._create("jamd_lexicon_create", eng.h, C.byref(d))

    @classmethod
    def from_file(cls, eng: Engine, path, bingram=None):
        """jamd_lexicon_load(): a JAMDLEX1 blob read by the library itself; with `bingram` the N-gram half comes from
        that binary N-gram file (jamd_lexicon_load_ngram())."""
        if bingram is not None:
            return cls._load(eng, "jamd_lexicon_load_ngram", [path, bingram], lex=None)
        return cls._load(eng, "jamd_lexicon_load", [path], lex=None)

    def lm_table(self) -> int:
        """1 = the cross-word LM table exists, 0 = the kernels compute its entries (jamd_lexicon_lm_table)."""
        return load().jamd_lexicon_lm_table(self.h)


class Beam(_Handle):
    """First-pass work area for a batch of utterances (jamd_beam)."""
    _destroy = "jamd_beam_destroy"

    def __init__(self, eng: Engine, lexicon: Lexicon, beam_width: int, score_pruning_width: float = -1.0,
                 max_utts: int = 1, atoms_per_utt: int = 1 << 16):
        self.eng, self.lexicon = eng, lexicon
        self.max_utts, self.atoms_per_utt = max_utts, atoms_per_utt
        self._create("jamd_beam_create", eng.h, lexicon.h, beam_width, score_pruning_width, max_utts, atoms_per_utt)
        # test knob: JAMD_TEST_SHAPE=half runs every work area that can in the half workgroup shape (the results must
        # not depend on it), so the whole GPU suite can be replayed over that shape
        if os.environ.get("JAMD_TEST_SHAPE") == "half":
            load().jamd_beam_set_workgroup_shape(self.h, 2)

    def set_strict_order(self, on: bool = True):
        _call("jamd_beam_set_strict_order", self.h, 1 if on else 0)

    ORDER_MODES = {"fast": 0, "strict": 1, "exact": 2, "exact_serial": 3}

    def set_order_mode(self, mode):
        """'exact' (default where available), 'exact_serial', 'fast' or 'strict' -- see julius_amd.h."""
        m = self.ORDER_MODES[mode] if isinstance(mode, str) else int(mode)
        _call("jamd_beam_set_order_mode", self.h, m)
        return self

    def order_mode(self) -> str:
        m = load().jamd_beam_order_mode(self.h)
        return {v: k for k, v in self.ORDER_MODES.items()}[m]

    SHAPES = {"auto": 0, "full": 1, "half": 2}

    def set_workgroup_shape(self, shape):
        """'auto' (default), 'full' (one utterance per CU) or 'half' (two per CU) -- see julius_amd.h."""
        m = self.SHAPES[shape] if isinstance(shape, str) else int(shape)
        _call("jamd_beam_set_workgroup_shape", self.h, m)
        return self

    def workgroup_shape(self, nutt: int = 1) -> str:
        m = load().jamd_beam_workgroup_shape(self.h, nutt)
        return {v: k for k, v in self.SHAPES.items()}[m]

    def wait_started(self):
        """Host waits until the latest first-pass launch is next to run (jamd_beam_wait_started)."""
        _call("jamd_beam_wait_started", self.h)

    def stream_wait_resident(self, stream: int = 0):
        """Work queued on `stream` behind this call starts once the latest first-pass launch holds its CUs
        (jamd_beam_stream_wait_resident: a wait on device memory, no host involvement)."""
        _call("jamd_beam_stream_wait_resident", self.h, stream)

    def debug_preset_resident(self, count: int):
        _call("jamd_beam_debug_preset_resident", self.h, count)

    def debug_resident(self):
        a, b = C.c_uint(), C.c_uint()
        _call("jamd_beam_debug_resident", self.h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def exact_layout(self) -> str:
        """'narrow' / 'wide' LDS image of the exact-order kernel for this work area, or 'none' (jamd_beam_exact_layout)."""
        return {0: "none", 1: "narrow", 2: "wide"}[load().jamd_beam_exact_layout(self.h)]

    def prune_order(self, scores):
        """sort_token_no_order() alone: the visiting order the exact-order kernel derives for tokens with
        these scores (creation order) under this work area's beam width."""
        sc = _f32(scores)
        out = np.zeros(len(sc), np.int32)
        n = C.c_int()
        _call("jamd_beam_prune_order", self.h, sc.ctypes.data, len(sc), out.ctypes.data, C.byref(n))
        return out[:n.value].copy()

    def prune_arrange(self, scores):
        """sort_token_no_order() with the whole array out: (visiting order, tindex[0..n)) -- jamd_beam_prune_arrange()."""
        sc = _f32(scores)
        out = np.zeros(len(sc), np.int32)
        arr = np.zeros(len(sc), np.int32)
        n = C.c_int()
        _call("jamd_beam_prune_arrange", self.h, sc.ctypes.data, len(sc), out.ctypes.data, C.byref(n), arr.ctypes.data)
        return out[:n.value].copy(), arr

    def prune_info(self):
        """Rounds of the sweep replay in the latest prune_order() call (-1 = it gave the frame up, 0 = not used)."""
        r, us, ne = C.c_int(), C.c_int(), C.c_int()
        _call("jamd_beam_prune_info", self.h, C.byref(r), C.byref(us), C.byref(ne))
        self.last_sweep_us, self.last_sweep_events = us.value, ne.value
        return r.value

    def prune_stats(self, utt=0, reset=False):
        """Counters of utterance `utt` in the exact-order kernel since the work area was created or they were last
        reset (jamd_beam_prune_stats): [0..7] frames by the path their rank pruning step took, [8..11] work sums
        (tokens created, survivors visited, word ends, frames), [12] multipath frames that sorted mid-frame, and the
        lane split of the state-set reductions: [13] frames that ran two lanes per set, [14] frames that ran one,
        [15] reductions summed over the frames (four-lane frames = [11] - [13] - [14]; a multipath lexicon leaves
        [13..15] at 0).  The frames are the turns of the kernel's frame loop: under an N-gram the initial token is
        scored before it, so T input frames count as T - 1."""
        st = np.zeros(16, np.int32)
        _call("jamd_beam_prune_stats", self.h, utt, st.ctypes.data, 1 if reset else 0)
        return [int(x) for x in st]

    def stream_begin(self, nutt: int):
        self._nutt = nutt
        _call("jamd_beam_stream_begin", self.h, nutt)

    def stream_push_dev(self, dev_scores: int, nstate: int, chunk_off, final: bool = False, stream: int = 0):
        off = _i32(chunk_off)
        _call("jamd_beam_stream_push_dev", self.h, dev_scores or None, nstate, off.ctypes.data, len(off) - 1,
              1 if final else 0, stream or None)

    def pass1_dev(self, dev_scores: int, nstate: int, utt_off, stream: int = 0):
        off = _i32(utt_off)
        self._nutt = len(off) - 1
        _call("jamd_beam_pass1_dev", self.h, dev_scores, nstate, off.ctypes.data, self._nutt, stream or None)

    def results(self, nutt=None):
        n = self._nutt if nutt is None else nutt
        arr = (Pass1Result * n)()
        _call("jamd_beam_results", self.h, arr, n)
        return list(arr)

    def trellis(self, utt: int):
        from . import lexblob
        n = C.c_int()
        _call("jamd_beam_trellis", self.h, utt, None, 0, C.byref(n))
        atoms = np.zeros(max(n.value, 1), dtype=lexblob.ATOM_DTYPE)
        _call("jamd_beam_trellis", self.h, utt, atoms.ctypes.data, n.value, C.byref(n))
        return atoms[:n.value]

    def pass1_host(self, score_list):
        """Convenience for tests: list of [T_u][S] host score matrices -> (results, trellises)."""
        S = score_list[0].shape[1]
        off = np.zeros(len(score_list) + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in score_list])
        allsc = _f32(np.concatenate(score_list, axis=0))
        d = DevBuf(self.eng, allsc.nbytes).upload(allsc)
        self.pass1_dev(d.ptr, S, off)
        res = self.results()
        tre = [self.trellis(u) for u in range(len(score_list))]
        d.free()
        return res, tre


# ---- front end ------------------------------------------------------------------------------------------------------

F_BASE = {"MFCC": 6, "FBANK": 7, "MELSPEC": 8}
F_QUAL = {"E": 0x40, "N": 0x80, "D": 0x100, "A": 0x200, "Z": 0x800, "0": 0x2000}


def param_kind(name: str) -> int:
    """HTK parameter kind name ("MFCC_E_D_N_Z") -> code, as param_str2code() (libsent/src/anlz/paramtypes.c)."""
    base, *quals = name.upper().split("_")
    if base not in F_BASE or any(q not in F_QUAL for q in quals):
        raise JamdError(f"parameter kind {name!r}: base MFCC / FBANK / MELSPEC with _E _N _D _A _Z _0 only")
    code = F_BASE[base]
    for q in quals:
        code |= F_QUAL[q]
    return code


def ss_read(path) -> np.ndarray:
    """A noise spectrum file of mkss / -ssload (big-endian count, then big-endian floats) -> float32 [count]."""
    n = _count("jamd_frontend_ss_read", str(path).encode(), None, 0)
    out = np.zeros(n, np.float32)
    if load().jamd_frontend_ss_read(str(path).encode(), out.ctypes.data, n) != n:
        raise JamdError(f"jamd_frontend_ss_read failed: {load().jamd_last_error().decode()}")
    return out


def ss_write(path, noise):
    noise = _f32(noise).ravel()
    _call("jamd_frontend_ss_write", str(path).encode(), noise.ctypes.data, len(noise))


class Frontend(_Handle):
    """Audio front end (jamd_frontend): Wav2MFCC() of libsent/src/wav2mfcc/wav2mfcc-buffer.c plus the
    splicing of libjulius/src/wav2mfcc.c, on the device.  int16 PCM in, features [T][veclen * splice] out."""
    _destroy = "jamd_frontend_destroy"

    def __init__(self, eng: Engine, desc: FrontendDesc, cmean=None, cvar=None):
        self.eng, self.desc = eng, desc
        self._cm = _f32(cmean) if cmean is not None else None
        self._cv = _f32(cvar) if cvar is not None else None
        desc.cmean_init, desc.cvar_init = _ptr(self._cm), _ptr(self._cv)
        self._create("jamd_frontend_create", eng.h, C.byref(desc))
        self.veclen = load().jamd_frontend_veclen(self.h)
        self.fftn = load().jamd_frontend_fftn(self.h)

    @staticmethod
    def desc_for(kind, vecsize: int, htkconf=None, **fields) -> FrontendDesc:
        """make_default_para() + calc_para_from_header(kind, vecsize), an optional HTK config file on top
        (then the kind again, as the AM header is applied after the config), then `fields` verbatim."""
        code = param_kind(kind) if isinstance(kind, str) else int(kind)
        d = FrontendDesc()
        _call("jamd_frontend_default_desc", code, int(vecsize), C.byref(d))
        if htkconf is not None:
            _call("jamd_frontend_htkconf", str(htkconf).encode(), C.byref(d))
            _call("jamd_frontend_set_kind", C.byref(d), code, int(vecsize))
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    @classmethod
    def from_kind(cls, eng: Engine, kind, vecsize: int, cmean=None, cvar=None, **fields):
        return cls(eng, cls.desc_for(kind, vecsize, **fields), cmean, cvar)

    @classmethod
    def from_htkconf(cls, eng: Engine, path, kind, vecsize: int, cmean=None, cvar=None, **fields):
        return cls(eng, cls.desc_for(kind, vecsize, htkconf=path, **fields), cmean, cvar)

    def frames(self, nsamples: int) -> int:
        return load().jamd_frontend_frames(C.byref(self.desc), int(nsamples))

    _pack = staticmethod(pack_chunks)        # (the name tools and tests know it by)

    def run_host(self, utts):
        """list of int16 arrays -> (features [sum T][veclen * splice] float32, frame_off [nutt + 1] int32)."""
        samples, off = pack_chunks(utts)
        T = sum(self.frames(off[u + 1] - off[u]) for u in range(len(utts)))
        out = np.zeros((max(T, 0), self.veclen), np.float32)
        foff = np.zeros(len(utts) + 1, np.int32)
        _call("jamd_frontend_run_host", self.h, samples.ctypes.data, off.ctypes.data, len(utts), out.ctypes.data,
              foff.ctypes.data)
        return out, foff

    def set_ss(self, mode, calc_len_ms: int = 300, alpha: float = 2.0, floor: float = 0.5, noise=None):
        """Spectral subtraction for every later run: SS_CALC (-sscalc, head of calc_len_ms per utterance), SS_LOAD
        (-ssload, `noise` float32 [fftn]) or SS_OFF.  A refused call raises and leaves the object as it was."""
        mode = {"off": SS_OFF, "calc": SS_CALC, "load": SS_LOAD}.get(mode, mode)
        nz = _f32(noise).ravel() if noise is not None else None
        ss = FrontendSS(int(mode), int(calc_len_ms), float(alpha), float(floor), _ptr(nz), len(nz) if nz is not None else 0)
        _call("jamd_frontend_set_ss", self.h, C.byref(ss))

    def noise_host(self, utts, head_samples: int = 0):
        """new_SS_calculate() over the first min(head_samples, length) samples of every utterance (0: all of it):
        list of int16 arrays -> float32 [nutt][fftn]."""
        samples, off = pack_chunks(utts)
        out = np.zeros((len(utts), self.fftn), np.float32)
        _call("jamd_frontend_noise_host", self.h, samples.ctypes.data, off.ctypes.data, len(utts), int(head_samples),
              out.ctypes.data)
        return out

    def noise_dev(self, dev_samples: int, sample_off, dev_noise: int, head_samples: int = 0, stream: int = 0):
        off = _off64(sample_off)
        _call("jamd_frontend_noise_dev", self.h, dev_samples, off.ctypes.data, len(off) - 1, int(head_samples),
              dev_noise, stream or None)

    def run_dev(self, dev_samples: int, sample_off, dev_out: int, stream: int = 0):
        """Device samples and features; sample_off host int64 [nutt + 1].  Returns frame_off [nutt + 1]."""
        off = _off64(sample_off)
        foff = np.zeros(len(off), np.int32)
        _call("jamd_frontend_run_dev", self.h, dev_samples, off.ctypes.data, len(off) - 1, dev_out, foff.ctypes.data,
              stream or None)
        return foff


def cmn_read(path, veclen: int, mfcc_dim: int, want_var: bool = False):
    """A -cmnload file (ASCII <CEPSNORM> or the old binary form) -> (mean [veclen], variance [veclen] or None), as
    CMN_load_from_file() reads it; mfcc_dim counts the cepstra plus c0.  Raises where the reference refuses the file."""
    cm, cv = np.zeros(veclen, np.float32), np.zeros(veclen, np.float32)
    r = _count("jamd_frontend_cmn_read", str(path).encode(), int(veclen), int(mfcc_dim), 1 if want_var else 0,
               cm.ctypes.data, cv.ctypes.data)
    return cm, (cv if r == 1 else None)


def cmn_write(path, cmean, cvar=None):
    """CMN_save_to_file(): the ASCII form, with a <VARIANCE> block when cvar is given."""
    cm = _f32(cmean).ravel()
    cv = _f32(cvar).ravel() if cvar is not None else None
    assert cv is None or len(cv) == len(cm)
    _call("jamd_frontend_cmn_write", str(path).encode(), len(cm), cm.ctypes.data, _ptr(cv))


class LiveFrontend(_Handle):
    """Live-input front end (jamd_frontend_live) over a created Frontend: per channel and call one whole segment (run_*)
    or the next chunk of an open one (push_*), the vectors of RealTimeMFCC() and the flush loop of RealTimeParam()
    (libjulius/src/realtime-1stpass.c), with the MAP-CMN / energy state of every channel kept on the device between
    calls."""
    _destroy = "jamd_frontend_live_destroy"

    def __init__(self, fe: Frontend, nchan: int, map_cmn: bool = True, map_weight: float = 100.0, cmean=None, cvar=None):
        self.fe, self.nchan = fe, int(nchan)      # (keeps the parent alive)
        self.veclen = fe.veclen
        self.base_veclen = fe.desc.veclen
        cm = _f32(cmean) if cmean is not None else None
        cv = _f32(cvar) if cvar is not None else None
        d = FrontendLiveDesc(1 if map_cmn else 0, float(map_weight), _ptr(cm), _ptr(cv))
        self._create("jamd_frontend_live_create", fe.h, C.byref(d), self.nchan)

    def frames(self, nsamples: int) -> int:
        return load().jamd_frontend_live_frames(C.byref(self.fe.desc), int(nsamples))

    def run_host(self, segs):
        """One int16 array per channel (empty = idle) -> (rows [sum T][veclen * splice], frame_off [nchan + 1])."""
        assert len(segs) == self.nchan
        samples, off = pack_chunks(segs)
        if len(samples) == 0:
            samples = np.zeros(1, np.int16)
        T = sum(self.frames(off[c + 1] - off[c]) for c in range(self.nchan))
        out = np.zeros((T, self.veclen), np.float32)
        foff = np.zeros(self.nchan + 1, np.int32)
        buf = out if T else np.zeros((1, self.veclen), np.float32)
        _call("jamd_frontend_live_run_host", self.h, samples.ctypes.data, off.ctypes.data, buf.ctypes.data,
              foff.ctypes.data)
        return out, foff

    def run_dev(self, dev_samples: int, sample_off, dev_out: int, stream: int = 0):
        """Device samples and rows; sample_off host int64 [nchan + 1].  Returns frame_off [nchan + 1]."""
        off = _off64(sample_off, self.nchan)
        foff = np.zeros(len(off), np.int32)
        _call("jamd_frontend_live_run_dev", self.h, dev_samples, off.ctypes.data, dev_out, foff.ctypes.data,
              stream or None)
        return foff

    def push_frames(self, samples_before: int, chunk: int, final: bool = False) -> int:
        """Rows a push of `chunk` samples yields on a segment that has taken samples_before."""
        return load().jamd_frontend_live_push_frames(C.byref(self.fe.desc), int(samples_before), int(chunk),
                                                     1 if final else 0)

    def stream_cap(self, max_rows: int):
        """Rows of an open segment kept per channel for the variance re-estimation (cvn with splice 1)."""
        _call("jamd_frontend_live_stream_cap", self.h, int(max_rows))

    def push_host(self, chunks, final=None):
        """The next int16 chunk of every channel's open segment (empty = none; the first opens one); `final` marks the
        channels whose segment ends behind it -> (rows completed [sum T][veclen * splice], frame_off [nchan + 1])."""
        assert len(chunks) == self.nchan
        samples, off = pack_chunks(chunks)
        if len(samples) == 0:
            samples = np.zeros(1, np.int16)
        m = _mask(final, self.nchan)
        d = self.fe.desc                         # a push completes at most the frames its samples and the delays hold
        max_rows = int(off[-1]) // d.frameshift + self.nchan * (d.delWin + d.accWin + 2)
        buf = np.zeros((max_rows, self.veclen), np.float32)
        foff = np.zeros(self.nchan + 1, np.int32)
        _call("jamd_frontend_live_push_host", self.h, samples.ctypes.data, off.ctypes.data, _ptr(m), buf.ctypes.data,
              foff.ctypes.data)
        return buf[:int(foff[-1])].copy(), foff

    def push_dev(self, dev_samples: int, sample_off, dev_out: int, final=None, stream: int = 0):
        """Device samples and rows; sample_off host int64 [nchan + 1].  Returns frame_off [nchan + 1]."""
        off = _off64(sample_off, self.nchan)
        m = _mask(final, self.nchan)
        foff = np.zeros(len(off), np.int32)
        _call("jamd_frontend_live_push_dev", self.h, dev_samples or None, off.ctypes.data, _ptr(m), dev_out or None,
              foff.ctypes.data, stream or None)
        return foff

    def commit(self, update=None, stream: int = 0):
        """CMN_realtime_update() for the channels whose entry of `update` is true (None: every channel)."""
        _call("jamd_frontend_live_commit", self.h, _ptr(_mask(update, self.nchan)), stream or None)

    def state(self, chan: int):
        """(cmean_init [veclen], cvar_init [veclen], energy maximum, flags) of one channel, after everything queued."""
        cm, cv = np.zeros(self.base_veclen, np.float32), np.zeros(self.base_veclen, np.float32)
        em, fl = C.c_float(0), C.c_int(0)
        _call("jamd_frontend_live_state_get", self.h, int(chan), cm.ctypes.data, cv.ctypes.data, C.addressof(em),
              C.addressof(fl))
        return cm, cv, np.float32(em.value), fl.value

    def set_state(self, chan: int, cmean, cvar=None):
        cm = _f32(cmean).ravel()
        cv = _f32(cvar).ravel() if cvar is not None else None
        assert len(cm) == self.base_veclen and (cv is None or len(cv) == self.base_veclen)
        _call("jamd_frontend_live_state_set", self.h, int(chan), cm.ctypes.data, _ptr(cv))


# ---- audio input ----------------------------------------------------------------------------------------------------

def adin_fir_read(path, cap: int = 513) -> np.ndarray:
    """A FIR coefficient file in the text format of the reference's load_filter() -> float64 [n]."""
    out = np.zeros(int(cap), np.float64)
    n = _count("jamd_adin_fir_read", str(path).encode(), out.ctypes.data, int(cap))
    return out[:n].copy()


class Adin(_Handle):
    """Audio conditioning in front of the front ends (jamd_adin): per push and channel one ad_read() chunk through
    ds48to16() (-48), the level scaling (-lvscale), strip_zero() and sub_zmean() (-zmean) of adin_cut()
    (libjulius/src/adin-cut.c:470-545), with the filter and DC state of every channel kept on the device."""
    _destroy = "jamd_adin_destroy"

    def __init__(self, eng: Engine, nchan: int, desc: "AdinDesc | None" = None, **fields):
        self.eng, self.nchan = eng, int(nchan)
        self.desc = desc if desc is not None else self.desc_for(**fields)
        self._create("jamd_adin_create", eng.h, C.byref(self.desc), self.nchan)

    @staticmethod
    def desc_for(fir_3to4=None, fir_2to1=None, down48=None, level_coef: float = 1.0, strip_zero: bool = True,
                 zmean: bool = False) -> AdinDesc:
        """jamd_adin_default(), then the fields given; down48 defaults to whether tables were passed."""
        d = AdinDesc()
        _call("jamd_adin_default", C.byref(d))
        d._keep = []                             # (the descriptor borrows the tables)
        for name, t in (("3to4", fir_3to4), ("2to1", fir_2to1)):
            if t is not None:
                t = np.ascontiguousarray(t, dtype=np.float64)
                d._keep.append(t)
                setattr(d, "fir_" + name, t.ctypes.data)
                setattr(d, "n_" + name, len(t))
        d.down48 = int((fir_3to4 is not None and fir_2to1 is not None) if down48 is None else down48)
        d.level_coef, d.strip_zero, d.zmean = float(level_coef), int(bool(strip_zero)), int(bool(zmean))
        return d

    def ds_count(self, samples_before: int, chunk: int) -> int:
        """16 kHz samples a push of `chunk` 48 kHz samples completes behind samples_before (host only)."""
        return _count("jamd_adin_ds_count", C.byref(self.desc), int(samples_before), int(chunk))

    def push_cap(self, samples_before: int, chunk: int) -> int:
        return _count("jamd_adin_push_cap", C.byref(self.desc), int(samples_before), int(chunk))

    def reset(self, mask=None, what: int = ADIN_DS | ADIN_ZMEAN, stream: int = 0):
        _call("jamd_adin_reset", self.h, _ptr(_mask(mask, self.nchan)), int(what), stream or None)

    def push_host(self, chunks):
        """One int16 chunk per channel (empty = idle) -> (conditioned samples back to back, out_off int64 [nchan + 1])."""
        assert len(chunks) == self.nchan
        samples, off = pack_chunks(chunks)
        cap = sum(self.push_cap(int(self.state(c)[2][0]), len(chunks[c])) for c in range(self.nchan)) \
            if self.desc.down48 else len(samples)
        out = np.zeros(max(cap, 1), np.int16)
        ooff = np.zeros(self.nchan + 1, np.int64)
        _call("jamd_adin_push_host", self.h, samples.ctypes.data if len(samples) else None, off.ctypes.data,
              out.ctypes.data, ooff.ctypes.data)
        return out[:int(ooff[-1])].copy(), ooff

    def push_dev(self, dev_in: int, in_off, dev_out: int, stream: int = 0):
        """Device samples in and out; in_off host int64 [nchan + 1].  Returns out_off int64 [nchan + 1]: with dev_out
        what Frontend.run_dev() / LiveFrontend.push_dev() take as dev_samples and sample_off."""
        off = _off64(in_off, self.nchan)
        ooff = np.zeros(self.nchan + 1, np.int64)
        _call("jamd_adin_push_dev", self.h, dev_in or None, off.ctypes.data, dev_out or None, ooff.ctypes.data,
              stream or None)
        return ooff

    def state(self, chan: int):
        """(zlen, zmean, arrived [3], emitted [3]) of one channel, after everything queued."""
        zl, zm = C.c_int(0), C.c_float(0)
        arr, emi = np.zeros(3, np.int64), np.zeros(3, np.int64)
        _call("jamd_adin_state_get", self.h, int(chan), C.addressof(zl), C.addressof(zm), arr.ctypes.data,
              emi.ctypes.data)
        return zl.value, np.float32(zm.value), arr, emi


class AdinCut(_Handle):
    """Silence cutting between Adin and LiveFrontend (jamd_adin_cut): the trigger / head margin / tail margin / swap
    buffer logic of adin_cut() (libjulius/src/adin-cut.c:600-984) around count_zc_e(), for many channels per call, with
    every channel's state and the last samples of its stream kept on the device.  A push hands back the samples the
    reference would have passed on by then, cut into parts at segment ends; each part's row of offsets and final flags
    is one LiveFrontend.push_dev()."""
    _destroy = "jamd_adin_cut_destroy"

    def __init__(self, eng: Engine, nchan: int, desc: "AdinCutDesc | None" = None, fvad: "AdinCutFvad | None" = None,
                 **fields):
        """fvad (AdinCut.fvad_for()): the libfvad detector gates the trigger, as -fvad / -fvad_param do."""
        self.eng, self.nchan = eng, int(nchan)
        self.desc = desc if desc is not None else self.desc_for(**fields)
        self.fvad = fvad
        if fvad is None:
            self._create("jamd_adin_cut_create", eng.h, C.byref(self.desc), self.nchan)
        else:
            self._create("jamd_adin_cut_create_fvad", eng.h, C.byref(self.desc), C.byref(fvad), self.nchan)

    @staticmethod
    def fvad_for(model, mode: int, smoothnum: int = 5, thres: float = 0.5, sfreq: int = 16000) -> AdinCutFvad:
        """-fvad `mode` -fvad_param `smoothnum` `thres` with the caller's model (FvadModel)."""
        f = AdinCutFvad(FvadDesc(int(sfreq), int(mode), C.pointer(model) if model is not None else None), int(smoothnum),
                        float(thres))
        f._keep = model                          # (the descriptor borrows the model)
        return f

    def fvad_reset(self, mask=None, stream: int = 0):
        """A fresh detector for the channels of mask (None: all); the cutting state stays."""
        _call("jamd_adin_cut_fvad_reset", self.h, _ptr(_mask(mask, self.nchan)), stream or None)

    def fvad_state(self, chan: int) -> np.ndarray:
        """The detector of one channel as Fvad.state() gives it."""
        out = np.zeros(FVAD_STATE_INTS, np.int32)
        _call("jamd_adin_cut_fvad_state_get", self.h, int(chan), out.ctypes.data)
        return out

    @staticmethod
    def desc_for(**fields) -> AdinCutDesc:
        """jamd_adin_cut_default(), then the fields given (sfreq, level_thres, zero_cross_num, head_margin_msec,
        tail_margin_msec, chunk_size)."""
        d = AdinCutDesc()
        _call("jamd_adin_cut_default", C.byref(d))
        names = [f[0] for f in AdinCutDesc._fields_]
        for key, v in fields.items():
            if key not in names:
                raise TypeError(f"AdinCutDesc has no field {key!r}")
            setattr(d, key, int(v))
        return d

    def params(self):
        """(c_length, noise_zerocross, nc_max, sbsize) as adin_setup_param() computes them."""
        v = [C.c_int(0) for _ in range(4)]
        _call("jamd_adin_cut_params", C.byref(self.desc), *[C.addressof(x) for x in v])
        return tuple(x.value for x in v)

    def push_cap(self, chunk: int) -> int:
        return _count("jamd_adin_cut_push_cap", C.byref(self.desc), int(chunk))

    def parts_cap(self, chunk: int) -> int:
        return _count("jamd_adin_cut_parts_cap", C.byref(self.desc), int(chunk))

    def reset(self, mask=None, stream: int = 0):
        _call("jamd_adin_cut_reset", self.h, _ptr(_mask(mask, self.nchan)), stream or None)

    def _eos(self, eos):
        return _mask(eos, self.nchan)

    def _tables(self, max_parts):
        return (np.zeros((max_parts, self.nchan + 1), np.int64), np.zeros((max_parts, self.nchan), np.uint8),
                np.full((max_parts, self.nchan), -1, np.int64))

    def push_host(self, chunks, eos=None, max_parts=None):
        """One int16 chunk per channel (empty = none), `eos` marks the channels whose stream ends behind it ->
        (samples, part_off [nparts][nchan + 1], part_final [nparts][nchan], part_start [nparts][nchan])."""
        assert len(chunks) == self.nchan
        samples, off = pack_chunks(chunks)
        m = self._eos(eos)
        lens = [len(c) for c in chunks]
        if max_parts is None:
            max_parts = max(self.parts_cap(n) for n in lens)
        out = np.zeros(sum(self.push_cap(n) for n in lens), np.int16)
        poff, pfin, pst = self._tables(int(max_parts))
        np_ = C.c_int(0)
        _call("jamd_adin_cut_push_host", self.h, samples.ctypes.data if len(samples) else None, off.ctypes.data,
              _ptr(m), out.ctypes.data, int(max_parts), C.addressof(np_), poff.ctypes.data, pfin.ctypes.data,
              pst.ctypes.data)
        n = np_.value
        total = int(poff[n - 1, -1]) if n else 0
        return out[:total].copy(), poff[:n].copy(), pfin[:n].copy(), pst[:n].copy()

    def push_dev(self, dev_in: int, in_off, dev_out: int, eos=None, max_parts=None, stream: int = 0):
        """Device samples in and out; in_off host int64 [nchan + 1].  Returns (part_off [nparts][nchan + 1], part_final
        [nparts][nchan], part_start [nparts][nchan]): with dev_out, rows of the first two are what
        LiveFrontend.push_dev() takes as sample_off and final."""
        off = _off64(in_off, self.nchan)
        m = self._eos(eos)
        if max_parts is None:
            max_parts = max(self.parts_cap(int(off[c + 1] - off[c])) for c in range(self.nchan))
        poff, pfin, pst = self._tables(int(max_parts))
        np_ = C.c_int(0)
        _call("jamd_adin_cut_push_dev", self.h, dev_in or None, off.ctypes.data, _ptr(m), dev_out or None,
              int(max_parts), C.addressof(np_), poff.ctypes.data, pfin.ctypes.data, pst.ctypes.data, stream or None)
        n = np_.value
        return poff[:n].copy(), pfin[:n].copy(), pst[:n].copy()

    def state(self, chan: int):
        """(is_valid, nc, rest_tail, sblen, zero_cross, carried, stream_pos) of one channel, after everything queued."""
        v = [C.c_int(0) for _ in range(6)]
        pos = C.c_int64(0)
        _call("jamd_adin_cut_state_get", self.h, int(chan), *[C.addressof(x) for x in v], C.addressof(pos))
        return tuple(x.value for x in v) + (pos.value,)


class Fvad(_Handle):
    """The voice-activity detector behind -fvad (jamd_fvad): libfvad's decision for every 10 ms frame of many channels
    per call, bit for bit, with every channel's filter states, adapted models, minimum tracker, hangover and the samples
    of an incomplete frame kept on the device.  A push hands back one byte per completed frame: the core's raw value
    (0 noise, 1 speech, 2 + the hangover left)."""
    _destroy = "jamd_fvad_destroy"

    def __init__(self, eng: Engine, nchan: int, model: "FvadModel | None", sfreq: int = 16000, mode: int = 0):
        self.eng, self.nchan, self.model = eng, int(nchan), model
        self.desc = self.desc_for(model, sfreq, mode)
        self._create("jamd_fvad_create", eng.h, C.byref(self.desc), self.nchan)

    @staticmethod
    def desc_for(model, sfreq: int = 16000, mode: int = 0) -> FvadDesc:
        d = FvadDesc(int(sfreq), int(mode), C.pointer(model) if model is not None else None)
        d._keep = model                          # (the descriptor borrows the model)
        return d

    @staticmethod
    def frames(sfreq: int, samples_before: int, chunk: int) -> int:
        """Frames a push of `chunk` samples completes behind samples_before (host only)."""
        d = FvadDesc(int(sfreq), 0, None)
        return _count("jamd_fvad_frames", C.byref(d), int(samples_before), int(chunk))

    def reset(self, mask=None, stream: int = 0):
        _call("jamd_fvad_reset", self.h, _ptr(_mask(mask, self.nchan)), stream or None)

    def push_host(self, chunks):
        """One int16 chunk per channel (empty = idle) -> (raw values back to back uint8, out_off int64 [nchan + 1])."""
        assert len(chunks) == self.nchan
        samples, off = pack_chunks(chunks)
        out = np.zeros(len(samples) // (self.desc.sfreq // 100) + self.nchan + 1, np.uint8)
        ooff = np.zeros(self.nchan + 1, np.int64)
        _call("jamd_fvad_push_host", self.h, samples.ctypes.data if len(samples) else None, off.ctypes.data,
              out.ctypes.data, ooff.ctypes.data)
        return out[:int(ooff[-1])].copy(), ooff

    def push_dev(self, dev_in: int, in_off, dev_out: int, stream: int = 0):
        """Device samples in, device bytes out; in_off host int64 [nchan + 1].  Returns out_off int64 [nchan + 1]."""
        off = _off64(in_off, self.nchan)
        ooff = np.zeros(self.nchan + 1, np.int64)
        _call("jamd_fvad_push_dev", self.h, dev_in or None, off.ctypes.data, dev_out or None, ooff.ctypes.data,
              stream or None)
        return ooff

    def state(self, chan: int) -> np.ndarray:
        """One channel's core as int32 [FVAD_STATE_INTS], in the order stated in julius_amd.h, after everything queued."""
        out = np.zeros(FVAD_STATE_INTS, np.int32)
        _call("jamd_fvad_state_get", self.h, int(chan), out.ctypes.data)
        return out
