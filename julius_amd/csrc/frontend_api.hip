// frontend_api.hip -- the C ABI of the buffered audio front end (jamd_frontend_*): descriptor and table entries over
// frontend_tables.h, validation, the object and its scratch, the offset tables of a call, spectral subtraction's
// settings and files.  It launches nothing: the kernels and their launchers are in frontend.hip (frontend_host.h).
#include "frontend_host.h"
#include "ss_file.h"

// The device side of a created object: its tables, FeParams, the LDS reservation.
static int fe_init_device(jamd_frontend *f, const jamd_frontend_desc *d) {
  JAMD_HIP(hipSetDevice(f->eng->device));
  FeParams &p = f->p;
  const FeTables &w = f->tb;
  p.framesize = d->framesize; p.frameshift = d->frameshift; p.fftN = w.fftN; p.logn = w.n;
  p.klo = w.klo; p.khi = w.khi; p.fbank_num = d->fbank_num; p.mfcc_dim = d->mfcc_dim; p.baselen = d->baselen;
  p.veclen = d->veclen; p.splice = d->splice;
  p.zmean = d->zmeanframe != 0; p.energy = d->energy != 0; p.raw_e = d->raw_e != 0; p.c0 = d->c0 != 0;
  p.fbank_only = d->basetype != JAMD_F_MFCC; p.log_fbank = d->basetype != JAMD_F_MELSPEC; p.usepower = d->usepower != 0;
  p.enormal = d->enormal != 0; p.delta = d->delta; p.acc = d->acc; p.absesup = d->absesup;
  p.delWin = d->delWin; p.accWin = d->accWin; p.cmn = d->cmn != 0; p.cvn = d->cvn != 0;
  p.basedim = d->mfcc_dim + (d->c0 ? 1 : 0);
  p.preEmph = d->preEmph; p.sqrt2var = w.sqrt2var; p.escale = d->escale; p.silFloor = d->silFloor;
  // CMN() takes cmean_init whenever it is set; MVN() does unless static_cvn_only, which keeps only the variance
  p.cmean_static = d->cmean_init && (!p.cvn || !d->static_cvn_only);
  p.cvar_static = p.cvn && d->cmean_init != nullptr;
  int rc;
#define FE_UP(field, vec)                                                                    \
  if ((rc = f->t_##field.upload((vec).data(), (vec).size())) != JAMD_OK) return rc;         \
  p.field = f->t_##field;
  FE_UP(ham, w.ham)
  FE_UP(twRe, w.twRe)
  FE_UP(twIm, w.twIm)
  FE_UP(dct, w.dct)
  FE_UP(wcep, w.wcep)
  FE_UP(loChan, w.loChan)
  FE_UP(loWt, w.loWt)
  FE_UP(kfirst, w.kfirst)
  FE_UP(klast, w.klast)
  if (p.cmean_static) {
    std::vector<float> cm(d->cmean_init, d->cmean_init + p.basedim);
    FE_UP(cmean, cm)
  }
  if (p.cvar_static) {
    std::vector<double> cs(d->veclen);
    for (int i = 0; i < d->veclen; i++) cs[i] = sqrt(d->cvar_init[i]);   // sqrt(c->cvar_init[i]) in double
    FE_UP(cvar_sqrt, cs)
  }
#undef FE_UP
  return fe_reserve_lds(f);
}

// Head frames of every utterance (head_samples <= 0: the whole utterance) -> hoff [nutt + 1]; false with the error
// set when the spectra of the batch pass an int, sample_off is not in order or a head holds no full frame.
static bool fe_head_frames(const jamd_frontend *f, const char *who, const int64_t *sample_off, int nutt,
                           long long head_samples, std::vector<int> &hoff) {
  if ((long long)nutt * f->tb.fftN > 0x7fffffffLL) { jamd_set_error("%s: batch too large", who); return false; }
  hoff.assign(nutt + 1, 0);
  std::string err;
  long long Hall = 0;
  for (int u = 0; u < nutt; u++) {
    long long n = fe_span(who, "utterance", sample_off, u, err);
    if (n < 0) { jamd_refuse("%s", err.c_str()); return false; }
    if (head_samples > 0 && head_samples < n) n = head_samples;
    const long long H = fe_frames_raw(f->d, n);
    if (H < 1) {
      jamd_set_error("%s: the head of utterance %d (%lld samples) holds no full frame", who, u, n);
      return false;
    }
    hoff[u] = (int)Hall;
    Hall += H;
    if (Hall > 0x7fffffffLL) { jamd_set_error("%s: batch too large (%lld head frames)", who, Hall); return false; }
  }
  hoff[nutt] = (int)Hall;
  return true;
}

extern "C" {

int jamd_frontend_set_kind(jamd_frontend_desc *d, int param_type, int vec_size) {
  if (!d) return jamd_refuse("jamd_frontend_set_kind: d is NULL");
  fe_set_kind(d, param_type, vec_size);
  return JAMD_OK;
}

int jamd_frontend_default_desc(int param_type, int vec_size, jamd_frontend_desc *d) {
  if (!d) return jamd_refuse("jamd_frontend_default_desc: d is NULL");
  fe_default_desc(param_type, vec_size, d);
  return JAMD_OK;
}

int jamd_frontend_htkconf(const char *path, jamd_frontend_desc *para) {
  if (!path || !para) return jamd_refuse("jamd_frontend_htkconf: NULL argument");
  std::string err;
  return fe_htkconf(path, para, err) ? JAMD_OK : jamd_refuse("%s", err.c_str());
}

int jamd_frontend_table(const jamd_frontend_desc *d, const char *name, void *out, int cap) {
  if (!d || !name) return jamd_refuse("jamd_frontend_table: NULL argument");
  std::string err;
  const int n = fe_table(d, name, out, cap, err);
  return n < 0 ? jamd_refuse("%s", err.c_str()) : n;
}

void jamd_frontend_destroy(jamd_frontend *f) {
  if (!f) return;
  delete f;                                  // (the engine is not looked at: it may have gone first)
}

int jamd_frontend_create(jamd_engine *e, const jamd_frontend_desc *d, jamd_frontend **out) {
  if (!e || !d || !out) return jamd_refuse("jamd_frontend_create: NULL argument");
  *out = nullptr;
  if (d->ss)
    return jamd_refuse("jamd_frontend_create: ss != 0 in the descriptor, which carries none of the parameters of spectral "
                     "subtraction: leave it 0 and call jamd_frontend_set_ss() on the created object");
  if (d->realtime) return jamd_refuse("jamd_frontend_create: realtime input / MAP-CMN is not served (buffered front end only)");
  if (d->basetype != JAMD_F_MFCC && d->basetype != JAMD_F_FBANK && d->basetype != JAMD_F_MELSPEC)
    return jamd_refuse("jamd_frontend_create: parameter kind %d is not MFCC, FBANK or MELSPEC", d->basetype);
  if (d->basetype != JAMD_F_MFCC && (d->energy || d->c0))
    return jamd_refuse("jamd_frontend_create: _E / _0 with a filter-bank kind (the reference leaves those slots unset)");
  if ((d->absesup && !(d->energy && d->delta)) || (d->acc && !d->delta))
    return jamd_refuse("jamd_frontend_create: _N needs _E and _D, _A needs _D");
  if (d->mfcc_dim < 1 || d->veclen < 1 || d->splice < 1 || d->delWin < 1 || (d->acc && d->accWin < 1))
    return jamd_refuse("jamd_frontend_create: kind 0x%x with vector size %d gives %d cepstra (splice %d, windows %d/%d)",
                     d->paramtype, d->vecsize, d->mfcc_dim, d->splice, d->delWin, d->accWin);
  if (d->cvn && d->cmean_init && !d->cvar_init) return jamd_refuse("jamd_frontend_create: static CVN needs cvar_init");
  std::unique_ptr<jamd_frontend> f(new jamd_frontend());   // (its members own what they hold)
  f->eng = e;
  f->d = *d;
  f->d.cmean_init = nullptr; f->d.cvar_init = nullptr;
  std::string err;
  if (!fe_build_tables(d, f->tb, err)) return jamd_refuse("%s", err.c_str());
  int rc;
  if ((rc = fe_init_device(f.get(), d)) != JAMD_OK) return rc;
  *out = f.release();
  return JAMD_OK;
}

int jamd_frontend_veclen(const jamd_frontend *f) { return f ? f->d.veclen * f->d.splice : JAMD_EINVAL; }

int jamd_frontend_frames(const jamd_frontend_desc *d, int64_t nsamples) {
  if (!d || d->framesize < 1 || d->frameshift < 1 || d->splice < 1)
    return jamd_refuse("jamd_frontend_frames: NULL descriptor, or framesize / frameshift / splice < 1");
  long long T = fe_frames_raw(*d, nsamples) - (d->splice - 1);
  return T > 0x7fffffff ? 0x7fffffff : (int)T;
}

int jamd_frontend_fftn(const jamd_frontend *f) { return f ? f->tb.fftN : JAMD_EINVAL; }

int jamd_frontend_ss_default(jamd_frontend_ss *ss) {
  if (!ss) return jamd_refuse("jamd_frontend_ss_default: ss is NULL");
  // default.c:158-162 with DEF_SSALPHA / DEF_SSFLOOR of mfcc.h:68-69
  ss->mode = JAMD_SS_OFF; ss->calc_len_ms = 300;
  ss->alpha = 2.0f; ss->floor = 0.5f;
  ss->noise = nullptr; ss->noise_len = 0;
  return JAMD_OK;
}

int jamd_frontend_set_ss(jamd_frontend *f, const jamd_frontend_ss *ss) {
  if (!f || !ss) return jamd_refuse("jamd_frontend_set_ss: NULL argument");
  long long head = 0;
  if (ss->mode == JAMD_SS_CALC) {
    // m_fusion.c:1409: the head must hold a frame (the reference's product is an int; one past int is refused here)
    head = (long long)ss->calc_len_ms * f->d.smp_freq / 1000;
    if (head < f->d.framesize || (long long)ss->calc_len_ms * f->d.smp_freq > 0x7fffffffLL)
      return jamd_refuse("jamd_frontend_set_ss: head length for SS (%d msec = %lld samples) is shorter than a frame (%d "
                       "samples), or out of range", ss->calc_len_ms, head, f->d.framesize);
  } else if (ss->mode == JAMD_SS_LOAD) {
    if (!ss->noise || ss->noise_len != f->tb.fftN)   // Wav2MFCC() refuses ssbuflen != fftN (wav2mfcc-buffer.c:64-69)
      return jamd_refuse("jamd_frontend_set_ss: JAMD_SS_LOAD needs a noise spectrum of fftN = %d values (got %s, length %d)",
                       f->tb.fftN, ss->noise ? "one" : "NULL", ss->noise_len);
    JAMD_HIP(hipSetDevice(f->eng->device));
    // a buffer of its own per upload: a run queued earlier keeps reading the spectrum it was launched with
    JamdDev<float> q;
    int rc;
    if ((rc = q.upload(ss->noise, f->tb.fftN)) != JAMD_OK) return rc;
    f->d_ssload.swap(q);                           // (the old one goes with q: hipFree waits for the device)
  } else if (ss->mode != JAMD_SS_OFF)
    return jamd_refuse("jamd_frontend_set_ss: unknown mode %d (JAMD_SS_OFF, JAMD_SS_CALC, JAMD_SS_LOAD)", ss->mode);
  f->ss_mode = ss->mode; f->ss_head = head;
  f->ss_alpha = ss->alpha; f->ss_floor = ss->floor;
  return JAMD_OK;
}

int jamd_frontend_ss_read(const char *path, float *out, int cap) {
  if (!path || (cap > 0 && !out)) return jamd_refuse("jamd_frontend_ss_read: NULL argument");
  std::string err;
  const int n = ssf_read(path, out, cap > 0 ? cap : 0, err);
  if (n < 0) return jamd_refuse("jamd_frontend_ss_read: %s", err.c_str());
  return n;
}

int jamd_frontend_ss_write(const char *path, const float *noise, int n) {
  if (!path || !noise || n < 0) return jamd_refuse("jamd_frontend_ss_write: NULL argument or n < 0");
  std::string err;
  if (ssf_write(path, noise, n, err) != 0) return jamd_refuse("jamd_frontend_ss_write: %s", err.c_str());
  return JAMD_OK;
}

int jamd_frontend_noise_dev(jamd_frontend *f, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                            int64_t head_samples, float *dev_noise, void *stream) {
  if (!f || !dev_samples || !sample_off || !dev_noise || nutt < 1)
    return jamd_refuse("jamd_frontend_noise_dev: NULL argument or nutt < 1");
  std::vector<int> hoff;
  if (!fe_head_frames(f, "jamd_frontend_noise_dev", sample_off, nutt, head_samples, hoff)) return JAMD_EINVAL;
  JAMD_HIP(hipSetDevice(f->eng->device));
  hipStream_t st = jamd_stream(f->eng, stream);
  int rc;
  if ((rc = fe_put_offsets(f, st, sample_off, nutt, {&hoff})) != JAMD_OK) return rc;
  const long long *d_soff = (const long long *)f->off.d.p;
  return fe_launch_noise(f, st, dev_samples, d_soff, (const int *)(d_soff + nutt + 1), nutt, hoff[nutt], dev_noise);
}

int jamd_frontend_noise_host(jamd_frontend *f, const int16_t *samples, const int64_t *sample_off, int nutt,
                             int64_t head_samples, float *noise) {
  if (!f || !samples || !sample_off || !noise || nutt < 1)
    return jamd_refuse("jamd_frontend_noise_host: NULL argument or nutt < 1");
  std::vector<int> hoff;
  if (!fe_head_frames(f, "jamd_frontend_noise_host", sample_off, nutt, head_samples, hoff)) return JAMD_EINVAL;
  return jamd_host_call(&f->stage, f->eng, samples, (size_t)sample_off[nutt], noise, (size_t)nutt * f->tb.fftN,
                      [&](const int16_t *in, float *o, hipStream_t st) -> long long {
                        const int rc = jamd_frontend_noise_dev(f, in, sample_off, nutt, head_samples, o, st);
                        return rc != JAMD_OK ? rc : (long long)nutt * f->tb.fftN;
                      });
}

int jamd_frontend_run_dev(jamd_frontend *f, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                          float *dev_out, int *frame_off, void *stream) {
  if (!f || !dev_samples || !sample_off || !dev_out || nutt < 1)
    return jamd_refuse("jamd_frontend_run_dev: NULL argument or nutt < 1");
  const jamd_frontend_desc &d = f->d;
  std::vector<int> foff(nutt + 1), ooff(nutt + 1);
  std::string err;
  long long Tall = 0, Tout = 0;
  for (int u = 0; u < nutt; u++) {
    const long long n = fe_span("jamd_frontend_run_dev", "utterance", sample_off, u, err);
    if (n < 0) return jamd_refuse("%s", err.c_str());
    long long T = fe_frames_raw(d, n);
    if (T - (d.splice - 1) < 1) return jamd_refuse("jamd_frontend_run_dev: utterance %d too short (%lld samples)", u, n);
    foff[u] = (int)Tall; ooff[u] = (int)Tout;
    Tall += T; Tout += T - (d.splice - 1);
    if ((Tall + 1) * (long long)d.vecbuflen * d.splice > 0x7fffffffLL)
      return jamd_refuse("jamd_frontend_run_dev: batch too large (%lld frames)", Tall);
  }
  foff[nutt] = (int)Tall; ooff[nutt] = (int)Tout;
  const bool calc = f->ss_mode == JAMD_SS_CALC;
  std::vector<int> hoff;                     // -sscalc: the head frames (every utterance holds a frame, so its head does)
  if (calc && !fe_head_frames(f, "jamd_frontend_run_dev", sample_off, nutt, f->ss_head, hoff)) return JAMD_EINVAL;
  JAMD_HIP(hipSetDevice(f->eng->device));
  hipStream_t st = jamd_stream(f->eng, stream);
  int rc;
  if ((rc = f->d_stat.grow((size_t)Tall * d.baselen * sizeof(float))) != JAMD_OK) return rc;
  if ((rc = f->d_feat.grow((size_t)Tall * d.veclen * sizeof(float))) != JAMD_OK) return rc;
  if ((rc = f->d_ms.grow((size_t)nutt * (2 * d.veclen + 1) * sizeof(float))) != JAMD_OK) return rc;
  if (calc) rc = fe_put_offsets(f, st, sample_off, nutt, {&foff, &ooff, &hoff});
  else rc = fe_put_offsets(f, st, sample_off, nutt, {&foff, &ooff});
  if (rc != JAMD_OK) return rc;
  const long long *d_soff = (const long long *)f->off.d.p;
  const int *d_foff = (const int *)(d_soff + nutt + 1), *d_ooff = d_foff + nutt + 1;
  if (calc) {                                // the spectrum of every utterance's head first, on this stream
    if ((rc = f->d_noise.grow((size_t)nutt * f->tb.fftN * sizeof(float))) != JAMD_OK) return rc;
    if ((rc = fe_launch_noise(f, st, dev_samples, d_soff, d_ooff + nutt + 1, nutt, hoff[nutt], f->d_noise)) != JAMD_OK)
      return rc;
  }
  if ((rc = fe_launch_frames(f, st, dev_samples, d_soff, d_foff, nutt, (int)Tall)) != JAMD_OK) return rc;
  if ((rc = fe_launch_feats(f, st, d_foff, d_ooff, nutt, (int)Tall, Tout, dev_out)) != JAMD_OK) return rc;
  if (frame_off) memcpy(frame_off, ooff.data(), sizeof(int) * (nutt + 1));
  return JAMD_OK;
}

int jamd_frontend_run_host(jamd_frontend *f, const int16_t *samples, const int64_t *sample_off, int nutt, float *out,
                           int *frame_off) {
  if (!f || !samples || !sample_off || !out || nutt < 1)
    return jamd_refuse("jamd_frontend_run_host: NULL argument or nutt < 1");
  std::string err;
  long long Tout = 0;
  for (int u = 0; u < nutt; u++) {
    const long long n = fe_span("jamd_frontend_run_host", "utterance", sample_off, u, err);
    if (n < 0) return jamd_refuse("%s", err.c_str());
    const int T = jamd_frontend_frames(&f->d, n);
    if (T < 1) return jamd_refuse("jamd_frontend_run_host: utterance %d too short (%lld samples)", u, n);
    Tout += T;
  }
  return jamd_host_call(&f->stage, f->eng, samples, (size_t)sample_off[nutt], out, (size_t)Tout * f->d.veclen * f->d.splice,
                      [&](const int16_t *in, float *o, hipStream_t st) -> long long {
                        const int rc = jamd_frontend_run_dev(f, in, sample_off, nutt, o, frame_off, st);
                        return rc != JAMD_OK ? rc : Tout * f->d.veclen * f->d.splice;
                      });
}

}  // extern "C"
