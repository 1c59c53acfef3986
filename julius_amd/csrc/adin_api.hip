// adin_api.hip -- the C ABI of the audio conditioning stage (jamd_adin_*): validation, the object and the per-channel
// state it keeps on the device, the tables of a push (counts from adin_plan.h), the coefficient file.  It launches
// nothing: the kernels and their launchers are in adin.hip (adin_host.h).
#include "adin_host.h"

extern "C" {

int jamd_adin_default(jamd_adin_desc *d) {
  if (!d) return jamd_refuse("jamd_adin_default: d is NULL");
  d->down48 = 0; d->fir_3to4 = nullptr; d->n_3to4 = 0; d->fir_2to1 = nullptr; d->n_2to1 = 0;
  d->level_coef = 1.0f;
  d->strip_zero = 1;                         // default.c:92
  d->zmean = 0;
  return JAMD_OK;
}

int jamd_adin_fir_read(const char *path, double *out, int cap) {
  if (!path || !out || cap < 1) return jamd_refuse("jamd_adin_fir_read: NULL argument or cap < 1");
  std::string err;
  const int n = ad_fir_read(path, out, cap, err);
  if (n < 0) return jamd_refuse("jamd_adin_fir_read: %s: %s", path, err.c_str());
  return n;
}

int64_t jamd_adin_ds_count(const jamd_adin_desc *d, int64_t samples_before, int64_t chunk) {
  std::string err;
  if (!ad_check_desc(d, false, err)) return jamd_refuse("jamd_adin_ds_count: %s", err.c_str());
  if (samples_before < 0 || chunk < 0) return jamd_refuse("jamd_adin_ds_count: a negative sample count");
  if (!d->down48) return chunk;
  const AdCascade c = ad_cascade(d->n_3to4, d->n_2to1);
  return ad_cascade_emitted(c, samples_before + chunk) - ad_cascade_emitted(c, samples_before);
}

int64_t jamd_adin_push_cap(const jamd_adin_desc *d, int64_t samples_before, int64_t chunk) {
  return jamd_adin_ds_count(d, samples_before, chunk);
}

void jamd_adin_destroy(jamd_adin *a) {
  if (!a) return;
  delete a;                                  // (the engine is not looked at: it may have gone first)
}

int jamd_adin_create(jamd_engine *e, const jamd_adin_desc *d, int nchan, jamd_adin **out) {
  if (!e || !d || !out || nchan < 1) return jamd_refuse("jamd_adin_create: NULL argument or nchan < 1");
  *out = nullptr;
  std::string err;
  if (!ad_check_desc(d, true, err)) return jamd_refuse("jamd_adin_create: %s", err.c_str());
  std::unique_ptr<jamd_adin> a(new jamd_adin());   // (its members own what they hold)
  a->eng = e; a->nchan = nchan; a->d = *d;
  a->d.fir_3to4 = nullptr; a->d.fir_2to1 = nullptr;
  a->d.strip_zero = d->strip_zero != 0; a->d.zmean = d->zmean != 0; a->d.down48 = d->down48 != 0;
  const size_t C = nchan;
  int rc;
  JAMD_HIP(hipSetDevice(e->device));
  if ((rc = a->d_zlen.alloc(C, true)) != JAMD_OK || (rc = a->d_zmean.alloc(C, true)) != JAMD_OK ||
      (rc = a->d_cnt.alloc(C)) != JAMD_OK || (rc = a->d_ooff.alloc(C + 1)) != JAMD_OK || (rc = a->d_mask.alloc(C)) != JAMD_OK ||
      (rc = a->h_ooff.grow((C + 1) * sizeof(long long))) != JAMD_OK)
    return rc;
  if (a->d.down48) {
    a->cas = ad_cascade(d->n_3to4, d->n_2to1);
    const double *src[2] = {d->fir_3to4, d->fir_2to1};
    const int ns[2] = {d->n_3to4, d->n_2to1};
    for (int i = 0; i < 2; i++) {
      if ((rc = a->d_fir[i].alloc(kAdMaxTaps, true)) != JAMD_OK) return rc;
      JAMD_HIP(hipMemcpy(a->d_fir[i], src[i], ns[i] * sizeof(double), hipMemcpyHostToDevice));
    }
    for (int s = 0; s < 3; s++) {            // the samples before the stream start: 0.0
      if ((rc = a->d_hist[s].alloc(C * (a->cas.st[s].hist + kAdBlock - 1), true)) != JAMD_OK) return rc;
      a->arrived[s].assign(nchan, 0);
    }
  }
  *out = a.release();
  return JAMD_OK;
}

int jamd_adin_reset(jamd_adin *a, const unsigned char *mask, int what, void *stream) {
  if (!a || !(what & (JAMD_ADIN_DS | JAMD_ADIN_ZMEAN)) || (what & ~(JAMD_ADIN_DS | JAMD_ADIN_ZMEAN)))
    return jamd_refuse("jamd_adin_reset: NULL object, or `what` is not JAMD_ADIN_DS | JAMD_ADIN_ZMEAN or one of them");
  JAMD_HIP(hipSetDevice(a->eng->device));
  hipStream_t st = jamd_stream(a->eng, stream);
  // (a copy from pageable memory has left the host array when the call returns)
  if (mask) JAMD_HIP(hipMemcpyAsync(a->d_mask, mask, (size_t)a->nchan, hipMemcpyHostToDevice, st));
  int rc;
  if ((rc = ad_launch_reset(a, st, mask ? a->d_mask : nullptr, what)) != JAMD_OK) return rc;
  if ((what & JAMD_ADIN_DS) && a->d.down48)
    for (int c = 0; c < a->nchan; c++)
      if (!mask || mask[c])
        for (int s = 0; s < 3; s++) a->arrived[s][c] = 0;
  return JAMD_OK;
}

int jamd_adin_push_dev(jamd_adin *a, const int16_t *dev_in, const int64_t *in_off, int16_t *dev_out, int64_t *out_off,
                       void *stream) {
  if (!a || !in_off || !out_off) return jamd_refuse("jamd_adin_push_dev: NULL argument");
  const int nchan = a->nchan;
  const bool ds = a->d.down48 != 0;
  const size_t nst = ds ? 3 * (size_t)nchan : 0, ntab = nst * sizeof(AdStageTab) + nchan * sizeof(AdChanTab);
  int rc;
  JAMD_HIP(hipSetDevice(a->eng->device));
  if ((rc = a->tab.begin(ntab)) != JAMD_OK) return rc;
  AdStageTab *h_st = (AdStageTab *)a->tab.h.p;
  AdChanTab *h_ch = (AdChanTab *)(h_st + nst);
  std::vector<long long> after[3];
  if (ds) for (int s = 0; s < 3; s++) after[s] = a->arrived[s];
  long long M[3] = {0, 0, 0}, pre = 0;       // outputs of the three stages, samples behind them, over all channels
  int max_raw[3] = {0, 0, 0}, max_n = 0;
  for (int c = 0; c < nchan; c++) {
    long long n;
    if ((rc = jamd_span("jamd_adin_push_dev", in_off, c, &n)) != JAMD_OK) return rc;
    long long src = in_off[c];
    if (ds) {
      for (int s = 0; s < 3; s++) {
        const AdPush p = ad_push(a->cas.st[s], a->arrived[s][c], n);
        h_st[s * nchan + c] = AdStageTab{src, M[s], p.n_in, p.pend, p.t_b, p.n_raw, p.drop, p.adv};
        after[s][c] += n;
        if (p.n_raw > max_raw[s]) max_raw[s] = p.n_raw;
        src = M[s]; M[s] += p.n_out; n = p.n_out;
      }
    }
    h_ch[c] = AdChanTab{src, pre, (int)n, 0};
    pre += n;
    if (n > max_n) max_n = (int)n;
  }
  if ((in_off[nchan] > 0 && !dev_in) || (pre > 0 && !dev_out)) return jamd_refuse("jamd_adin_push_dev: NULL buffer");
  hipStream_t st = jamd_stream(a->eng, stream);
  if (ds) {
    for (int s = 0; s < 2; s++)
      if ((rc = a->d_mid[s].grow((size_t)(M[s] > 0 ? M[s] : 1) * sizeof(double))) != JAMD_OK) return rc;
    if ((rc = a->d_ds.grow((size_t)(M[2] > 0 ? M[2] : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  }
  if ((rc = a->d_pre.grow((size_t)(pre > 0 ? pre : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if (in_off[nchan] > in_off[0]) {           // a push without a sample anywhere leaves every channel idle
    if ((rc = a->tab.send(ntab, st)) != JAMD_OK) return rc;
    const AdStageTab *d_st = (const AdStageTab *)a->tab.d.p;
    const AdChanTab *d_ch = (const AdChanTab *)(d_st + nst);
    if (ds) {
      const void *in[3] = {dev_in, a->d_mid[0], a->d_mid[1]};
      void *out[3] = {a->d_mid[0], a->d_mid[1], a->d_ds};
      for (int s = 0; s < 3; s++)
        if (max_raw[s] > 0 && (rc = ad_launch_fir(a, st, s, d_st + s * nchan, in[s], out[s], max_raw[s])) != JAMD_OK) return rc;
      if ((rc = ad_launch_hist(a, st, d_st, dev_in)) != JAMD_OK) return rc;
      for (int s = 0; s < 3; s++) a->arrived[s].swap(after[s]);
    }
    if (max_n > 0 && (rc = ad_launch_post(a, st, d_ch, ds ? a->d_ds : dev_in, dev_out, max_n)) != JAMD_OK) return rc;
  }
  if (a->d.strip_zero && max_n > 0) {        // the counts are data
    JAMD_HIP(hipMemcpyAsync(a->h_ooff.p, a->d_ooff, (nchan + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    JAMD_HIP(hipStreamSynchronize(st));
    memcpy(out_off, a->h_ooff.p, (nchan + 1) * sizeof(long long));
  } else {
    for (int c = 0; c < nchan; c++) out_off[c] = h_ch[c].pre_off;
    out_off[nchan] = pre;
  }
  return JAMD_OK;
}

int jamd_adin_push_host(jamd_adin *a, const int16_t *samples, const int64_t *in_off, int16_t *out, int64_t *out_off) {
  if (!a || !in_off || !out_off) return jamd_refuse("jamd_adin_push_host: NULL argument");
  int rc;
  long long cap = 0;
  for (int c = 0; c < a->nchan; c++) {
    long long n;
    if ((rc = jamd_span("jamd_adin_push_host", in_off, c, &n)) != JAMD_OK) return rc;
    cap += a->d.down48 ? ad_cascade_emitted(a->cas, a->arrived[0][c] + n) - ad_cascade_emitted(a->cas, a->arrived[0][c]) : n;
  }
  const long long ns = in_off[a->nchan];
  if ((ns > 0 && !samples) || (cap > 0 && !out)) return jamd_refuse("jamd_adin_push_host: NULL buffer");
  return jamd_host_call(&a->stage, a->eng, samples, (size_t)(ns > 0 ? ns : 0), out, (size_t)cap,
                        [&](const int16_t *in, int16_t *o, hipStream_t st) -> long long {
                          const int r = jamd_adin_push_dev(a, in, in_off, o, out_off, st);
                          return r != JAMD_OK ? r : out_off[a->nchan];
                        });
}

int jamd_adin_state_get(jamd_adin *a, int chan, int *zlen, float *zmean, int64_t *arrived, int64_t *emitted) {
  if (!a || chan < 0 || chan >= a->nchan) return jamd_refuse("jamd_adin_state_get: NULL object or channel out of range");
  JAMD_HIP(hipSetDevice(a->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  if (zlen) JAMD_HIP(hipMemcpy(zlen, a->d_zlen + chan, sizeof(int), hipMemcpyDeviceToHost));
  if (zmean) JAMD_HIP(hipMemcpy(zmean, a->d_zmean + chan, sizeof(float), hipMemcpyDeviceToHost));
  for (int s = 0; s < 3; s++) {
    const long long n = a->d.down48 ? a->arrived[s][chan] : 0;
    if (arrived) arrived[s] = n;
    if (emitted) emitted[s] = a->d.down48 ? ad_emitted(a->cas.st[s], n) : 0;
  }
  return JAMD_OK;
}

}  // extern "C"
