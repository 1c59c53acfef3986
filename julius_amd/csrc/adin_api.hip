// adin_api.hip -- the C ABI of the audio conditioning stage (jamd_adin_*): validation, the object and the per-channel
// state it keeps on the device, the tables of a push (counts from adin_plan.h), the coefficient file.  It launches
// nothing: the kernels and their launchers are in adin.hip (adin_host.h).
#include "adin_host.h"

constexpr long long kAdMaxChunk = 0x3fffffffLL;              // samples of one channel in one push

static int ad_span(const char *who, const int64_t *off, int c, long long *n) {
  *n = off[c + 1] - off[c];
  if (off[c] < 0 || *n < 0 || *n > kAdMaxChunk)
    return fe_refuse("%s: channel %d: offsets [%lld, %lld) are negative, descending or more than %lld samples", who, c,
                     (long long)off[c], (long long)off[c + 1], kAdMaxChunk);
  return JAMD_OK;
}

extern "C" {

int jamd_adin_default(jamd_adin_desc *d) {
  if (!d) return fe_refuse("jamd_adin_default: d is NULL");
  d->down48 = 0; d->fir_3to4 = nullptr; d->n_3to4 = 0; d->fir_2to1 = nullptr; d->n_2to1 = 0;
  d->level_coef = 1.0f;
  d->strip_zero = 1;                         // default.c:92
  d->zmean = 0;
  return JAMD_OK;
}

int jamd_adin_fir_read(const char *path, double *out, int cap) {
  if (!path || !out || cap < 1) return fe_refuse("jamd_adin_fir_read: NULL argument or cap < 1");
  std::string err;
  const int n = ad_fir_read(path, out, cap, err);
  if (n < 0) return fe_refuse("jamd_adin_fir_read: %s: %s", path, err.c_str());
  return n;
}

int64_t jamd_adin_ds_count(const jamd_adin_desc *d, int64_t samples_before, int64_t chunk) {
  std::string err;
  if (!ad_check_desc(d, false, err)) return fe_refuse("jamd_adin_ds_count: %s", err.c_str());
  if (samples_before < 0 || chunk < 0) return fe_refuse("jamd_adin_ds_count: a negative sample count");
  if (!d->down48) return chunk;
  const AdCascade c = ad_cascade(d->n_3to4, d->n_2to1);
  return ad_cascade_emitted(c, samples_before + chunk) - ad_cascade_emitted(c, samples_before);
}

int64_t jamd_adin_push_cap(const jamd_adin_desc *d, int64_t samples_before, int64_t chunk) {
  return jamd_adin_ds_count(d, samples_before, chunk);
}

void jamd_adin_destroy(jamd_adin *a) {
  if (!a) return;
  for (void *q : {(void *)a->d_fir[0], (void *)a->d_fir[1], (void *)a->d_hist[0], (void *)a->d_hist[1], (void *)a->d_hist[2],
                  (void *)a->d_zlen, (void *)a->d_zmean, (void *)a->d_mid[0], (void *)a->d_mid[1], (void *)a->d_ds,
                  (void *)a->d_pre, (void *)a->d_cnt, (void *)a->d_ooff, (void *)a->d_mask, (void *)a->d_hin, (void *)a->d_hout})
    (void)hipFree(q);
  fe_pin_free(&a->tab);
  if (a->h_ooff) (void)hipHostFree(a->h_ooff);
  delete a;
}

int jamd_adin_create(jamd_engine *e, const jamd_adin_desc *d, int nchan, jamd_adin **out) {
  if (!e || !d || !out || nchan < 1) return fe_refuse("jamd_adin_create: NULL argument or nchan < 1");
  *out = nullptr;
  std::string err;
  if (!ad_check_desc(d, true, err)) return fe_refuse("jamd_adin_create: %s", err.c_str());
  jamd_adin *a = new jamd_adin();
  a->eng = e; a->nchan = nchan; a->d = *d;
  a->d.fir_3to4 = nullptr; a->d.fir_2to1 = nullptr;
  a->d.strip_zero = d->strip_zero != 0; a->d.zmean = d->zmean != 0; a->d.down48 = d->down48 != 0;
  const size_t C = nchan;
  hipError_t r = hipSetDevice(e->device);
  if (r == hipSuccess) r = hipMalloc((void **)&a->d_zlen, C * sizeof(int));
  if (r == hipSuccess) r = hipMalloc((void **)&a->d_zmean, C * sizeof(float));
  if (r == hipSuccess) r = hipMalloc((void **)&a->d_cnt, C * sizeof(int));
  if (r == hipSuccess) r = hipMalloc((void **)&a->d_ooff, (C + 1) * sizeof(long long));
  if (r == hipSuccess) r = hipMalloc((void **)&a->d_mask, C);
  if (r == hipSuccess) r = hipHostMalloc((void **)&a->h_ooff, (C + 1) * sizeof(long long), hipHostMallocDefault);
  if (r == hipSuccess) r = hipMemset(a->d_zlen, 0, C * sizeof(int));
  if (r == hipSuccess) r = hipMemset(a->d_zmean, 0, C * sizeof(float));
  if (a->d.down48) {
    a->cas = ad_cascade(d->n_3to4, d->n_2to1);
    const double *src[2] = {d->fir_3to4, d->fir_2to1};
    const int ns[2] = {d->n_3to4, d->n_2to1};
    for (int i = 0; i < 2 && r == hipSuccess; i++) {
      r = hipMalloc((void **)&a->d_fir[i], kAdMaxTaps * sizeof(double));
      if (r == hipSuccess) r = hipMemset(a->d_fir[i], 0, kAdMaxTaps * sizeof(double));
      if (r == hipSuccess) r = hipMemcpy(a->d_fir[i], src[i], ns[i] * sizeof(double), hipMemcpyHostToDevice);
    }
    for (int s = 0; s < 3 && r == hipSuccess; s++) {
      const size_t nb = C * (a->cas.st[s].hist + kAdBlock - 1) * sizeof(double);
      r = hipMalloc((void **)&a->d_hist[s], nb);
      if (r == hipSuccess) r = hipMemset(a->d_hist[s], 0, nb);   // the samples before the stream start: 0.0
      a->arrived[s].assign(nchan, 0);
    }
  }
  if (r != hipSuccess) {
    jamd_set_error("jamd_adin_create: device allocation failed: %s", hipGetErrorString(r));
    jamd_adin_destroy(a);
    return r == hipErrorOutOfMemory ? JAMD_ENOMEM : JAMD_ENODEV;
  }
  *out = a;
  return JAMD_OK;
}

int jamd_adin_reset(jamd_adin *a, const unsigned char *mask, int what, void *stream) {
  if (!a || !(what & (JAMD_ADIN_DS | JAMD_ADIN_ZMEAN)) || (what & ~(JAMD_ADIN_DS | JAMD_ADIN_ZMEAN)))
    return fe_refuse("jamd_adin_reset: NULL object, or `what` is not JAMD_ADIN_DS | JAMD_ADIN_ZMEAN or one of them");
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
  if (!a || !in_off || !out_off) return fe_refuse("jamd_adin_push_dev: NULL argument");
  const int nchan = a->nchan;
  const bool ds = a->d.down48 != 0;
  const size_t nst = ds ? 3 * (size_t)nchan : 0, ntab = nst * sizeof(AdStageTab) + nchan * sizeof(AdChanTab);
  int rc;
  JAMD_HIP(hipSetDevice(a->eng->device));
  if ((rc = fe_pin_begin(&a->tab, ntab)) != JAMD_OK) return rc;
  AdStageTab *h_st = (AdStageTab *)a->tab.h;
  AdChanTab *h_ch = (AdChanTab *)(h_st + nst);
  std::vector<long long> after[3];
  if (ds) for (int s = 0; s < 3; s++) after[s] = a->arrived[s];
  long long M[3] = {0, 0, 0}, pre = 0;       // outputs of the three stages, samples behind them, over all channels
  int max_raw[3] = {0, 0, 0}, max_n = 0;
  for (int c = 0; c < nchan; c++) {
    long long n;
    if ((rc = ad_span("jamd_adin_push_dev", in_off, c, &n)) != JAMD_OK) return rc;
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
  if ((in_off[nchan] > 0 && !dev_in) || (pre > 0 && !dev_out)) return fe_refuse("jamd_adin_push_dev: NULL buffer");
  hipStream_t st = jamd_stream(a->eng, stream);
  if (ds) {
    for (int s = 0; s < 2; s++)
      if ((rc = jamd_grow(&a->d_mid[s], &a->mid_cap[s], (size_t)(M[s] > 0 ? M[s] : 1) * sizeof(double))) != JAMD_OK) return rc;
    if ((rc = jamd_grow(&a->d_ds, &a->ds_cap, (size_t)(M[2] > 0 ? M[2] : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  }
  if ((rc = jamd_grow(&a->d_pre, &a->pre_cap, (size_t)(pre > 0 ? pre : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if (in_off[nchan] > in_off[0]) {           // a push without a sample anywhere leaves every channel idle
    if ((rc = fe_pin_send(&a->tab, ntab, st)) != JAMD_OK) return rc;
    const AdStageTab *d_st = (const AdStageTab *)a->tab.d;
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
    JAMD_HIP(hipMemcpyAsync(a->h_ooff, a->d_ooff, (nchan + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    JAMD_HIP(hipStreamSynchronize(st));
    for (int c = 0; c <= nchan; c++) out_off[c] = a->h_ooff[c];
  } else {
    for (int c = 0; c < nchan; c++) out_off[c] = h_ch[c].pre_off;
    out_off[nchan] = pre;
  }
  return JAMD_OK;
}

int jamd_adin_push_host(jamd_adin *a, const int16_t *samples, const int64_t *in_off, int16_t *out, int64_t *out_off) {
  if (!a || !in_off || !out_off) return fe_refuse("jamd_adin_push_host: NULL argument");
  int rc;
  long long cap = 0;
  for (int c = 0; c < a->nchan; c++) {
    long long n;
    if ((rc = ad_span("jamd_adin_push_host", in_off, c, &n)) != JAMD_OK) return rc;
    cap += a->d.down48 ? ad_cascade_emitted(a->cas, a->arrived[0][c] + n) - ad_cascade_emitted(a->cas, a->arrived[0][c]) : n;
  }
  const long long ns = in_off[a->nchan];
  if ((ns > 0 && !samples) || (cap > 0 && !out)) return fe_refuse("jamd_adin_push_host: NULL buffer");
  JAMD_HIP(hipSetDevice(a->eng->device));
  if ((rc = jamd_grow(&a->d_hin, &a->hin_cap, (size_t)(ns > 0 ? ns : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&a->d_hout, &a->hout_cap, (size_t)(cap > 0 ? cap : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  hipStream_t st = a->eng->stream;
  if (ns > 0) JAMD_HIP(hipMemcpyAsync(a->d_hin, samples, (size_t)ns * sizeof(int16_t), hipMemcpyHostToDevice, st));
  if ((rc = jamd_adin_push_dev(a, a->d_hin, in_off, a->d_hout, out_off, st)) != JAMD_OK) return rc;
  const long long no = out_off[a->nchan];
  if (no > 0) JAMD_HIP(hipMemcpyAsync(out, a->d_hout, (size_t)no * sizeof(int16_t), hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  return JAMD_OK;
}

int jamd_adin_state_get(jamd_adin *a, int chan, int *zlen, float *zmean, int64_t *arrived, int64_t *emitted) {
  if (!a || chan < 0 || chan >= a->nchan) return fe_refuse("jamd_adin_state_get: NULL object or channel out of range");
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
