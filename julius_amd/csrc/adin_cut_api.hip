// adin_cut_api.hip -- the C ABI of the silence cutting stage (jamd_adin_cut_*): validation, the object and the
// per-channel state it keeps on the device, the table of a push, the wait for the part tables and the decision whether
// the push goes ahead.  It launches nothing: the kernels and their launchers are in adin_cut.hip (adin_cut_host.h).
#include "adin_cut_host.h"

constexpr long long kAcMaxChunk = 0x3fffffffLL;              // samples of one channel in one push
constexpr int kAcMaxParts = 65535;                           // (the gather's grid)

static int ac_span(const char *who, const int64_t *off, int c, long long *n) {
  *n = off[c + 1] - off[c];
  if (off[c] < 0 || *n < 0 || *n > kAcMaxChunk)
    return fe_refuse("%s: channel %d: offsets [%lld, %lld) are negative, descending or more than %lld samples", who, c,
                     (long long)off[c], (long long)off[c + 1], kAcMaxChunk);
  return JAMD_OK;
}

extern "C" {

int jamd_adin_cut_default(jamd_adin_cut_desc *d) {
  if (!d) return fe_refuse("jamd_adin_cut_default: d is NULL");
  d->sfreq = 16000;
  d->level_thres = 2000; d->zero_cross_num = 60; d->head_margin_msec = 300; d->tail_margin_msec = 400;   // default.c:75-79
  d->chunk_size = 1000;                                      // default.c:80
  return JAMD_OK;
}

int jamd_adin_cut_params(const jamd_adin_cut_desc *d, int *c_length, int *noise_zerocross, int *nc_max, int *sbsize) {
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return fe_refuse("jamd_adin_cut_params: %s", err.c_str());
  if (c_length) *c_length = p.c_length;
  if (noise_zerocross) *noise_zerocross = p.noise_zerocross;
  if (nc_max) *nc_max = p.nc_max;
  if (sbsize) *sbsize = p.sbsize;
  return JAMD_OK;
}

int64_t jamd_adin_cut_push_cap(const jamd_adin_cut_desc *d, int64_t chunk) {
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return fe_refuse("jamd_adin_cut_push_cap: %s", err.c_str());
  if (chunk < 0) return fe_refuse("jamd_adin_cut_push_cap: a negative sample count");
  return ac_push_cap(d, p, chunk);
}

int64_t jamd_adin_cut_parts_cap(const jamd_adin_cut_desc *d, int64_t chunk) {
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return fe_refuse("jamd_adin_cut_parts_cap: %s", err.c_str());
  if (chunk < 0) return fe_refuse("jamd_adin_cut_parts_cap: a negative sample count");
  return ac_parts_cap(d, p, chunk);
}

void jamd_adin_cut_destroy(jamd_adin_cut *k) {
  if (!k) return;
  for (void *q : {(void *)k->d_state, (void *)k->d_next, (void *)k->d_hs, (void *)k->d_hc, (void *)k->d_strig, (void *)k->d_scum,
                  (void *)k->d_mask, (void *)k->d_cnt, (void *)k->d_pa, (void *)k->d_pl, (void *)k->d_used, (void *)k->d_tabs,
                  (void *)k->d_hin, (void *)k->d_hout})
    (void)hipFree(q);
  fe_pin_free(&k->tab);
  if (k->h_tabs) (void)hipHostFree(k->h_tabs);
  delete k;
}

int jamd_adin_cut_create(jamd_engine *e, const jamd_adin_cut_desc *d, int nchan, jamd_adin_cut **out) {
  if (!e || !d || !out || nchan < 1 || nchan > 65535) return fe_refuse("jamd_adin_cut_create: NULL argument or nchan not in 1 ... 65535");
  *out = nullptr;
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return fe_refuse("jamd_adin_cut_create: %s", err.c_str());
  jamd_adin_cut *k = new jamd_adin_cut();
  k->eng = e; k->nchan = nchan; k->d = *d; k->p = p;
  k->g = AcDev{d->level_thres, d->chunk_size, p.c_length, p.noise_zerocross, p.nc_max, p.sbsize, p.hist, nchan};
  const size_t C = nchan;
  hipError_t r = hipSetDevice(e->device);
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_state, C * sizeof(AcState));
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_next, C * sizeof(AcState));
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_hs, C * p.hist * sizeof(int16_t));
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_hc, C * p.hist * sizeof(unsigned));
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_strig, C * sizeof(int));
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_scum, C * sizeof(unsigned));
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_used, C * sizeof(int));
  if (r == hipSuccess) r = hipMalloc((void **)&k->d_mask, C);
  if (r == hipSuccess) r = hipMemset(k->d_state, 0, C * sizeof(AcState));   // need_init: all zero, sign ZC_POSITIVE
  if (r == hipSuccess) r = hipMemset(k->d_hs, 0, C * p.hist * sizeof(int16_t));
  if (r == hipSuccess) r = hipMemset(k->d_hc, 0, C * p.hist * sizeof(unsigned));
  if (r != hipSuccess) {
    jamd_set_error("jamd_adin_cut_create: device allocation failed: %s", hipGetErrorString(r));
    jamd_adin_cut_destroy(k);
    return r == hipErrorOutOfMemory ? JAMD_ENOMEM : JAMD_ENODEV;
  }
  *out = k;
  return JAMD_OK;
}

int jamd_adin_cut_reset(jamd_adin_cut *k, const unsigned char *mask, void *stream) {
  if (!k) return fe_refuse("jamd_adin_cut_reset: NULL object");
  JAMD_HIP(hipSetDevice(k->eng->device));
  hipStream_t st = jamd_stream(k->eng, stream);
  // (a copy from pageable memory has left the host array when the call returns)
  if (mask) JAMD_HIP(hipMemcpyAsync(k->d_mask, mask, (size_t)k->nchan, hipMemcpyHostToDevice, st));
  return ac_launch_reset(k, st, mask ? k->d_mask : nullptr);
}

int jamd_adin_cut_push_dev(jamd_adin_cut *k, const int16_t *dev_in, const int64_t *in_off, const unsigned char *eos,
                           int16_t *dev_out, int max_parts, int *nparts, int64_t *part_off, unsigned char *part_final,
                           int64_t *part_start, void *stream) {
  if (!k || !in_off || !nparts || !part_off || !part_final || !part_start)
    return fe_refuse("jamd_adin_cut_push_dev: NULL argument");
  if (max_parts < 1 || max_parts > kAcMaxParts) return fe_refuse("jamd_adin_cut_push_dev: max_parts not in 1 ... %d", kAcMaxParts);
  const int nchan = k->nchan, cap = max_parts;
  int rc;
  *nparts = 0;
  JAMD_HIP(hipSetDevice(k->eng->device));
  if ((rc = fe_pin_begin(&k->tab, nchan * sizeof(AcChanTab))) != JAMD_OK) return rc;
  AcChanTab *h_ch = (AcChanTab *)k->tab.h;
  long long total = 0, room = 0;
  bool any = false;
  for (int c = 0; c < nchan; c++) {
    long long n;
    if ((rc = ac_span("jamd_adin_cut_push_dev", in_off, c, &n)) != JAMD_OK) return rc;
    h_ch[c] = AcChanTab{in_off[c], total, (int)n, eos && eos[c] ? 1 : 0};
    total += n;
    if (n > 0 || h_ch[c].eos) { any = true; room += ac_push_cap(&k->d, k->p, n); }
  }
  if (total > 0 && !dev_in) return fe_refuse("jamd_adin_cut_push_dev: NULL input");
  if (!any) return JAMD_OK;                                  // every channel idle
  hipStream_t st = jamd_stream(k->eng, stream);
  const size_t tb = ac_tabs_bytes(nchan, cap), cells = (size_t)cap * nchan;
  if ((rc = jamd_grow(&k->d_cnt, &k->cnt_cap, (size_t)(total > 0 ? total : 1) * sizeof(unsigned))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&k->d_pa, &k->pa_cap, cells * sizeof(long long))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&k->d_pl, &k->pl_cap, cells * sizeof(int))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&k->d_tabs, &k->tabs_cap, tb)) != JAMD_OK) return rc;
  if (k->h_tabs_cap < tb) {
    if (k->h_tabs) JAMD_HIP(hipHostFree(k->h_tabs));
    k->h_tabs = nullptr; k->h_tabs_cap = 0;
    JAMD_HIP(hipHostMalloc((void **)&k->h_tabs, tb, hipHostMallocDefault));
    k->h_tabs_cap = tb;
  }
  if ((rc = fe_pin_send(&k->tab, nchan * sizeof(AcChanTab), st)) != JAMD_OK) return rc;
  const AcChanTab *d_ch = (const AcChanTab *)k->tab.d;
  const AcTabs dt = ac_tabs_at(k->d_tabs, nchan, cap), ht = ac_tabs_at(k->h_tabs, nchan, cap);
  if ((rc = ac_launch_plan(k, st, d_ch, dev_in, dt, cap)) != JAMD_OK) return rc;
  JAMD_HIP(hipMemcpyAsync(k->h_tabs, k->d_tabs, tb, hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));                        // the part count is data
  const long long np = ht.nparts[0];
  *nparts = (int)np;
  if (np > cap) return fe_refuse("jamd_adin_cut_push_dev: the push needs %lld parts, max_parts is %d", np, cap);
  int max_len = 0;
  for (long long p = 0; p < np; p++) {
    const long long *off = ht.off + p * (nchan + 1);
    for (int c = 0; c < nchan; c++) {
      part_off[p * (nchan + 1) + c] = off[c];
      part_final[p * nchan + c] = ht.fin[p * nchan + c];
      part_start[p * nchan + c] = ht.start[p * nchan + c];
      if (off[c + 1] - off[c] > max_len) max_len = (int)(off[c + 1] - off[c]);
    }
    part_off[p * (nchan + 1) + nchan] = off[nchan];
  }
  const long long nout = np > 0 ? ht.off[(np - 1) * (nchan + 1) + nchan] : 0;
  if (nout > room) {                                         // (dev_out is sized by the bound)
    jamd_set_error("jamd_adin_cut_push_dev: %lld samples to deliver, jamd_adin_cut_push_cap() promised %lld at the most", nout, room);
    return JAMD_ELAUNCH;
  }
  if (nout > 0 && !dev_out) return fe_refuse("jamd_adin_cut_push_dev: NULL output");
  if (max_len > 0 && (rc = ac_launch_gather(k, st, d_ch, dev_in, dt, cap, (int)np, max_len, dev_out)) != JAMD_OK) return rc;
  return ac_launch_advance(k, st, d_ch, dev_in);
}

int jamd_adin_cut_push_host(jamd_adin_cut *k, const int16_t *samples, const int64_t *in_off, const unsigned char *eos,
                            int16_t *out, int max_parts, int *nparts, int64_t *part_off, unsigned char *part_final,
                            int64_t *part_start) {
  if (!k || !in_off || !nparts) return fe_refuse("jamd_adin_cut_push_host: NULL argument");
  int rc;
  long long cap = 0;
  for (int c = 0; c < k->nchan; c++) {
    long long n;
    if ((rc = ac_span("jamd_adin_cut_push_host", in_off, c, &n)) != JAMD_OK) return rc;
    cap += ac_push_cap(&k->d, k->p, n);
  }
  const long long lo = in_off[0], ns = in_off[k->nchan] - lo;
  if (ns > 0 && !samples) return fe_refuse("jamd_adin_cut_push_host: NULL input");
  JAMD_HIP(hipSetDevice(k->eng->device));
  if ((rc = jamd_grow(&k->d_hin, &k->hin_cap, (size_t)(ns > 0 ? ns : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&k->d_hout, &k->hout_cap, (size_t)cap * sizeof(int16_t))) != JAMD_OK) return rc;
  hipStream_t st = k->eng->stream;
  if (ns > 0) JAMD_HIP(hipMemcpyAsync(k->d_hin, samples + lo, (size_t)ns * sizeof(int16_t), hipMemcpyHostToDevice, st));
  std::vector<int64_t> off(k->nchan + 1);
  for (int c = 0; c <= k->nchan; c++) off[c] = in_off[c] - lo;
  if ((rc = jamd_adin_cut_push_dev(k, k->d_hin, off.data(), eos, k->d_hout, max_parts, nparts, part_off, part_final, part_start,
                                   st)) != JAMD_OK)
    return rc;
  const long long no = *nparts > 0 ? part_off[(size_t)(*nparts - 1) * (k->nchan + 1) + k->nchan] : 0;
  if (no > 0 && !out) return fe_refuse("jamd_adin_cut_push_host: NULL output");
  if (no > 0) JAMD_HIP(hipMemcpyAsync(out, k->d_hout, (size_t)no * sizeof(int16_t), hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  return JAMD_OK;
}

int jamd_adin_cut_state_get(jamd_adin_cut *k, int chan, int *is_valid, int *nc, int *rest_tail, int *sblen, int *zero_cross,
                            int *carried, int64_t *stream_pos) {
  if (!k || chan < 0 || chan >= k->nchan) return fe_refuse("jamd_adin_cut_state_get: NULL object or channel out of range");
  JAMD_HIP(hipSetDevice(k->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  AcState s;
  JAMD_HIP(hipMemcpy(&s, k->d_state + chan, sizeof s, hipMemcpyDeviceToHost));
  if (is_valid) *is_valid = s.is_valid;
  if (nc) *nc = s.nc;
  if (rest_tail) *rest_tail = s.rest_tail;
  if (sblen) *sblen = s.sblen;
  if (zero_cross) *zero_cross = s.zc;
  if (carried) *carried = s.carried;
  if (stream_pos) *stream_pos = s.pos;
  return JAMD_OK;
}

}  // extern "C"
