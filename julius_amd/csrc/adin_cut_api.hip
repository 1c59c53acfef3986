// adin_cut_api.hip -- the C ABI of the silence cutting stage (jamd_adin_cut_*): validation, the object and the
// per-channel state it keeps on the device, the table of a push, the wait for the part tables and the decision whether
// the push goes ahead.  It launches nothing: the kernels and their launchers are in adin_cut.hip (adin_cut_host.h).
#include "adin_cut_host.h"

constexpr int kAcMaxParts = 65535;                           // (the gather's grid)

extern "C" {

int jamd_adin_cut_default(jamd_adin_cut_desc *d) {
  if (!d) return jamd_refuse("jamd_adin_cut_default: d is NULL");
  d->sfreq = 16000;
  d->level_thres = 2000; d->zero_cross_num = 60; d->head_margin_msec = 300; d->tail_margin_msec = 400;   // default.c:75-79
  d->chunk_size = 1000;                                      // default.c:80
  return JAMD_OK;
}

int jamd_adin_cut_params(const jamd_adin_cut_desc *d, int *c_length, int *noise_zerocross, int *nc_max, int *sbsize) {
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return jamd_refuse("jamd_adin_cut_params: %s", err.c_str());
  if (c_length) *c_length = p.c_length;
  if (noise_zerocross) *noise_zerocross = p.noise_zerocross;
  if (nc_max) *nc_max = p.nc_max;
  if (sbsize) *sbsize = p.sbsize;
  return JAMD_OK;
}

int64_t jamd_adin_cut_push_cap(const jamd_adin_cut_desc *d, int64_t chunk) {
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return jamd_refuse("jamd_adin_cut_push_cap: %s", err.c_str());
  if (chunk < 0) return jamd_refuse("jamd_adin_cut_push_cap: a negative sample count");
  return ac_push_cap(d, p, chunk);
}

int64_t jamd_adin_cut_parts_cap(const jamd_adin_cut_desc *d, int64_t chunk) {
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return jamd_refuse("jamd_adin_cut_parts_cap: %s", err.c_str());
  if (chunk < 0) return jamd_refuse("jamd_adin_cut_parts_cap: a negative sample count");
  return ac_parts_cap(d, p, chunk);
}

void jamd_adin_cut_destroy(jamd_adin_cut *k) {
  if (!k) return;
  delete k;                                  // (the engine is not looked at: it may have gone first)
}

int jamd_adin_cut_create(jamd_engine *e, const jamd_adin_cut_desc *d, int nchan, jamd_adin_cut **out) {
  if (!e || !d || !out || nchan < 1 || nchan > 65535) return jamd_refuse("jamd_adin_cut_create: NULL argument or nchan not in 1 ... 65535");
  *out = nullptr;
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return jamd_refuse("jamd_adin_cut_create: %s", err.c_str());
  std::unique_ptr<jamd_adin_cut> k(new jamd_adin_cut());   // (its members own what they hold)
  k->eng = e; k->nchan = nchan; k->d = *d; k->p = p;
  k->g = AcDev{d->level_thres, d->chunk_size, p.c_length, p.noise_zerocross, p.nc_max, p.sbsize, p.hist, nchan};
  const size_t C = nchan;
  int rc;
  JAMD_HIP(hipSetDevice(e->device));
  // need_init: all zero, sign ZC_POSITIVE
  if ((rc = k->d_state.alloc(C, true)) != JAMD_OK || (rc = k->d_next.alloc(C)) != JAMD_OK ||
      (rc = k->d_hs.alloc(C * p.hist, true)) != JAMD_OK || (rc = k->d_hc.alloc(C * p.hist, true)) != JAMD_OK ||
      (rc = k->d_strig.alloc(C)) != JAMD_OK || (rc = k->d_scum.alloc(C)) != JAMD_OK || (rc = k->d_used.alloc(C)) != JAMD_OK ||
      (rc = k->d_mask.alloc(C)) != JAMD_OK)
    return rc;
  *out = k.release();
  return JAMD_OK;
}

int jamd_adin_cut_reset(jamd_adin_cut *k, const unsigned char *mask, void *stream) {
  if (!k) return jamd_refuse("jamd_adin_cut_reset: NULL object");
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
    return jamd_refuse("jamd_adin_cut_push_dev: NULL argument");
  if (max_parts < 1 || max_parts > kAcMaxParts) return jamd_refuse("jamd_adin_cut_push_dev: max_parts not in 1 ... %d", kAcMaxParts);
  const int nchan = k->nchan, cap = max_parts;
  int rc;
  *nparts = 0;
  JAMD_HIP(hipSetDevice(k->eng->device));
  if ((rc = k->tab.begin(nchan * sizeof(AcChanTab))) != JAMD_OK) return rc;
  AcChanTab *h_ch = (AcChanTab *)k->tab.h.p;
  long long total = 0, room = 0;
  bool any = false;
  for (int c = 0; c < nchan; c++) {
    long long n;
    if ((rc = jamd_span("jamd_adin_cut_push_dev", in_off, c, &n)) != JAMD_OK) return rc;
    h_ch[c] = AcChanTab{in_off[c], total, (int)n, eos && eos[c] ? 1 : 0};
    total += n;
    if (n > 0 || h_ch[c].eos) { any = true; room += ac_push_cap(&k->d, k->p, n); }
  }
  if (total > 0 && !dev_in) return jamd_refuse("jamd_adin_cut_push_dev: NULL input");
  if (!any) return JAMD_OK;                                  // every channel idle
  hipStream_t st = jamd_stream(k->eng, stream);
  const size_t tb = ac_tabs_bytes(nchan, cap), cells = (size_t)cap * nchan;
  if ((rc = k->d_cnt.grow((size_t)(total > 0 ? total : 1) * sizeof(unsigned))) != JAMD_OK) return rc;
  if ((rc = k->d_pa.grow(cells * sizeof(long long))) != JAMD_OK) return rc;
  if ((rc = k->d_pl.grow(cells * sizeof(int))) != JAMD_OK) return rc;
  if ((rc = k->d_tabs.grow(tb)) != JAMD_OK) return rc;
  if ((rc = k->h_tabs.grow(tb)) != JAMD_OK) return rc;
  if ((rc = k->tab.send(nchan * sizeof(AcChanTab), st)) != JAMD_OK) return rc;
  const AcChanTab *d_ch = (const AcChanTab *)k->tab.d.p;
  const AcTabs dt = ac_tabs_at(k->d_tabs.p, nchan, cap), ht = ac_tabs_at(k->h_tabs.p, nchan, cap);
  if ((rc = ac_launch_plan(k, st, d_ch, dev_in, dt, cap)) != JAMD_OK) return rc;
  JAMD_HIP(hipMemcpyAsync(k->h_tabs.p, k->d_tabs, tb, hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));                        // the part count is data
  const long long np = ht.nparts[0];
  *nparts = (int)np;
  if (np > cap) return jamd_refuse("jamd_adin_cut_push_dev: the push needs %lld parts, max_parts is %d", np, cap);
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
  if (nout > 0 && !dev_out) return jamd_refuse("jamd_adin_cut_push_dev: NULL output");
  if (max_len > 0 && (rc = ac_launch_gather(k, st, d_ch, dev_in, dt, cap, (int)np, max_len, dev_out)) != JAMD_OK) return rc;
  return ac_launch_advance(k, st, d_ch, dev_in);
}

int jamd_adin_cut_push_host(jamd_adin_cut *k, const int16_t *samples, const int64_t *in_off, const unsigned char *eos,
                            int16_t *out, int max_parts, int *nparts, int64_t *part_off, unsigned char *part_final,
                            int64_t *part_start) {
  if (!k || !in_off || !nparts) return jamd_refuse("jamd_adin_cut_push_host: NULL argument");
  int rc;
  long long cap = 0;
  for (int c = 0; c < k->nchan; c++) {
    long long n;
    if ((rc = jamd_span("jamd_adin_cut_push_host", in_off, c, &n)) != JAMD_OK) return rc;
    cap += ac_push_cap(&k->d, k->p, n);
  }
  const long long lo = in_off[0], ns = in_off[k->nchan] - lo;
  if (ns > 0 && !samples) return jamd_refuse("jamd_adin_cut_push_host: NULL input");
  std::vector<int64_t> off(k->nchan + 1);    // the staged samples start at 0
  for (int c = 0; c <= k->nchan; c++) off[c] = in_off[c] - lo;
  return jamd_host_call(&k->stage, k->eng, ns > 0 ? samples + lo : nullptr, (size_t)(ns > 0 ? ns : 0), out, (size_t)cap,
                        [&](const int16_t *in, int16_t *o, hipStream_t st) -> long long {
                          const int r = jamd_adin_cut_push_dev(k, in, off.data(), eos, o, max_parts, nparts, part_off, part_final,
                                                               part_start, st);
                          if (r != JAMD_OK) return r;
                          const long long no = *nparts > 0 ? part_off[(size_t)(*nparts - 1) * (k->nchan + 1) + k->nchan] : 0;
                          if (no > 0 && !out) return jamd_refuse("jamd_adin_cut_push_host: NULL output");
                          return no;
                        });
}

int jamd_adin_cut_state_get(jamd_adin_cut *k, int chan, int *is_valid, int *nc, int *rest_tail, int *sblen, int *zero_cross,
                            int *carried, int64_t *stream_pos) {
  if (!k || chan < 0 || chan >= k->nchan) return jamd_refuse("jamd_adin_cut_state_get: NULL object or channel out of range");
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
