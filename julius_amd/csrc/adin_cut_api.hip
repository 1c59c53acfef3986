// adin_cut_api.hip -- the C ABI of the silence cutting stage (jamd_adin_cut_*): validation, the object and the
// per-channel state it keeps on the device, the table of a push, the wait for the part tables and the decision whether
// the push goes ahead.  It launches nothing: the kernels and their launchers are in adin_cut.hip (adin_cut_host.h).
#include "adin_cut_host.h"

constexpr int kAcMaxParts = 65535;                           // (the gather's grid)
constexpr int kAcMaxSpeechLen = 320000;                      // MAXSPEECHLEN: fvad_proceed()'s buffer

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

// The object of either entry; fv == NULL: without the gate
static int ac_create(const char *who, jamd_engine *e, const jamd_adin_cut_desc *d, const jamd_adin_cut_fvad *fv, int nchan,
                     jamd_adin_cut **out) {
  if (!e || !d || !out || nchan < 1 || nchan > 65535) return jamd_refuse("%s: NULL argument or nchan not in 1 ... 65535", who);
  *out = nullptr;
  AcParams p;
  std::string err;
  if (!ac_params(d, p, err)) return jamd_refuse("%s: %s", who, err.c_str());
  int fs = 0;
  if (fv) {
    if (!fv_check_desc(&fv->det, err)) return jamd_refuse("%s: %s", who, err.c_str());
    if (fv->det.sfreq != d->sfreq)
      return jamd_refuse("%s: the detector's sfreq (%d) is not the cutting's (%d)", who, fv->det.sfreq, d->sfreq);
    if (fv->smoothnum < 1 || fv->smoothnum > JAMD_FVAD_SMOOTH_MAX)
      return jamd_refuse("%s: smoothnum %d is not in 1 ... %d", who, fv->smoothnum, JAMD_FVAD_SMOOTH_MAX);
    if (!(fv->thres >= 0.0f && fv->thres <= 1.0f)) return jamd_refuse("%s: thres %g is not in 0 ... 1", who, (double)fv->thres);
    fs = fv_frame_size(d->sfreq);
    if ((long long)d->chunk_size + fs > kAcMaxSpeechLen)
      return jamd_refuse("%s: chunk_size %d + a frame of %d samples > %d (MAXSPEECHLEN): fvad_proceed() would drop samples", who,
                         d->chunk_size, fs, kAcMaxSpeechLen);
    // a frame that ends in a push can begin chunk_size - 1 + fs samples behind it
    if (p.hist < d->chunk_size + fs) p.hist = d->chunk_size + fs;
  }
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
  if (fv) {
    k->gate.reset(new FvGate());
    FvGate &q = *k->gate;
    q.fs = fs; q.N = fv->smoothnum; q.cmin = fv_gate_cmin(fv->smoothnum, fv->thres); q.vhist = fv->smoothnum + 1;
    const FvModel m = fv_model(fv->det.model, fv->det.mode);
    if ((rc = q.d_model.upload(&m, 1)) != JAMD_OK || (rc = q.d_s16.alloc(C * kFvKept)) != JAMD_OK ||
        (rc = q.d_s16n.alloc(C * kFvKept)) != JAMD_OK || (rc = q.d_s32.alloc(C * 3)) != JAMD_OK ||
        (rc = q.d_s32n.alloc(C * 3)) != JAMD_OK || (rc = q.d_vh.alloc(C * q.vhist, true)) != JAMD_OK)
      return rc;
    if ((rc = fv_launch_reset_at(e->stream, q.d_model, nullptr, q.d_s16, q.d_s32, nullptr, nchan)) != JAMD_OK) return rc;
    JAMD_HIP(hipStreamSynchronize(e->stream));   // (a push may come on another stream)
  }
  *out = k.release();
  return JAMD_OK;
}

int jamd_adin_cut_create(jamd_engine *e, const jamd_adin_cut_desc *d, int nchan, jamd_adin_cut **out) {
  return ac_create("jamd_adin_cut_create", e, d, nullptr, nchan, out);
}

int jamd_adin_cut_create_fvad(jamd_engine *e, const jamd_adin_cut_desc *d, const jamd_adin_cut_fvad *fv, int nchan,
                              jamd_adin_cut **out) {
  if (!fv) return jamd_refuse("jamd_adin_cut_create_fvad: the gate's descriptor (fv) is NULL; jamd_adin_cut_create() makes an object without the gate");
  return ac_create("jamd_adin_cut_create_fvad", e, d, fv, nchan, out);
}

int jamd_adin_cut_fvad_reset(jamd_adin_cut *k, const unsigned char *mask, void *stream) {
  if (!k || !k->gate) return jamd_refuse("jamd_adin_cut_fvad_reset: NULL object, or one made without the gate");
  JAMD_HIP(hipSetDevice(k->eng->device));
  hipStream_t st = jamd_stream(k->eng, stream);
  if (mask) JAMD_HIP(hipMemcpyAsync(k->d_mask, mask, (size_t)k->nchan, hipMemcpyHostToDevice, st));
  return fv_launch_reset_at(st, k->gate->d_model, mask ? k->d_mask.p : nullptr, k->gate->d_s16, k->gate->d_s32, nullptr, k->nchan);
}

int jamd_adin_cut_fvad_state_get(jamd_adin_cut *k, int chan, int *state) {
  if (!k || !k->gate || !state || chan < 0 || chan >= k->nchan)
    return jamd_refuse("jamd_adin_cut_fvad_state_get: NULL argument, an object made without the gate, or channel out of range");
  JAMD_HIP(hipSetDevice(k->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  const size_t C = k->nchan;
  short s16[kFvKept];
  int s32[3];
  JAMD_HIP(hipMemcpy2D(s16, sizeof(short), k->gate->d_s16 + chan, C * sizeof(short), sizeof(short), kFvKept, hipMemcpyDeviceToHost));
  JAMD_HIP(hipMemcpy2D(s32, sizeof(int), k->gate->d_s32 + chan, C * sizeof(int), sizeof(int), 3, hipMemcpyDeviceToHost));
  fv_state_ints(s16, s32, 0, state);
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
  FvGate *gate = k->gate.get();
  if (gate && (rc = gate->vtab.begin(nchan * sizeof(long long))) != JAMD_OK) return rc;
  long long *h_voff = gate ? (long long *)gate->vtab.h.p : nullptr;
  long long total = 0, room = 0, vtotal = 0;
  bool any = false;
  for (int c = 0; c < nchan; c++) {
    long long n;
    if ((rc = jamd_span("jamd_adin_cut_push_dev", in_off, c, &n)) != JAMD_OK) return rc;
    h_ch[c] = AcChanTab{in_off[c], total, (int)n, eos && eos[c] ? 1 : 0};
    if (gate) { h_voff[c] = vtotal; vtotal += ac_gate_frames_cap(n, k->d.chunk_size, gate->fs); }
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
  const long long *d_voff = gate ? (const long long *)gate->vtab.d.p : nullptr;
  if (gate) {                                                // the detector first: the blocks read its counts
    if ((rc = gate->d_vnew.grow((size_t)vtotal * sizeof(unsigned))) != JAMD_OK) return rc;
    if ((rc = gate->vtab.send(nchan * sizeof(long long), st)) != JAMD_OK) return rc;
    if ((rc = acg_launch_frames(k, st, d_ch, d_voff, dev_in)) != JAMD_OK) return rc;
  }
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
  if (gate && (rc = acg_launch_advance(k, st, d_ch, d_voff)) != JAMD_OK) return rc;
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
