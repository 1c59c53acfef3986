// frontend_live_api.hip -- the C ABI of the live-input front end (jamd_frontend_live_*, jamd_frontend_cmn_*): validation,
// the object and the per-channel state it keeps on the device, the tables of a run or a push (counts from
// frontend_tables.h), the -cmnload / -cmnsave file.  The base coefficients come from the parent jamd_frontend's frame
// kernel, in the parent's scratch.  It launches nothing: the kernels and their launchers are in frontend.hip and
// frontend_live.hip (frontend_host.h).
#include "frontend_host.h"
#include "cmn_file.h"

static int lv_refuse_ss_calc(jamd_frontend_live *l, const char *who) {
  if (l->f->ss_mode != JAMD_SS_CALC) return JAMD_OK;
  return jamd_refuse("%s: JAMD_SS_CALC is set on the parent front end: a live segment has no head known in advance (use "
                   "JAMD_SS_LOAD or JAMD_SS_OFF)", who);
}

// The base coefficients of the B frames tabs[0] (boff) describes, through the parent: sample_off and `tabs` go up to
// f->off.d, the frame kernel leaves f->d_stat [B][baselen]; both hold until the next call on the parent.  Returns the
// tables on the device in *d_tabs.
static int lv_base_frames(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const int64_t *sample_off, int nchan,
                          long long B, std::initializer_list<const std::vector<int> *> tabs, const int **d_tabs) {
  int rc;
  if ((rc = f->d_stat.grow((size_t)(B > 0 ? B : 1) * f->d.baselen * sizeof(float))) != JAMD_OK) return rc;
  if ((rc = fe_put_offsets(f, st, sample_off, nchan, tabs)) != JAMD_OK) return rc;
  const long long *d_soff = (const long long *)f->off.d.p;
  *d_tabs = (const int *)(d_soff + nchan + 1);
  return B > 0 ? fe_launch_frames(f, st, dev_samples, d_soff, *d_tabs, nchan, (int)B) : JAMD_OK;
}

extern "C" {

int jamd_frontend_live_default(jamd_frontend_live_desc *d) {
  if (!d) return jamd_refuse("jamd_frontend_live_default: d is NULL");
  d->map_cmn = 1; d->map_weight = 100.0f;    // default.c:153-156
  d->cmean_init = nullptr; d->cvar_init = nullptr;
  return JAMD_OK;
}

int jamd_frontend_live_frames(const jamd_frontend_desc *d, int64_t nsamples) {
  if (!d || d->framesize < 1 || d->frameshift < 1 || d->splice < 1 || (d->delta && d->delWin < 1) ||
      (d->acc && d->accWin < 1))
    return jamd_refuse("jamd_frontend_live_frames: NULL descriptor, or framesize / frameshift / splice / window < 1");
  const long long T = lv_counts(*d, nsamples).To;
  return T > 0x7fffffff ? 0x7fffffff : (int)T;
}

void jamd_frontend_live_destroy(jamd_frontend_live *l) {
  if (!l) return;
  delete l;                                  // (the parent is not looked at: it may have gone first)
}

int jamd_frontend_live_state_set(jamd_frontend_live *l, int chan, const float *cmean, const float *cvar) {
  if (!l || !cmean || chan < 0 || chan >= l->nchan)
    return jamd_refuse("jamd_frontend_live_state_set: NULL argument or channel out of range");
  if (l->p.var && !cvar) return jamd_refuse("jamd_frontend_live_state_set: the kind has cvn: a variance is needed");
  if (!l->open.empty() && l->open[chan]) {
    jamd_set_error("jamd_frontend_live_state_set: channel %d has an open segment (end it with a final push first)", chan);
    return JAMD_ESTATE;
  }
  JAMD_HIP(hipSetDevice(l->f->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  const size_t V = l->p.veclen;
  JAMD_HIP(hipMemcpy(l->s.cmean + chan * V, cmean, V * sizeof(float), hipMemcpyHostToDevice));
  if (l->p.var) JAMD_HIP(hipMemcpy(l->s.cvar + chan * V, cvar, V * sizeof(float), hipMemcpyHostToDevice));
  const int fl = kSet | kLoaded;             // CMN_load_from_file() :647-648
  JAMD_HIP(hipMemcpy(l->s.flags + chan, &fl, sizeof(int), hipMemcpyHostToDevice));
  return JAMD_OK;
}

int jamd_frontend_live_state_get(jamd_frontend_live *l, int chan, float *cmean, float *cvar, float *emax, int *flags) {
  if (!l || chan < 0 || chan >= l->nchan)
    return jamd_refuse("jamd_frontend_live_state_get: NULL object or channel out of range");
  JAMD_HIP(hipSetDevice(l->f->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  const size_t V = l->p.veclen;
  if (cmean) JAMD_HIP(hipMemcpy(cmean, l->s.cmean + chan * V, V * sizeof(float), hipMemcpyDeviceToHost));
  if (cvar) JAMD_HIP(hipMemcpy(cvar, l->s.cvar + chan * V, V * sizeof(float), hipMemcpyDeviceToHost));
  if (emax) JAMD_HIP(hipMemcpy(emax, l->s.emax + chan, sizeof(float), hipMemcpyDeviceToHost));
  if (flags) JAMD_HIP(hipMemcpy(flags, l->s.flags + chan, sizeof(int), hipMemcpyDeviceToHost));
  return JAMD_OK;
}

int jamd_frontend_live_create(jamd_frontend *f, const jamd_frontend_live_desc *ld, int nchan, jamd_frontend_live **out) {
  if (!f || !ld || !out || nchan < 1) return jamd_refuse("jamd_frontend_live_create: NULL argument or nchan < 1");
  *out = nullptr;
  const jamd_frontend_desc &d = f->d;
  if (d.absesup && d.acc)
    return jamd_refuse("jamd_frontend_live_create: _N together with _A is not served: the reference's flush loop "
                     "(realtime-1stpass.c:1233-1241) strips the absolute energy before the acceleration buffer, its main "
                     "loop after it, so the last frames of every segment carry a stale slot");
  if (d.frameshift > d.framesize + 1)
    return jamd_refuse("jamd_frontend_live_create: frameshift %d beyond the live window of %d samples (the reference's "
                     "window shift has no meaning there)", d.frameshift, d.framesize + 1);
  if (d.cvn && ld->cmean_init && !ld->cvar_init)
    return jamd_refuse("jamd_frontend_live_create: the kind has cvn: an initial mean needs an initial variance");
  if ((long long)nchan * d.veclen > 0x7fffffffLL / kRing)
    return jamd_refuse("jamd_frontend_live_create: %d channels of %d elements are too many", nchan, d.veclen);
  std::unique_ptr<jamd_frontend_live> l(new jamd_frontend_live());   // (its members own what they hold)
  l->f = f; l->nchan = nchan;
  LvParams &p = l->p;
  p.nchan = nchan; p.veclen = d.veclen; p.baselen = d.baselen; p.nb = d.baselen - (d.absesup ? 1 : 0);
  p.splice = d.splice; p.delta = d.delta; p.acc = d.acc; p.delWin = d.delWin; p.accWin = d.accWin;
  p.Bd = 0; p.Ba = 0;                        // WMP_deltabuf_new(): B = 2 * sum of theta^2, an int
  for (int i = 1; i <= d.delWin; i++) p.Bd += i * i;
  for (int i = 1; i <= d.accWin; i++) p.Ba += i * i;
  p.Bd *= 2; p.Ba *= 2;
  p.enorm = d.energy && d.enormal; p.mean = d.cmn != 0; p.var = d.cvn != 0;
  p.mfcc_dim = d.mfcc_dim + (d.c0 ? 1 : 0);
  p.do_map = ld->map_cmn != 0; p.cweight = ld->map_weight;
  p.escale = d.escale; p.silFloor = d.silFloor;
  p.R = 2 * ((d.delta ? d.delWin : 0) + (d.acc ? d.accWin : 0));
  if (p.R < 1) p.R = 1;
  p.fs = d.framesize;
  l->open.assign(nchan, 0); l->ns.assign(nchan, 0);
  const size_t C = nchan, V = d.veclen, CV = C * V;
  // floats: emax | cmean | cvar | now_sum | now_var | all_var | ring_sum | rmax | ring | sp ;
  // ints: flags now_fn all_fn head cnum cmax | ring_fn ; int16: res
  const size_t nring = C * p.R * d.baselen, nsp = CV * (d.splice - 1), nres = C * d.framesize;
  const size_t nfl = C + 5 * CV + CV * kRing + C + nring + nsp, nin = 6 * C + C * kRing;
  const size_t nstate = nfl * sizeof(float) + nin * sizeof(int) + nres * sizeof(int16_t);
  JAMD_HIP(hipSetDevice(f->eng->device));
  int rc;
  if ((rc = l->state.alloc(nstate, true)) != JAMD_OK) return rc;
  if ((rc = l->d_upd.alloc(C)) != JAMD_OK) return rc;
  LvState &s = l->s;
  float *q = (float *)l->state.p;
  s.emax = q; q += C;
  s.cmean = q; q += CV; s.cvar = q; q += CV; s.now_sum = q; q += CV; s.now_var = q; q += CV; s.all_var = q; q += CV;
  s.ring_sum = q; q += CV * kRing;
  s.rmax = q; q += C; s.ring = q; q += nring; s.sp = q; q += nsp;
  int *r = (int *)q;
  s.flags = r; r += C; s.now_fn = r; r += C; s.all_fn = r; r += C; s.head = r; r += C; s.cnum = r; r += C; s.cmax = r; r += C;
  s.ring_fn = r; r += C * kRing;
  s.res = (int16_t *)r;
  // energy_max_init(): 5.0; CMN_realtime_new(): clist_max = CPSTEP
  std::vector<float> five(C, 5.0f);
  std::vector<int> step(C, LV_CPSTEP);
  JAMD_HIP(hipMemcpy(s.emax, five.data(), C * sizeof(float), hipMemcpyHostToDevice));
  JAMD_HIP(hipMemcpy(s.cmax, step.data(), C * sizeof(int), hipMemcpyHostToDevice));
  // the tables of a push, so that no push allocates them
  if ((rc = l->tab.begin(sizeof(long long) * (C + 1) + 3 * sizeof(int) * (C + 1))) != JAMD_OK) return rc;
  if (ld->cmean_init && (d.cmn || d.cvn)) {
    for (int c = 0; c < nchan; c++)
      if ((rc = jamd_frontend_live_state_set(l.get(), c, ld->cmean_init, ld->cvar_init)) != JAMD_OK) return rc;
  }
  *out = l.release();
  return JAMD_OK;
}

int jamd_frontend_live_run_dev(jamd_frontend_live *l, const int16_t *dev_samples, const int64_t *sample_off,
                               float *dev_out, int *frame_off, void *stream) {
  if (!l || !dev_samples || !sample_off || !dev_out) return jamd_refuse("jamd_frontend_live_run_dev: NULL argument");
  int rc;
  if ((rc = lv_refuse_ss_calc(l, "jamd_frontend_live_run_dev")) != JAMD_OK) return rc;
  if (l->nopen) {
    jamd_set_error("jamd_frontend_live_run_dev: %d channel(s) have an open segment (end them with a final push first)", l->nopen);
    return JAMD_ESTATE;
  }
  const jamd_frontend_desc &d = l->f->d;
  const int nchan = l->nchan;
  std::vector<int> boff(nchan + 1), noff(nchan + 1), ooff(nchan + 1), act(nchan + 1, 0), zero(nchan + 1, 0);
  std::string err;
  long long B = 0, N = 0, O = 0;
  for (int c = 0; c < nchan; c++) {
    const long long n = fe_span("jamd_frontend_live_run_dev", "channel", sample_off, c, err);
    if (n < 0) return jamd_refuse("%s", err.c_str());
    const LvCounts k = lv_counts(d, n);
    boff[c] = (int)B; noff[c] = (int)N; ooff[c] = (int)O;
    act[c] = (n > 0 ? kActive | kFinal : 0) | (k.reest ? kReest : 0);
    B += k.Tb; N += k.Nf; O += k.To;
    if ((B + 1) * (long long)d.vecbuflen * d.splice > 0x7fffffffLL)
      return jamd_refuse("jamd_frontend_live_run_dev: batch too large (%lld frames)", B);
  }
  boff[nchan] = (int)B; noff[nchan] = (int)N; ooff[nchan] = (int)O;
  JAMD_HIP(hipSetDevice(l->f->eng->device));
  hipStream_t st = jamd_stream(l->f->eng, stream);
  if ((rc = l->d_feat.grow((size_t)(N > 0 ? N : 1) * d.veclen * sizeof(float))) != JAMD_OK) return rc;
  const int *d_tabs;                         // (a whole segment: nothing in the ring, frames from 0)
  if ((rc = lv_base_frames(l->f, st, dev_samples, sample_off, nchan, B, {&boff, &noff, &ooff, &act, &zero}, &d_tabs)) != JAMD_OK)
    return rc;
  if ((rc = lv_launch(l, st, d_tabs, N, O, nullptr, dev_out)) != JAMD_OK) return rc;
  if (frame_off) memcpy(frame_off, ooff.data(), sizeof(int) * (nchan + 1));
  return JAMD_OK;
}

int jamd_frontend_live_push_frames(const jamd_frontend_desc *d, int64_t samples_before, int64_t chunk, int final) {
  if (!d || d->framesize < 1 || d->frameshift < 1 || d->splice < 1 || (d->delta && d->delWin < 1) ||
      (d->acc && d->accWin < 1) || samples_before < 0 || chunk < 0)
    return jamd_refuse("jamd_frontend_live_push_frames: NULL descriptor, framesize / frameshift / splice / window < 1, or a "
                     "negative sample count");
  const long long T = lv_push(*d, samples_before, chunk, final != 0).rows;
  return T > 0x7fffffff ? 0x7fffffff : (int)T;
}

int jamd_frontend_live_stream_cap(jamd_frontend_live *l, int max_rows) {
  if (!l || max_rows < 1) return jamd_refuse("jamd_frontend_live_stream_cap: NULL object or max_rows < 1");
  if (l->nopen) {
    jamd_set_error("jamd_frontend_live_stream_cap: %d channel(s) have an open segment", l->nopen);
    return JAMD_ESTATE;
  }
  l->hist_cap = max_rows;
  return JAMD_OK;
}

int jamd_frontend_live_push_dev(jamd_frontend_live *l, const int16_t *dev_samples, const int64_t *sample_off,
                                const unsigned char *final, float *dev_out, int *frame_off, void *stream) {
  if (!l || !sample_off) return jamd_refuse("jamd_frontend_live_push_dev: NULL argument");
  int rc;
  if ((rc = lv_refuse_ss_calc(l, "jamd_frontend_live_push_dev")) != JAMD_OK) return rc;
  const jamd_frontend_desc &d = l->f->d;
  const int nchan = l->nchan;
  const bool keep_rows = d.cvn && d.splice == 1;
  std::vector<int> boff(nchan + 1), noff(nchan + 1), ooff(nchan + 1), act(nchan + 1, 0), told(nchan + 1, 0), f0(nchan + 1, 0);
  std::vector<int64_t> soff(nchan + 1);
  std::vector<long long> ns_after(l->ns);
  std::vector<char> open_after(l->open);
  const size_t ntab = sizeof(long long) * (nchan + 1) + 3 * sizeof(int) * (nchan + 1);
  JAMD_HIP(hipSetDevice(l->f->eng->device));
  if ((rc = l->tab.begin(ntab)) != JAMD_OK) return rc;
  long long *h_coff = (long long *)l->tab.h.p;
  int *h_soff = (int *)(h_coff + nchan + 1), *h_rlen = h_soff + nchan + 1, *h_newr = h_rlen + nchan + 1;
  std::string err;
  long long B = 0, N = 0, O = 0, S = 0, need_rows = 0;
  bool any = false;
  for (int c = 0; c < nchan; c++) {
    const long long n = fe_span("jamd_frontend_live_push_dev", "channel", sample_off, c, err);
    if (n < 0) return jamd_refuse("%s", err.c_str());
    const bool fin = final && final[c], was = l->open[c] != 0;
    boff[c] = (int)B; noff[c] = (int)N; ooff[c] = (int)O;
    soff[c] = S; h_coff[c] = sample_off[c]; h_soff[c] = (int)S; h_rlen[c] = 0; h_newr[c] = 0;
    if (n == 0 && !(fin && was)) continue;     // idle, or an end without a segment
    any = true;
    const long long n_old = was ? l->ns[c] : 0;
    const LvPush q = lv_push(d, n_old, n, fin);
    if (keep_rows && q.F_new > l->hist_cap)
      return jamd_refuse("jamd_frontend_live_push_dev: channel %d would hold %lld rows of an open segment, beyond the cap of %d "
                       "(jamd_frontend_live_stream_cap())", c, q.F_new, l->hist_cap);
    if (q.F_new > need_rows) need_rows = q.F_new;
    act[c] = kActive | (was ? kCont : 0) | (fin ? kFinal : 0) | (q.reest ? kReest : 0);
    told[c] = (int)q.Tb_old; f0[c] = (int)q.F_old;
    h_rlen[c] = (int)q.r_old; h_newr[c] = (int)q.r_new;
    B += q.Tb_new - q.Tb_old; N += q.F_new - q.F_old; O += q.rows;
    S += q.r_old + n;
    open_after[c] = !fin; ns_after[c] = fin ? 0 : n_old + n;
    if ((B + 1) * (long long)d.vecbuflen * d.splice > 0x7fffffffLL || S > 0x7fffffffLL || q.Tb_new > 0x7fffffffLL)
      return jamd_refuse("jamd_frontend_live_push_dev: batch too large (%lld frames, %lld samples)", B, S);
  }
  boff[nchan] = (int)B; noff[nchan] = (int)N; ooff[nchan] = (int)O;
  soff[nchan] = S; h_coff[nchan] = sample_off[nchan]; h_soff[nchan] = (int)S; h_rlen[nchan] = 0; h_newr[nchan] = 0;
  if ((sample_off[nchan] > 0 && !dev_samples) || (O > 0 && !dev_out))
    return jamd_refuse("jamd_frontend_live_push_dev: NULL buffer");
  if (frame_off) memcpy(frame_off, ooff.data(), sizeof(int) * (nchan + 1));
  if (!any) return JAMD_OK;
  hipStream_t st = jamd_stream(l->f->eng, stream);
  if ((rc = l->d_feat.grow((size_t)(N > 0 ? N : 1) * d.veclen * sizeof(float))) != JAMD_OK) return rc;
  if ((rc = l->d_stage.grow((size_t)(S > 0 ? S : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if (keep_rows && need_rows > l->hist_rows) {
    // the history grows: at least twofold, never beyond the cap; the rows of the open segments move over
    long long rows = 2LL * l->hist_rows > need_rows ? 2LL * l->hist_rows : need_rows;
    if (rows < 256) rows = 256;
    if (rows > l->hist_cap) rows = l->hist_cap;
    JamdDev<float> nh;
    if ((rc = nh.grow((size_t)nchan * rows * d.veclen * sizeof(float))) != JAMD_OK) return rc;
    if (l->d_hist && (rc = lv_launch_grow(l, st, nh, l->hist_rows, rows)) != JAMD_OK) return rc;
    l->d_hist.swap(nh);                        // (the old rows go with nh)
    l->hist_rows = (int)rows;
  }
  if ((rc = l->tab.send(ntab, st)) != JAMD_OK) return rc;
  const long long *d_coff = (const long long *)l->tab.d.p;
  const int *d_soff = (const int *)(d_coff + nchan + 1);
  const LvPacked pk{l->d_stage, d_coff, d_soff, d_soff + nchan + 1, d_soff + 2 * (nchan + 1)};
  if (S > 0 && (rc = lv_launch_pack(l, st, dev_samples, pk, S)) != JAMD_OK) return rc;
  const int *d_tabs;
  if ((rc = lv_base_frames(l->f, st, l->d_stage, soff.data(), nchan, B, {&boff, &noff, &ooff, &act, &told, &f0}, &d_tabs)) != JAMD_OK)
    return rc;
  if ((rc = lv_launch(l, st, d_tabs, N, O, &pk, dev_out)) != JAMD_OK) return rc;
  l->open.swap(open_after); l->ns.swap(ns_after);
  l->nopen = 0;
  for (int c = 0; c < nchan; c++) l->nopen += l->open[c] != 0;
  return JAMD_OK;
}

int jamd_frontend_live_run_host(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off, float *out,
                                int *frame_off) {
  if (!l || !samples || !sample_off || !out) return jamd_refuse("jamd_frontend_live_run_host: NULL argument");
  std::string err;
  long long O = 0;
  for (int c = 0; c < l->nchan; c++) {
    const long long n = fe_span("jamd_frontend_live_run_host", "channel", sample_off, c, err);
    if (n < 0) return jamd_refuse("%s", err.c_str());
    O += lv_counts(l->f->d, n).To;
  }
  return jamd_host_call(&l->stage, l->f->eng, samples, (size_t)sample_off[l->nchan], out, (size_t)O * l->f->d.veclen * l->f->d.splice,
                      [&](const int16_t *in, float *o, hipStream_t st) -> long long {
                        const int rc = jamd_frontend_live_run_dev(l, in, sample_off, o, frame_off, st);
                        return rc != JAMD_OK ? rc : O * l->f->d.veclen * l->f->d.splice;
                      });
}

int jamd_frontend_live_push_host(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off,
                                 const unsigned char *final, float *out, int *frame_off) {
  if (!l || !sample_off) return jamd_refuse("jamd_frontend_live_push_host: NULL argument");
  std::string err;
  long long O = 0;
  for (int c = 0; c < l->nchan; c++) {
    const long long n = fe_span("jamd_frontend_live_push_host", "channel", sample_off, c, err);
    if (n < 0) return jamd_refuse("%s", err.c_str());
    const bool fin = final && final[c];
    if (n == 0 && !(fin && l->open[c])) continue;
    O += jamd_frontend_live_push_frames(&l->f->d, l->open[c] ? l->ns[c] : 0, n, fin);
  }
  if ((sample_off[l->nchan] > 0 && !samples) || (O > 0 && !out))
    return jamd_refuse("jamd_frontend_live_push_host: NULL buffer");
  return jamd_host_call(&l->stage, l->f->eng, samples, (size_t)sample_off[l->nchan], out, (size_t)O * l->f->d.veclen * l->f->d.splice,
                      [&](const int16_t *in, float *o, hipStream_t st) -> long long {
                        const int rc = jamd_frontend_live_push_dev(l, in, sample_off, final, o, frame_off, st);
                        return rc != JAMD_OK ? rc : O * l->f->d.veclen * l->f->d.splice;
                      });
}

int jamd_frontend_live_commit(jamd_frontend_live *l, const unsigned char *update, void *stream) {
  if (!l) return jamd_refuse("jamd_frontend_live_commit: NULL object");
  for (int c = 0; c < l->nchan && l->nopen; c++)
    if (l->open[c] && (!update || update[c])) {
      jamd_set_error("jamd_frontend_live_commit: channel %d has an open segment (end it with a final push first)", c);
      return JAMD_ESTATE;
    }
  if (!l->p.mean && !l->p.var) return JAMD_OK;     // no CMNWork in the reference either
  JAMD_HIP(hipSetDevice(l->f->eng->device));
  hipStream_t st = jamd_stream(l->f->eng, stream);
  // (a copy from pageable memory has left the host array when the call returns)
  if (update) JAMD_HIP(hipMemcpyAsync(l->d_upd, update, (size_t)l->nchan, hipMemcpyHostToDevice, st));
  return lv_launch_commit(l, st, update ? l->d_upd : nullptr);
}

int jamd_frontend_cmn_read(const char *path, int veclen, int mfcc_dim, int want_var, float *cmean, float *cvar) {
  if (!path || !cmean || (want_var && !cvar)) return jamd_refuse("jamd_frontend_cmn_read: NULL argument");
  std::string err;
  const int r = cmnf_read(path, veclen, mfcc_dim, want_var != 0, cmean, cvar, err);
  if (r < 0) return jamd_refuse("jamd_frontend_cmn_read: %s: %s", path, err.c_str());
  return r;
}

int jamd_frontend_cmn_write(const char *path, int veclen, const float *cmean, const float *cvar) {
  if (!path || !cmean || veclen < 1) return jamd_refuse("jamd_frontend_cmn_write: NULL argument or veclen < 1");
  std::string err;
  if (cmnf_write(path, veclen, cmean, cvar, err) != 0) return jamd_refuse("jamd_frontend_cmn_write: %s", err.c_str());
  return JAMD_OK;
}

}  // extern "C"
