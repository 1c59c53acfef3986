// fvad_api.hip -- the C ABI of the voice-activity detector (jamd_fvad_*): validation, the object and the per-channel
// cores it keeps on the device, the table of a push with its closed-form frame counts, the model file.  It launches
// nothing: the kernels and their launchers are in fvad.hip (fvad_host.h).
#include "fvad_host.h"

extern "C" {

int jamd_fvad_model_read(const char *path, jamd_fvad_model *m) {
  if (!path || !m) return jamd_refuse("jamd_fvad_model_read: NULL argument");
  std::string err;
  if (!fv_model_read(path, m, err)) return jamd_refuse("jamd_fvad_model_read: %s: %s", path, err.c_str());
  return JAMD_OK;
}

int64_t jamd_fvad_frames(const jamd_fvad_desc *d, int64_t samples_before, int64_t chunk) {
  if (!d) return jamd_refuse("jamd_fvad_frames: the descriptor is NULL");
  const int fs = fv_frame_size(d->sfreq);
  if (!fs) return jamd_refuse("jamd_fvad_frames: sfreq %d: the detector takes 8000 or 16000", d->sfreq);
  if (samples_before < 0 || chunk < 0) return jamd_refuse("jamd_fvad_frames: a negative sample count");
  return fv_frames_done(samples_before + chunk, fs) - fv_frames_done(samples_before, fs);
}

void jamd_fvad_destroy(jamd_fvad *f) {
  if (!f) return;
  delete f;                                  // (the engine is not looked at: it may have gone first)
}

int jamd_fvad_create(jamd_engine *e, const jamd_fvad_desc *d, int nchan, jamd_fvad **out) {
  if (!e || !d || !out || nchan < 1 || nchan > 65535) return jamd_refuse("jamd_fvad_create: NULL argument or nchan not in 1 ... 65535");
  *out = nullptr;
  std::string err;
  if (!fv_check_desc(d, err)) return jamd_refuse("jamd_fvad_create: %s", err.c_str());
  std::unique_ptr<jamd_fvad> f(new jamd_fvad());   // (its members own what they hold)
  f->eng = e; f->nchan = nchan; f->sfreq = d->sfreq; f->mode = d->mode; f->fs = fv_frame_size(d->sfreq);
  f->arrived.assign(nchan, 0);
  const size_t C = nchan;
  const FvModel m = fv_model(d->model, d->mode);
  int rc;
  JAMD_HIP(hipSetDevice(e->device));
  if ((rc = f->d_model.upload(&m, 1)) != JAMD_OK || (rc = f->d_s16.alloc(C * kFvKept)) != JAMD_OK ||
      (rc = f->d_s32.alloc(C * 3)) != JAMD_OK || (rc = f->d_pend.alloc(C * kFvMaxFrame, true)) != JAMD_OK ||
      (rc = f->d_npend.alloc(C, true)) != JAMD_OK || (rc = f->d_mask.alloc(C)) != JAMD_OK)
    return rc;
  if ((rc = fv_launch_reset(f.get(), e->stream, nullptr)) != JAMD_OK) return rc;
  JAMD_HIP(hipStreamSynchronize(e->stream));   // (a push may come on another stream)
  *out = f.release();
  return JAMD_OK;
}

int jamd_fvad_reset(jamd_fvad *f, const unsigned char *mask, void *stream) {
  if (!f) return jamd_refuse("jamd_fvad_reset: NULL object");
  JAMD_HIP(hipSetDevice(f->eng->device));
  hipStream_t st = jamd_stream(f->eng, stream);
  // (a copy from pageable memory has left the host array when the call returns)
  if (mask) JAMD_HIP(hipMemcpyAsync(f->d_mask, mask, (size_t)f->nchan, hipMemcpyHostToDevice, st));
  int rc;
  if ((rc = fv_launch_reset(f, st, mask ? f->d_mask : nullptr)) != JAMD_OK) return rc;
  for (int c = 0; c < f->nchan; c++)
    if (!mask || mask[c]) f->arrived[c] = 0;
  return JAMD_OK;
}

int jamd_fvad_push_dev(jamd_fvad *f, const int16_t *dev_in, const int64_t *in_off, unsigned char *dev_out, int64_t *out_off,
                       void *stream) {
  if (!f || !in_off || !out_off) return jamd_refuse("jamd_fvad_push_dev: NULL argument");
  const int nchan = f->nchan;
  int rc;
  JAMD_HIP(hipSetDevice(f->eng->device));
  if ((rc = f->tab.begin(nchan * sizeof(FvChanTab))) != JAMD_OK) return rc;
  FvChanTab *h_ch = (FvChanTab *)f->tab.h.p;
  long long nin = 0, nout = 0;
  for (int c = 0; c < nchan; c++) {
    long long n;
    if ((rc = jamd_span("jamd_fvad_push_dev", in_off, c, &n)) != JAMD_OK) return rc;
    const long long nf = fv_frames_done(f->arrived[c] + n, f->fs) - fv_frames_done(f->arrived[c], f->fs);
    h_ch[c] = FvChanTab{in_off[c], nout, (int)n, (int)nf};
    out_off[c] = nout;
    nin += n; nout += nf;
  }
  out_off[nchan] = nout;
  if ((nin > 0 && !dev_in) || (nout > 0 && !dev_out)) return jamd_refuse("jamd_fvad_push_dev: NULL buffer");
  if (nin == 0) return JAMD_OK;              // every channel idle
  hipStream_t st = jamd_stream(f->eng, stream);
  if ((rc = f->tab.send(nchan * sizeof(FvChanTab), st)) != JAMD_OK) return rc;
  if ((rc = fv_launch_push(f, st, (const FvChanTab *)f->tab.d.p, dev_in, dev_out)) != JAMD_OK) return rc;
  for (int c = 0; c < nchan; c++) f->arrived[c] += h_ch[c].n;
  return JAMD_OK;
}

int jamd_fvad_push_host(jamd_fvad *f, const int16_t *samples, const int64_t *in_off, unsigned char *out, int64_t *out_off) {
  if (!f || !in_off || !out_off) return jamd_refuse("jamd_fvad_push_host: NULL argument");
  int rc;
  long long cap = 0;
  for (int c = 0; c < f->nchan; c++) {
    long long n;
    if ((rc = jamd_span("jamd_fvad_push_host", in_off, c, &n)) != JAMD_OK) return rc;
    cap += fv_frames_done(f->arrived[c] + n, f->fs) - fv_frames_done(f->arrived[c], f->fs);
  }
  const long long lo = in_off[0], ns = in_off[f->nchan] - lo;
  if ((ns > 0 && !samples) || (cap > 0 && !out)) return jamd_refuse("jamd_fvad_push_host: NULL buffer");
  std::vector<int64_t> off(f->nchan + 1);    // the staged samples start at 0
  for (int c = 0; c <= f->nchan; c++) off[c] = in_off[c] - lo;
  return jamd_host_call(&f->stage, f->eng, ns > 0 ? samples + lo : nullptr, (size_t)(ns > 0 ? ns : 0), out, (size_t)cap,
                        [&](const int16_t *in, unsigned char *o, hipStream_t st) -> long long {
                          const int r = jamd_fvad_push_dev(f, in, off.data(), o, out_off, st);
                          return r != JAMD_OK ? r : out_off[f->nchan];
                        });
}

int jamd_fvad_state_get(jamd_fvad *f, int chan, int *state) {
  if (!f || !state || chan < 0 || chan >= f->nchan) return jamd_refuse("jamd_fvad_state_get: NULL argument or channel out of range");
  JAMD_HIP(hipSetDevice(f->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  const size_t C = f->nchan;
  short s16[kFvKept];
  int s32[3], npend;
  JAMD_HIP(hipMemcpy2D(s16, sizeof(short), f->d_s16 + chan, C * sizeof(short), sizeof(short), kFvKept, hipMemcpyDeviceToHost));
  JAMD_HIP(hipMemcpy2D(s32, sizeof(int), f->d_s32 + chan, C * sizeof(int), sizeof(int), 3, hipMemcpyDeviceToHost));
  JAMD_HIP(hipMemcpy(&npend, f->d_npend + chan, sizeof(int), hipMemcpyDeviceToHost));
  fv_state_ints(s16, s32, npend, state);
  return JAMD_OK;
}

}  // extern "C"
