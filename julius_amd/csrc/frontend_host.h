// frontend_host.h -- the host side of the audio front end: the two objects, which frontend_api.hip (jamd_frontend,
// buffered input) and frontend_live_api.hip (jamd_frontend_live, made from a jamd_frontend) build and own -- validation,
// offset tables, scratch, the C ABI -- and the launchers through which they reach the kernels: frontend.hip (frame
// kernel, noise spectrum, the chain behind the base coefficients) and frontend_live.hip (the live chain, commit).  The
// API units launch nothing themselves; a launcher checks nothing.  What needs no device is in frontend_tables.h.
// Internal, not installed.
#pragma once
#include <initializer_list>

#include "jamd_internal.h"
#include "frontend_tables.h"

#define JAMD_FE_LOCAL __attribute__((visibility("hidden")))

// ---- shared by both objects
// A table that goes up through pinned memory: `h` is rewritten only once the upload that read it is done.
struct FePinned { char *h = nullptr, *d = nullptr; size_t h_cap = 0, d_cap = 0; hipEvent_t ev = nullptr; };
// Waits for the last upload and makes room: `h` may then be filled with `bytes`.
static inline int fe_pin_begin(FePinned *t, size_t bytes) {
  int rc;
  if ((rc = jamd_grow(&t->d, &t->d_cap, bytes)) != JAMD_OK) return rc;
  if (t->ev) JAMD_HIP(hipEventSynchronize(t->ev));
  else JAMD_HIP(hipEventCreateWithFlags(&t->ev, hipEventDisableTiming));
  if (t->h_cap < bytes) {
    if (t->h) JAMD_HIP(hipHostFree(t->h));
    t->h = nullptr; t->h_cap = 0;
    JAMD_HIP(hipHostMalloc((void **)&t->h, bytes, hipHostMallocDefault));
    t->h_cap = bytes;
  }
  return JAMD_OK;
}
static inline int fe_pin_send(FePinned *t, size_t bytes, hipStream_t st) {
  JAMD_HIP(hipMemcpyAsync(t->d, t->h, bytes, hipMemcpyHostToDevice, st));
  JAMD_HIP(hipEventRecord(t->ev, st));
  return JAMD_OK;
}
static inline void fe_pin_free(FePinned *t) {
  (void)hipFree(t->d);
  if (t->ev) { (void)hipEventSynchronize(t->ev); (void)hipEventDestroy(t->ev); }
  if (t->h) (void)hipHostFree(t->h);
}

// The _host form of an entry around its _dev form: ns samples up to d_in, dev(d_in, d_out, stream) on the engine's
// stream, nout values down from d_out, and the stream waited for.
struct FeStage { int16_t *d_in = nullptr; size_t in_cap = 0; float *d_out = nullptr; size_t out_cap = 0; };
template <typename Dev>
static int fe_host_call(FeStage *g, jamd_engine *eng, const int16_t *samples, size_t ns, float *out, size_t nout, Dev dev) {
  JAMD_HIP(hipSetDevice(eng->device));
  int rc;
  if ((rc = jamd_grow(&g->d_in, &g->in_cap, (ns > 0 ? ns : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&g->d_out, &g->out_cap, (nout > 0 ? nout : 1) * sizeof(float))) != JAMD_OK) return rc;
  hipStream_t st = eng->stream;
  if (ns) JAMD_HIP(hipMemcpyAsync(g->d_in, samples, ns * sizeof(int16_t), hipMemcpyHostToDevice, st));
  if ((rc = dev(g->d_in, g->d_out, st)) != JAMD_OK) return rc;
  if (nout) JAMD_HIP(hipMemcpyAsync(out, g->d_out, nout * sizeof(float), hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  return JAMD_OK;
}

// A refused argument: `if (bad) return fe_refuse("...", ...);` sets the error text and returns JAMD_EINVAL.
__attribute__((format(printf, 1, 2))) static inline int fe_refuse(const char *fmt, ...) {
  char b[512];                               // (what jamd_last_error() keeps)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  jamd_set_error("%s", b);
  return JAMD_EINVAL;
}

// ---- the buffered front end
struct FeParams {
  int framesize, frameshift, fftN, logn, klo, khi, fbank_num, mfcc_dim, baselen, veclen, splice, nutt;
  int zmean, energy, raw_e, c0, fbank_only, log_fbank, usepower;
  int enormal, delta, acc, absesup, delWin, accWin, cmn, cvn, cmean_static, cvar_static, basedim;
  float preEmph, sqrt2var, escale, silFloor;
  const double *ham, *twRe, *twIm, *dct, *wcep, *cvar_sqrt;
  const short *loChan;
  const float *loWt, *cmean;
  const int *kfirst, *klast;
};

struct jamd_frontend {
  jamd_engine *eng = nullptr;
  jamd_frontend_desc d{};                    // as created (cmean_init / cvar_init NULL); nothing alters it afterwards
  FeTables tb;
  FeParams p{};
  size_t lds = 0;
  int fpb = 0;                               // frames (waves) per workgroup of the frame kernel (fe_reserve_lds)
  std::vector<void *> owned;                 // device tables
  // scratch of a run; a live object made from this one shares d_stat and off (one stream per object)
  float *d_stat = nullptr; size_t stat_cap = 0;
  float *d_feat = nullptr; size_t feat_cap = 0;
  float *d_ms = nullptr; size_t ms_cap = 0;  // mean[nutt][veclen] | sd[nutt][veclen] | emax[nutt]
  FePinned off;                              // soff (int64 [nutt + 1]) | int32 tables [nutt + 1]: foff, ...
  FeStage stage;                             // run_host, noise_host
  // spectral subtraction (jamd_frontend_set_ss)
  int ss_mode = JAMD_SS_OFF;
  long long ss_head = 0;                     // -sscalclen in samples
  float ss_alpha = 0.f, ss_floor = 0.f;
  float *d_ssload = nullptr;                 // -ssload: the one spectrum [fftN]
  float *d_noise = nullptr; size_t noise_cap = 0;   // -sscalc: [nutt][fftN]
  double *d_mag = nullptr; size_t mag_cap = 0;      // |X| of the head frames [head frames][fftN]
};

// sample_off and the int tables `tabs` (each [nutt + 1]) -> f->off.d, back to back, on `st`.
static inline int fe_put_offsets(jamd_frontend *f, hipStream_t st, const int64_t *sample_off, int nutt,
                                 std::initializer_list<const std::vector<int> *> tabs) {
  const size_t row = sizeof(int) * (nutt + 1), offb = sizeof(long long) * (nutt + 1) + tabs.size() * row;
  int rc;
  if ((rc = fe_pin_begin(&f->off, offb)) != JAMD_OK) return rc;
  memcpy(f->off.h, sample_off, sizeof(long long) * (nutt + 1));
  char *q = f->off.h + sizeof(long long) * (nutt + 1);
  for (const std::vector<int> *t : tabs) { memcpy(q, t->data(), row); q += row; }
  return fe_pin_send(&f->off, offb, st);
}

// ---- frontend.hip
// The frame kernel's workgroup shape and dynamic LDS for f->tb -> f->fpb, f->lds, reserved on every kernel that takes it.
JAMD_FE_LOCAL int fe_reserve_lds(jamd_frontend *f);
// WMP_calc() of the T frames d_foff describes -> f->d_stat [T][baselen]: frame t of utterance u is the window at
// d_soff[u] + t * frameshift.  By f->ss_mode with the spectrum f->d_ssload, or row u of f->d_noise (JAMD_SS_CALC).
JAMD_FE_LOCAL int fe_launch_frames(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const long long *d_soff,
                                   const int *d_foff, int nutt, int T);
// The noise spectrum of the Htot head frames d_hoff describes -> dev_noise [nutt][fftN] (grows f->d_mag)
JAMD_FE_LOCAL int fe_launch_noise(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const long long *d_soff,
                                  const int *d_hoff, int nutt, int Htot, float *dev_noise);
// Behind the base coefficients of a buffered run: f->d_stat -> energy maximum, deltas (f->d_feat), statistics (f->d_ms)
// where the kind needs them, then the Tout normalised, spliced rows -> dev_out.
JAMD_FE_LOCAL int fe_launch_feats(jamd_frontend *f, hipStream_t st, const int *d_foff, const int *d_ooff, int nutt, int T,
                                  long long Tout, float *dev_out);

// ---- the live front end
#define LV_CPMAX 500            // mfcc.h:47-48
#define LV_CPSTEP 5

// Segments in the history of one channel.  CMN_realtime_update() sums the list newest first until CPMAX frames are
// reached, and lengthens the list (by CPSTEP) only while the whole list plus the new segment stays below CPMAX; every
// entry holds a frame or more, so clist_max never passes CPMAX - 1 + CPSTEP.
constexpr int kRing = 512;
constexpr int kSet = 1, kLoaded = 2;         // flags: cmean_init_set, loaded_from_file
// per-call channel bits: takes part; the variance is re-estimated; the segment was open before; it ends here
constexpr int kActive = 1, kReest = 2, kCont = 4, kFinal = 8;
constexpr int kHistDefault = 3000;           // rows of an open segment kept for the re-estimation (jamd_frontend_live_stream_cap())

struct LvParams {
  int nchan, veclen, baselen, nb, splice, delta, acc, delWin, accWin, Bd, Ba, enorm, mean, var, mfcc_dim, do_map;
  int R, fs;                                 // slots of the base-vector ring; framesize
  float escale, silFloor, cweight;
};

struct LvState {
  float *emax;                               // [nchan] ENERGYWork.max
  float *cmean, *cvar;                       // [nchan][veclen] cmean_init, cvar_init
  int *flags;                                // [nchan] kSet | kLoaded
  float *now_sum, *now_var; int *now_fn;     // CMNWork.now
  float *all_var; int *all_fn;               // CMNWork.all
  float *ring_sum; int *ring_fn;             // [nchan][kRing][veclen] / [nchan][kRing]: clist, newest at head
  int *head, *cnum, *cmax;                   // [nchan]
  // the open segment of a channel (jamd_frontend_live_push_*)
  float *rmax;                               // [nchan] ENERGYWork.max so far
  float *ring;                               // [nchan][R][baselen] raw base vectors, frame t in slot t % R
  float *sp;                                 // [nchan][splice - 1][veclen] normalised vectors, frame t in slot t % (splice - 1)
  int16_t *res;                              // [nchan][framesize] samples behind the last whole window
};

struct jamd_frontend_live {
  jamd_frontend *f = nullptr;                // the parent: descriptor, ss_mode, frame kernel, d_stat and off
  int nchan = 0;
  LvParams p{};
  LvState s{};
  void *state = nullptr;                     // one allocation behind every array of `s`
  float *d_feat = nullptr; size_t feat_cap = 0;
  unsigned char *d_upd = nullptr;            // [nchan] the commit mask
  FeStage stage;                             // run_host, push_host
  // open segments (jamd_frontend_live_push_*): per channel whether one is open and the samples it has taken
  std::vector<char> open;
  std::vector<long long> ns;
  int nopen = 0;
  int16_t *d_stage = nullptr; size_t stage_cap = 0;   // [residue | chunk] of every channel
  FePinned tab;                              // coff (int64 [nchan + 1]) | soff | rlen | newr (int [nchan + 1])
  float *d_hist = nullptr;                   // [nchan][hist_rows][veclen], cvn with splice 1 only
  int hist_rows = 0, hist_cap = kHistDefault;
};

// ---- frontend_live.hip
// A push's staged batch and its tables on the device (l->tab.d)
struct LvPacked { const int16_t *staged; const long long *coff; const int *soff, *rlen, *newr; };
// [residue | chunk] of every channel, S samples in all -> pk.staged
JAMD_FE_LOCAL int lv_launch_pack(jamd_frontend_live *l, hipStream_t st, const int16_t *dev_samples, const LvPacked &pk, long long S);
// What both entries launch behind the base frames (l->f->d_stat): d_tabs are boff | noff | ooff | act | told | f0 on the
// device, N feature frames and O rows in all.  pk (a push) names the staged batch; a whole segment has none, and one
// table of zeros behind act serves as its told and its f0.
JAMD_FE_LOCAL int lv_launch(jamd_frontend_live *l, hipStream_t st, const int *d_tabs, long long N, long long O,
                            const LvPacked *pk, float *dev_out);
// [nchan][from][veclen] of l->d_hist -> [nchan][to][veclen] at dst, and the stream waited for (JAMD_ELAUNCH with the error set)
JAMD_FE_LOCAL int lv_launch_grow(jamd_frontend_live *l, hipStream_t st, float *dst, long long from_rows, long long to_rows);
// CMN_realtime_update() of the channels d_mask names (NULL: all)
JAMD_FE_LOCAL int lv_launch_commit(jamd_frontend_live *l, hipStream_t st, const unsigned char *d_mask);
