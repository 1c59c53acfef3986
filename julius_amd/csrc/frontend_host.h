// frontend_host.h -- the host side of the audio front end: the two objects, which frontend_api.hip (jamd_frontend,
// buffered input) and frontend_live_api.hip (jamd_frontend_live, made from a jamd_frontend) build and own -- validation,
// offset tables, scratch, the C ABI -- and the launchers through which they reach the kernels: frontend.hip (frame
// kernel, noise spectrum, the chain behind the base coefficients) and frontend_live.hip (the live chain, commit).  The
// API units launch nothing themselves; a launcher checks nothing.  What needs no device is in frontend_tables.h.
// Internal, not installed.
#pragma once
#include <initializer_list>

#include "jamd_host.h"
#include "frontend_tables.h"

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

struct JAMD_LOCAL jamd_frontend {
  jamd_engine *eng = nullptr;
  jamd_frontend_desc d{};                    // as created (cmean_init / cvar_init NULL); nothing alters it afterwards
  FeTables tb;
  FeParams p{};
  size_t lds = 0;
  int fpb = 0;                               // frames (waves) per workgroup of the frame kernel (fe_reserve_lds)
  JamdDev<double> t_ham, t_twRe, t_twIm, t_dct, t_wcep, t_cvar_sqrt;   // the device tables p names
  JamdDev<short> t_loChan;
  JamdDev<float> t_loWt, t_cmean;
  JamdDev<int> t_kfirst, t_klast;
  // scratch of a run; a live object made from this one shares d_stat and off (one stream per object)
  JamdDev<float> d_stat, d_feat;
  JamdDev<float> d_ms;                       // mean[nutt][veclen] | sd[nutt][veclen] | emax[nutt]
  JamdPinned off;                            // soff (int64 [nutt + 1]) | int32 tables [nutt + 1]: foff, ...
  JamdStage<int16_t, float> stage;           // run_host, noise_host
  // spectral subtraction (jamd_frontend_set_ss)
  int ss_mode = JAMD_SS_OFF;
  long long ss_head = 0;                     // -sscalclen in samples
  float ss_alpha = 0.f, ss_floor = 0.f;
  JamdDev<float> d_ssload;                   // -ssload: the one spectrum [fftN]
  JamdDev<float> d_noise;                    // -sscalc: [nutt][fftN]
  JamdDev<double> d_mag;                     // |X| of the head frames [head frames][fftN]
};

// sample_off and the int tables `tabs` (each [nutt + 1]) -> f->off.d, back to back, on `st`.
static inline int fe_put_offsets(jamd_frontend *f, hipStream_t st, const int64_t *sample_off, int nutt,
                                 std::initializer_list<const std::vector<int> *> tabs) {
  const size_t row = sizeof(int) * (nutt + 1), offb = sizeof(long long) * (nutt + 1) + tabs.size() * row;
  int rc;
  if ((rc = f->off.begin(offb)) != JAMD_OK) return rc;
  memcpy(f->off.h.p, sample_off, sizeof(long long) * (nutt + 1));
  char *q = f->off.h.p + sizeof(long long) * (nutt + 1);
  for (const std::vector<int> *t : tabs) { memcpy(q, t->data(), row); q += row; }
  return f->off.send(offb, st);
}

// ---- frontend.hip
// The frame kernel's workgroup shape and dynamic LDS for f->tb -> f->fpb, f->lds, reserved on every kernel that takes it.
JAMD_LOCAL int fe_reserve_lds(jamd_frontend *f);
// WMP_calc() of the T frames d_foff describes -> f->d_stat [T][baselen]: frame t of utterance u is the window at
// d_soff[u] + t * frameshift.  By f->ss_mode with the spectrum f->d_ssload, or row u of f->d_noise (JAMD_SS_CALC).
JAMD_LOCAL int fe_launch_frames(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const long long *d_soff,
                                   const int *d_foff, int nutt, int T);
// The noise spectrum of the Htot head frames d_hoff describes -> dev_noise [nutt][fftN] (grows f->d_mag)
JAMD_LOCAL int fe_launch_noise(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const long long *d_soff,
                                  const int *d_hoff, int nutt, int Htot, float *dev_noise);
// Behind the base coefficients of a buffered run: f->d_stat -> energy maximum, deltas (f->d_feat), statistics (f->d_ms)
// where the kind needs them, then the Tout normalised, spliced rows -> dev_out.
JAMD_LOCAL int fe_launch_feats(jamd_frontend *f, hipStream_t st, const int *d_foff, const int *d_ooff, int nutt, int T,
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

struct JAMD_LOCAL jamd_frontend_live {
  jamd_frontend *f = nullptr;                // the parent: descriptor, ss_mode, frame kernel, d_stat and off
  int nchan = 0;
  LvParams p{};
  LvState s{};
  JamdDev<char> state;                       // one allocation behind every array of `s`
  JamdDev<float> d_feat;
  JamdDev<unsigned char> d_upd;              // [nchan] the commit mask
  JamdStage<int16_t, float> stage;           // run_host, push_host
  // open segments (jamd_frontend_live_push_*): per channel whether one is open and the samples it has taken
  std::vector<char> open;
  std::vector<long long> ns;
  int nopen = 0;
  JamdDev<int16_t> d_stage;                  // [residue | chunk] of every channel
  JamdPinned tab;                            // coff (int64 [nchan + 1]) | soff | rlen | newr (int [nchan + 1])
  JamdDev<float> d_hist;                     // [nchan][hist_rows][veclen], cvn with splice 1 only
  int hist_rows = 0, hist_cap = kHistDefault;
};

// ---- frontend_live.hip
// A push's staged batch and its tables on the device (l->tab.d)
struct LvPacked { const int16_t *staged; const long long *coff; const int *soff, *rlen, *newr; };
// [residue | chunk] of every channel, S samples in all -> pk.staged
JAMD_LOCAL int lv_launch_pack(jamd_frontend_live *l, hipStream_t st, const int16_t *dev_samples, const LvPacked &pk, long long S);
// What both entries launch behind the base frames (l->f->d_stat): d_tabs are boff | noff | ooff | act | told | f0 on the
// device, N feature frames and O rows in all.  pk (a push) names the staged batch; a whole segment has none, and one
// table of zeros behind act serves as its told and its f0.
JAMD_LOCAL int lv_launch(jamd_frontend_live *l, hipStream_t st, const int *d_tabs, long long N, long long O,
                            const LvPacked *pk, float *dev_out);
// [nchan][from][veclen] of l->d_hist -> [nchan][to][veclen] at dst, and the stream waited for (JAMD_ELAUNCH with the error set)
JAMD_LOCAL int lv_launch_grow(jamd_frontend_live *l, hipStream_t st, float *dst, long long from_rows, long long to_rows);
// CMN_realtime_update() of the channels d_mask names (NULL: all)
JAMD_LOCAL int lv_launch_commit(jamd_frontend_live *l, hipStream_t st, const unsigned char *d_mask);
