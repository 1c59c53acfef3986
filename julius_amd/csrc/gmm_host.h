// gmm_host.h -- the host side of GMM scoring: the model object, which gmm_api.hip builds and owns (packing, validation,
// scratch, the C ABI of jamd_gmm), and the launchers through which it reaches the kernels: gmm_outprob.hip (K1, its
// narrow and generic-D forms, per-Gaussian scores) and gmm_pruned.hip (gprune safe, tied-mixture codebooks).
// gmm_api.hip launches nothing itself; a launcher checks nothing but what its kernel's shape demands.  Internal, not installed.
#pragma once
#include <vector>

#include "jamd_internal.h"

struct jamd_gmm {
  jamd_engine *eng = nullptr;
  int S = 0, D = 0, E = 0, nbook = 0;
  int gprune = 0, gprune_num = 0;
  int rec = 0;                    // floats per entry record
  int maxmix = 0;
  // device model
  float *d_rec = nullptr;         // [E][rec]: mean[D], ivar[D], gconst, logw
  float *d_rec_ring = nullptr;    // [E_plain][80], D = 39 only: the plain states' records again, in the order K1's record ring
                                  //   loads them -- five 64-byte chunks: [gconst, logw, mean 0..6, ivar 0..6], then
                                  //   [mean of 8 dims, ivar of the same 8 dims] for dims 7.., 15.., 23.., 31..38
  int *d_st_off = nullptr;        // [S+1] original entry offsets (index d_ent_logw)
  int *d_st_off_plain = nullptr;  // [S+1] offsets into d_rec; a tied-mixture state has an empty range
  int E_plain = 0;
  // tied-mixture
  int *d_st_book = nullptr;       // [S]
  int *d_book_off = nullptr;      // [nbook+1] into book records
  std::vector<int> h_book_off;    // host copy of the same
  float *d_book_rec = nullptr;    // [sum book sizes][rec] (logw unused)
  float *d_ent_logw = nullptr;    // [E] entry weights (tied states index by codebook position)
  int *d_tied_states = nullptr;   // [ntied] ids of tied-mixture states
  int ntied = 0;
  int maxbook = 0;                // largest codebook
  int tm_cap = 0;                 // slots per (frame, book) in the codebook cache
  bool has_null = false;          // some mixture entry names no density (NULL density): K1 keeps its LOG_ZERO selects
  int hist_method = 0;            // JAMD_GPRUNE_HEU / _BEAM over tied-mixture codebooks (history pruning), else 0
  int *d_cur_utt_off = nullptr;   // [cur_nutt + 1] utterance boundaries of the running call (a codebook's history -- heu / beam
  int cur_nutt = 0; size_t utt_off_bytes = 0;   //   thresholds, safe's visiting order -- restarts at every utterance's first frame)
  // scratch
  float *d_frames = nullptr; size_t frames_cap = 0;
  float *d_out = nullptr; size_t out_cap = 0;
  float *d_tm_score = nullptr; int *d_tm_id = nullptr; int *d_tm_num = nullptr;
  float *d_narrow = nullptr; size_t narrow_cap = 0;   // [kNarrowT][E_plain] weighted Gaussian scores of a narrow call (K1n, gmm_outprob.hip)
  size_t tm_cap_bytes = 0, tm_id_bytes = 0, tm_num_bytes = 0;
  int *d_tm_flag = nullptr; size_t tm_flag_bytes = 0;   // [T][nbook] gprune safe: (frame, codebook)s whose list depends on the visiting order
  char last_kernel[64] = {0};
  // pinned staging copy of the running call's utterance boundaries (history pruning only) and the event behind its
  // upload: the buffer is rewritten only when the copy that read it is done
  int *h_utt_off = nullptr; size_t h_utt_off_cap = 0; hipEvent_t ev_utt_off = nullptr;
};

// The launchers added with this header stay inside the library (the two older ones keep the linkage they had).
#define JAMD_GMM_LOCAL __attribute__((visibility("hidden")))

// ---- gmm_outprob.hip
// Plain states, every Gaussian (gprune none): K1, or K1n for a call of a handful of frames, or the generic-D kernel.
JAMD_GMM_LOCAL int jamd_gmm_launch_plain(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st);
// Per-Gaussian scores out[T][E] of the E records at `rec` (the plain entries or the codebook Gaussians).
JAMD_GMM_LOCAL int jamd_gmm_launch_dens(jamd_gmm *g, const float *rec, int E, const float *frames, int T, float *out,
                                        hipStream_t st);

// ---- gmm_pruned.hip
// Plain states under gprune safe (K1s).
int jamd_gmm_launch_safe(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st);
// Tied-mixture states: the codebook cache c_score / c_id / c_num (K2, or K2h with history pruning; under any pruning
// the call's utterance boundaries are needed in d_cur_utt_off), then -- unless out is NULL -- the states' scores from it.
int jamd_gmm_launch_tmix(jamd_gmm *g, const float *frames, int T, float *out, float *c_score,
                         int *c_id, int *c_num, hipStream_t st);
