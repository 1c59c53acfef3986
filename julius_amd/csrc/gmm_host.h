// gmm_host.h -- the host side of GMM scoring: the model object, which gmm_api.hip builds and owns (packing, validation,
// scratch, the C ABI of jamd_gmm), and the launchers through which it reaches the kernels: gmm_outprob.hip (K1, its
// narrow and generic-D forms, per-Gaussian scores) and gmm_pruned.hip (gprune safe, tied-mixture codebooks).
// gmm_api.hip launches nothing itself; a launcher checks nothing but what its kernel's shape demands.  Internal, not installed.
#pragma once
#include "jamd_host.h"

struct JAMD_LOCAL jamd_gmm {
  jamd_engine *eng = nullptr;
  int S = 0, D = 0, E = 0, nbook = 0;
  int gprune = 0, gprune_num = 0;
  int rec = 0;                    // floats per entry record
  int maxmix = 0;
  // device model
  JamdDev<float> d_rec;          // [E][rec]: mean[D], ivar[D], gconst, logw
  JamdDev<float> d_rec_ring;     // [E_plain][80], D = 39 only: the plain states' records again, in the order K1's record ring
                                  //   loads them -- five 64-byte chunks: [gconst, logw, mean 0..6, ivar 0..6], then
                                  //   [mean of 8 dims, ivar of the same 8 dims] for dims 7.., 15.., 23.., 31..38
  JamdDev<int> d_st_off;         // [S+1] original entry offsets (index d_ent_logw)
  JamdDev<int> d_st_off_plain;   // [S+1] offsets into d_rec; a tied-mixture state has an empty range
  int E_plain = 0;
  // tied-mixture
  JamdDev<int> d_st_book;        // [S]
  JamdDev<int> d_book_off;       // [nbook+1] into book records
  std::vector<int> h_book_off;    // host copy of the same
  JamdDev<float> d_book_rec;     // [sum book sizes][rec] (logw unused)
  JamdDev<float> d_ent_logw;     // [E] entry weights (tied states index by codebook position)
  JamdDev<int> d_tied_states;    // [ntied] ids of tied-mixture states
  int ntied = 0;
  int maxbook = 0;                // largest codebook
  int tm_cap = 0;                 // slots per (frame, book) in the codebook cache
  bool has_null = false;          // some mixture entry names no density (NULL density): K1 keeps its LOG_ZERO selects
  int hist_method = 0;            // JAMD_GPRUNE_HEU / _BEAM over tied-mixture codebooks (history pruning), else 0
  JamdPinned utt;                 // utt.d: int [cur_nutt + 1] utterance boundaries of the running call (a codebook's history -- heu /
  int cur_nutt = 0;               //   beam thresholds, safe's visiting order -- restarts at every utterance's first frame)
  // scratch
  JamdStage<float, float> stage;  // outprob_host
  JamdStage<float, float> dens_stage;   // dens_host
  JamdDev<float> d_tm_score; JamdDev<int> d_tm_id, d_tm_num;
  JamdDev<float> d_narrow;        // [kNarrowT][E_plain] weighted Gaussian scores of a narrow call (K1n, gmm_outprob.hip)
  JamdDev<int> d_tm_flag;         // [T][nbook] gprune safe: (frame, codebook)s whose list depends on the visiting order
  // K1's pull form (D = 39; gmm_deal.h, gmm_outprob.hip), set up once by jamd_gmm_pull_setup()
  JamdDev<int> d_pull_heads;      // eight ticket heads, one per 128-byte line, zeroed on the call's stream before a pull launch
  int pull_cap = 0;               // blocks of the pull kernel the device holds at once, rounded down to a multiple of 8
  int pull_min = 0;               // the pull form serves a call of more blocks than this (negative: never)
  int pull_grid = 0;              // blocks of a pull launch when > 0 (development), else pull_cap
  int pull_tail = -1;             // tiles at the end of every share dealt in pieces (gmm_deal.h); negative: the default
  int pull_sub = 0;               // states of such a piece; 0: kGdSub (gd_tail_make)
  char last_kernel[96] = {0};
};

// (The two older launchers keep the linkage they had.)
// ---- gmm_outprob.hip
// Plain states, every Gaussian (gprune none): K1, or K1n for a call of a handful of frames, or the generic-D kernel.
JAMD_LOCAL int jamd_gmm_launch_plain(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st);
// Once per model, from jamd_gmm_create(): what K1's pull form needs (the ticket heads, the device's capacity for the
// model's instantiation, the two development switches), so that the stream-ordered call allocates and asks nothing.
JAMD_LOCAL int jamd_gmm_pull_setup(jamd_gmm *g);
// Per-Gaussian scores out[T][E] of the E records at `rec` (the plain entries or the codebook Gaussians).
JAMD_LOCAL int jamd_gmm_launch_dens(jamd_gmm *g, const float *rec, int E, const float *frames, int T, float *out,
                                        hipStream_t st);

// ---- gmm_pruned.hip
// Plain states under gprune safe (K1s).
int jamd_gmm_launch_safe(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st);
// Tied-mixture states: the codebook cache c_score / c_id / c_num (K2, or K2h with history pruning; under any pruning
// the call's utterance boundaries are needed in g->utt.d), then -- unless out is NULL -- the states' scores from it.
int jamd_gmm_launch_tmix(jamd_gmm *g, const float *frames, int T, float *out, float *c_score,
                         int *c_id, int *c_num, hipStream_t st);
