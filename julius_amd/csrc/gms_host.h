// gms_host.h -- the host side of Gaussian mixture selection: the object, which gms_api.hip builds and owns (validation,
// the selection model, scratch, the C ABI of jamd_gms), and the launcher through which it reaches the kernels in
// gms.hip.  The API unit launches nothing itself; the launcher checks nothing.  Internal, not installed.
#pragma once
#include "jamd_host.h"

struct JAMD_LOCAL jamd_gms {
  jamd_engine *eng = nullptr;
  jamd_gmm *gs = nullptr;          // the selection model (per-Gaussian scores)
  int Sgs = 0, Egs = 0, S = 0, nbest = 0, strict = 0;
  JamdDev<int> d_st_off;           // [Sgs + 1]
  JamdDev<float> d_logw;           // [Egs]
  JamdDev<int> d_state2gs;         // [S]
  JamdDev<int> d_utt_off;
  JamdDev<float> d_dens, d_fs;
  JamdStage<float, float> stage;   // apply_host: the frames up, the scores up and down
  ~jamd_gms() { if (gs) jamd_gmm_destroy(gs); }
};

// The selection kernel's dynamic LDS: fs[Sgs] | idx[Sgs] | last[Sgs] | st_off[Sgs+1] | logw[Egs] | padding | row[2][EgsPad]
static inline int gms_egs_pad(int Egs) { return (Egs + 63) & ~63; }
static inline size_t gms_lds_bytes(int Sgs, int Egs) {
  return sizeof(float) * ((size_t)3 * Sgs + Sgs + 1 + Egs + 64 + 2 * (size_t)gms_egs_pad(Egs));
}

// ---- gms.hip
// m->d_dens (the selection model's per-Gaussian scores of T frames) and m->d_utt_off [nutt + 1] -> m->d_fs; then the
// fallback scores into dev_scores [T][S]
JAMD_LOCAL int gms_launch(jamd_gms *m, hipStream_t st, int T, int nutt, float *dev_scores);
