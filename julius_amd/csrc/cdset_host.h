// cdset_host.h -- the host side of the state-set scores: the object, which cdset_api.hip builds and owns (validation,
// the set tables, the C ABI of jamd_cdset), and the launcher through which it reaches the kernel in cdset.hip.  The API
// unit launches nothing itself; the launcher checks nothing.  Internal, not installed.
#pragma once
#include "jamd_host.h"

struct JAMD_LOCAL jamd_cdset {
  jamd_engine *eng = nullptr;
  int nset = 0, nstates = 0, method = 0, nbest = 0, maxset = 0;
  JamdDev<int> d_off, d_states;            // [nset + 1], [nstates]
};

// ---- cdset.hip
// The score of every set in every of the T rows of dev_scores [T][nstate] -> dev_cd [T][nset]
JAMD_LOCAL int cdset_launch(jamd_cdset *c, hipStream_t st, const float *dev_scores, int T, int nstate, float *dev_cd);
