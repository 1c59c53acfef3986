// rejgmm_host.h -- the host side of GMM-based input rejection: the object, which rejgmm_api.hip builds and owns
// (validation, the model's tables, scratch, the verdict, the C ABI of jamd_rejgmm), and the launchers through which it
// reaches the kernels in rejgmm.hip.  The API unit launches nothing itself; a launcher checks nothing.  Internal, not
// installed.
#pragma once
#include <string>

#include "jamd_host.h"

struct JAMD_LOCAL jamd_rejgmm {
  jamd_engine *eng = nullptr;
  int D = 0, nmodel = 0, gprune_num = 0, maxmix = 0;
  JamdDev<float> d_mean, d_ivar, d_gconst, d_logw;
  JamdDev<int> d_st_off, d_ent_dens, d_model_state;
  JamdDev<int> d_utt_off;
  JamdStage<float, float> stage;           // scores_host: out is frame scores [T][nmodel] | utterance sums [nutt][nmodel]
  std::vector<std::string> names;          // model names / is_voice: only known when loaded from a file
  std::vector<unsigned char> is_voice;
};

// ---- rejgmm.hip
// Every model's score of every frame -> dev_out [T][nmodel]
JAMD_LOCAL int rejgmm_launch_frames(jamd_rejgmm *m, hipStream_t st, const float *dev_frames, int T, float *dev_out);
// The sums over the utterances m->d_utt_off [nutt + 1] describes -> dev_out [nutt][nmodel]
JAMD_LOCAL int rejgmm_launch_sums(jamd_rejgmm *m, hipStream_t st, const float *dev_frame_scores, int nutt, float *dev_out);
