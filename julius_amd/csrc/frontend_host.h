// frontend_host.h -- what csrc/frontend_live.hip takes from csrc/frontend.hip.  The live front end is made from a
// created jamd_frontend and launches its frame kernel (WMP_calc(), bit for bit) at the live frame grid; the kernel, its
// tables and the struct stay where they are, in frontend.hip, and the live unit reaches them through the calls below.
// No device code crosses the two units.
#pragma once
#include "jamd_internal.h"
#include <vector>

struct FeInfo {
  jamd_engine *eng;
  jamd_frontend_desc d;                      // as created (cmean_init / cvar_init NULL)
  int ss_mode;                               // JAMD_SS_* as jamd_frontend_set_ss() left it
  int fftN;
};
void fe_info(const jamd_frontend *f, FeInfo *out);

// The base coefficients of the frames tabs[0] (foff) describes: uploads sample_off and the int tables `tabs` (each
// [nutt + 1]) through the parent's pinned staging, then launches fe_frame_kernel<kSS> (kSS by the parent's ss_mode,
// which must not be JAMD_SS_CALC) over foff[nutt] frames on `st`: frame t of utterance u is the window at
// sample_off[u] + t * frameshift.  foff[nutt] == 0 launches nothing.  *d_stat [foff[nutt]][baselen] lies in the parent's
// scratch and *d_tabs is the uploaded tables back to back (foff first); both hold until the next call on `f`.
int fe_base_frames(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                   const std::vector<const std::vector<int> *> &tabs, const float **d_stat, const int **d_tabs);
