// rejgmm.hip -- GMM-based input verification / rejection (-gmm, -gmmnum, -gmmreject) on gfx950: the kernels and their
// launchers; the C ABI of jamd_rejgmm is in rejgmm_api.hip (rejgmm_host.h).
//
// Replaces the scoring of libjulius/src/gmm.c: gmm_proceed() (gmm.c:574-600) scores every frame
// against a handful of one-state GMMs ("speech", "noise", ...) and adds the scores up per model;
// gmm_end() (gmm.c:614-660) then picks the winner.  gmm.c carries a private copy of the safe pruning
// that is NOT libsent's arithmetic: the Gaussians visited while the top-N list is not yet full are
// scored by gmm_compute_g_base() (gmm.c:177-194: squared distances summed from 0, gconst added
// last), the later ones by gmm_compute_g_safe() (gmm.c:218-240: gconst first; LOG_ZERO once the
// partial sum passes -2 x the list's last score -- the partial sums only grow, so that is decided
// by the final sum).  Everything else is cache_push() / addlog_array() as in calc_mix().
//
// The work is tiny (T x a few models x tens of Gaussians) and HBM-trivial; what matters is that it is
// the reference's number.  One thread per (frame, model); the running sums of an utterance are float
// additions in frame order (gmm.c:599), one thread per (utterance, model).
#include "gmm_dev.h"
#include "rejgmm_host.h"

namespace {
using namespace jamd;

template <int NMAX>
__global__ void __launch_bounds__(256)
rejgmm_frame_kernel(const float *__restrict__ mean, const float *__restrict__ ivar, const float *__restrict__ gconst,
                    const int *__restrict__ st_off, const int *__restrict__ ent_dens, const float *__restrict__ logw,
                    const int *__restrict__ model_state, const float *__restrict__ frames,
                    const float *__restrict__ tbl, float *__restrict__ out, int T, int nmodel, int D,
                    int gprune_num, float addmin_f) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * nmodel) return;
  const int t = (int)(idx / nmodel), k = (int)(idx % nmodel);
  const float *__restrict__ vec = frames + (size_t)t * D;
  const int s = model_state[k];
  const int e0 = st_off[s], n = st_off[s + 1] - e0;
  const int cap = gprune_num < NMAX ? gprune_num : NMAX;           // list slots ever used (n <= NMAX)
  float sc[NMAX]; int id[NMAX];
  int len = 0;
#pragma unroll
  for (int i = 0; i < NMAX; i++) { sc[i] = JAMD_LOG_ZERO; id[i] = 0; }
  for (int i = 0; i < n; i++) {                                     // gmm_gprune_safe(), gmm.c:296-313
    const int g = ent_dens[e0 + i];
    float last = JAMD_LOG_ZERO;                                     // thres: the list's last score
#pragma unroll
    for (int j = 0; j < NMAX; j++) if (j == len - 1) last = sc[j];
    float score = JAMD_LOG_ZERO;
    if (len < gprune_num) {
      if (g >= 0) {                                                 // gmm_compute_g_base()
        const float *__restrict__ m = mean + (size_t)g * D, *__restrict__ v = ivar + (size_t)g * D;
        float tmp = 0.0f;
        for (int d = 0; d < D; d++) { const float x = vec[d] - m[d]; tmp += x * x * v[d]; }
        score = (tmp + gconst[g]) * -0.5f;
      }
    } else {
      if (g >= 0) {                                                 // gmm_compute_g_safe()
        const float *__restrict__ m = mean + (size_t)g * D, *__restrict__ v = ivar + (size_t)g * D;
        const float fthres = last * -2.0f;
        float tmp = gconst[g];
        for (int d = 0; d < D; d++) { const float x = vec[d] - m[d]; tmp += x * x * v[d]; }
        score = tmp > fthres ? JAMD_LOG_ZERO : tmp * -0.5f;
      }
      if (score <= last) continue;
    }
    topn_push<NMAX>(sc, id, len, cap, score, i);
  }
  // gmm_calc_mix(), gmm.c:335-370: weights of the survivors, log-sum from the last slot down
  float y = JAMD_LOG_ZERO;
#pragma unroll
  for (int i = NMAX - 1; i >= 0; i--) {
    if (i < len) {
      float w = 0.0f;
      // id[i] is a register value; the weight is a gather
      w = logw[e0 + id[i]];
      y = addlog_step(y, sc[i] + w, tbl, addmin_f);
    }
  }
  out[(size_t)t * nmodel + k] = finish_state(y);
}

// gmm_proceed(), gmm.c:599: gmm_score[k] += score, frame after frame
__global__ void __launch_bounds__(64)
rejgmm_sum_kernel(const float *__restrict__ fsc, const int *__restrict__ utt_off, float *__restrict__ out,
                  int nutt, int nmodel) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nutt * nmodel) return;
  const int u = idx / nmodel, k = idx % nmodel;
  float acc = 0.0f;
  for (int t = utt_off[u]; t < utt_off[u + 1]; t++) acc += fsc[(size_t)t * nmodel + k];
  out[idx] = acc;
}

}  // namespace

// ---- launchers (rejgmm_host.h)
int rejgmm_launch_frames(jamd_rejgmm *m, hipStream_t st, const float *dev_frames, int T, float *dev_out) {
  const long total = (long)T * m->nmodel;
  const dim3 grid((unsigned)((total + 255) / 256));
  const int need = m->gprune_num < m->maxmix ? m->gprune_num : m->maxmix;
  return dispatch_topn<4>(need, [&](auto n) {
    hipLaunchKernelGGL((rejgmm_frame_kernel<decltype(n)::value>), grid, dim3(256), 0, st, m->d_mean, m->d_ivar, m->d_gconst,
                       m->d_st_off, m->d_ent_dens, m->d_logw, m->d_model_state, dev_frames, m->eng->d_addlog,
                       dev_out, T, m->nmodel, m->D, m->gprune_num, m->eng->addmin_f);
    return JAMD_OK;
  });
}

int rejgmm_launch_sums(jamd_rejgmm *m, hipStream_t st, const float *dev_frame_scores, int nutt, float *dev_out) {
  hipLaunchKernelGGL(rejgmm_sum_kernel, dim3((nutt * m->nmodel + 63) / 64), dim3(64), 0, st, dev_frame_scores,
                     m->d_utt_off, dev_out, nutt, m->nmodel);
  return JAMD_OK;
}
