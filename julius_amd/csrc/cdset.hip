// cdset.hip -- pseudo-phone state-set scores (K5): the kernel and its launcher; the C ABI of jamd_cdset is in
// cdset_api.hip (cdset_host.h).
//
// Replaces outprob_cd() (libsent/src/phmm/outprob.c:383-400) and its three
// reductions over a CD_State_Set (htk_hmm.h:249-253), reading one row of the
// [T][S] state-score matrix instead of calling outprob_state() per member:
//   IWCD_MAX    outprob_cd_max()    outprob.c:332-344   running maximum from LOG_ZERO
//   IWCD_AVG    outprob_cd_avg()    outprob.c:356-370   float sum of members > LOG_ZERO,
//                                                        in member order, / (float)count
//   IWCD_NBEST  outprob_cd_nbest()  outprob.c:287-321   descending insertion list of at
//                                                        most N, summed best-first, / (float)n
// An empty / all-LOG_ZERO set yields 0/0 = NaN for avg and nbest exactly as the
// reference's float division does.
// One thread per (frame, set); consecutive threads take consecutive sets so
// the [T][nset] output is written coalesced; member gathers hit L2.
#include "jamd_device.h"
#include "cdset_host.h"

namespace {

__global__ void __launch_bounds__(256)
cdset_kernel(const float *__restrict__ scores, const int *__restrict__ off,
             const int *__restrict__ states, float *__restrict__ cd, int T, int S, int nset,
             int method, int nbest) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nset) return;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {         // gridDim.y is capped (65535 limit): frames are strided
    const float *row = scores + (size_t)t * S;
    const float r = jamd::cd_reduce(row, states, off[i], off[i + 1], method, nbest);
    cd[(size_t)t * nset + i] = r;
  }
}

}  // namespace

// ---- launcher (cdset_host.h)
int cdset_launch(jamd_cdset *c, hipStream_t st, const float *dev_scores, int T, int nstate, float *dev_cd) {
  const dim3 grid((c->nset + 255) / 256, T < 4096 ? T : 4096);
  hipLaunchKernelGGL(cdset_kernel, grid, dim3(256), 0, st, dev_scores,
                     c->d_off, c->d_states, dev_cd, T, nstate, c->nset, c->method, c->nbest);
  return JAMD_OK;
}
