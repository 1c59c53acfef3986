// beam_lexicon.hip -- the one kernel of the tree lexicon: it builds the cross-word LM table (LexDev::iwtab) when
// jamd_lexicon_create() (beam_lexicon_api.hip) has uploaded the arena.
#include "jamd_device.h"

#include "beam_host.h"

namespace {
using namespace jamdb;
// the cross-word LM table (LexDev::iwtab): one thread per (context, isolated root)
__global__ void __launch_bounds__(256) iwtab_build_kernel(LexDev lx, float *tab, int nctx, int niso) {
  const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= (size_t)nctx * niso) return;
  const int ctx = (int)(x / niso), i = (int)(x - (size_t)ctx * niso);
  const int w = lx.iso_root(i).y;
  tab[x] = bigram_prob(lx, ctx, lx.wton(w)) + lx.cprob(w);
}

}  // namespace

namespace jamdb {

hipError_t iwtab_build(const LexDev &lx, float *tab, int nctx, int niso, hipStream_t st) {
  const size_t cells = (size_t)nctx * niso;
  hipLaunchKernelGGL(iwtab_build_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, lx, tab, nctx, niso);
  const hipError_t le = hipGetLastError();
  return le != hipSuccess ? le : hipStreamSynchronize(st);
}

}  // namespace jamdb
