// gmm_ms_dev.h -- what the multi-stream kernels share (gmm_ms.hip: K1m; gmm_ms_tied.hip: K1mt): the frames of a wave
// in LDS, transposed [d][128], and the Gaussian of one stream's slice of them.  Internal, not installed.
#pragma once
#include "gmm_dev.h"

namespace jamd {

constexpr int kMsFPW = 128;    // frames per wave: one packed pair per lane

// compute_g_base() (gprune_none.c:59-82) over one stream's slice: gauss_pair<0>'s arithmetic -- gconst, then per
// dimension ascending a subtract, two multiplies and an add, each rounded, * -0.5, LOG_ZERO for a NULL density (gconst
// NaN) -- with the dimensions taken eight at a time, so that the sixteen scalar loads of a group are in flight together
// and are waited for once.  (One dimension per load, as gauss_pair<0> walks a run-time length, the wave stands on a
// scalar-load latency per dimension: with the frames in LDS a CU holds one block, one wave per SIMD, and nothing hides
// it -- 78.9 ms against 59.0 ms at the benchmark's shape, profiles/gmm_ms_timing.json.)  vs -> the slice's first
// dimension in the wave's transposed frames, r -> record [mean(len) ivar(len) gconst ...].
__device__ __forceinline__ f2 gauss_slice(const float *vs, int lane, int len, const float *__restrict__ r) {
  const float gc = r[2 * len];
  const float *__restrict__ mu = r, *__restrict__ iv = r + len;
  f2 acc = {gc, gc};
  int d = 0;
  for (; d + 8 <= len; d += 8) {
    float m[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { m[j] = mu[d + j]; v[j] = iv[d + j]; }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      f2 x = f2{vs[(d + j) * kMsFPW + lane], vs[(d + j) * kMsFPW + 64 + lane]} - f2{m[j], m[j]};
      x = x * x;
      x = x * f2{v[j], v[j]};
      acc = acc + x;
    }
  }
  for (; d < len; d++) {
    const float m = mu[d], v = iv[d];
    f2 x = f2{vs[d * kMsFPW + lane], vs[d * kMsFPW + 64 + lane]} - f2{m, m};
    x = x * x;
    x = x * f2{v, v};
    acc = acc + x;
  }
  f2 sc = {acc.x * -0.5f, acc.y * -0.5f};
  if (gc != gc) sc = f2{JAMD_LOG_ZERO, JAMD_LOG_ZERO};
  return sc;
}

}  // namespace jamd
