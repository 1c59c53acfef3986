// gmm_ms.hip -- K1m: state likelihoods of a MULTI-STREAM GMM acoustic model for gfx950 (CDNA4).
//
// Replaces, for a whole block of frames at once, calc_mix()'s loop over OP_nstream streams
// (libsent/src/phmm/calc_mix.c:52-80) with the per-state stream weights, over the stream slices outprob_state() sets
// up (outprob.c:199-203), under gprune_none() / compute_g_base() (gprune_none.c:59-147) and addlog_array()
// (addlog.c:103-123).
//
// Arithmetic contract (bit-exact with the reference's x86-64 object code; -ffp-contract=off, nothing is fused):
//   * streams ascending; stream s sees o[off_s .. off_s + vsize_s)
//   * per Gaussian K1's four separately rounded fp32 operations per dimension from gconst, dims ascending, * -0.5
//     (LOG_ZERO for a NULL density), + ln w; the table log-sum from the pdf's LAST entry to its first
//   * `if (logprob <= LOG_ZERO) continue;` else logprobsum += logprob * weight: a rounded multiply, a rounded add,
//     from 0.0f
//   * finish_state() on the weighted sum: 0 or <= LOG_ZERO -> LOG_ZERO, else (float)((double)sum * .434294482)
//
// K1's plan: ONE LANE = ONE FRAME (a packed pair per lane), every Gaussian record is wave-uniform and comes in by
// scalar loads, the D-loop is packed fp32, the mixture log-sum an in-lane scan, the results leave through the wave's
// LDS tile in row segments.  What differs: a stream's slice starts at a run-time offset, and the register file cannot
// be indexed by one -- so the wave's 128 frames sit in LDS transposed [d][128] (load_frames<0>, as the generic-D form
// of K1 holds them) and a slice is that base plus off_s * 128; the per-pdf loop is gauss_pair<0>'s arithmetic over the
// slice's length (gauss_slice, gmm_ms_dev.h), and the stream loop carries the two weighted sums of the lane's frames.  See
// DESIGN.md "K1m".
#include "gmm_ms_dev.h"
#include "gmm_ms_host.h"

namespace {
using namespace jamd;

constexpr int kWaves = 4;    // waves per workgroup
constexpr int kNS = 16;      // states per block = the width of the output tile (as K1)
constexpr int kFPW = kMsFPW;  // frames per wave: one packed pair per lane

template <int NS>
__global__ void __launch_bounds__(64 * kWaves)
gmm_ms_kernel(const float *__restrict__ rec, const JamdMsPdf *__restrict__ pdf,
              const JamdMsStream *__restrict__ strm, const int *__restrict__ st_pdf,
              const float *__restrict__ st_w, const float *__restrict__ frames,
              const float *__restrict__ tbl, float *__restrict__ out, int T, int S, int D, int nstream,
              int nfb, int nstb, float addmin_f) {
  __shared__ float tile[kWaves][kFPW][NS + 1];
  extern __shared__ __align__(16) float dyn[];  // [kWaves][D][kFPW]

  int fb, sb;
  if (!decode_block(nfb, nstb, fb, sb)) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int t0 = (fb * kWaves + wave) * kFPW;
  if (t0 >= T) return;
  float *vt = dyn + (size_t)wave * D * kFPW;
  load_frames<0>(nullptr, vt, frames, t0, T, D, lane);

  const int s_begin = sb * NS;
  const int ns = min(NS, S - s_begin);
  for (int si = 0; si < ns; si++) {
    const int *__restrict__ sp = st_pdf + (size_t)(s_begin + si) * nstream;
    const float *__restrict__ sw = st_w + (size_t)(s_begin + si) * nstream;
    float sum0 = 0.0f, sum1 = 0.0f;          // logprobsum of the lane's two frames
    for (int k = 0; k < nstream; k++) {
      const JamdMsStream sd = strm[k];
      const JamdMsPdf pd = pdf[sp[k]];
      const float w = sw[k];
      const float *vs = vt + sd.off * kFPW;  // the stream's slice of the transposed frames
      const int len = sd.len;
      const int REC = ((2 * len + 2) + 3) & ~3;
      float y0 = JAMD_LOG_ZERO, y1 = JAMD_LOG_ZERO;
      for (int e = pd.n - 1; e >= 0; e--) {
        const float *__restrict__ r = rec + (size_t)pd.rec + (size_t)e * REC;
        const float lw = r[2 * len + 1];
        const f2 g = gauss_slice(vs, lane, len, r);              // (LOG_ZERO for a NULL density, then the weight as K1)
        y0 = addlog_step(y0, g.x + lw, tbl, addmin_f);
        y1 = addlog_step(y1, g.y + lw, tbl, addmin_f);
      }
      // calc_mix.c:74-76: a stream whose outprob is zero is skipped
      if (!(y0 <= JAMD_LOG_ZERO)) { const float p = y0 * w; sum0 = sum0 + p; }
      if (!(y1 <= JAMD_LOG_ZERO)) { const float p = y1 * w; sum1 = sum1 + p; }
    }
    tile[wave][lane][si] = finish_state(sum0);
    tile[wave][64 + lane][si] = finish_state(sum1);
  }
  store_tile<NS, kFPW>(tile[wave], out, t0, T, S, s_begin, ns, lane);
}

}  // namespace

int jamd_gmm_ms_setup(jamd_gmm_ms *g) {
  g->dyn_lds = sizeof(float) * kWaves * (size_t)g->D * kFPW;
  // The attribute belongs to the kernel, not to the model: it is raised to all a CU has beside the static tile, the
  // same value for every model, so that a model made later never lowers it under one made before.
  const void *kernel = (const void *)gmm_ms_kernel<kNS>;
  constexpr size_t kCuLds = 160u * 1024u;
  hipFuncAttributes fa;
  JAMD_HIP(hipFuncGetAttributes(&fa, kernel));
  if (fa.sharedSizeBytes + g->dyn_lds > kCuLds)
    return jamd_refuse("jamd_gmm_ms_create: veclen=%d needs %zu bytes of LDS per workgroup (%zu static + %zu), the CU has %zu",
                       g->D, fa.sharedSizeBytes + g->dyn_lds, (size_t)fa.sharedSizeBytes, g->dyn_lds, kCuLds);
  JAMD_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kCuLds - fa.sharedSizeBytes)));
  return JAMD_OK;
}

int jamd_gmm_ms_launch(jamd_gmm_ms *g, const float *frames, int T, float *out, hipStream_t st) {
  constexpr int FPB = kWaves * kFPW;
  const int nfb = (T + FPB - 1) / FPB;
  const int nstb = (g->S + kNS - 1) / kNS;
  const int grid = xcd_grid(nstb, nfb);
  hipLaunchKernelGGL((gmm_ms_kernel<kNS>), dim3(grid), dim3(64 * kWaves), g->dyn_lds, st,
                     g->d_rec, g->d_pdf, g->d_stream, g->d_st_pdf, g->d_st_w, frames, g->eng->d_addlog, out, T, g->S,
                     g->D, g->nstream, nfb, nstb, g->eng->addmin_f);
  snprintf(g->last_kernel, sizeof(g->last_kernel), "gmm_ms<NS=%d> D=%d nstream=%d grid=%d", kNS, g->D, g->nstream, grid);
  return JAMD_OK;
}
