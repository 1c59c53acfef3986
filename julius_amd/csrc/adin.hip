// adin.hip -- the kernels of the audio conditioning stage (jamd_adin) and their launchers (adin_host.h): the three FIR
// stages of ds48to16() (libsent/src/adin/ds48to16.c), the level scaling of adin_cut() (adin-cut.c:511-516),
// strip_zero() (libsent/src/anlz/strip.c) and sub_zmean() (libsent/src/adin/zmean.c), bit-identical.
//
// A FIR stage is a function of its cumulative input stream (adin_plan.h): output m is the sum over ascending j of
// x[k - j] * h[i + intrate * j], product rounded, then added (firout(); -ffp-contract=off keeps it unfused).  One lane
// computes four outputs, so four independent add chains hide the latency of the dependent one.  A workgroup takes 1024
// outputs of one channel; its inputs Z = [history | pending | new] go into LDS once.
//   stage 0 (3 -> 4): lane l takes outputs 4l .. 4l + 3; the q-th of them has the same phase i on every lane, so the
//     coefficients are lane-uniform scalar loads; the four read the same inputs at shifted taps, so one LDS read (the
//     lanes a stride of 3 doubles apart) feeds four multiply-adds.
//   stages 1, 2 (2 -> 1): lane l takes outputs 4l .. 4l + 3 as well; they read the same inputs two taps apart, so one
//     LDS read feeds four multiply-adds (one read per tap left the kernel bound by LDS bandwidth: 15 doubles per cycle
//     and CU); the coefficients are lane-uniform, the inputs lie in eight sub-arrays so that a read is conflict-free.
// Level, the strip flags, the compaction scan and the subtraction are lane-parallel; the float sum of sub_zmean() is
// not associative and is walked in order by one lane per channel, out of LDS, as fe_stats / lv_cmn walk theirs.
#include "adin_host.h"

constexpr int kThreads = 256;
constexpr int kOuts = kAdFirTile / kThreads;                 // outputs per lane
static_assert(kOuts == 4, "the stage kernels are written for four outputs per lane");
constexpr int kHalo = kAdStripWin - 1;                       // neighbours a strip decision looks at, each side

// Z[z] of one channel and stage: the stage's kept inputs, then the push's
template <typename TIN>
__device__ __forceinline__ double ad_z(const double *hist, const TIN *in, int npre, int zlen, int z) {
  return z < npre ? hist[z] : (z < zlen ? (double)in[z - npre] : 0.0);
}

// 48 -> 64 kHz.  grid (tiles, nchan)
__global__ __launch_bounds__(kThreads) void ad_fir_3to4_kernel(const AdStageTab *__restrict__ tab, const double *__restrict__ hist_all,
                                                               int hp, int H, int hdn_len, const double *__restrict__ h,
                                                               const int16_t *__restrict__ in, double *__restrict__ out) {
  const int c = blockIdx.y, tid = threadIdx.x;
  const AdStageTab t = tab[c];
  const int r0 = blockIdx.x * kAdFirTile;
  if (r0 >= t.n_raw) return;
  // outputs r0 + r', tick t_b + 3 (r0 + r'): input 3 r0 / 4 + (t_b + 3 r') / 4 behind Z[H]; r' < 1024 needs 768 of them
  __shared__ double x[128 + 3 * kAdFirTile / 4 + 4];
  const double *hist = hist_all + (size_t)c * hp;
  const int16_t *src = in + t.in_off;
  const int npre = H + t.pend, zlen = npre + t.n_in, kb = 3 * (r0 / 4);
  for (int u = tid; u < H + 3 * kAdFirTile / 4 + 3; u += kThreads) x[u] = ad_z(hist, src, npre, zlen, kb + u);
  __syncthreads();
  // output q of the lane sits at tick t_b + 12l + 3q: input 3l + (t_b + 3q) / 4, phase (t_b + 3q) % 4.  With n = j less
  // that input's offset the four outputs share X[H + 3l - n], and the coefficient is h[t_b + 3q + 4n] where that
  // index lies in the table: one LDS read, four lane-uniform coefficients, each output summing over ascending j.
  double acc[kOuts];
#pragma unroll
  for (int q = 0; q < kOuts; q++) acc[q] = 0.0;
  const double *mine = x + H + 3 * tid;
  const int g0 = t.t_b, main_end = (hdn_len - (g0 + 3 * (kOuts - 1))) >> 2;   // up to here all four indices are inside
  for (int n = -2; n < 0; n++) {
    const double xv = mine[-n];
#pragma unroll
    for (int q = 1; q < kOuts; q++) {
      const int idx = g0 + 3 * q + 4 * n;
      if (idx >= 0 && idx <= hdn_len) acc[q] += xv * h[idx];
    }
  }
#pragma unroll 4
  for (int n = 0; n <= main_end; n++) {
    const double xv = mine[-n];
#pragma unroll
    for (int q = 0; q < kOuts; q++) acc[q] += xv * h[g0 + 3 * q + 4 * n];
  }
  for (int n = main_end < 0 ? 0 : main_end + 1; g0 + 4 * n <= hdn_len; n++) {
    const double xv = mine[-n];
#pragma unroll
    for (int q = 0; q < kOuts; q++)
      if (g0 + 3 * q + 4 * n <= hdn_len) acc[q] += xv * h[g0 + 3 * q + 4 * n];
  }
#pragma unroll
  for (int q = 0; q < kOuts; q++) {
    const int r = r0 + 4 * tid + q;
    if (r < t.n_raw && r >= t.drop) out[t.out_off + (r - t.drop)] = acc[q];
  }
}

// 64 -> 32 and 32 -> 16 kHz.  grid (tiles, nchan).  Lane l takes outputs 4l .. 4l + 3 of the tile: tap j of output q reads
// X[8l + 2q + H - j] (X = Z from the tile's first input on), so with t = j - 2q the four outputs share X[8l + H - t] and
// one LDS read feeds four multiply-adds, each output still summing over ascending j.  X[8i + k] lies at xs[k][i]: the
// lanes of a read are a stride of one double apart.  The last stage stores C's `short = double`: truncation through a
// 32-bit integer, wrapping as the reference's compiled code does where the filter overshoots the rails.
constexpr int kSubW = (2 * kAdFirTile + 512) / 8 + 4;        // 324: the eight sub-arrays start eight banks apart

template <typename TOUT>
__global__ __launch_bounds__(kThreads) void ad_fir_2to1_kernel(const AdStageTab *__restrict__ tab, const double *__restrict__ hist_all,
                                                               int hp, int H, int hdn_len, const double *__restrict__ h,
                                                               const double *__restrict__ in, TOUT *__restrict__ out) {
  const int c = blockIdx.y, tid = threadIdx.x;
  const AdStageTab t = tab[c];
  const int r0 = blockIdx.x * kAdFirTile;
  if (r0 >= t.n_raw) return;
  __shared__ double xs[8 * kSubW];
  const double *hist = hist_all + (size_t)c * hp;
  const double *src = in + t.in_off;
  const int npre = H + t.pend, zlen = npre + t.n_in;
  for (int u = tid; u < 2 * kAdFirTile + H; u += kThreads) xs[(u & 7) * kSubW + (u >> 3)] = ad_z(hist, src, npre, zlen, 2 * r0 + u);
  __syncthreads();
  double acc[kOuts];
#pragma unroll
  for (int q = 0; q < kOuts; q++) acc[q] = 0.0;
  const double *mine = xs + tid;
  auto x_at = [&](int tt) { const int m = H - tt; return mine[(m & 7) * kSubW + (m >> 3)]; };
  const int main_end = hdn_len - 2 * (kOuts - 1);            // up to here every output has a tap at t
  for (int tt = -2 * (kOuts - 1); tt < 0; tt++) {            // the later outputs begin before the first one
    const double x = x_at(tt);
#pragma unroll
    for (int q = 1; q < kOuts; q++)
      if (tt + 2 * q >= 0 && tt + 2 * q <= hdn_len) acc[q] += x * h[tt + 2 * q];
  }
#pragma unroll 4
  for (int tt = 0; tt <= main_end; tt++) {
    const double x = x_at(tt);
#pragma unroll
    for (int q = 0; q < kOuts; q++) acc[q] += x * h[tt + 2 * q];
  }
  for (int tt = main_end < 0 ? 0 : main_end + 1; tt <= hdn_len; tt++) {
    const double x = x_at(tt);
#pragma unroll
    for (int q = 0; q < kOuts; q++)
      if (tt + 2 * q <= hdn_len) acc[q] += x * h[tt + 2 * q];
  }
#pragma unroll
  for (int q = 0; q < kOuts; q++) {
    const int r = r0 + 4 * tid + q;
    if (r < t.n_raw && r >= t.drop) {
      if constexpr (sizeof(TOUT) == 2) out[t.out_off + (r - t.drop)] = (int16_t)(int)acc[q];
      else out[t.out_off + (r - t.drop)] = acc[q];
    }
  }
}

struct AdHistArgs {
  double *hist[3];
  int hp[3], H[3];
  const int16_t *in0;
  const double *in1, *in2;
};

// Z moves on by the inputs the push consumed: the last H consumed and what is pending stay.  grid (nchan, 3); one
// workgroup owns one channel's stage, reads all of it (at most 767 values), then writes.
__global__ __launch_bounds__(kThreads) void ad_hist_kernel(const AdStageTab *__restrict__ tab, int nchan, AdHistArgs g) {
  const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const AdStageTab t = tab[s * nchan + c];
  if (t.n_in == 0) return;
  double *hist = g.hist[s] + (size_t)c * g.hp[s];
  const int npre = g.H[s] + t.pend, zlen = npre + t.n_in, keep = zlen - t.adv;
  double v[3];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const int i = tid + kThreads * q;
    v[q] = 0.0;
    if (i < keep) {
      const int z = i + t.adv;
      v[q] = s == 0 ? ad_z(hist, g.in0 + t.in_off, npre, zlen, z)
                    : ad_z(hist, (s == 1 ? g.in1 : g.in2) + t.in_off, npre, zlen, z);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const int i = tid + kThreads * q;
    if (i < keep) hist[i] = v[q];
  }
}

__device__ __forceinline__ bool ad_invalid(int v) { return v == 0 || v == -32767; }   // strip.c IS_INVALID_SAMPLE

// One workgroup per channel, over its chunk in steps of 1024 samples: the level, the strip decision of every sample
// from its 15 neighbours each side (clipped at the chunk's ends), a prefix sum to compact, and -- while the channel's
// zlen at the chunk's start is below ZMEANSAMPLES -- lane 0 adding the kept samples to sub_zmean()'s float sum in order.
__global__ __launch_bounds__(kThreads) void ad_strip_kernel(const AdChanTab *__restrict__ tab, const int16_t *__restrict__ src,
                                                            int do_level, float coef, int do_strip, int do_zmean,
                                                            int16_t *__restrict__ pre, int *__restrict__ cnt,
                                                            int *__restrict__ zlen_all, float *__restrict__ zmean_all) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const AdChanTab t = tab[c];
  if (t.n == 0) {                                            // idle: neither strip_zero() nor sub_zmean() is called
    if (tid == 0) cnt[c] = 0;
    return;
  }
  __shared__ int16_t v[kAdPostTile + 2 * kHalo], kept[kAdPostTile];
  __shared__ int wsum[kThreads / 64];
  const int16_t *in = src + t.src_off;
  int16_t *dst = pre + t.pre_off;
  const int zlen0 = do_zmean ? zlen_all[c] : 0;
  const bool update = do_zmean && zlen0 < kAdZmeanSamples;
  float sum = update ? zmean_all[c] * zlen0 : 0.f;           // (lane 0's is the one that counts)
  int total = 0;
  for (int base = 0; base < t.n; base += kAdPostTile) {
    for (int u = tid; u < kAdPostTile + 2 * kHalo; u += kThreads) {
      const long long g = (long long)base - kHalo + u;
      int s = 1;                                             // beyond the chunk: never part of a run
      if (g >= 0 && g < t.n) {
        s = in[g];
        if (do_level) s = (int16_t)(int)((float)s * coef);
      }
      v[u] = (int16_t)s;
    }
    __syncthreads();
    int mine[4];
    unsigned km = 0;                                         // which of the lane's four samples stay
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = 4 * tid + q;
      const int s = v[kHalo + i];
      mine[q] = s;
      bool keep = base + i < t.n;
      if (keep && do_strip && ad_invalid(s)) {
        int run = 1;
        for (int k = 1; k <= kHalo && ad_invalid(v[kHalo + i - k]); k++) run++;
        for (int k = 1; k <= kHalo && ad_invalid(v[kHalo + i + k]); k++) run++;
        keep = run < kAdStripWin;
      }
      if (keep) km |= 1u << q;
    }
    const int nk = __popc(km);
    // exclusive prefix of nk over the workgroup
    int inc = nk;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if ((tid & 63) >= d) inc += o;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    int before = inc - nk, tile = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
      if (w < (tid >> 6)) before += wsum[w];
      tile += wsum[w];
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (km >> q & 1) {
        kept[before] = (int16_t)mine[q];
        dst[total + before] = (int16_t)mine[q];
        before++;
      }
    __syncthreads();
    if (update && tid == 0)
      for (int i = 0; i < tile; i++) sum += (float)kept[i];
    total += tile;
    __syncthreads();
  }
  if (tid == 0) {
    cnt[c] = total;
    if (update) {                                            // 0 / 0 where everything was stripped from a fresh channel: NaN, as there
      const int zl = zlen0 + total;
      zlen_all[c] = zl;
      zmean_all[c] = sum / (float)zl;
    }
  }
}

// ooff[c] = cnt[0] + ... + cnt[c - 1], ooff[nchan] the total.  One workgroup.
__global__ __launch_bounds__(kThreads) void ad_offsets_kernel(const int *__restrict__ cnt, int nchan, long long *__restrict__ ooff) {
  __shared__ long long part[kThreads];
  const int tid = threadIdx.x, per = (nchan + kThreads - 1) / kThreads;
  const int lo = tid * per, hi = lo + per < nchan ? lo + per : nchan;
  long long s = 0;
  for (int c = lo; c < hi; c++) s += cnt[c];
  part[tid] = s;
  __syncthreads();
  long long run = 0;
  for (int i = 0; i < tid; i++) run += part[i];
  for (int c = lo; c < hi; c++) { ooff[c] = run; run += cnt[c]; }
  if (tid == kThreads - 1) ooff[nchan] = run;                // (the last lane's run ends at the total, with or without entries)
}

// The second loop of sub_zmean(): d = (float)s - zmean clipped to the rails, rounded half away from zero in double
// (the reference's 0.5 is a double).  A NaN mean passes every comparison and converts to 0 in the compiled reference.
__device__ __forceinline__ int16_t ad_sub_zmean(int16_t s, float zmean) {
  float d = (float)s - zmean;
  if (d != d) return 0;
  if (d < -32768.0f) d = -32768.0f;
  if (d > 32767.0f) d = 32767.0f;
  return d > 0 ? (int16_t)(int)((double)d + 0.5) : (int16_t)(int)((double)d - 0.5);
}

// grid (tiles, nchan)
__global__ __launch_bounds__(kThreads) void ad_emit_kernel(const AdChanTab *__restrict__ tab, const int16_t *__restrict__ pre,
                                                           const int *__restrict__ cnt, const long long *__restrict__ ooff,
                                                           int do_zmean, const float *__restrict__ zmean_all,
                                                           int16_t *__restrict__ out) {
  const int c = blockIdx.y, n = cnt[c];
  const int i0 = blockIdx.x * kAdPostTile;
  if (i0 >= n) return;
  const int16_t *p = pre + tab[c].pre_off;
  int16_t *o = out + ooff[c];
  const float zm = do_zmean ? zmean_all[c] : 0.f;
  for (int i = i0 + threadIdx.x; i < i0 + kAdPostTile && i < n; i += kThreads) o[i] = do_zmean ? ad_sub_zmean(p[i], zm) : p[i];
}

__global__ __launch_bounds__(kThreads) void ad_reset_kernel(const unsigned char *__restrict__ mask, int what, AdHistArgs g,
                                                            int *__restrict__ zlen, float *__restrict__ zmean) {
  const int c = blockIdx.x;
  if (mask && !mask[c]) return;
  if (what & JAMD_ADIN_DS)
    for (int s = 0; s < 3; s++)
      if (g.hist[s])
        for (int i = threadIdx.x; i < g.hp[s]; i += kThreads) g.hist[s][(size_t)c * g.hp[s] + i] = 0.0;
  if ((what & JAMD_ADIN_ZMEAN) && threadIdx.x == 0) { zlen[c] = 0; zmean[c] = 0.f; }
}

static AdHistArgs ad_hist_args(jamd_adin *a, const int16_t *in0) {
  AdHistArgs g{};
  for (int s = 0; s < 3; s++) {
    g.hist[s] = a->d_hist[s];
    g.H[s] = a->cas.st[s].hist;
    g.hp[s] = a->cas.st[s].hist + kAdBlock - 1;
  }
  g.in0 = in0; g.in1 = a->d_mid[0]; g.in2 = a->d_mid[1];
  return g;
}

int ad_launch_fir(jamd_adin *a, hipStream_t st, int s, const AdStageTab *d_tab, const void *in, void *out, int max_raw) {
  const AdStage &g = a->cas.st[s];
  const dim3 grid((unsigned)((max_raw + kAdFirTile - 1) / kAdFirTile), (unsigned)a->nchan);
  const int hp = g.hist + kAdBlock - 1;
  if (s == 0)
    hipLaunchKernelGGL(ad_fir_3to4_kernel, grid, dim3(kThreads), 0, st, d_tab, a->d_hist[0], hp, g.hist, g.hdn_len, a->d_fir[0],
                       (const int16_t *)in, (double *)out);
  else if (s == 1)
    hipLaunchKernelGGL(ad_fir_2to1_kernel<double>, grid, dim3(kThreads), 0, st, d_tab, a->d_hist[1], hp, g.hist, g.hdn_len,
                       a->d_fir[1], (const double *)in, (double *)out);
  else
    hipLaunchKernelGGL(ad_fir_2to1_kernel<int16_t>, grid, dim3(kThreads), 0, st, d_tab, a->d_hist[2], hp, g.hist, g.hdn_len,
                       a->d_fir[1], (const double *)in, (int16_t *)out);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int ad_launch_hist(jamd_adin *a, hipStream_t st, const AdStageTab *d_tab, const int16_t *in0) {
  hipLaunchKernelGGL(ad_hist_kernel, dim3((unsigned)a->nchan, 3), dim3(kThreads), 0, st, d_tab, a->nchan, ad_hist_args(a, in0));
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int ad_launch_post(jamd_adin *a, hipStream_t st, const AdChanTab *d_tab, const int16_t *src, int16_t *dev_out, int max_n) {
  const jamd_adin_desc &d = a->d;
  hipLaunchKernelGGL(ad_strip_kernel, dim3((unsigned)a->nchan), dim3(kThreads), 0, st, d_tab, src, d.level_coef != 1.0f ? 1 : 0,
                     d.level_coef, d.strip_zero, d.zmean, a->d_pre, a->d_cnt, a->d_zlen, a->d_zmean);
  JAMD_HIP(hipGetLastError());
  hipLaunchKernelGGL(ad_offsets_kernel, dim3(1), dim3(kThreads), 0, st, a->d_cnt, a->nchan, a->d_ooff);
  JAMD_HIP(hipGetLastError());
  const dim3 grid((unsigned)((max_n + kAdPostTile - 1) / kAdPostTile), (unsigned)a->nchan);
  hipLaunchKernelGGL(ad_emit_kernel, grid, dim3(kThreads), 0, st, d_tab, a->d_pre, a->d_cnt, a->d_ooff, d.zmean, a->d_zmean,
                     dev_out);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int ad_launch_reset(jamd_adin *a, hipStream_t st, const unsigned char *d_mask, int what) {
  hipLaunchKernelGGL(ad_reset_kernel, dim3((unsigned)a->nchan), dim3(kThreads), 0, st, d_mask, what, ad_hist_args(a, nullptr),
                     a->d_zlen, a->d_zmean);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}
