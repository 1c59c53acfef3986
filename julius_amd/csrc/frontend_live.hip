// frontend_live.hip -- the live-input front end on gfx950: many independent channels per call, a whole segment each
// (jamd_frontend_live_run_*) or the next chunk of an open segment (jamd_frontend_live_push_*).
//
// Reproduces, bit for bit, the vectors the reference stores into mfcc->param for a microphone, a socket or -realtime:
// RealTimeMFCC() (libjulius/src/realtime-1stpass.c:496-602) for the main loop and the flush loop of RealTimeParam()
// (:1215-1304) for the tail, with the pipelined pieces of libsent/src/wav2mfcc/wav2mfcc-pipe.c: energy_max_normalize(),
// the cyclic delta / acceleration buffers (WMP_deltabuf_*), CMN_realtime() and CMN_realtime_update().  The base
// coefficients are WMP_calc(), which the buffered front end's frame kernel already computes (frontend.hip, launched
// by frontend_live_api.hip through frontend_host.h); everything behind it differs from the buffered front end in every normalised element and
// is computed here.  Like the rest of the library this unit is compiled with -ffp-contract=off, and every expression
// keeps the reference's types.
//
// A segment of Tb base frames yields (see jamd_frontend_live_frames()):
//   Nd = Tb when there is no _D, else Tb if Tb >= delWin, else 0        frames out of the delta buffer
//   Nf = Nd when there is no _A, else Nd if Nd >= accWin, else 0        frames out of the acceleration buffer
//   Nf - (splice - 1) rows                                               (none when that is < 1)
// because the flush loop ends at the first WMP_deltabuf_flush() that finds its slot empty.  In the cyclic buffers a
// missing neighbour takes the last valid vector on its side; the slots that are valid when frame t is computed are
// exactly the frames of the segment within the window, so that vector is frame 0 on the left and frame Nd - 1 on the
// right, also for segments shorter than the buffers.  The two loops disagree on the last block of an _A vector (see
// lv_feat_kernel): the tail of every segment is reproduced as the flush loop stores it.
//
// The reference is frame-synchronous, so the rows of a segment do not depend on how its samples were cut.  A push
// continues the segment from what the device keeps per channel: the samples behind the last whole window (at most
// framesize), the last 2 * (delWin + accWin) raw base vectors in a ring (frame t in slot t % R; lv_base() normalises the
// energy on read, with the maximum the segment was opened with), the running energy maximum, the CMN chains
// (now.mfcc_sum / now.mfcc_var / now.framenum), the last splice - 1 normalised vectors and, for the variance
// re-estimation alone, every row handed out so far.  A push that does not end the segment emits the frames
// t < Tb - delWin - accWin: their right neighbours all exist and none of them lies in the flush loop's tail, so the
// same lv_feat_kernel serves both entries with T = the base frames so far.  Every count follows from the channel's
// sample count, which the host object keeps.
//
//   lv_pack_kernel     push only, one lane per sample: [residue | chunk] of every channel -> one staging batch, over
//                      which the parent's frame kernel runs
//   lv_feat_kernel     one lane per (frame, element): normalised energy, delta, acceleration -> feat[Nf][veclen]
//   lv_keep_kernel     one workgroup per channel, behind lv_feat_kernel, which reads what it overwrites: the energy
//                      maximum, max(0, max_t f) (order-free), into the channel's state when the segment ends; for a
//                      push also the new residue and the base vectors the ring has to hold
//   lv_cmn_kernel      one lane per (channel, element): the float chains of CMN_realtime() over t, from the stored
//                      state when the segment was open; normalises, splices and stores the rows; leaves now.mfcc_sum /
//                      now.mfcc_var / now.framenum in the channel's state
//   lv_copy_kernel     one lane per output element: splicing alone, for whole segments of kinds without _Z and cvn
//   lv_commit_kernel   one lane per (channel, element): CMN_realtime_update()
//   lv_commit_scalars  one lane per channel: the frame counts, the list's length and head, cmean_init_set
//
// This unit holds the kernels and, at its end, their launchers (declared in frontend_host.h); the jamd_frontend_live_*
// entries that call them are in frontend_live_api.hip, the counts of a segment in frontend_tables.h.
#include "jamd_device.h"
#include "frontend_host.h"
#include <cmath>
#include <cstdint>

namespace {

// Where the base vectors of one channel's segment lie: frames below `told` in the ring, the others in this call's batch.
struct LvSrc { const float *stat, *ring; int told; };

// tmpmfcc[n] of frame t of the segment after energy_max_normalize() (wav2mfcc-pipe.c:740-746).  kRingSrc false: a
// whole segment, every frame in the batch.
template <bool kRingSrc>
__device__ __forceinline__ float lv_base(const LvParams &p, const LvSrc &b, float max_last, float min_last, int t, int n) {
  float f;
  if (kRingSrc && t < b.told) f = b.ring[(size_t)(t % p.R) * p.baselen + n];
  else f = b.stat[(size_t)(t - b.told) * p.baselen + n];
  if (p.enorm && n == p.baselen - 1) {
    if (f < min_last) f = min_last;
    f = (float)(1.0 - (max_last - f) * p.escale);
  }
  return f;
}

// WMP_deltabuf_calc() (:122-153) of the delta buffer at frame t of a segment of T frames
template <bool kRingSrc>
__device__ __forceinline__ float lv_delta(const LvParams &p, const LvSrc &b, float max_last, float min_last, int T, int t,
                                          int n) {
  float sum = 0.0f;
  for (int theta = 1; theta <= p.delWin; theta++) {
    const float A1 = lv_base<kRingSrc>(p, b, max_last, min_last, t - theta < 0 ? 0 : t - theta, n);
    const float A2 = lv_base<kRingSrc>(p, b, max_last, min_last, t + theta >= T ? T - 1 : t + theta, n);
    sum += theta * (A2 - A1);
  }
  return sum / p.Bd;
}

// Frames f0[c] .. of channel c, whose segment has told[c] base frames in the ring and boff[c + 1] - boff[c] new ones in
// `stat`: T is their sum.  A whole segment (kRingSrc false) has told == f0 == 0 and reads neither table.  A frame whose neighbours pass T - 1 or that lies in the
// last delWin + accWin is asked for only when the segment ends, so T is then the segment's length.
template <bool kRingSrc>
__global__ void __launch_bounds__(256)
lv_feat_kernel(LvParams p, const float *__restrict__ stat, const float *__restrict__ ring, const int *__restrict__ boff,
               const int *__restrict__ told, const int *__restrict__ f0, const int *__restrict__ noff,
               const float *__restrict__ emax, int Ntot, float *__restrict__ feat) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Ntot * p.veclen) return;
  const int g = (int)(idx / p.veclen), e = (int)(idx % p.veclen);
  const int c = jamd::find_span(noff, p.nchan, g);
  const LvSrc b{stat + (size_t)boff[c] * p.baselen, ring + (size_t)c * p.R * p.baselen, kRingSrc ? told[c] : 0};
  const int t = (kRingSrc ? f0[c] : 0) + (g - noff[c]), T = b.told + (boff[c + 1] - boff[c]);
  float max_last = 0.0f, min_last = 0.0f;
  if (p.enorm) {                              // energy_max_prepare()
    max_last = emax[c];
    min_last = (float)(max_last - (p.silFloor * JAMD_LOG_TEN) / 10.0);
  }
  float v;
  if (e < p.nb) v = lv_base<kRingSrc>(p, b, max_last, min_last, t, e);
  else if (e < p.nb + p.baselen) v = lv_delta<kRingSrc>(p, b, max_last, min_last, T, t, e - p.nb);
  else {
    // The acceleration buffer runs over the delta buffer's vectors [base][delta] and appends its own deltas of both:
    // [base][delta][d base][d delta].  RealTimeMFCC() keeps the last block (:573-574).  The flush loop keeps the block
    // at veclen - baselen, which is the third (:1251-1252, :1275-1276): the frames it emits, the last
    // delWin + accWin of the segment, carry the accWin-delta of the base coefficients there.
    const int n = e - p.nb - p.baselen;
    const bool tail = t >= T - p.delWin - p.accWin;
    float sum = 0.0f;
    for (int theta = 1; theta <= p.accWin; theta++) {
      const int t1 = t - theta < 0 ? 0 : t - theta, t2 = t + theta >= T ? T - 1 : t + theta;
      float A1, A2;
      if (tail) {
        A1 = lv_base<kRingSrc>(p, b, max_last, min_last, t1, n);
        A2 = lv_base<kRingSrc>(p, b, max_last, min_last, t2, n);
      } else {
        A1 = lv_delta<kRingSrc>(p, b, max_last, min_last, T, t1, n);
        A2 = lv_delta<kRingSrc>(p, b, max_last, min_last, T, t2, n);
      }
      sum += theta * (A2 - A1);
    }
    v = sum / p.Ba;
  }
  feat[idx] = v;
}

// [residue | chunk] of every channel, back to back at soff (the parent's frame kernel takes one contiguous batch).
__global__ void __launch_bounds__(256)
lv_pack_kernel(LvParams p, const int16_t *__restrict__ chunk, const long long *__restrict__ coff,
               const int *__restrict__ soff, const int *__restrict__ rlen, const int16_t *__restrict__ res, int total,
               int16_t *__restrict__ staged) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = jamd::find_span(soff, p.nchan, idx), j = idx - soff[c], r = rlen[c];
  staged[idx] = j < r ? res[(size_t)c * p.fs + j] : chunk[coff[c] + (j - r)];
}

// energy_max_prepare() sets max to 0.0 and energy_max_normalize() raises it over every base frame, also of a segment
// too short to emit anything; the next segment reads it, so it moves to emax only where the segment ends.  With
// `staged` (a push) the channel also keeps the last newr samples of its staged batch and the newest R base vectors.
// Launched behind lv_feat_kernel, which reads the previous maximum and the ring's previous contents.
__global__ void __launch_bounds__(256)
lv_keep_kernel(LvParams p, LvState s, const float *__restrict__ stat, const int *__restrict__ boff,
               const int *__restrict__ told, const int *__restrict__ act, const int16_t *__restrict__ staged,
               const int *__restrict__ soff, const int *__restrict__ newr) {
  __shared__ float red[256];
  const int c = blockIdx.x, a = act[c];
  if (!(a & kActive)) return;
  const int b0 = boff[c], nb = boff[c + 1] - b0;
  if (staged) {
    const int nr = newr[c];
    const int16_t *src = staged + soff[c + 1] - nr;
    for (int k = threadIdx.x; k < nr; k += 256) s.res[(size_t)c * p.fs + k] = src[k];
    const int keep = nb < p.R ? nb : p.R, T = told[c] + nb;        // frames T - keep .. T - 1
    float *ring = s.ring + (size_t)c * p.R * p.baselen;
    for (int k = threadIdx.x; k < keep * p.baselen; k += 256) {
      const int j = nb - keep + k / p.baselen, n = k % p.baselen;
      ring[(size_t)((T - nb + j) % p.R) * p.baselen + n] = stat[(size_t)(b0 + j) * p.baselen + n];
    }
  }
  if (!p.enorm) return;
  float m = 0.0f;
  for (int t = b0 + threadIdx.x; t < b0 + nb; t += 256) m = fmaxf(m, stat[(size_t)t * p.baselen + p.baselen - 1]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    m = red[0];
    if (a & kCont) m = fmaxf(m, s.rmax[c]);
    if (a & kFinal) s.emax[c] = m; else s.rmax[c] = m;
  }
}

// CMN_realtime() (:342-399) over the N frames f0[c] .. of the channel, after CMN_realtime_prepare() or, with kCont,
// from the chains the last push left; consecutive lanes take consecutive elements of one frame.  Frame t lands in row
// t - i at block i of every row it is part of (splice_mfcc()); of the rows this call completes, the first is
// max(0, f0 - (splice - 1)), and the frames below f0 they hold come from `sp`.  With splice 1 and every frame stored,
// CMN_realtime_update() would recompute now.mfcc_var from the stored (normalised) vectors against the un-normalised
// mean (:418-434): that is done here where the segment ends, over the rows of this call (hist NULL: a whole segment)
// or over `hist`, which then takes every row of the open segment ([nchan][hcap][veclen]).
__global__ void __launch_bounds__(64)
lv_cmn_kernel(LvParams p, LvState s, const float *__restrict__ feat, const int *__restrict__ noff,
              const int *__restrict__ ooff, const int *__restrict__ act, const int *__restrict__ f0tab,
              float *__restrict__ out, float *__restrict__ hist, int hcap) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= p.nchan * p.veclen) return;
  const int c = idx / p.veclen, d = idx % p.veclen;
  const int a = act[c];
  if (!(a & kActive)) return;
  const int n0 = noff[c], N = noff[c + 1] - n0, o0 = ooff[c], To = ooff[c + 1] - o0, f0 = f0tab[c];
  const int VL = p.veclen * p.splice, S1 = p.splice - 1;
  const int r0 = f0 > S1 ? f0 - S1 : 0;
  const float *col = feat + (size_t)n0 * p.veclen + d;
  const bool set = (s.flags[c] & kSet) != 0;
  const float cinit = s.cmean[idx];
  const double sd = (set && p.var) ? sqrt((double)s.cvar[idx]) : 1.0;
  float sum = 0.0f, var = 0.0f;
  if (a & kCont) {
    sum = s.now_sum[idx]; var = s.now_var[idx];
    for (int tf = r0; tf < f0; tf++) {        // (S1 > 0: r0 == f0 otherwise)
      const float m = s.sp[((size_t)c * S1 + tf % S1) * p.veclen + d];
      for (int i = 0; i < p.splice; i++) {
        const int o = tf - i - r0;
        if (o >= 0 && o < To) out[(size_t)(o0 + o) * VL + i * p.veclen + d] = m;
      }
    }
  }
  float *rows = hist ? hist + (size_t)c * hcap * p.veclen : out + (size_t)o0 * VL;
  const int sp0 = S1 > 0 && !(a & kFinal) ? N - S1 : N;   // the vectors the next push splices: the last S1, unless it ends
  for (int t = 0; t < N; t++) {
    const int tf = f0 + t;
    float m = col[(size_t)t * p.veclen];
    sum += m;
    double x;
    if (set) {
      if (p.do_map) {
        x = sum + p.cweight * cinit;
        const double y = (double)(tf + 1) + p.cweight;
        x /= y;
      } else {
        x = cinit;
      }
    } else {
      x = sum / (tf + 1);
    }
    if (p.var) var += (m - x) * (m - x);
    if (p.mean && d < p.mfcc_dim) m -= x;
    if (p.var && set) m /= sd;
    for (int i = 0; i < p.splice; i++) {
      const int o = tf - i - r0;
      if (o >= 0 && o < To) out[(size_t)(o0 + o) * VL + i * p.veclen + d] = m;
    }
    if (t >= sp0) s.sp[((size_t)c * S1 + tf % S1) * p.veclen + d] = m;
    if (hist) rows[(size_t)tf * p.veclen + d] = m;
  }
  const int Nall = f0 + N;
  if (p.var && (a & kReest)) {
    const float mean = sum / (float)Nall;
    float x = 0.0f;
    for (int t = 0; t < Nall; t++) {
      const float v = rows[(size_t)t * VL + d];
      x += (v - mean) * (v - mean);
    }
    var = x;
  }
  s.now_sum[idx] = sum;
  s.now_var[idx] = var;
  if (d == 0) s.now_fn[c] = Nall;
}

// [nchan][from][veclen] -> [nchan][to][veclen] when the row history grows
__global__ void __launch_bounds__(256)
lv_grow_kernel(const float *__restrict__ src, float *__restrict__ dst, long long from, long long to, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  dst[(idx / from) * to + idx % from] = src[idx];
}

__global__ void __launch_bounds__(256)
lv_copy_kernel(LvParams p, const float *__restrict__ feat, const int *__restrict__ noff, const int *__restrict__ ooff,
               int Tout, float *__restrict__ out) {
  const int VL = p.veclen * p.splice;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Tout * VL) return;
  const int o = (int)(idx / VL), k = (int)(idx % VL);
  const int c = jamd::find_span(ooff, p.nchan, o);
  const int i = k / p.veclen, d = k % p.veclen;
  out[idx] = feat[(size_t)(noff[c] + (o - ooff[c]) + i) * p.veclen + d];
}

// Frames CMN_realtime_update() sums for channel c: now, then the list newest first until CPMAX is reached.
__device__ __forceinline__ int lv_list_frames(const LvState &s, int c, int *last) {
  int frames = s.now_fn[c], i = 0;
  const int head = s.head[c], num = s.cnum[c];
  for (; i < num; i++) {
    frames += s.ring_fn[c * kRing + ((head + i) & (kRing - 1))];
    if (frames >= LV_CPMAX) { i++; break; }
  }
  *last = i;                                  // entries summed
  return frames;
}

// CMN_realtime_update() (:407-479) per element.  The scalars it reads change only in lv_commit_scalars, behind it.
__global__ void __launch_bounds__(64)
lv_commit_kernel(LvParams p, LvState s, const unsigned char *__restrict__ update) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= p.nchan * p.veclen) return;
  const int c = idx / p.veclen, d = idx % p.veclen;
  if ((update && !update[c]) || s.now_fn[c] == 0) return;
  int used;
  const int frames = lv_list_frames(s, c, &used);
  const int head = s.head[c];
  const float *ring = s.ring_sum + (size_t)c * kRing * p.veclen;
  float cm = s.now_sum[idx];
  for (int i = 0; i < used; i++) cm += ring[(size_t)((head + i) & (kRing - 1)) * p.veclen + d];
  cm /= (float)frames;
  s.cmean[idx] = cm;
  if (p.var && !(s.flags[c] & kLoaded)) {
    const int an = s.all_fn[c], nn = s.now_fn[c];
    const float av = (s.all_var[idx] * an + s.now_var[idx]) / (an + nn);
    s.all_var[idx] = av;
    s.cvar[idx] = av;
  }
  s.ring_sum[((size_t)c * kRing + ((head + kRing - 1) & (kRing - 1))) * p.veclen + d] = s.now_sum[idx];
}

__global__ void __launch_bounds__(64)
lv_commit_scalars(LvParams p, LvState s, const unsigned char *__restrict__ update) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= p.nchan) return;
  if ((update && !update[c]) || s.now_fn[c] == 0) return;
  int used;
  const int frames = lv_list_frames(s, c, &used);
  const int fl = s.flags[c];
  if (p.var && !(fl & kLoaded)) s.all_fn[c] += s.now_fn[c];
  s.flags[c] = fl | kSet;
  int num = s.cnum[c], max = s.cmax[c];
  if (num == max && frames < LV_CPMAX && max + LV_CPSTEP <= kRing) max += LV_CPSTEP;
  const int head = (s.head[c] + kRing - 1) & (kRing - 1);
  s.ring_fn[c * kRing + head] = s.now_fn[c];
  s.head[c] = head;
  if (num < max) num++;
  s.cnum[c] = num; s.cmax[c] = max;
}

}  // namespace

// ---------------------------------------------------------------------------------- launchers (frontend_host.h)
int lv_launch_pack(jamd_frontend_live *l, hipStream_t st, const int16_t *dev_samples, const LvPacked &pk, long long S) {
  hipLaunchKernelGGL(lv_pack_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, l->p, dev_samples, pk.coff, pk.soff,
                     pk.rlen, l->s.res, (int)S, l->d_stage);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int lv_launch(jamd_frontend_live *l, hipStream_t st, const int *d_boff, long long N, long long O, const LvPacked *pk,
              float *dev_out) {
  const LvParams &p = l->p;
  const int nchan = l->nchan;
  const int *d_noff = d_boff + nchan + 1, *d_ooff = d_noff + nchan + 1, *d_act = d_ooff + nchan + 1;
  const int *d_told = d_act + nchan + 1, *d_f0 = pk ? d_told + nchan + 1 : d_told;   // (a whole segment: one table of zeros)
  const float *d_stat = l->f->d_stat;
  const long long nfeat = N * p.veclen;
  if (nfeat > 0) {
    const dim3 grid((unsigned)((nfeat + 255) / 256));
    if (pk)
      hipLaunchKernelGGL(lv_feat_kernel<true>, grid, dim3(256), 0, st, p, d_stat, l->s.ring, d_boff, d_told, d_f0, d_noff,
                         l->s.emax, (int)N, l->d_feat);
    else
      hipLaunchKernelGGL(lv_feat_kernel<false>, grid, dim3(256), 0, st, p, d_stat, l->s.ring, d_boff, d_told, d_f0, d_noff,
                         l->s.emax, (int)N, l->d_feat);
    JAMD_HIP(hipGetLastError());
  }
  if (pk || p.enorm) {
    hipLaunchKernelGGL(lv_keep_kernel, dim3(nchan), dim3(256), 0, st, p, l->s, d_stat, d_boff, d_told, d_act,
                       pk ? pk->staged : nullptr, pk ? pk->soff : nullptr, pk ? pk->newr : nullptr);
    JAMD_HIP(hipGetLastError());
  }
  if (p.mean || p.var || pk) {               // (a push always takes the chain: it keeps the vectors splicing needs)
    hipLaunchKernelGGL(lv_cmn_kernel, dim3((nchan * p.veclen + 63) / 64), dim3(64), 0, st, p, l->s, l->d_feat, d_noff,
                       d_ooff, d_act, d_f0, dev_out, pk && p.var && p.splice == 1 ? l->d_hist : nullptr, l->hist_rows);
    JAMD_HIP(hipGetLastError());
  } else if (O > 0) {
    const long long nout = O * p.veclen * p.splice;
    hipLaunchKernelGGL(lv_copy_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, p, l->d_feat, d_noff, d_ooff,
                       (int)O, dev_out);
    JAMD_HIP(hipGetLastError());
  }
  return JAMD_OK;
}

int lv_launch_grow(jamd_frontend_live *l, hipStream_t st, float *dst, long long from_rows, long long to_rows) {
  const long long from = from_rows * l->p.veclen, total = from * l->nchan;
  hipLaunchKernelGGL(lv_grow_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, l->d_hist, dst, from,
                     to_rows * l->p.veclen, total);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) return JAMD_OK;
  jamd_set_error("jamd_frontend_live_push_dev: moving the row history failed: %s", hipGetErrorString(e));
  return JAMD_ELAUNCH;
}

int lv_launch_commit(jamd_frontend_live *l, hipStream_t st, const unsigned char *d_mask) {
  const LvParams &p = l->p;
  hipLaunchKernelGGL(lv_commit_kernel, dim3((p.nchan * p.veclen + 63) / 64), dim3(64), 0, st, p, l->s, d_mask);
  JAMD_HIP(hipGetLastError());
  hipLaunchKernelGGL(lv_commit_scalars, dim3((p.nchan + 63) / 64), dim3(64), 0, st, p, l->s, d_mask);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}
