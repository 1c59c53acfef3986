// frontend_live.hip -- the live-input front end on gfx950: many independent channels per call, a whole segment each
// (jamd_frontend_live_run_*) or the next chunk of an open segment (jamd_frontend_live_push_*).
//
// Reproduces, bit for bit, the vectors the reference stores into mfcc->param for a microphone, a socket or -realtime:
// RealTimeMFCC() (libjulius/src/realtime-1stpass.c:496-602) for the main loop and the flush loop of RealTimeParam()
// (:1215-1304) for the tail, with the pipelined pieces of libsent/src/wav2mfcc/wav2mfcc-pipe.c: energy_max_normalize(),
// the cyclic delta / acceleration buffers (WMP_deltabuf_*), CMN_realtime() and CMN_realtime_update().  The base
// coefficients are WMP_calc(), which the buffered front end's frame kernel already computes (frontend.hip, reached
// through frontend_host.h); everything behind it differs from the buffered front end in every normalised element and
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
#include "jamd_device.h"
#include "frontend_host.h"
#include "cmn_file.h"
#include <cmath>
#include <cstdint>

#define LV_LOG_TEN 2.30258509   // stddefs.h:109
#define LV_CPMAX 500            // mfcc.h:47-48
#define LV_CPSTEP 5

namespace {

// Segments in the history of one channel.  CMN_realtime_update() sums the list newest first until CPMAX frames are
// reached, and lengthens the list (by CPSTEP) only while the whole list plus the new segment stays below CPMAX; every
// entry holds a frame or more, so clist_max never passes CPMAX - 1 + CPSTEP.
constexpr int kRing = 512;
constexpr int kSet = 1, kLoaded = 2;         // flags: cmean_init_set, loaded_from_file
// per-call channel bits: takes part; the variance is re-estimated; the segment was open before; it ends here
constexpr int kActive = 1, kReest = 2, kCont = 4, kFinal = 8;
constexpr int kHistDefault = 3000;           // rows of an open segment kept for the re-estimation (jamd_frontend_live_stream_cap())

struct LvParams {
  int nchan, veclen, baselen, nb, splice, delta, acc, delWin, accWin, Bd, Ba, enorm, mean, var, mfcc_dim, do_map;
  int R, fs;                                 // slots of the base-vector ring; framesize
  float escale, silFloor, cweight;
};

struct LvState {
  float *emax;                               // [nchan] ENERGYWork.max
  float *cmean, *cvar;                       // [nchan][veclen] cmean_init, cvar_init
  int *flags;                                // [nchan] kSet | kLoaded
  float *now_sum, *now_var; int *now_fn;     // CMNWork.now
  float *all_var; int *all_fn;               // CMNWork.all
  float *ring_sum; int *ring_fn;             // [nchan][kRing][veclen] / [nchan][kRing]: clist, newest at head
  int *head, *cnum, *cmax;                   // [nchan]
  // the open segment of a channel (jamd_frontend_live_push_*)
  float *rmax;                               // [nchan] ENERGYWork.max so far
  float *ring;                               // [nchan][R][baselen] raw base vectors, frame t in slot t % R
  float *sp;                                 // [nchan][splice - 1][veclen] normalised vectors, frame t in slot t % (splice - 1)
  int16_t *res;                              // [nchan][framesize] samples behind the last whole window
};

// Where the base vectors of one channel's segment lie: frames below `told` in the ring, the others in this call's batch.
struct LvSrc { const float *stat, *ring; int told; };

__device__ __forceinline__ int lv_find(const int *off, int n, int g) {   // the last u with off[u] <= g
  int lo = 0, hi = n;
  while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}

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
  const int c = lv_find(noff, p.nchan, g);
  const LvSrc b{stat + (size_t)boff[c] * p.baselen, ring + (size_t)c * p.R * p.baselen, kRingSrc ? told[c] : 0};
  const int t = (kRingSrc ? f0[c] : 0) + (g - noff[c]), T = b.told + (boff[c + 1] - boff[c]);
  float max_last = 0.0f, min_last = 0.0f;
  if (p.enorm) {                              // energy_max_prepare()
    max_last = emax[c];
    min_last = (float)(max_last - (p.silFloor * LV_LOG_TEN) / 10.0);
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
  const int c = lv_find(soff, p.nchan, idx), j = idx - soff[c], r = rlen[c];
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
  const int c = lv_find(ooff, p.nchan, o);
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

struct LvCounts { long long Tb, Nf, To; bool reest; };

// The frame counts of one segment of n samples (realtime-1stpass.c:290, :853-859, :1197-1287).
LvCounts lv_counts(const jamd_frontend_desc &d, long long n) {
  LvCounts k{0, 0, 0, false};
  if (n >= (long long)d.framesize + 1) k.Tb = (n - d.framesize - 1) / d.frameshift + 1;
  long long Nd = k.Tb;
  if (d.delta && k.Tb < d.delWin) Nd = 0;
  k.Nf = Nd;
  long long holes = 0;
  if (d.acc) {
    if (Nd < d.accWin) k.Nf = 0;
    // a delta vector that the flush loop hands to an acceleration buffer still in its delay advances the reference's
    // frame counter without a vector being stored (:1249-1257): samplenum then differs from now.framenum
    const long long Md = k.Tb > d.delWin ? k.Tb - d.delWin : 0;
    const long long lim = Nd < d.accWin ? Nd : d.accWin;
    holes = lim > Md ? lim - Md : 0;
  }
  k.To = k.Nf - (d.splice - 1);
  if (k.To < 0) k.To = 0;
  k.reest = d.splice == 1 && k.Nf > 0 && holes == 0;
  return k;
}

}  // namespace

struct jamd_frontend_live {
  jamd_frontend *f = nullptr;
  FeInfo in{};
  int nchan = 0;
  LvParams p{};
  LvState s{};
  void *state = nullptr;                     // one allocation behind every array of `s`
  float *d_feat = nullptr; size_t feat_cap = 0;
  unsigned char *d_upd = nullptr;            // [nchan] the commit mask
  int16_t *d_in = nullptr; size_t in_cap = 0;   // run_host staging
  float *d_out = nullptr; size_t out_cap = 0;
  // open segments (jamd_frontend_live_push_*): per channel whether one is open and the samples it has taken
  std::vector<char> open;
  std::vector<long long> ns;
  int nopen = 0;
  int16_t *d_stage = nullptr; size_t stage_cap = 0;   // [residue | chunk] of every channel
  char *h_tab = nullptr, *d_tab = nullptr;   // coff (int64 [nchan + 1]) | soff | rlen | newr (int [nchan + 1]), pinned / device
  hipEvent_t ev_tab = nullptr;               // the upload that last read h_tab
  float *d_hist = nullptr;                   // [nchan][hist_rows][veclen], cvn with splice 1 only
  int hist_rows = 0, hist_cap = kHistDefault;
};

// Frames out of the main loop for Tb base frames of a segment that has not ended, and rows those complete.
static long long lv_open_frames(const jamd_frontend_desc &d, long long Tb) {
  const long long L = (d.delta ? d.delWin : 0) + (d.acc ? d.accWin : 0);
  return Tb > L ? Tb - L : 0;
}
static long long lv_rows_of(const jamd_frontend_desc &d, long long frames) {
  return frames > d.splice - 1 ? frames - (d.splice - 1) : 0;
}

extern "C" {

int jamd_frontend_live_default(jamd_frontend_live_desc *d) {
  if (!d) { jamd_set_error("jamd_frontend_live_default: d is NULL"); return JAMD_EINVAL; }
  d->map_cmn = 1; d->map_weight = 100.0f;    // default.c:153-156
  d->cmean_init = nullptr; d->cvar_init = nullptr;
  return JAMD_OK;
}

int jamd_frontend_live_frames(const jamd_frontend_desc *d, int64_t nsamples) {
  if (!d || d->framesize < 1 || d->frameshift < 1 || d->splice < 1 || (d->delta && d->delWin < 1) ||
      (d->acc && d->accWin < 1)) {
    jamd_set_error("jamd_frontend_live_frames: NULL descriptor, or framesize / frameshift / splice / window < 1");
    return JAMD_EINVAL;
  }
  const long long T = lv_counts(*d, nsamples).To;
  return T > 0x7fffffff ? 0x7fffffff : (int)T;
}

void jamd_frontend_live_destroy(jamd_frontend_live *l) {
  if (!l) return;
  if (l->state) (void)hipFree(l->state);
  if (l->d_feat) (void)hipFree(l->d_feat);
  if (l->d_upd) (void)hipFree(l->d_upd);
  if (l->d_in) (void)hipFree(l->d_in);
  if (l->d_out) (void)hipFree(l->d_out);
  if (l->d_stage) (void)hipFree(l->d_stage);
  if (l->d_tab) (void)hipFree(l->d_tab);
  if (l->d_hist) (void)hipFree(l->d_hist);
  if (l->h_tab) (void)hipHostFree(l->h_tab);
  if (l->ev_tab) (void)hipEventDestroy(l->ev_tab);
  delete l;
}

int jamd_frontend_live_state_set(jamd_frontend_live *l, int chan, const float *cmean, const float *cvar) {
  if (!l || !cmean || chan < 0 || chan >= l->nchan) {
    jamd_set_error("jamd_frontend_live_state_set: NULL argument or channel out of range");
    return JAMD_EINVAL;
  }
  if (l->p.var && !cvar) { jamd_set_error("jamd_frontend_live_state_set: the kind has cvn: a variance is needed"); return JAMD_EINVAL; }
  if (!l->open.empty() && l->open[chan]) {
    jamd_set_error("jamd_frontend_live_state_set: channel %d has an open segment (end it with a final push first)", chan);
    return JAMD_ESTATE;
  }
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  const size_t V = l->p.veclen;
  JAMD_HIP(hipMemcpy(l->s.cmean + chan * V, cmean, V * sizeof(float), hipMemcpyHostToDevice));
  if (l->p.var) JAMD_HIP(hipMemcpy(l->s.cvar + chan * V, cvar, V * sizeof(float), hipMemcpyHostToDevice));
  const int fl = kSet | kLoaded;             // CMN_load_from_file() :647-648
  JAMD_HIP(hipMemcpy(l->s.flags + chan, &fl, sizeof(int), hipMemcpyHostToDevice));
  return JAMD_OK;
}

int jamd_frontend_live_state_get(jamd_frontend_live *l, int chan, float *cmean, float *cvar, float *emax, int *flags) {
  if (!l || chan < 0 || chan >= l->nchan) {
    jamd_set_error("jamd_frontend_live_state_get: NULL object or channel out of range");
    return JAMD_EINVAL;
  }
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  const size_t V = l->p.veclen;
  if (cmean) JAMD_HIP(hipMemcpy(cmean, l->s.cmean + chan * V, V * sizeof(float), hipMemcpyDeviceToHost));
  if (cvar) JAMD_HIP(hipMemcpy(cvar, l->s.cvar + chan * V, V * sizeof(float), hipMemcpyDeviceToHost));
  if (emax) JAMD_HIP(hipMemcpy(emax, l->s.emax + chan, sizeof(float), hipMemcpyDeviceToHost));
  if (flags) JAMD_HIP(hipMemcpy(flags, l->s.flags + chan, sizeof(int), hipMemcpyDeviceToHost));
  return JAMD_OK;
}

int jamd_frontend_live_create(jamd_frontend *f, const jamd_frontend_live_desc *ld, int nchan, jamd_frontend_live **out) {
  if (!f || !ld || !out || nchan < 1) { jamd_set_error("jamd_frontend_live_create: NULL argument or nchan < 1"); return JAMD_EINVAL; }
  *out = nullptr;
  FeInfo in;
  fe_info(f, &in);
  const jamd_frontend_desc &d = in.d;
  if (d.absesup && d.acc) {
    jamd_set_error("jamd_frontend_live_create: _N together with _A is not served: the reference's flush loop "
                   "(realtime-1stpass.c:1233-1241) strips the absolute energy before the acceleration buffer, its main "
                   "loop after it, so the last frames of every segment carry a stale slot");
    return JAMD_EINVAL;
  }
  if (d.frameshift > d.framesize + 1) {
    jamd_set_error("jamd_frontend_live_create: frameshift %d beyond the live window of %d samples (the reference's "
                   "window shift has no meaning there)", d.frameshift, d.framesize + 1);
    return JAMD_EINVAL;
  }
  if (d.cvn && ld->cmean_init && !ld->cvar_init) {
    jamd_set_error("jamd_frontend_live_create: the kind has cvn: an initial mean needs an initial variance");
    return JAMD_EINVAL;
  }
  if ((long long)nchan * d.veclen > 0x7fffffffLL / kRing) {
    jamd_set_error("jamd_frontend_live_create: %d channels of %d elements are too many", nchan, d.veclen);
    return JAMD_EINVAL;
  }
  jamd_frontend_live *l = new jamd_frontend_live();
  l->f = f; l->in = in; l->nchan = nchan;
  LvParams &p = l->p;
  p.nchan = nchan; p.veclen = d.veclen; p.baselen = d.baselen; p.nb = d.baselen - (d.absesup ? 1 : 0);
  p.splice = d.splice; p.delta = d.delta; p.acc = d.acc; p.delWin = d.delWin; p.accWin = d.accWin;
  p.Bd = 0; p.Ba = 0;                        // WMP_deltabuf_new(): B = 2 * sum of theta^2, an int
  for (int i = 1; i <= d.delWin; i++) p.Bd += i * i;
  for (int i = 1; i <= d.accWin; i++) p.Ba += i * i;
  p.Bd *= 2; p.Ba *= 2;
  p.enorm = d.energy && d.enormal; p.mean = d.cmn != 0; p.var = d.cvn != 0;
  p.mfcc_dim = d.mfcc_dim + (d.c0 ? 1 : 0);
  p.do_map = ld->map_cmn != 0; p.cweight = ld->map_weight;
  p.escale = d.escale; p.silFloor = d.silFloor;
  p.R = 2 * ((d.delta ? d.delWin : 0) + (d.acc ? d.accWin : 0));
  if (p.R < 1) p.R = 1;
  p.fs = d.framesize;
  l->open.assign(nchan, 0); l->ns.assign(nchan, 0);
  hipError_t e = hipSetDevice(in.eng->device);
  const size_t C = nchan, V = d.veclen, CV = C * V;
  // floats: emax | cmean | cvar | now_sum | now_var | all_var | ring_sum | rmax | ring | sp ;
  // ints: flags now_fn all_fn head cnum cmax | ring_fn ; int16: res
  const size_t nring = C * p.R * d.baselen, nsp = CV * (d.splice - 1), nres = C * d.framesize;
  const size_t nfl = C + 5 * CV + CV * kRing + C + nring + nsp, nin = 6 * C + C * kRing;
  const size_t nstate = nfl * sizeof(float) + nin * sizeof(int) + nres * sizeof(int16_t);
  const size_t ntab = sizeof(long long) * (C + 1) + 3 * sizeof(int) * (C + 1);
  if (e == hipSuccess) e = hipMalloc(&l->state, nstate);
  if (e == hipSuccess) e = hipMalloc((void **)&l->d_upd, C);
  if (e == hipSuccess) e = hipMalloc((void **)&l->d_tab, ntab);
  if (e == hipSuccess) e = hipHostMalloc((void **)&l->h_tab, ntab, hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&l->ev_tab, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMemset(l->state, 0, nstate);
  if (e != hipSuccess) {
    jamd_set_error("jamd_frontend_live_create: device allocation failed: %s", hipGetErrorString(e));
    jamd_frontend_live_destroy(l);
    return e == hipErrorOutOfMemory ? JAMD_ENOMEM : JAMD_ENODEV;
  }
  LvState &s = l->s;
  float *q = (float *)l->state;
  s.emax = q; q += C;
  s.cmean = q; q += CV; s.cvar = q; q += CV; s.now_sum = q; q += CV; s.now_var = q; q += CV; s.all_var = q; q += CV;
  s.ring_sum = q; q += CV * kRing;
  s.rmax = q; q += C; s.ring = q; q += nring; s.sp = q; q += nsp;
  int *r = (int *)q;
  s.flags = r; r += C; s.now_fn = r; r += C; s.all_fn = r; r += C; s.head = r; r += C; s.cnum = r; r += C; s.cmax = r; r += C;
  s.ring_fn = r; r += C * kRing;
  s.res = (int16_t *)r;
  // energy_max_init(): 5.0; CMN_realtime_new(): clist_max = CPSTEP
  std::vector<float> five(C, 5.0f);
  std::vector<int> step(C, LV_CPSTEP);
  e = hipMemcpy(s.emax, five.data(), C * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s.cmax, step.data(), C * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    jamd_set_error("jamd_frontend_live_create: hipMemcpy failed: %s", hipGetErrorString(e));
    jamd_frontend_live_destroy(l);
    return JAMD_ENODEV;
  }
  if (ld->cmean_init && (d.cmn || d.cvn)) {
    for (int c = 0; c < nchan; c++) {
      const int rc = jamd_frontend_live_state_set(l, c, ld->cmean_init, ld->cvar_init);
      if (rc != JAMD_OK) { jamd_frontend_live_destroy(l); return rc; }
    }
  }
  *out = l;
  return JAMD_OK;
}

}  // extern "C"

// What both entries launch behind the base frames: tabs are boff | noff | ooff | act | told | f0 on the device, N
// feature frames and O rows in all.  pk (a push) names the staged batch and its tables.
struct LvPacked { const int16_t *staged; const int *soff, *newr; };
static int lv_launch(jamd_frontend_live *l, hipStream_t st, const float *d_stat, const int *d_boff, const int *d_told,
                     const int *d_f0, long long N, long long O, const LvPacked *pk, float *dev_out) {
  const LvParams &p = l->p;
  const int nchan = l->nchan;
  const int *d_noff = d_boff + nchan + 1, *d_ooff = d_noff + nchan + 1, *d_act = d_ooff + nchan + 1;
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

static int lv_refuse_ss_calc(jamd_frontend_live *l, const char *who) {
  FeInfo in;
  fe_info(l->f, &in);
  if (in.ss_mode != JAMD_SS_CALC) return JAMD_OK;
  jamd_set_error("%s: JAMD_SS_CALC is set on the parent front end: a live segment has no head known in advance (use "
                 "JAMD_SS_LOAD or JAMD_SS_OFF)", who);
  return JAMD_EINVAL;
}

extern "C" {

int jamd_frontend_live_run_dev(jamd_frontend_live *l, const int16_t *dev_samples, const int64_t *sample_off,
                               float *dev_out, int *frame_off, void *stream) {
  if (!l || !dev_samples || !sample_off || !dev_out) { jamd_set_error("jamd_frontend_live_run_dev: NULL argument"); return JAMD_EINVAL; }
  int rc;
  if ((rc = lv_refuse_ss_calc(l, "jamd_frontend_live_run_dev")) != JAMD_OK) return rc;
  if (l->nopen) {
    jamd_set_error("jamd_frontend_live_run_dev: %d channel(s) have an open segment (end them with a final push first)", l->nopen);
    return JAMD_ESTATE;
  }
  const jamd_frontend_desc &d = l->in.d;
  const int nchan = l->nchan;
  std::vector<int> boff(nchan + 1), noff(nchan + 1), ooff(nchan + 1), act(nchan + 1, 0), zero(nchan + 1, 0);
  long long B = 0, N = 0, O = 0;
  for (int c = 0; c < nchan; c++) {
    if (sample_off[c] < 0 || sample_off[c + 1] < sample_off[c]) {
      jamd_set_error("jamd_frontend_live_run_dev: sample_off is not non-decreasing from 0 at channel %d", c);
      return JAMD_EINVAL;
    }
    const long long n = sample_off[c + 1] - sample_off[c];
    const LvCounts k = lv_counts(d, n);
    boff[c] = (int)B; noff[c] = (int)N; ooff[c] = (int)O;
    act[c] = (n > 0 ? kActive | kFinal : 0) | (k.reest ? kReest : 0);
    B += k.Tb; N += k.Nf; O += k.To;
    if ((B + 1) * (long long)d.vecbuflen * d.splice > 0x7fffffffLL) {
      jamd_set_error("jamd_frontend_live_run_dev: batch too large (%lld frames)", B);
      return JAMD_EINVAL;
    }
  }
  boff[nchan] = (int)B; noff[nchan] = (int)N; ooff[nchan] = (int)O;
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  hipStream_t st = jamd_stream(l->in.eng, stream);
  if ((rc = jamd_grow(&l->d_feat, &l->feat_cap, (size_t)(N > 0 ? N : 1) * d.veclen * sizeof(float))) != JAMD_OK) return rc;
  const float *d_stat; const int *d_tabs;
  if ((rc = fe_base_frames(l->f, st, dev_samples, sample_off, nchan, {&boff, &noff, &ooff, &act, &zero}, &d_stat, &d_tabs)) != JAMD_OK)
    return rc;
  const int *d_zero = d_tabs + 4 * (nchan + 1);   // a whole segment: nothing in the ring, frames from 0
  if ((rc = lv_launch(l, st, d_stat, d_tabs, d_zero, d_zero, N, O, nullptr, dev_out)) != JAMD_OK) return rc;
  if (frame_off) memcpy(frame_off, ooff.data(), sizeof(int) * (nchan + 1));
  return JAMD_OK;
}

int jamd_frontend_live_push_frames(const jamd_frontend_desc *d, int64_t samples_before, int64_t chunk, int final) {
  if (!d || d->framesize < 1 || d->frameshift < 1 || d->splice < 1 || (d->delta && d->delWin < 1) ||
      (d->acc && d->accWin < 1) || samples_before < 0 || chunk < 0) {
    jamd_set_error("jamd_frontend_live_push_frames: NULL descriptor, framesize / frameshift / splice / window < 1, or a "
                   "negative sample count");
    return JAMD_EINVAL;
  }
  const long long before = lv_rows_of(*d, lv_open_frames(*d, lv_counts(*d, samples_before).Tb));
  const LvCounts k = lv_counts(*d, samples_before + chunk);
  const long long T = (final ? k.To : lv_rows_of(*d, lv_open_frames(*d, k.Tb))) - before;
  return T > 0x7fffffff ? 0x7fffffff : (int)T;
}

int jamd_frontend_live_stream_cap(jamd_frontend_live *l, int max_rows) {
  if (!l || max_rows < 1) { jamd_set_error("jamd_frontend_live_stream_cap: NULL object or max_rows < 1"); return JAMD_EINVAL; }
  if (l->nopen) {
    jamd_set_error("jamd_frontend_live_stream_cap: %d channel(s) have an open segment", l->nopen);
    return JAMD_ESTATE;
  }
  l->hist_cap = max_rows;
  return JAMD_OK;
}

int jamd_frontend_live_push_dev(jamd_frontend_live *l, const int16_t *dev_samples, const int64_t *sample_off,
                                const unsigned char *final, float *dev_out, int *frame_off, void *stream) {
  if (!l || !sample_off) { jamd_set_error("jamd_frontend_live_push_dev: NULL argument"); return JAMD_EINVAL; }
  int rc;
  if ((rc = lv_refuse_ss_calc(l, "jamd_frontend_live_push_dev")) != JAMD_OK) return rc;
  const jamd_frontend_desc &d = l->in.d;
  const int nchan = l->nchan;
  const bool keep_rows = d.cvn && d.splice == 1;
  std::vector<int> boff(nchan + 1), noff(nchan + 1), ooff(nchan + 1), act(nchan + 1, 0), told(nchan + 1, 0), f0(nchan + 1, 0);
  std::vector<int64_t> soff(nchan + 1);
  std::vector<long long> ns_after(l->ns);
  std::vector<char> open_after(l->open);
  // (h_tab is rewritten only once the upload that read it is done)
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  JAMD_HIP(hipEventSynchronize(l->ev_tab));
  long long *h_coff = (long long *)l->h_tab;
  int *h_soff = (int *)(h_coff + nchan + 1), *h_rlen = h_soff + nchan + 1, *h_newr = h_rlen + nchan + 1;
  long long B = 0, N = 0, O = 0, S = 0, need_rows = 0;
  bool any = false;
  for (int c = 0; c < nchan; c++) {
    if (sample_off[c] < 0 || sample_off[c + 1] < sample_off[c]) {
      jamd_set_error("jamd_frontend_live_push_dev: sample_off is not non-decreasing from 0 at channel %d", c);
      return JAMD_EINVAL;
    }
    const long long n = sample_off[c + 1] - sample_off[c];
    const bool fin = final && final[c], was = l->open[c] != 0;
    boff[c] = (int)B; noff[c] = (int)N; ooff[c] = (int)O;
    soff[c] = S; h_coff[c] = sample_off[c]; h_soff[c] = (int)S; h_rlen[c] = 0; h_newr[c] = 0;
    if (n == 0 && !(fin && was)) continue;     // idle, or an end without a segment
    any = true;
    const long long n_old = was ? l->ns[c] : 0, n_new = n_old + n;
    const LvCounts ko = lv_counts(d, n_old), kn = lv_counts(d, n_new);
    const long long r_old = n_old - ko.Tb * d.frameshift;
    const long long F_old = lv_open_frames(d, ko.Tb), F_new = fin ? kn.Nf : lv_open_frames(d, kn.Tb);
    if (keep_rows && F_new > l->hist_cap) {
      jamd_set_error("jamd_frontend_live_push_dev: channel %d would hold %lld rows of an open segment, beyond the cap of %d "
                     "(jamd_frontend_live_stream_cap())", c, F_new, l->hist_cap);
      return JAMD_EINVAL;
    }
    if (F_new > need_rows) need_rows = F_new;
    act[c] = kActive | (was ? kCont : 0) | (fin ? kFinal : 0) | (fin && kn.reest ? kReest : 0);
    told[c] = (int)ko.Tb; f0[c] = (int)F_old;
    h_rlen[c] = (int)r_old;
    h_newr[c] = fin ? 0 : (int)(n_new - kn.Tb * d.frameshift);
    B += kn.Tb - ko.Tb; N += F_new - F_old; O += lv_rows_of(d, F_new) - lv_rows_of(d, F_old);
    S += r_old + n;
    open_after[c] = !fin; ns_after[c] = fin ? 0 : n_new;
    if ((B + 1) * (long long)d.vecbuflen * d.splice > 0x7fffffffLL || S > 0x7fffffffLL || kn.Tb > 0x7fffffffLL) {
      jamd_set_error("jamd_frontend_live_push_dev: batch too large (%lld frames, %lld samples)", B, S);
      return JAMD_EINVAL;
    }
  }
  boff[nchan] = (int)B; noff[nchan] = (int)N; ooff[nchan] = (int)O;
  soff[nchan] = S; h_coff[nchan] = sample_off[nchan]; h_soff[nchan] = (int)S; h_rlen[nchan] = 0; h_newr[nchan] = 0;
  if ((sample_off[nchan] > 0 && !dev_samples) || (O > 0 && !dev_out)) {
    jamd_set_error("jamd_frontend_live_push_dev: NULL buffer");
    return JAMD_EINVAL;
  }
  if (frame_off) memcpy(frame_off, ooff.data(), sizeof(int) * (nchan + 1));
  if (!any) return JAMD_OK;
  hipStream_t st = jamd_stream(l->in.eng, stream);
  if ((rc = jamd_grow(&l->d_feat, &l->feat_cap, (size_t)(N > 0 ? N : 1) * d.veclen * sizeof(float))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&l->d_stage, &l->stage_cap, (size_t)(S > 0 ? S : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if (keep_rows && need_rows > l->hist_rows) {
    // the history grows: at least twofold, never beyond the cap; the rows of the open segments move over
    long long rows = 2LL * l->hist_rows > need_rows ? 2LL * l->hist_rows : need_rows;
    if (rows < 256) rows = 256;
    if (rows > l->hist_cap) rows = l->hist_cap;
    float *nh = nullptr;
    JAMD_HIP(hipMalloc((void **)&nh, (size_t)nchan * rows * d.veclen * sizeof(float)));
    if (l->d_hist) {
      const long long from = (long long)l->hist_rows * d.veclen, total = from * nchan;
      hipLaunchKernelGGL(lv_grow_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, l->d_hist, nh, from,
                         rows * d.veclen, total);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) {
        (void)hipFree(nh);
        jamd_set_error("jamd_frontend_live_push_dev: moving the row history failed: %s", hipGetErrorString(e));
        return JAMD_ELAUNCH;
      }
      JAMD_HIP(hipFree(l->d_hist));
    }
    l->d_hist = nh; l->hist_rows = (int)rows;
  }
  const size_t ntab = sizeof(long long) * (nchan + 1) + 3 * sizeof(int) * (nchan + 1);
  JAMD_HIP(hipMemcpyAsync(l->d_tab, l->h_tab, ntab, hipMemcpyHostToDevice, st));
  JAMD_HIP(hipEventRecord(l->ev_tab, st));
  const long long *d_coff = (const long long *)l->d_tab;
  const int *d_soff = (const int *)(d_coff + nchan + 1), *d_rlen = d_soff + nchan + 1, *d_newr = d_rlen + nchan + 1;
  if (S > 0) {
    hipLaunchKernelGGL(lv_pack_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, l->p, dev_samples, d_coff, d_soff,
                       d_rlen, l->s.res, (int)S, l->d_stage);
    JAMD_HIP(hipGetLastError());
  }
  const float *d_stat; const int *d_tabs;
  if ((rc = fe_base_frames(l->f, st, l->d_stage, soff.data(), nchan, {&boff, &noff, &ooff, &act, &told, &f0}, &d_stat,
                           &d_tabs)) != JAMD_OK)
    return rc;
  const LvPacked pk{l->d_stage, d_soff, d_newr};
  if ((rc = lv_launch(l, st, d_stat, d_tabs, d_tabs + 4 * (nchan + 1), d_tabs + 5 * (nchan + 1), N, O, &pk, dev_out)) != JAMD_OK)
    return rc;
  l->open.swap(open_after); l->ns.swap(ns_after);
  l->nopen = 0;
  for (int c = 0; c < nchan; c++) l->nopen += l->open[c] != 0;
  return JAMD_OK;
}

// Host buffers around _run_dev / _push_dev: `rows` is what the call will deliver.
static int lv_host_call(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off, const unsigned char *final,
                        bool push, long long rows, float *out, int *frame_off) {
  const int nchan = l->nchan;
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  int rc;
  const size_t ns = (size_t)sample_off[nchan], no = (size_t)rows * l->in.d.veclen * l->in.d.splice;
  if ((rc = jamd_grow(&l->d_in, &l->in_cap, (ns > 0 ? ns : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&l->d_out, &l->out_cap, (no > 0 ? no : 1) * sizeof(float))) != JAMD_OK) return rc;
  hipStream_t st = l->in.eng->stream;
  if (ns) JAMD_HIP(hipMemcpyAsync(l->d_in, samples, ns * sizeof(int16_t), hipMemcpyHostToDevice, st));
  rc = push ? jamd_frontend_live_push_dev(l, l->d_in, sample_off, final, l->d_out, frame_off, st)
            : jamd_frontend_live_run_dev(l, l->d_in, sample_off, l->d_out, frame_off, st);
  if (rc != JAMD_OK) return rc;
  if (no) JAMD_HIP(hipMemcpyAsync(out, l->d_out, no * sizeof(float), hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  return JAMD_OK;
}

int jamd_frontend_live_run_host(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off, float *out,
                                int *frame_off) {
  if (!l || !samples || !sample_off || !out) { jamd_set_error("jamd_frontend_live_run_host: NULL argument"); return JAMD_EINVAL; }
  long long O = 0;
  for (int c = 0; c < l->nchan; c++) {
    if (sample_off[c] < 0 || sample_off[c + 1] < sample_off[c]) {
      jamd_set_error("jamd_frontend_live_run_host: sample_off is not non-decreasing from 0 at channel %d", c);
      return JAMD_EINVAL;
    }
    O += lv_counts(l->in.d, sample_off[c + 1] - sample_off[c]).To;
  }
  return lv_host_call(l, samples, sample_off, nullptr, false, O, out, frame_off);
}

int jamd_frontend_live_push_host(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off,
                                 const unsigned char *final, float *out, int *frame_off) {
  if (!l || !sample_off) { jamd_set_error("jamd_frontend_live_push_host: NULL argument"); return JAMD_EINVAL; }
  long long O = 0;
  for (int c = 0; c < l->nchan; c++) {
    if (sample_off[c] < 0 || sample_off[c + 1] < sample_off[c]) {
      jamd_set_error("jamd_frontend_live_push_host: sample_off is not non-decreasing from 0 at channel %d", c);
      return JAMD_EINVAL;
    }
    const long long n = sample_off[c + 1] - sample_off[c];
    const bool fin = final && final[c];
    if (n == 0 && !(fin && l->open[c])) continue;
    O += jamd_frontend_live_push_frames(&l->in.d, l->open[c] ? l->ns[c] : 0, n, fin);
  }
  if ((sample_off[l->nchan] > 0 && !samples) || (O > 0 && !out)) {
    jamd_set_error("jamd_frontend_live_push_host: NULL buffer");
    return JAMD_EINVAL;
  }
  return lv_host_call(l, samples, sample_off, final, true, O, out, frame_off);
}

int jamd_frontend_live_commit(jamd_frontend_live *l, const unsigned char *update, void *stream) {
  if (!l) { jamd_set_error("jamd_frontend_live_commit: NULL object"); return JAMD_EINVAL; }
  const LvParams &p = l->p;
  for (int c = 0; c < l->nchan && l->nopen; c++)
    if (l->open[c] && (!update || update[c])) {
      jamd_set_error("jamd_frontend_live_commit: channel %d has an open segment (end it with a final push first)", c);
      return JAMD_ESTATE;
    }
  if (!p.mean && !p.var) return JAMD_OK;     // no CMNWork in the reference either
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  hipStream_t st = jamd_stream(l->in.eng, stream);
  // (a copy from pageable memory has left the host array when the call returns)
  if (update) JAMD_HIP(hipMemcpyAsync(l->d_upd, update, (size_t)l->nchan, hipMemcpyHostToDevice, st));
  const unsigned char *m = update ? l->d_upd : nullptr;
  hipLaunchKernelGGL(lv_commit_kernel, dim3((p.nchan * p.veclen + 63) / 64), dim3(64), 0, st, p, l->s, m);
  JAMD_HIP(hipGetLastError());
  hipLaunchKernelGGL(lv_commit_scalars, dim3((p.nchan + 63) / 64), dim3(64), 0, st, p, l->s, m);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int jamd_frontend_cmn_read(const char *path, int veclen, int mfcc_dim, int want_var, float *cmean, float *cvar) {
  if (!path || !cmean || (want_var && !cvar)) { jamd_set_error("jamd_frontend_cmn_read: NULL argument"); return JAMD_EINVAL; }
  std::string err;
  const int r = cmnf_read(path, veclen, mfcc_dim, want_var != 0, cmean, cvar, err);
  if (r < 0) { jamd_set_error("jamd_frontend_cmn_read: %s: %s", path, err.c_str()); return JAMD_EINVAL; }
  return r;
}

int jamd_frontend_cmn_write(const char *path, int veclen, const float *cmean, const float *cvar) {
  if (!path || !cmean || veclen < 1) { jamd_set_error("jamd_frontend_cmn_write: NULL argument or veclen < 1"); return JAMD_EINVAL; }
  std::string err;
  if (cmnf_write(path, veclen, cmean, cvar, err) != 0) { jamd_set_error("jamd_frontend_cmn_write: %s", err.c_str()); return JAMD_EINVAL; }
  return JAMD_OK;
}

}  // extern "C"
