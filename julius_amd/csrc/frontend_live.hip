// frontend_live.hip -- the live-input front end on gfx950: whole segments of many independent channels per call.
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
//   lv_feat_kernel     one lane per (frame, element): normalised energy, delta, acceleration -> feat[Nf][veclen]
//   lv_emax_kernel     one workgroup per channel: the channel's new energy maximum, max(0, max_t f) (order-free)
//   lv_cmn_kernel      one lane per (channel, element): the float chains of CMN_realtime() over t; normalises, splices
//                      and stores the rows; leaves now.mfcc_sum / now.mfcc_var / now.framenum in the channel's state
//   lv_copy_kernel     one lane per output element: splicing alone, for kinds without _Z and without cvn
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
constexpr int kActive = 1, kReest = 2;       // per-call channel bits: has samples; the variance is re-estimated

struct LvParams {
  int nchan, veclen, baselen, nb, splice, delta, acc, delWin, accWin, Bd, Ba, enorm, mean, var, mfcc_dim, do_map;
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
};

__device__ __forceinline__ int lv_find(const int *off, int n, int g) {   // the last u with off[u] <= g
  int lo = 0, hi = n;
  while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}

// tmpmfcc[n] of base frame g after energy_max_normalize() (wav2mfcc-pipe.c:740-746)
__device__ __forceinline__ float lv_base(const LvParams &p, const float *stat, float max_last, float min_last, int g, int n) {
  float f = stat[(size_t)g * p.baselen + n];
  if (p.enorm && n == p.baselen - 1) {
    if (f < min_last) f = min_last;
    f = (float)(1.0 - (max_last - f) * p.escale);
  }
  return f;
}

// WMP_deltabuf_calc() (:122-153) of the delta buffer at frame t of a segment of T frames starting at base frame g0
__device__ __forceinline__ float lv_delta(const LvParams &p, const float *stat, float max_last, float min_last, int g0,
                                          int T, int t, int n) {
  float sum = 0.0f;
  for (int theta = 1; theta <= p.delWin; theta++) {
    const float A1 = lv_base(p, stat, max_last, min_last, g0 + (t - theta < 0 ? 0 : t - theta), n);
    const float A2 = lv_base(p, stat, max_last, min_last, g0 + (t + theta >= T ? T - 1 : t + theta), n);
    sum += theta * (A2 - A1);
  }
  return sum / p.Bd;
}

__global__ void __launch_bounds__(256)
lv_feat_kernel(LvParams p, const float *__restrict__ stat, const int *__restrict__ boff, const int *__restrict__ noff,
               const float *__restrict__ emax, int Ntot, float *__restrict__ feat) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Ntot * p.veclen) return;
  const int g = (int)(idx / p.veclen), e = (int)(idx % p.veclen);
  const int c = lv_find(noff, p.nchan, g);
  const int t = g - noff[c], g0 = boff[c], T = boff[c + 1] - g0;   // (a channel with frames here has Nf == Tb)
  float max_last = 0.0f, min_last = 0.0f;
  if (p.enorm) {                              // energy_max_prepare()
    max_last = emax[c];
    min_last = (float)(max_last - (p.silFloor * LV_LOG_TEN) / 10.0);
  }
  float v;
  if (e < p.nb) v = lv_base(p, stat, max_last, min_last, g0 + t, e);
  else if (e < p.nb + p.baselen) v = lv_delta(p, stat, max_last, min_last, g0, T, t, e - p.nb);
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
        A1 = lv_base(p, stat, max_last, min_last, g0 + t1, n);
        A2 = lv_base(p, stat, max_last, min_last, g0 + t2, n);
      } else {
        A1 = lv_delta(p, stat, max_last, min_last, g0, T, t1, n);
        A2 = lv_delta(p, stat, max_last, min_last, g0, T, t2, n);
      }
      sum += theta * (A2 - A1);
    }
    v = sum / p.Ba;
  }
  feat[idx] = v;
}

// energy_max_prepare() sets max to 0.0 and energy_max_normalize() raises it over every base frame, also of a segment
// too short to emit anything.  Launched behind lv_feat_kernel, which reads the previous maximum.
__global__ void __launch_bounds__(256)
lv_emax_kernel(LvParams p, const float *__restrict__ stat, const int *__restrict__ boff, const int *__restrict__ act,
               float *__restrict__ emax) {
  __shared__ float red[256];
  const int c = blockIdx.x;
  if (!(act[c] & kActive)) return;
  float m = 0.0f;
  for (int t = boff[c] + threadIdx.x; t < boff[c + 1]; t += 256) m = fmaxf(m, stat[(size_t)t * p.baselen + p.baselen - 1]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) emax[c] = red[0];
}

// CMN_realtime() (:342-399) over the Nf frames of the channel, after CMN_realtime_prepare(); consecutive lanes take
// consecutive elements of one frame.  Frame t lands in row t - i at block i of every row it is part of (splice_mfcc()).
// With splice 1 and every frame stored, CMN_realtime_update() would recompute now.mfcc_var from the stored (normalised)
// vectors against the un-normalised mean (:418-434): that is done here, while the rows are at hand.
__global__ void __launch_bounds__(64)
lv_cmn_kernel(LvParams p, LvState s, const float *__restrict__ feat, const int *__restrict__ noff,
              const int *__restrict__ ooff, const int *__restrict__ act, float *__restrict__ out) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= p.nchan * p.veclen) return;
  const int c = idx / p.veclen, d = idx % p.veclen;
  if (!(act[c] & kActive)) return;
  const int n0 = noff[c], N = noff[c + 1] - n0, o0 = ooff[c], To = ooff[c + 1] - o0;
  const int VL = p.veclen * p.splice;
  const float *col = feat + (size_t)n0 * p.veclen + d;
  const bool set = (s.flags[c] & kSet) != 0;
  const float cinit = s.cmean[idx];
  const double sd = (set && p.var) ? sqrt((double)s.cvar[idx]) : 1.0;
  float sum = 0.0f, var = 0.0f;
  for (int t = 0; t < N; t++) {
    float m = col[(size_t)t * p.veclen];
    sum += m;
    double x;
    if (set) {
      if (p.do_map) {
        x = sum + p.cweight * cinit;
        const double y = (double)(t + 1) + p.cweight;
        x /= y;
      } else {
        x = cinit;
      }
    } else {
      x = sum / (t + 1);
    }
    if (p.var) var += (m - x) * (m - x);
    if (p.mean && d < p.mfcc_dim) m -= x;
    if (p.var && set) m /= sd;
    for (int i = 0; i < p.splice; i++) {
      const int o = t - i;
      if (o >= 0 && o < To) out[(size_t)(o0 + o) * VL + i * p.veclen + d] = m;
    }
  }
  if (p.var && (act[c] & kReest)) {
    const float mean = sum / (float)N;
    float x = 0.0f;
    for (int t = 0; t < N; t++) {
      const float v = out[(size_t)(o0 + t) * VL + d];
      x += (v - mean) * (v - mean);
    }
    var = x;
  }
  s.now_sum[idx] = sum;
  s.now_var[idx] = var;
  if (d == 0) s.now_fn[c] = N;
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
};

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
  delete l;
}

int jamd_frontend_live_state_set(jamd_frontend_live *l, int chan, const float *cmean, const float *cvar) {
  if (!l || !cmean || chan < 0 || chan >= l->nchan) {
    jamd_set_error("jamd_frontend_live_state_set: NULL argument or channel out of range");
    return JAMD_EINVAL;
  }
  if (l->p.var && !cvar) { jamd_set_error("jamd_frontend_live_state_set: the kind has cvn: a variance is needed"); return JAMD_EINVAL; }
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
  hipError_t e = hipSetDevice(in.eng->device);
  const size_t C = nchan, V = d.veclen, CV = C * V;
  // floats: emax | cmean | cvar | now_sum | now_var | all_var | ring_sum ; ints: flags now_fn all_fn head cnum cmax | ring_fn
  const size_t nfl = C + 5 * CV + CV * kRing, nin = 6 * C + C * kRing;
  if (e == hipSuccess) e = hipMalloc(&l->state, nfl * sizeof(float) + nin * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void **)&l->d_upd, C);
  if (e == hipSuccess) e = hipMemset(l->state, 0, nfl * sizeof(float) + nin * sizeof(int));
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
  int *r = (int *)q;
  s.flags = r; r += C; s.now_fn = r; r += C; s.all_fn = r; r += C; s.head = r; r += C; s.cnum = r; r += C; s.cmax = r; r += C;
  s.ring_fn = r;
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

int jamd_frontend_live_run_dev(jamd_frontend_live *l, const int16_t *dev_samples, const int64_t *sample_off,
                               float *dev_out, int *frame_off, void *stream) {
  if (!l || !dev_samples || !sample_off || !dev_out) { jamd_set_error("jamd_frontend_live_run_dev: NULL argument"); return JAMD_EINVAL; }
  FeInfo in;
  fe_info(l->f, &in);
  if (in.ss_mode == JAMD_SS_CALC) {
    jamd_set_error("jamd_frontend_live_run_dev: JAMD_SS_CALC is set on the parent front end: a live segment has no "
                   "head known in advance (use JAMD_SS_LOAD or JAMD_SS_OFF)");
    return JAMD_EINVAL;
  }
  const jamd_frontend_desc &d = l->in.d;
  const int nchan = l->nchan;
  std::vector<int> boff(nchan + 1), noff(nchan + 1), ooff(nchan + 1), act(nchan + 1, 0);
  long long B = 0, N = 0, O = 0;
  for (int c = 0; c < nchan; c++) {
    if (sample_off[c] < 0 || sample_off[c + 1] < sample_off[c]) {
      jamd_set_error("jamd_frontend_live_run_dev: sample_off is not non-decreasing from 0 at channel %d", c);
      return JAMD_EINVAL;
    }
    const long long n = sample_off[c + 1] - sample_off[c];
    const LvCounts k = lv_counts(d, n);
    boff[c] = (int)B; noff[c] = (int)N; ooff[c] = (int)O;
    act[c] = (n > 0 ? kActive : 0) | (k.reest ? kReest : 0);
    B += k.Tb; N += k.Nf; O += k.To;
    if ((B + 1) * (long long)d.vecbuflen * d.splice > 0x7fffffffLL) {
      jamd_set_error("jamd_frontend_live_run_dev: batch too large (%lld frames)", B);
      return JAMD_EINVAL;
    }
  }
  boff[nchan] = (int)B; noff[nchan] = (int)N; ooff[nchan] = (int)O;
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  hipStream_t st = jamd_stream(l->in.eng, stream);
  int rc;
  if ((rc = jamd_grow(&l->d_feat, &l->feat_cap, (size_t)(N > 0 ? N : 1) * d.veclen * sizeof(float))) != JAMD_OK) return rc;
  const float *d_stat; const int *d_tabs;
  if ((rc = fe_base_frames(l->f, st, dev_samples, sample_off, nchan, {&boff, &noff, &ooff, &act}, &d_stat, &d_tabs)) != JAMD_OK)
    return rc;
  const int *d_boff = d_tabs, *d_noff = d_boff + nchan + 1, *d_ooff = d_noff + nchan + 1, *d_act = d_ooff + nchan + 1;
  const LvParams &p = l->p;
  const long long nfeat = N * d.veclen;
  if (nfeat > 0) {
    hipLaunchKernelGGL(lv_feat_kernel, dim3((unsigned)((nfeat + 255) / 256)), dim3(256), 0, st, p, d_stat, d_boff, d_noff,
                       l->s.emax, (int)N, l->d_feat);
    JAMD_HIP(hipGetLastError());
  }
  if (p.enorm) {
    hipLaunchKernelGGL(lv_emax_kernel, dim3(nchan), dim3(256), 0, st, p, d_stat, d_boff, d_act, l->s.emax);
    JAMD_HIP(hipGetLastError());
  }
  if (p.mean || p.var) {
    hipLaunchKernelGGL(lv_cmn_kernel, dim3((nchan * d.veclen + 63) / 64), dim3(64), 0, st, p, l->s, l->d_feat, d_noff,
                       d_ooff, d_act, dev_out);
    JAMD_HIP(hipGetLastError());
  } else if (O > 0) {
    const long long nout = O * d.veclen * d.splice;
    hipLaunchKernelGGL(lv_copy_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, p, l->d_feat, d_noff, d_ooff,
                       (int)O, dev_out);
    JAMD_HIP(hipGetLastError());
  }
  if (frame_off) memcpy(frame_off, ooff.data(), sizeof(int) * (nchan + 1));
  return JAMD_OK;
}

int jamd_frontend_live_run_host(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off, float *out,
                                int *frame_off) {
  if (!l || !samples || !sample_off || !out) { jamd_set_error("jamd_frontend_live_run_host: NULL argument"); return JAMD_EINVAL; }
  const int nchan = l->nchan;
  long long O = 0;
  for (int c = 0; c < nchan; c++) {
    if (sample_off[c] < 0 || sample_off[c + 1] < sample_off[c]) {
      jamd_set_error("jamd_frontend_live_run_host: sample_off is not non-decreasing from 0 at channel %d", c);
      return JAMD_EINVAL;
    }
    O += lv_counts(l->in.d, sample_off[c + 1] - sample_off[c]).To;
  }
  JAMD_HIP(hipSetDevice(l->in.eng->device));
  int rc;
  const size_t ns = (size_t)sample_off[nchan], no = (size_t)O * l->in.d.veclen * l->in.d.splice;
  if ((rc = jamd_grow(&l->d_in, &l->in_cap, (ns > 0 ? ns : 1) * sizeof(int16_t))) != JAMD_OK) return rc;
  if ((rc = jamd_grow(&l->d_out, &l->out_cap, (no > 0 ? no : 1) * sizeof(float))) != JAMD_OK) return rc;
  hipStream_t st = l->in.eng->stream;
  if (ns) JAMD_HIP(hipMemcpyAsync(l->d_in, samples, ns * sizeof(int16_t), hipMemcpyHostToDevice, st));
  if ((rc = jamd_frontend_live_run_dev(l, l->d_in, sample_off, l->d_out, frame_off, st)) != JAMD_OK) return rc;
  if (no) JAMD_HIP(hipMemcpyAsync(out, l->d_out, no * sizeof(float), hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  return JAMD_OK;
}

int jamd_frontend_live_commit(jamd_frontend_live *l, const unsigned char *update, void *stream) {
  if (!l) { jamd_set_error("jamd_frontend_live_commit: NULL object"); return JAMD_EINVAL; }
  const LvParams &p = l->p;
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
