// adin_cut.hip -- the kernels of the silence cutting stage (jamd_adin_cut) and their launchers (adin_cut_host.h): the
// rest of adin_cut() (libjulius/src/adin-cut.c:600-984) around count_zc_e() (libsent/src/adin/zc-e.c), bit-identical.
// Integer only, no atomics.
//
// count_zc_e() is a recurrence over samples with four states (is_trig x sign): a sample maps each state to a next
// state, and those maps compose associatively, so they are scanned -- across a wave with __shfl_up, across waves
// through LDS, across the 1024-sample steps of a channel's workgroup by the carried state.  With the state that enters
// each sample known, its crossing flag is; a prefix sum turns the flags into the running count C[q] (crossings among
// stream samples 0 ... q, modulo 2^32), and the count count_zc_e() returns at a block that ends behind sample e - 1 is
// C[e - 1] - C[e - 1 - c_length]: the old flag of a slot leaves before the new one enters.  The recurrence does not
// look at block boundaries, so it runs over every new sample at once, the ones included that wait for their block.
//
// The blocks themselves are few (one per chunk_size samples) and strictly in order: one lane per channel walks them.
// Everything the reference delivers is a contiguous range of the stream -- the head margin [e - valid_len, e - w), the
// swap buffer [e - w - sblen, e - w), the block [e - w, e) -- and within a segment the ranges follow each other without
// a gap (the swap buffer holds exactly what the tail left out), so a channel's part is one range [a, a + len).  The
// gather copies it out of [history | new samples]; the history is a ring by stream index, as is the count's.
#include "adin_cut_host.h"

constexpr int kThreads = 256;
constexpr unsigned kMapId = 0xE4;            // state s -> s, two bits each

// One sample of count_zc_e() on state s = is_trig * 2 + (sign == ZC_NEGATIVE).  abs() in int: -32768 counts as 32768.
__device__ __forceinline__ int ac_step(int s, int v, int trigger, int *cross) {
  int trig = s >> 1, neg = s & 1;
  const int x = trig && (neg ? v > 0 : v < 0);
  if (x) { trig = 0; neg ^= 1; }
  if ((v < 0 ? -v : v) > trigger) trig = 1;
  *cross = x;
  return trig * 2 + neg;
}

__device__ __forceinline__ unsigned ac_map(int v, int trigger) {
  unsigned m = 0;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    int x;
    m |= (unsigned)ac_step(s, v, trigger, &x) << (2 * s);
  }
  return m;
}

// first f, then g
__device__ __forceinline__ unsigned ac_then(unsigned f, unsigned g) {
  unsigned h = 0;
#pragma unroll
  for (int s = 0; s < 4; s++) h |= ((g >> (2 * ((f >> (2 * s)) & 3))) & 3) << (2 * s);
  return h;
}

__device__ __forceinline__ int ac_apply(unsigned f, int s) { return (f >> (2 * s)) & 3; }

// One workgroup per channel, over its new samples in steps of 1024, four consecutive samples per lane.
__global__ __launch_bounds__(kThreads) void ac_scan_kernel(const AcChanTab *__restrict__ tab, const int16_t *__restrict__ src,
                                                           const AcState *__restrict__ state, int trigger,
                                                           unsigned *__restrict__ cnt, int *__restrict__ strig,
                                                           unsigned *__restrict__ scum) {
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const AcChanTab t = tab[c];
  int carry = state[c].trig;
  unsigned cum = state[c].cum;
  __shared__ unsigned wmap[kThreads / 64];
  __shared__ int wsum[kThreads / 64];
  const int16_t *in = src + t.src_off;
  unsigned *out = cnt + t.cnt_off;
  for (int base = 0; base < t.n; base += kAcTile) {
    int v[4];
    unsigned mine = kMapId;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = base + 4 * tid + q;
      v[q] = i < t.n ? in[i] : 0;
      if (i < t.n) mine = ac_then(mine, ac_map(v[q], trigger));
    }
    unsigned inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(inc, d, 64);
      if (lane >= d) inc = ac_then(o, inc);
    }
    if (lane == 63) wmap[w] = inc;
    unsigned before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = kMapId;
    __syncthreads();
    unsigned pre = kMapId, all = kMapId;
#pragma unroll
    for (int k = 0; k < kThreads / 64; k++) {
      if (k < w) pre = ac_then(pre, wmap[k]);
      all = ac_then(all, wmap[k]);
    }
    int s = ac_apply(ac_then(pre, before), carry);
    carry = ac_apply(all, carry);
    unsigned flags = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (base + 4 * tid + q < t.n) {
        int x;
        s = ac_step(s, v[q], trigger, &x);
        flags |= (unsigned)x << q;
      }
    const int nk = __popc(flags);
    int sum = nk;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(sum, d, 64);
      if (lane >= d) sum += o;
    }
    if (lane == 63) wsum[w] = sum;
    __syncthreads();
    unsigned run = cum + (unsigned)(sum - nk);
#pragma unroll
    for (int k = 0; k < kThreads / 64; k++) {
      if (k < w) run += (unsigned)wsum[k];
      cum += (unsigned)wsum[k];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = base + 4 * tid + q;
      run += flags >> q & 1;
      if (i < t.n) out[i] = run;
    }
  }
  if (tid == 0) { strig[c] = carry; scum[c] = cum; }
}

struct AcPlanArgs {
  const AcChanTab *tab;
  const AcState *state;
  const unsigned *cnt, *hc;
  const int *strig;
  const unsigned *scum;
  AcState *next;
  long long *pa;
  int *pl, *used;
  AcTabs t;
  int cap;
};

// One lane per channel walks the channel's blocks in order (adin-cut.c:647-984).  GATE: the block triggers only if
// fvad_proceed() says so too (:662-668): of the last N frames processed by the block's end, cmin or more were speech.
template <bool GATE>
__device__ __forceinline__ void ac_blocks(const AcDev &g, const AcPlanArgs &a, const AcGateDev &v) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= g.nchan) return;
  const AcChanTab t = a.tab[c];
  AcState s = a.state[c];
  for (int p = 0; p < a.cap; p++) {
    a.pa[(size_t)p * g.nchan + c] = 0;
    a.pl[(size_t)p * g.nchan + c] = 0;
    a.t.start[(size_t)p * g.nchan + c] = -1;
    a.t.fin[(size_t)p * g.nchan + c] = 0;
  }
  if (t.n == 0 && !t.eos) {                                  // idle
    a.next[c] = s;
    a.used[c] = 0;
    return;
  }
  const long long B = s.pos;
  const unsigned *cnt = a.cnt + t.cnt_off, *hc = a.hc + (size_t)c * g.hist;
  const long long F0 = GATE ? ac_gate_span(s, t, g.chunk, v.fs).F0 : 0;
  auto speech_at = [&](long long k) -> unsigned {            // V[k]
    if (k <= 0) return 0u;
    return k > F0 ? v.vnew[v.voff[c] + (k - F0 - 1)] : v.vh[(size_t)c * v.vhist + k % v.vhist];
  };
  auto count_at = [&](long long q) -> unsigned {             // C[q]
    if (q < 0) return 0u;
    return q >= B ? cnt[q - B] : hc[q % g.hist];
  };
  int part = 0;
  long long ra = -1, rb = -1;                                // what the open part has been handed so far
  auto deliver = [&](long long from, long long to) {
    if (to <= from) return;
    if (ra < 0) ra = from;
    rb = to;
  };
  auto close_part = [&](int fin) {
    if (part < a.cap) {
      a.pa[(size_t)part * g.nchan + c] = ra < 0 ? 0 : ra;
      a.pl[(size_t)part * g.nchan + c] = ra < 0 ? 0 : (int)(rb - ra);
      a.t.fin[(size_t)part * g.nchan + c] = (unsigned char)fin;
    }
    part++;
    ra = rb = -1;
  };
  long long avail = s.carried + (long long)t.n, e = B - s.carried;   // e: the stream index behind the last block
  while (avail > 0) {
    int w = g.chunk;
    if (avail < w) {
      if (!t.eos) break;
      w = (int)avail;                                        // the stream's short last block
    }
    e += w;
    avail -= w;
    const int zc = (int)(count_at(e - 1) - count_at(e - 1 - g.c_length));
    s.zc = zc;
    bool open = true;
    if (GATE) {
      const long long n = fv_gate_frames(e, v.fs);
      open = (int)(speech_at(n) - speech_at(n - v.N)) >= v.cmin;
    }
    if (open && zc > g.noise_zc) {
      if (!s.is_valid) {                                     // trigger: the cycle buffer less this block first
        s.is_valid = 1;
        s.nc = 0;
        const long long valid_len = e < g.c_length ? e : g.c_length;
        if (part < a.cap) a.t.start[(size_t)part * g.nchan + c] = e - valid_len;
        deliver(e - valid_len, e - w);
      } else if (s.nc > 0) {                                 // re-trigger inside the tail: the swap buffer first
        s.nc = 0;
        if (s.sblen > 0) {
          deliver(e - w - s.sblen, e - w);
          s.sblen = 0;
        }
      }
    } else if (s.is_valid) {
      if (s.nc == 0) {
        s.rest_tail = g.sbsize - g.c_length;
        s.sblen = 0;
      }
      s.nc++;
    }
    if (s.is_valid) {
      if (s.nc > 0 && s.rest_tail == 0) {
        s.sblen += w;                                        // behind the tail margin: kept for a re-trigger
      } else {
        if (s.nc > 0) s.rest_tail = s.rest_tail < w ? 0 : s.rest_tail - w;
        deliver(e - w, e);
      }
      if (s.nc >= g.nc_max) {                                // end by silence
        s.is_valid = 0;
        s.sblen = 0;
        close_part(1);
      }
    }
  }
  if (t.eos) {
    if (s.is_valid) close_part(1);
    s = AcState{};                                           // need_init
  } else {
    s.carried = (int)avail;
    s.pos = B + t.n;
    s.trig = a.strig[c];
    s.cum = a.scum[c];
  }
  if (ra >= 0) close_part(0);
  a.next[c] = s;
  a.used[c] = part;
}

// Without the gate: the kernel, its arguments and its registers are what they were before there was one
__global__ __launch_bounds__(64) void ac_blocks_kernel(AcDev g, AcPlanArgs a) { ac_blocks<false>(g, a, AcGateDev{}); }
__global__ __launch_bounds__(64) void ac_blocks_gated_kernel(AcDev g, AcPlanArgs a, AcGateDev v) { ac_blocks<true>(g, a, v); }

// The part count, and per part the offsets of the channels' ranges, part after part.  One workgroup.
__global__ __launch_bounds__(kThreads) void ac_offsets_kernel(const int *__restrict__ used, const int *__restrict__ pl, int nchan,
                                                              int cap, AcTabs t) {
  __shared__ long long sums[kThreads];
  __shared__ int most[kThreads];
  const int tid = threadIdx.x, per = (nchan + kThreads - 1) / kThreads;
  const int lo = tid * per < nchan ? tid * per : nchan, hi = lo + per < nchan ? lo + per : nchan;
  int m = 0;
  for (int c = lo; c < hi; c++) m = used[c] > m ? used[c] : m;
  most[tid] = m;
  __syncthreads();
  for (int i = 0; i < kThreads; i++) m = most[i] > m ? most[i] : m;
  if (tid == 0) t.nparts[0] = m;
  const int rows = m < cap ? m : cap;
  long long base = 0;
  for (int p = 0; p < rows; p++) {
    const int *len = pl + (size_t)p * nchan;
    long long s = 0;
    for (int c = lo; c < hi; c++) s += len[c];
    sums[tid] = s;
    __syncthreads();
    long long run = base, total = 0;
    for (int i = 0; i < kThreads; i++) {
      if (i < tid) run += sums[i];
      total += sums[i];
    }
    long long *off = t.off + (size_t)p * (nchan + 1);
    for (int c = lo; c < hi; c++) { off[c] = run; run += len[c]; }
    base += total;
    if (tid == 0) off[nchan] = base;
    __syncthreads();
  }
}

// grid (tiles, nchan, parts): stream samples [a, a + len) of the channel's part -> dev_out.  Behind the push's first
// sample they come out of the history ring; the rest is one run of the input, copied four bytes a lane where source and
// destination are aligned alike.
__global__ __launch_bounds__(kThreads) void ac_gather_kernel(const AcChanTab *__restrict__ tab, const int16_t *__restrict__ src,
                                                             const AcState *__restrict__ state, const int16_t *__restrict__ hs,
                                                             int hist, int nchan, const long long *__restrict__ pa,
                                                             const int *__restrict__ pl, const long long *__restrict__ poff,
                                                             int16_t *__restrict__ out) {
  const int c = blockIdx.y, p = blockIdx.z, tid = threadIdx.x;
  const int len = pl[(size_t)p * nchan + c];
  const int i0 = blockIdx.x * kAcCopyTile;
  if (i0 >= len) return;
  const int i1 = i0 + kAcCopyTile < len ? i0 + kAcCopyTile : len;
  const long long a = pa[(size_t)p * nchan + c], B = state[c].pos;
  int16_t *dst = out + poff[(size_t)p * (nchan + 1) + c];
  const int16_t *ring = hs + (size_t)c * hist;
  long long firstnew = B - a;                                // the part's first sample out of the input
  const int mid = firstnew <= i0 ? i0 : (firstnew >= i1 ? i1 : (int)firstnew);
  for (int i = i0 + tid; i < mid; i += kThreads) dst[i] = ring[(a + i) % hist];
  const int m = i1 - mid;
  if (m <= 0) return;
  const int16_t *s = src + tab[c].src_off + (a + mid - B);
  int16_t *d = dst + mid;
  if ((((uintptr_t)s ^ (uintptr_t)d) & 2) == 0) {
    const int head = ((uintptr_t)d & 2) ? 1 : 0, pairs = (m - head) / 2;
    if (tid == 0 && head) d[0] = s[0];
    const unsigned *s2 = (const unsigned *)(s + head);
    unsigned *d2 = (unsigned *)(d + head);
    for (int k = tid; k < pairs; k += kThreads) d2[k] = s2[k];
    if (tid == 0 && head + 2 * pairs < m) d[m - 1] = s[m - 1];
  } else {
    for (int i = tid; i < m; i += kThreads) d[i] = s[i];
  }
}

// One workgroup per channel: the newest `hist` samples of the push and their counts enter the rings, then the state the
// blocks kernel left becomes the channel's.
__global__ __launch_bounds__(kThreads) void ac_advance_kernel(const AcChanTab *__restrict__ tab, const int16_t *__restrict__ src,
                                                              const unsigned *__restrict__ cnt, int hist, int16_t *__restrict__ hs,
                                                              unsigned *__restrict__ hc, AcState *__restrict__ state,
                                                              const AcState *__restrict__ next) {
  const int c = blockIdx.x;
  const AcChanTab t = tab[c];
  if (t.n == 0 && !t.eos) return;
  const long long B = state[c].pos;
  const int16_t *in = src + t.src_off;
  const unsigned *cn = cnt + t.cnt_off;
  for (int i = (t.n > hist ? t.n - hist : 0) + threadIdx.x; i < t.n; i += kThreads) {
    const size_t slot = (size_t)c * hist + (B + i) % hist;
    hs[slot] = in[i];
    hc[slot] = cn[i];
  }
  __syncthreads();                                           // (every lane has read state[c].pos)
  if (threadIdx.x == 0) state[c] = next[c];
}

__global__ __launch_bounds__(kThreads) void ac_reset_kernel(const unsigned char *__restrict__ mask, int nchan,
                                                            AcState *__restrict__ state) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c < nchan && (!mask || mask[c])) state[c] = AcState{};
}

int ac_launch_plan(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const int16_t *dev_in, AcTabs t, int cap) {
  const unsigned nchan = (unsigned)k->nchan;
  hipLaunchKernelGGL(ac_scan_kernel, dim3(nchan), dim3(kThreads), 0, st, d_tab, dev_in, k->d_state, k->g.trigger, k->d_cnt,
                     k->d_strig, k->d_scum);
  JAMD_HIP(hipGetLastError());
  AcPlanArgs a{d_tab, k->d_state, k->d_cnt, k->d_hc, k->d_strig, k->d_scum, k->d_next, k->d_pa, k->d_pl, k->d_used, t, cap};
  if (k->gate) {
    const FvGate &q = *k->gate;
    const AcGateDev v{q.d_vnew, q.d_vh, (const long long *)q.vtab.d.p, q.fs, q.N, q.cmin, q.vhist};
    hipLaunchKernelGGL(ac_blocks_gated_kernel, dim3((nchan + 63) / 64), dim3(64), 0, st, k->g, a, v);
  } else {
    hipLaunchKernelGGL(ac_blocks_kernel, dim3((nchan + 63) / 64), dim3(64), 0, st, k->g, a);
  }
  JAMD_HIP(hipGetLastError());
  hipLaunchKernelGGL(ac_offsets_kernel, dim3(1), dim3(kThreads), 0, st, k->d_used, k->d_pl, k->nchan, cap, t);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int ac_launch_gather(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const int16_t *dev_in, AcTabs t, int cap,
                     int nparts, int max_len, int16_t *dev_out) {
  (void)cap;
  const dim3 grid((unsigned)((max_len + kAcCopyTile - 1) / kAcCopyTile), (unsigned)k->nchan, (unsigned)nparts);
  hipLaunchKernelGGL(ac_gather_kernel, grid, dim3(kThreads), 0, st, d_tab, dev_in, k->d_state, k->d_hs, k->g.hist, k->nchan,
                     k->d_pa, k->d_pl, t.off, dev_out);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int ac_launch_advance(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const int16_t *dev_in) {
  hipLaunchKernelGGL(ac_advance_kernel, dim3((unsigned)k->nchan), dim3(kThreads), 0, st, d_tab, dev_in, k->d_cnt, k->g.hist,
                     k->d_hs, k->d_hc, k->d_state, k->d_next);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int ac_launch_reset(jamd_adin_cut *k, hipStream_t st, const unsigned char *d_mask) {
  hipLaunchKernelGGL(ac_reset_kernel, dim3((unsigned)((k->nchan + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_mask,
                     k->nchan, k->d_state);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}
