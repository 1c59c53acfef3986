// gmm_dev.h -- device helpers of the Gaussian kernels (gmm_outprob.hip, gmm_pruned.hip, rejgmm.hip), each next to
// the host-side twin that picks its template argument or its grid.  What the other scoring kernels and the first pass
// share as well (addlog_step, finish_state, cd_reduce, wave_sync) is in jamd_device.h.  Internal, not installed.
#pragma once
#include <type_traits>

#include "jamd_device.h"

typedef float f2 __attribute__((ext_vector_type(2)));

namespace jamd {

// XCD-aware block decode: the dispatcher places block b on XCD b % 8 (MI355X_MICROARCH.md "Workgroup dispatch").
// With nstb = 8 k + r state ranges:
//   * the first 8 k ranges (the full rounds) are pinned to one XCD each -- all frame-blocks of a range are given the
//     same b % 8, frame block fastest -- so the range's records stay in that XCD's L2;
//   * the r leftover ranges hold L = r * nfb blocks, and those are dealt over ALL eight XCDs in equal shares: XCD x takes
//     the contiguous run m = x * per .. x * per + per - 1 (per = ceil(L / 8)) of the leftover blocks counted range by
//     range, frame block fastest.  per <= nfb, so a run touches at most two ranges: an XCD's L2 takes in the records
//     of at most two leftover ranges (a range's records land in about 8 / r + 1 L2s instead of one -- 82 KB each at
//     M = 16, D = 39).  Pinned like the full rounds, r of the XCDs would carry nfb blocks more than the others and
//     the launch would end with 8 - r XCDs idle for a whole block's time ("launch shape").  The price
//     is paid where the whole launch is one round and per is 1 or 2: nothing to save there, and a block that reads
//     its range alone in its XCD is slower than two that share it (a 1 000-frame call + 1 %).
// The grid is 8 k nfb + 8 per blocks (the first term a multiple of 8, so a leftover block's b % 8 is its share's
// number); the at most 7 blocks with m >= L are empty.
__device__ __forceinline__ bool decode_block(int nfb, int nstb, int &fb, int &sb) {
  const int b = blockIdx.x;
  const int x = b & 7;
  const int kfull = nstb & ~7, full = kfull * nfb;      // ranges and blocks of the full rounds
  const bool tail = b >= full;
  const int L = (nstb - kfull) * nfb, per = (L + 7) >> 3;
  const int n = tail ? x * per + ((b - full) >> 3) : b >> 3;
  if (tail && n >= L) return false;
  const int d = n / nfb;
  sb = tail ? kfull + d : x + 8 * d;
  fb = n - d * nfb;
  return true;
}
// ... and the grid it decodes: nfb frame-blocks for each of nstb ranges, the leftover blocks rounded up to a multiple of 8
static inline int xcd_grid(int nstb, int nfb) {
  const int kfull = nstb & ~7;
  return kfull * nfb + 8 * (((nstb - kfull) * nfb + 7) / 8);
}

// The vector lengths the kernels are compiled for: f(std::integral_constant<int, DT>) with DT = D for those, DT = 0
// (run-time dimension, frames in LDS) for every other.
template <typename F>
static inline int dispatch_veclen(int D, F &&f) {
  switch (D) {
    case 39: return f(std::integral_constant<int, 39>{});
    case 38: return f(std::integral_constant<int, 38>{});
    case 26: return f(std::integral_constant<int, 26>{});
    case 25: return f(std::integral_constant<int, 25>{});
    default: return f(std::integral_constant<int, 0>{});
  }
}

// Load the wave's 128 frames t0 .. t0 + 127 (clamped to T - 1): registers (DT>0) or LDS transposed
// [d][128 frames of the wave] (DT==0, conflict-free ds_read_b32).
template <int DT>
__device__ __forceinline__ void load_frames(f2 *v, float *vt, const float *frames,
                                            int t0, int T, int D, int lane) {
  int ta = t0 + lane, tb = ta + 64;
  if (ta > T - 1) ta = T - 1;
  if (tb > T - 1) tb = T - 1;
  const float *fa = frames + (size_t)ta * D, *fb = frames + (size_t)tb * D;
  if constexpr (DT > 0) {
#pragma unroll
    for (int d = 0; d < DT; d++) { v[d].x = fa[d]; v[d].y = fb[d]; }
  } else {
    for (int d = 0; d < D; d++) { vt[d * 128 + lane] = fa[d]; vt[d * 128 + 64 + lane] = fb[d]; }
    wave_sync();
  }
}

// compute_g_base() (gprune_none.c:59-82) for a packed pair of frames held in
// registers (DT > 0, compile-time dimension) or in LDS, transposed
// [d][128 frames of the wave] (DT == 0, run-time dimension D).
// r -> record [mean(D) ivar(D) gconst ...]; returns the two tmp*-0.5 scores,
// LOG_ZERO for a NULL density (gconst stored as NaN).
template <int DT>
__device__ __forceinline__ f2 gauss_pair(const f2 *v, const float *vt, int lane, int D,
                                         const float *__restrict__ r) {
  const float gc = r[2 * D];
  f2 acc = {gc, gc};
  if constexpr (DT > 0) {
#pragma unroll
    for (int d = 0; d < DT; d++) {
      const float mu = r[d], iv = r[DT + d];
      f2 x = v[d] - f2{mu, mu};
      x = x * x;
      x = x * f2{iv, iv};
      acc = acc + x;
    }
  } else {
    for (int d = 0; d < D; d++) {
      const float mu = r[d], iv = r[D + d];
      f2 x = f2{vt[d * 128 + lane], vt[d * 128 + 64 + lane]} - f2{mu, mu};
      x = x * x;
      x = x * f2{iv, iv};
      acc = acc + x;
    }
  }
  f2 sc = {acc.x * -0.5f, acc.y * -0.5f};
  if (gc != gc) sc = f2{JAMD_LOG_ZERO, JAMD_LOG_ZERO};
  return sc;
}

// The output-tile epilogue: results of up to NS columns (states, mixture entries) x ROWS frames of one wave are staged
// in a wave-private LDS tile [ROWS][NS + 1] and written as 64-byte row segments (a lane storing its own [t][s]
// element makes 64 scattered 4-byte stores per instruction).  Rows t0 .. of out[][stride], columns c0 .. c0 + nc - 1.
template <int NS, int ROWS>
__device__ __forceinline__ void store_tile(const float (*tile)[NS + 1], float *out, int t0, int T,
                                           int stride, int c0, int nc, int lane) {
  wave_sync();                     // the tile's writes, visible to the other lanes
  constexpr int RPI = 64 / NS;     // rows per store instruction
  const int col = lane % NS, rsub = lane / NS;
#pragma unroll 4
  for (int it = 0; it < ROWS / RPI; it++) {
    const int rr = it * RPI + rsub;
    const int t = t0 + rr;
    if (t < T && col < nc) out[(size_t)t * stride + c0 + col] = tile[rr][col];
  }
  wave_release();                  // read out before the next group of columns overwrites it
}

// cache_push() (gprune_common.c:88-126): keep the best `cap` (score,id) pairs
// in descending order in a register-resident list of NMAX slots.
//   bottom case (sc[len-1] >= score): append if there is room, else drop;
//   otherwise insert before the first element that is not greater.
template <int NMAX>
__device__ __forceinline__ void topn_push(float (&sc)[NMAX], int (&id)[NMAX], int &len, int cap,
                                          float score, int gid) {
  int p;
  float last = score;             // value of sc[len-1] (register array: no dynamic indexing)
#pragma unroll
  for (int i = 0; i < NMAX; i++) if (i == len - 1) last = sc[i];
  if (len > 0 && last >= score) {
    p = len;                      // bottom
  } else {
    p = 0;
#pragma unroll
    for (int i = 0; i < NMAX; i++) p += (i < len && sc[i] > score) ? 1 : 0;
  }
  if (p >= cap) return;
#pragma unroll
  for (int i = NMAX - 1; i >= 1; i--) {
    if (i > p && i < cap) { sc[i] = sc[i - 1]; id[i] = id[i - 1]; }
  }
#pragma unroll
  for (int i = 0; i < NMAX; i++) {
    if (i == p) { sc[i] = score; id[i] = gid; }
  }
  if (len < cap) len++;
}

// gprune_safe() without history (gprune_safe.c:185-196; the same loop closes gprune_heu() and gprune_beam()): while the
// list fills, a Gaussian is scored by compute_g_base(); once it is full, by compute_g_safe() (:76-97), which answers
// LOG_ZERO for a Gaussian whose score lies below the list's last entry (its partial sums only grow, so the final sum
// decides), and the caller drops what is not above that entry.  Normally that is the same as pushing the full score.
// Not for a frame so far from every Gaussian that the kept scores lie below LOG_ZERO itself: there the LOG_ZERO the
// reference got back IS above the last entry and enters the list as the Gaussian's score.
template <int NMAX>
__device__ __forceinline__ void topn_push_safe(float (&sc)[NMAX], int (&id)[NMAX], int &len, int cap,
                                               float score, int gid) {
  float last = score;             // value of sc[cap-1]
#pragma unroll
  for (int i = 0; i < NMAX; i++) if (i == cap - 1) last = sc[i];
  if (len == cap && score < last) score = JAMD_LOG_ZERO;
  topn_push<NMAX>(sc, id, len, cap, score, gid);
}

// Does the visiting order show in a list this score is pushed into?  It does where the score equals a kept one (which
// of two equal Gaussians survives, and where it sits, follows the order) and where compute_g_safe()'s LOG_ZERO can enter
// (above): some score at or below LOG_ZERO.  Without either the list is the N best scores whatever the order.
template <int NMAX>
__device__ __forceinline__ bool topn_order_shows(const float (&sc)[NMAX], int len, float score) {
  bool shows = !(score > JAMD_LOG_ZERO);
#pragma unroll
  for (int i = 0; i < NMAX; i++) shows |= (i < len && sc[i] == score);
  return shows;
}

// ... and the NMAX a list of `cap` entries is instantiated with: cap rounded up to LO, .., 16, 32, 64 (LO = 2 or 4).
template <int LO, typename F>
static inline int dispatch_topn(int cap, F &&f) {
  if constexpr (LO <= 2) if (cap <= 2) return f(std::integral_constant<int, 2>{});
  if (cap <= 4) return f(std::integral_constant<int, 4>{});
  if (cap <= 8) return f(std::integral_constant<int, 8>{});
  if (cap <= 16) return f(std::integral_constant<int, 16>{});
  if (cap <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

// The same list held by a WAVE, for the kernels in which one wave walks a codebook's frames in order (the history
// forms of gmm_pruned.hip, the order pass of gmm_ms_tied.hip).
struct TopList {                 // lane p holds entry p of the descending list (cap <= 64)
  float sc; int id; int len, cap;
  __device__ __forceinline__ void push(float score, int gid, int lane) {      // cache_push(), gprune_common.c:88-126
    const float last = __shfl(sc, len > 0 ? len - 1 : 0, 64);
    if (len > 0 && last >= score) {                                            // bottom: append if there is room
      if (len < cap) { if (lane == len) { sc = score; id = gid; } len++; }
      return;
    }
    const int p = __popcll(__ballot(lane < len && sc > score));                // entries strictly greater stay in front
    const float usc = __shfl_up(sc, 1, 64); const int uid = __shfl_up(id, 1, 64);
    if (lane > p && lane <= len && lane < cap) { sc = usc; id = uid; }
    if (lane == p) { sc = score; id = gid; }
    if (len < cap) len++;
  }
  // the branch without history: compute_g_safe()'s LOG_ZERO for a Gaussian below a full list's last entry (topn_push_safe())
  __device__ __forceinline__ void push_safe(float score, int gid, int lane) {
    if (len == cap && score < __shfl(sc, cap - 1, 64)) score = JAMD_LOG_ZERO;
    push(score, gid, lane);
  }
};

}  // namespace jamd
