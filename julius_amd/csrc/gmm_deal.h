// gmm_deal.h -- the deal of K1's PULL form (gmm_tile_ring_kernel<.., PULL = true>, gmm_outprob.hip): which tile a
// ticket names.  A tile is one state range of 16 states x one group of 128 frames (one wave's work); a launch holds
// nstb ranges x nfw groups.  The tiles are dealt into eight SHARES, one per XCD (a wave starts on share blockIdx.x & 7,
// the XCD the dispatcher placed its block on, and moves on to the next share when its own is exhausted), and every
// share is an ordered list of tickets 0 .. len - 1 that the waves draw from a counter.  With nstb = k8 + r, k8 a
// multiple of 8, the same deal as decode_block() (gmm_dev.h) at wave granularity:
//   * full rounds: share x holds the ranges x, x + 8, .. below k8, all groups of a range in a row (group fastest) --
//     a range's records stay in one XCD's L2 and a wave that draws two tickets in a row mostly keeps its range;
//   * leftover: the L = r * nfw tiles of the last r ranges, counted range by range with group fastest, are cut into
//     eight contiguous runs of per = ceil(L / 8); share x appends run x (the last runs may be short or empty).
// Plain C++, no HIP header: tests/gmm_deal_check.cpp compiles it alone, under the host sanitizers.
#pragma once

#if defined(__HIPCC__)
#define GD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GD_HD inline
#endif

constexpr int kGdShares = 8;          // XCDs of the device: ticket heads, shares
constexpr int kGdHeadStride = 32;     // ints between two ticket heads: each on its own 128-byte line

struct GmmDeal {
  int nfw;      // frame groups (of 128 frames) of the launch
  int k8;       // state ranges of the full rounds
  int full;     // tickets of the full rounds in every share: (k8 / 8) * nfw
  int L, per;   // leftover tiles, and the run of them one share holds
};

GD_HD GmmDeal gd_make(int nstb, int nfw) {
  GmmDeal d;
  d.nfw = nfw;
  d.k8 = nstb & ~7;
  d.full = (d.k8 >> 3) * nfw;
  d.L = (nstb - d.k8) * nfw;
  d.per = (d.L + 7) >> 3;
  return d;
}

// tickets of share x
GD_HD int gd_len(const GmmDeal &d, int x) {
  int left = d.L - x * d.per;
  if (left < 0) left = 0;
  if (left > d.per) left = d.per;
  return d.full + left;
}

// ticket n of share x -> (state range, frame group); false when the share has no such ticket
GD_HD bool gd_ticket(const GmmDeal &d, int x, int n, int &range, int &group) {
  if (n < 0) return false;
  if (n < d.full) {
    const int q = n / d.nfw;
    range = x + 8 * q;
    group = n - q * d.nfw;
    return true;
  }
  const int k = n - d.full;
  if (k >= d.per) return false;
  const int m = x * d.per + k;
  if (m >= d.L) return false;
  const int q = m / d.nfw;
  range = d.k8 + q;
  group = m - q * d.nfw;
  return true;
}

// Blocks of a pull launch: as many as the device holds at once (cap), a multiple of 8 so that every share starts with
// the same number of waves; `want` > 0 overrides it (development).  Never fewer than 8.
GD_HD int gd_pull_grid(int cap, int want) {
  int g = (want > 0 ? want : cap) & ~7;
  return g < 8 ? 8 : g;
}
