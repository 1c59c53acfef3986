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
// The kernel draws from the deal WITH A TAIL below (gd_tail_*): the same lists, the last tiles of every share in pieces
// of a few states, so that the launch drains by quarter tiles.
// Plain C++, no HIP header: tests/gmm_deal_check.cpp and tests/gmm_deal_tail_check.cpp compile it alone, under the host
// sanitizers.
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

// ---- the deal with a fine-grained TAIL.  A launch ends when the heads run dry with every wave slot somewhere inside a
// tile; the idle time of that drain is about half of the last tickets' length per slot.  So the LAST Q tiles of every
// share are handed out in pieces: share x's list is the list above with each of its last min(Q, len) tiles replaced by
// nsb / sub consecutive sub-tickets of `sub` states (tile-major, the piece fastest), len + (nsb / sub - 1) min(Q, len)
// tickets in all.  A ticket here names (state range, frame group, first state within the range, state count); Q = 0 is
// the deal above ticket for ticket.  The model's last range may hold fewer than nsb states: a sub-ticket whose first
// state lies at or past S is a valid ticket with no work (the caller compares with S and draws again).
constexpr int kGdSub = 4;             // states of a sub-ticket (a quarter of a 16-state tile)

struct GmmTail {
  int q;        // tiles at the end of every share that are dealt in pieces (clamped to the share's length when used)
  int nsb;      // states of a whole tile
  int sub;      // states of a piece: a power of two, at most nsb
  int shift;    // log2(nsb / sub)
};

// nsb and sub are powers of two, sub <= nsb; anything else falls back to kGdSub (nsb itself when that is smaller)
GD_HD GmmTail gd_tail_make(int q, int nsb, int sub) {
  GmmTail t;
  t.q = q < 0 ? 0 : q;
  t.nsb = nsb;
  if (sub < 1 || sub > nsb || (sub & (sub - 1)) != 0) sub = kGdSub < nsb ? kGdSub : nsb;
  t.sub = sub;
  t.shift = 0;
  while ((sub << t.shift) < nsb) t.shift++;
  return t;
}

// the default Q: twice the wave slots that start on one share (four waves per block, the blocks spread over the
// shares) -- 1 024 at 1 024 blocks.  Measured at the bench shape (profiles/ab_gmm_tail.txt): none, one, two, four and
// eight times the slots, pieces of 2, 4 and 8 states; two times and 4 states is the fastest.
GD_HD int gd_tail_default(int grid) { return 2 * (4 * grid / kGdShares); }

// tickets of share x
GD_HD int gd_tail_len(const GmmDeal &d, const GmmTail &t, int x) {
  const int len = gd_len(d, x);
  const int q = t.q < len ? t.q : len;
  return len + ((1 << t.shift) - 1) * q;
}

// ticket n of share x -> (state range, frame group, first state within the range, states); false when the share has
// no such ticket
GD_HD bool gd_tail_ticket(const GmmDeal &d, const GmmTail &t, int x, int n, int &range, int &group, int &s0, int &ns) {
  if (n < 0) return false;
  const int len = gd_len(d, x);
  const int whole = len - (t.q < len ? t.q : len);      // tickets in front of the tail: whole tiles
  s0 = 0;
  ns = t.nsb;
  if (n < whole) return gd_ticket(d, x, n, range, group);
  const int k = n - whole;
  const int tile = whole + (k >> t.shift);              // (>= len behind the share's end: gd_ticket refuses it)
  if (tile >= len) return false;
  s0 = (k & ((1 << t.shift) - 1)) * t.sub;
  ns = t.sub;
  return gd_ticket(d, x, tile, range, group);
}

// Blocks of a pull launch: as many as the device holds at once (cap), a multiple of 8 so that every share starts with
// the same number of waves; `want` > 0 overrides it (development).  Never fewer than 8.
GD_HD int gd_pull_grid(int cap, int want) {
  int g = (want > 0 ? want : cap) & ~7;
  return g < 8 ? 8 : g;
}
