// beam_prune.h -- the pruning step of the exact-order first pass: sort_token_no_order() (libjulius/src/beam.c:1492 over
// :1342-1480) with the reference's heap, by the whole workgroup.  PruneMem (the step's LDS regions) and PRUNE_MEM_FILL
// that fills it from the layout, the heap routines (level-parallel and overlapped heapify, the serial and the pipelined
// extraction loop), the radix select, the sweep replay (beam_sweep.h, brought in here), the wave-serial event replay
// (chain_scan / apply_event / replay_tail), exact_prune() itself with its PTICK* / PSTAT probes, and literal_sort(),
// the heap carried out literally.  beam_exact.hip's header comment has the method.
// Included by beam_exact.hip (K6x, the prune_order_kernel diagnostic) and beam_exact_mp.h (K6m).  Self-sufficient.
#pragma once
#include "beam_exact_dev.h"

namespace {

// ---- rank pruning with the reference's heap ----------------------------------------------------------
// pre-order key of heap position p (1-based): bit string of p below its leading one, left aligned, then
// the depth -- an ancestor sorts before its descendants, a left subtree before the right one
__device__ __forceinline__ unsigned prekey(unsigned p) {
  const int L = 31 - __clz((int)p);
  return (((p - (1u << L)) << (kMaxL - L)) << 5) | (unsigned)L;
}
__device__ __forceinline__ unsigned prekey_pos(unsigned key) {
  const int L = (int)(key & 31u);
  return (1u << L) + ((key >> 5) >> (kMaxL - L));
}
// is heap position p inside the subtree of position c?  (p == 0: nowhere)
__device__ __forceinline__ bool insub(unsigned p, unsigned c) {
  if (p < c) return false;
  const int d = __clz((int)c) - __clz((int)p);
  return (p >> d) == c;
}

struct PruneMem {                // LDS regions of the pruning step (they overlay the empty Viterbi cells)
  lds_u64 *compR, *compT;        // [b_cap] each: the sorted top list (score bits << 32 | ~prekey at collection time), and scratch for sorting it
  lds_u32 *vposR;                // [b_cap] current virtual heap position per rank
  lds_u32 *idR;                  // [b_cap] token id per rank
  lds_u32 *idT;                  // [b_cap] wide layout: token ids beside compT while the list is being sorted
  lds_u32 *hist;                 // [2048]
  lds_u32 *tailmask;             // [(beam + 31) / 32 + 1]
  lds_i32 *cand;                 // [kMaxCand] tail candidates in the order of their turns: extraction index i
  lds_i32 *occ;                  // [kMaxCand] rank of the element at the candidate's tail position, -1 = none
  lds_i32 *need;                 // [kMaxCand + 4] 1 = (re)scan wanted; [kMaxCand..] = ncand, cursor, finished
  lds_i32 *takers;               // [kMaxCand + 1][kTakers + 1] chain occupants per candidate (+ their count); last row: serial form
  lds_i32 *ordv;                 // [kMaxCand] candidate slots in the order of their turns
  int b_cap;
  unsigned char JAMD_LDS *sw_region;   // the sweep replay (beam_sweep.h): all of the pruning step's overlay, laid out afresh
  int sw_bytes;
  unsigned char *sw_glob;        // its global scratch (sweep_global_bytes()), nullptr = no sweep
  int *pstat;                    // [16] how the pruning steps of this utterance were resolved (XShared::pst), or nullptr
};

// fills `pm` with the regions as xbeam_place() laid them out in dynamic LDS; SW_GLOB = the sweep replay's global scratch or
// nullptr, PSTAT = where the step counts how it was resolved or nullptr.  A macro: the one build that had it as a function
// (and the kernels' own view lines behind the common ones) changed the code of all seventeen exact-order kernels.
#define PRUNE_MEM_FILL(pm, xw, dyn_lds, SW_GLOB, PSTAT)                                                                \
  pm.compR = (lds_u64 *)(dyn_lds + xw.off_compr); pm.compT = pm.compR + xw.b_cap;                                      \
  pm.vposR = (lds_u32 *)(dyn_lds + xw.off_vpos);                                                                       \
  pm.idR = (lds_u32 *)(dyn_lds + xw.off_id);                                                                           \
  pm.idT = (lds_u32 *)(dyn_lds + xw.off_idt);                                                                          \
  pm.hist = (lds_u32 *)(dyn_lds + xw.off_hist);                                                                        \
  pm.tailmask = (lds_u32 *)(dyn_lds + xw.off_tail);                                                                    \
  pm.cand = (lds_i32 *)(pm.tailmask + (xw.w.beam + 31) / 32 + 2);                                                      \
  pm.occ = pm.cand + kMaxCand; pm.need = pm.occ + kMaxCand; pm.takers = pm.need + kMaxCand + 4;                        \
  pm.ordv = pm.takers + (kMaxCand + 1) * (kTakers + 1);                                                                \
  pm.b_cap = xw.b_cap;                                                                                                \
  pm.sw_region = (unsigned char JAMD_LDS *)(dyn_lds + xw.off_dov); pm.sw_bytes = xw.off_row - xw.off_dov;             \
  pm.sw_glob = (SW_GLOB);                                                                                             \
  pm.pstat = (PSTAT)

template <bool UP, typename HP>
__device__ __forceinline__ void heap_sift(HP H, int n, int parent, unsigned long long s) {
  const unsigned sv = (unsigned)(s >> 32);
  int child;
  while ((child = parent * 2) <= n) {
    unsigned long long c = H[child];
    if (child < n) {
      const unsigned long long c2 = H[child + 1];
      const unsigned a = (unsigned)(c >> 32), b = (unsigned)(c2 >> 32);
      if (UP ? (a < b) : (a > b)) { child++; c = c2; }
    }
    const unsigned cv = (unsigned)(c >> 32);
    if (UP ? (sv >= cv) : (sv <= cv)) break;
    H[parent] = c;
    parent = child;
  }
  H[parent] = s;
}

// first loop of sort_token_upward/_downward (:1354-1367): level-parallel
template <bool UP, int NT, typename HP>
__device__ __forceinline__ void heapify_levels(HP H, int n) {
  const int top = n / 2;
  if (top >= 1) {
    for (int L = 31 - __clz(top); L >= 0; L--) {
      const int lo = 1 << L, hi = min((2 << L) - 1, top);
      for (int root = lo + tid_now(); root <= hi; root += NT) heap_sift<UP>(H, n, root, H[root]);
      __syncthreads();
    }
  }
}

// The same loop for a heap in LDS, with the levels overlapped.  A sift-down that starts at depth L is at depth L + t
// after t steps, where it reads the two children below and writes its own level; the sift that started one level
// further down wrote that children's level one step earlier IF it started one step earlier.  So the sifts of
// different levels can run together, one step apart (deepest level first), as long as a step's reads come before
// its writes and see the writes of the step before -- which is how the lanes of ONE wave execute.  Each wave takes
// four of the 64 subtrees rooted at depth 6 (several sifts per lane, their LDS reads in flight together); after one
// workgroup barrier wave 0 finishes depths 5..0 the same way.  A heap of 3 000 entries takes 10 + 17 dependent steps
// and one barrier instead of 66 steps and 11 barriers; the result is the sequential one (every sift reads
// exactly the values it would read in the reference's order).
struct SiftSlot { int parent, t0; unsigned long long s; bool live; };

template <bool UP, int R>
__device__ __forceinline__ void sift_overlapped(lds_u64 *H, int n, SiftSlot (&sl)[R], int gsteps) {
  for (int g = 0; g < gsteps; g++) {
    u32x4 ch[R]; bool run[R], leaf[R];
#pragma unroll
    for (int r = 0; r < R; r++) {                              // reads of this step
      run[r] = sl[r].live && g >= sl[r].t0;
      leaf[r] = 2 * sl[r].parent > n;
      ch[r] = u32x4{0u, 0u, 0u, 0u};
      if (run[r] && !leaf[r]) ch[r] = *(const lds_v4 *)&H[2 * sl[r].parent];
    }
    bool any = false;
#pragma unroll
    for (int r = 0; r < R; r++) {                              // decisions and writes
      if (!run[r]) { any |= sl[r].live; continue; }
      const int child = 2 * sl[r].parent;
      const unsigned a = ch[r].y, b = ch[r].w, sv = (unsigned)(sl[r].s >> 32);
      const bool right = child < n && (UP ? (a < b) : (a > b));
      const unsigned cv = right ? b : a;
      if (leaf[r] || (UP ? (sv >= cv) : (sv <= cv))) { H[sl[r].parent] = sl[r].s; sl[r].live = false; }
      else {
        H[sl[r].parent] = right ? (((unsigned long long)ch[r].w << 32) | ch[r].z) : (((unsigned long long)ch[r].y << 32) | ch[r].x);
        sl[r].parent = child + (right ? 1 : 0);
        any = true;
      }
    }
    wave_sync();
    if (!__any(any)) break;
  }
}

constexpr int kSplitLevel = 6;           // depths >= 6: 64 subtrees, 64 / (waves of the workgroup) per wave; depths < 6: wave 0
template <bool UP, int R, int NT>
__device__ __forceinline__ void heapify_subtrees(lds_u64 *H, int n, int Ltop, int Lmax) {
  constexpr int kSubPerWave = 64 / (NT / 64);
  const int tx = tid_now(), lane = tx & 63, wv = tx >> 6;
  const int D = Ltop - kSplitLevel + 1, top = n / 2;       // a subtree has 2^D - 1 roots: index 1 .. 2^D - 1 inside it
  SiftSlot sl[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int idx = r * 64 + lane;                          // R * 64 = kSubPerWave << D
    const int sub = idx >> D, within = idx & ((1 << D) - 1);
    const int d = within ? 31 - __clz(within) : 0;
    const int pos = (((1 << kSplitLevel) + kSubPerWave * wv + sub) << d) + (within - (1 << d));
    sl[r].live = within != 0 && sub < kSubPerWave && pos <= top;
    sl[r].parent = pos; sl[r].t0 = Ltop - (kSplitLevel + d);
    sl[r].s = sl[r].live ? H[pos] : 0ull;
  }
  sift_overlapped<UP, R>(H, n, sl, (Ltop - kSplitLevel) + (Lmax - kSplitLevel + 1));
}

// returns false when the heap is too deep for the register slots (the caller runs heapify_levels)
template <bool UP, int NT>
__device__ __forceinline__ bool heapify_overlapped(lds_u64 *H, int n) {
  const int top = n / 2;
  if (top < 1) return true;
  const int Ltop = 31 - __clz(top), Lmax = 31 - __clz(n);
  if (Ltop >= kSplitLevel) {
    const int D = Ltop - kSplitLevel + 1;
    constexpr int R5 = ((64 / (NT / 64)) << 5) / 64;      // register slots a lane needs at D = 5
    if (D <= 5) heapify_subtrees<UP, R5, NT>(H, n, Ltop, Lmax);
    else if (D == 6) heapify_subtrees<UP, 2 * R5, NT>(H, n, Ltop, Lmax);
    else if (D == 7 && R5 <= 2) heapify_subtrees<UP, (R5 <= 2 ? 4 * R5 : 1), NT>(H, n, Ltop, Lmax);
    else return false;
    __syncthreads();
  }
  const int tx = tid_now();
  if (tx < 64) {
    const int r = tx + 1, L = 31 - __clz(r);
    const int Lt = Ltop < kSplitLevel ? Ltop : kSplitLevel - 1;
    SiftSlot sl[1];
    sl[0].live = r <= top && L <= Lt;
    sl[0].parent = r; sl[0].t0 = Lt - L;
    sl[0].s = sl[0].live ? H[r] : 0ull;
    sift_overlapped<UP, 1>(H, n, sl, Lt + (Lmax + 1));
  }
  __syncthreads();
  return true;
}

// second loop (:1368-1383) on one lane
template <bool UP, typename HP>
__device__ __forceinline__ void heap_extract_serial(HP H, int n, int cnt) {
  int m = n;
  while (m > n - cnt) {
    const unsigned long long s = H[m];
    H[m] = H[1];
    m--;
    heap_sift<UP>(H, m, 1, s);
  }
}

// The same loop PIPELINED on one wave (heap in LDS).  Extraction e takes the tail element s = H[n - e + 1], puts the
// root there and lets s run down from the root; its step at depth d reads the two children at depth d + 1 and writes
// depth d.  Extraction e + 1 may therefore start two steps behind extraction e: every value it reads has received all
// earlier extractions' writes one step before at the latest (a step's reads come before its writes, and a step sees
// the writes of the step before -- the lanes of one wave).  One more dependency: the tail position n - e + 1 itself
// lies inside the heaps of the earlier extractions, which may still read it, move it up or end there; that is
// possible only for an extraction whose hole is an ancestor (or the position itself), and e waits until no such
// extraction is in flight.  Lane (e - 1) & 63 runs extraction e; about depth / 2 extractions are in flight, so the
// loop costs ~2 steps an extraction instead of one per level: 7x at 4000 extractions from 8000 tokens -- the form
// sort_token_downward() and the fall-backs of the closed-form extraction run in.  Reads and writes are the
// sequential loop's, so is the result.
template <bool UP>
__device__ __noinline__ void heap_extract_pipelined(lds_u64 *H, int n, int cnt) {
  // Branch-free body: idle lanes (p == 0) read H[0..1] and write H[0] (the unused slot in front of the heap), every lane
  // reads the starting extraction's tail element and the root (a broadcast), so no execution-mask juggling is left --
  // a single wave pays ~8 cycles per instruction, the count is what matters.
  H = uni(H); n = uni(n); cnt = uni(cnt);
  const int lane = threadIdx.x & 63;
  lds_u32 *H32 = (lds_u32 *)H;
  int p = 0, m = 0;                                              // p == 0: the lane is idle
  unsigned shi = 0u, slo = 0u;                                   // the element on its way down
  int e = 1;
  bool rest = false;                                             // a start in the previous step: this step starts nothing
  for (;;) {
    // may extraction e start in this step?
    bool st = false;
    const int q = n - e + 1;
    if (!rest && e <= cnt) st = __ballot(p != 0 && insub((unsigned)q, (unsigned)p)) == 0ull;
    rest = st;
    const bool mine = st && lane == ((e - 1) & 63);
    if (mine) { p = 1; m = n - e; }
    const int qe = st ? q : 0;
    // reads
    const unsigned long long tail = H[qe], root = H[1];
    const u32x4 ch = *(const lds_v4 *)&H[2 * p];
    wave_sync();
    // decisions and writes
    if (mine) { shi = (unsigned)(tail >> 32); slo = (unsigned)tail; }
    H[qe] = root;                                                // (no start: slot 0)
    const int child = 2 * p;
    const bool inner = p != 0 && child <= m;
    const bool right = inner && child < m && (UP ? (ch.y < ch.w) : (ch.y > ch.w));
    const unsigned cv = right ? ch.w : ch.y, cl = right ? ch.z : ch.x;
    const bool stop = !inner || (UP ? (shi >= cv) : (shi <= cv));
    H32[2 * p] = stop ? slo : cl;
    H32[2 * p + 1] = stop ? shi : cv;
    p = stop ? 0 : child + (right ? 1 : 0);
    wave_sync();
    e += st ? 1 : 0;
    if (e > cnt && __ballot(p != 0) == 0ull) break;
  }
}

// k-th largest of the score bits in H[1..n] (radix select, 11 bits a pass over the bits in which the
// frame's max and min differ).  Returns the value; all threads.
template <int NT, typename HP>
__device__ __forceinline__ unsigned kth_largest(XShared &sh, HP H, int n, int k, lds_u32 *hist, unsigned xm = 0u) {
  unsigned need = (unsigned)k;
  const unsigned maxb = xm ? ~uni(sh.minbits) : uni(sh.maxbits), diff = uni(sh.maxbits) ^ uni(sh.minbits);
  int remaining = diff ? 32 - __clz(diff) : 0;
  unsigned prefix = remaining < 32 ? (maxb >> remaining) : 0u;
  const int tid = tid_now();
  for (int i = tid; i < 2048; i += NT) hist[i] = 0;      // every pass leaves the histogram cleared (three barriers a pass)
  __syncthreads();
  while (remaining > 0) {
    const int w = remaining < 11 ? remaining : 11;
    const int shift = remaining - w;
    const unsigned dmask = (1u << w) - 1u;
    for (int p = 1 + tid; p <= n; p += NT) {
      const unsigned b = (unsigned)(H[p] >> 32) ^ xm;
      const unsigned hi = (shift + w < 32) ? (b >> (shift + w)) : 0u;
      if (hi == prefix) atomicAdd((unsigned *)&hist[(b >> shift) & dmask], 1u);
    }
    __syncthreads();
    {
      constexpr int BPT = 2048 / NT;                   // radix bins per thread
      static_assert(BPT * NT == 2048 && BPT >= 1, "the 2048 radix bins are scanned BPT per thread");
      unsigned h[BPT], pair = 0u;
#pragma unroll
      for (int x = 0; x < BPT; x++) { h[x] = hist[BPT * tid + x]; hist[BPT * tid + x] = 0u; pair += h[x]; }
      unsigned incl = pair;
      const int ln = tid & 63;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_down(incl, off, 64);
        if (ln + off < 64) incl += o;
      }
      if (ln == 0) sh.wsum[tid >> 6] = incl;
      __syncthreads();
      unsigned above = incl - pair;
      for (int wv = (tid >> 6) + 1; wv < NT / 64; wv++) above += sh.wsum[wv];
#pragma unroll
      for (int x = BPT - 1; x >= 0; x--) {
        if (above < need && need <= above + h[x]) { sh.sel_digit = (unsigned)(BPT * tid + x); sh.sel_need = need - above; sh.sel_count = h[x]; }
        above += h[x];
      }
    }
    __syncthreads();
    prefix = (prefix << w) | uni(sh.sel_digit);      // (written again only behind two more barriers)
    need = uni(sh.sel_need);
    remaining -= w;
  }
  return prefix;
}

#include "beam_sweep.h"

// ---- the events of the extraction loop, replayed by ONE wave (see the file header) -------------------
// Replays extraction i (1-based) when the tail position q = n - i + 1 may hold one of the top elements.
// Ranks 0..i-2 are out already, rank i-1 is at the root.  Wave 0 only; wave-uniform control flow.
//
// Who sits where: a heap position holds the best remaining element of its subtree that is not sitting
// further up.  Subtrees along a root-to-leaf chain are nested, so the occupants of a chain come out of ONE
// scan over the remaining ranks in order: the first element inside subtree(a_0) takes a_0, the next one
// inside subtree(a_1) takes a_1, and so on.
// A single wave runs this, so every dependent instruction costs its full latency: the scans keep the per-step
// work to a compare and a ballot (the chain scan reduces "inside subtree(a_d)" to "shares at least d path bits
// with q", computed once per element), fetch the next 64 ranks while the current ones are walked, and move
// values between lanes with v_readlane (the ballot's lane index is uniform), not with LDS permutes.
__device__ __forceinline__ bool scR_eq(const PruneMem &pm, int r, unsigned sc) { return ((const lds_u32 *)pm.compR)[2 * r + 1] == sc; }

// Occupants of the chain root -> q (q = n - i + 1) after i - 1 extractions, found by one scan over the remaining
// ranks (see above).  Returns the rank of the element sitting AT q, or -1 when the chain ends earlier (the
// element has moved up, or out, before its tail turn).  takers[0..*ntake) receives the ranks of the occupants
// in chain order (the replay uses them to tell which later candidates an event can affect).  One wave.
// (Everything goes in and out by value: a reference or an out parameter of a function that is not inlined is a round
// trip through scratch memory.)  Returns (rank at q, or -1) << 32 | number of occupants written.
__device__ __noinline__ unsigned long long chain_scan(const lds_u32 *vposR, int nB, int n, int i, lds_i32 *takers) {
  vposR = uni(vposR);
  nB = uni(nB); n = uni(n); i = uni(i); takers = uni(takers);
  const int lane = threadIdx.x & 63;
  const unsigned q = (unsigned)(n - i + 1);
  const int Lq = 31 - __clz((int)q);
  const int nchunk = (nB + 63) >> 6;
  int occq = -1, d = 0;
  bool walking = true;
  int c = (i - 1) >> 6;
  unsigned vn = (c * 64 + lane < nB) ? vposR[c * 64 + lane] : 0u;
  for (; c < nchunk && walking; c++) {
    const int r = c * 64 + lane;
    const unsigned v = (r >= i - 1) ? vn : 0u;
    if (c + 1 < nchunk) vn = ((c + 1) * 64 + lane < nB) ? vposR[(c + 1) * 64 + lane] : 0u;
    // m = how many levels of the chain root -> q contain v: v is inside subtree(q >> (Lq - d)) iff d <= m
    int m = -1;
    if (v != 0u) {
      const int Lv = 31 - __clz((int)v);
      const int L = Lv < Lq ? Lv : Lq;
      const unsigned x = (v >> (Lv - L)) ^ (q >> (Lq - L));
      m = L - (x ? 32 - __clz((int)x) : 0);
    }
    int from = 0;
    for (;;) {
      const unsigned long long mk = __ballot(m >= d && lane >= from);
      if (!mk) break;
      const int l = __ffsll((long long)mk) - 1;
      if (lane == 0 && d < kTakers) takers[d] = c * 64 + l;
      if (d == Lq) { occq = c * 64 + l; d++; walking = false; break; }
      d++; from = l + 1;
    }
  }
  return ((unsigned long long)(unsigned)occq << 32) | (unsigned)(d < kTakers ? d : kTakers);
}

// The event itself: the element of rank rs leaves the tail position q = n - i + 1, the root element is output,
// and s runs down the path of larger children among the elements still in the heap (size n - i) until it is
// >= the larger child (:1372-1381).  The larger child of the hole (left on ties) is the best remaining element
// of the hole's subtree: the same kind of single scan.  Then s takes its place among the equal scores still in
// the heap (ranks >= i) by the pre-order of the positions.  Returns the new rank and the new position (packed, see the end).
__device__ __noinline__ unsigned long long apply_event(lds_u64 *compR_, lds_u32 *vposR_, lds_u32 *idR_, int nB, int n, int k, int i, int rs) {
  PruneMem pm;
  pm.compR = uni(compR_); pm.vposR = uni(vposR_); pm.idR = uni(idR_);
  nB = uni(nB); n = uni(n); k = uni(k); i = uni(i); rs = uni(rs);
  const lds_u32 *vposR = pm.vposR;
  const int lane = threadIdx.x & 63;
  const int nchunk = (nB + 63) >> 6;
  const unsigned ssc = (unsigned)(pm.compR[rs] >> 32);
  const unsigned hs = (unsigned)(n - i);
  unsigned hole = 1u;
  {
    bool walking = true;
    int Lh = 0;
    int c = i >> 6;
    const lds_u32 *scR = (const lds_u32 *)pm.compR;      // score bits = the high word of a composite
    unsigned vn = (c * 64 + lane < nB) ? vposR[c * 64 + lane] : 0u;
    unsigned sn = (c * 64 + lane < nB) ? scR[2 * (c * 64 + lane) + 1] : 0u;
    for (; c < nchunk && walking; c++) {
      const int r = c * 64 + lane;
      const unsigned v = (r >= i && r != rs) ? vn : 0u;
      const unsigned scv = sn;
      if (c + 1 < nchunk) {
        vn = ((c + 1) * 64 + lane < nB) ? vposR[(c + 1) * 64 + lane] : 0u;
        sn = ((c + 1) * 64 + lane < nB) ? scR[2 * ((c + 1) * 64 + lane) + 1] : 0u;
      }
      const int Lv = v ? 31 - __clz((int)v) : -1;
      int from = 0;
      for (;;) {
        if (2u * hole > hs) { walking = false; break; }
        // strictly below the hole, and the child of the hole on the way there is inside the heap
        const int dd = Lv - Lh;
        const bool below = dd > 0 && (v >> dd) == hole && (v >> (dd - 1)) <= hs;
        const unsigned long long mk = __ballot(below && lane >= from);
        if (!mk) break;
        const int l = __ffsll((long long)mk) - 1;
        if (ssc >= (unsigned)__builtin_amdgcn_readlane((int)scv, l)) { walking = false; break; }
        const unsigned vl = (unsigned)__builtin_amdgcn_readlane((int)v, l);
        hole = vl >> ((31 - __clz((int)vl)) - Lh - 1);
        Lh++;
        from = l + 1;
      }
    }
  }
  // the equal scores still in the heap, [g0, g1): one look at the 64 ranks around rs, loops only past its edges
  int g0, g1;
  {
    const int r = rs - 32 + lane;
    const bool eq = r >= i && r < nB && scR_eq(pm, r, ssc);
    const unsigned long long mk = __ballot(eq);
    const unsigned below = (unsigned)mk, above = (unsigned)(mk >> 33);     // ranks rs-32..rs-1 / rs+1..rs+31
    const int ndn = below == 0xffffffffu ? 32 : __clz((int)~below);
    const int nup = (above & 0x7fffffffu) == 0x7fffffffu ? 31 : __ffs((int)~above) - 1;
    g0 = rs - ndn; g1 = rs + 1 + nup;
    if (ndn == 32) while (g0 > i && scR_eq(pm, g0 - 1, ssc)) g0--;
    if (nup == 31) while (g1 < nB && scR_eq(pm, g1, ssc)) g1++;
  }
  const unsigned hk = prekey(hole);
  int cnt = 0;
  for (int base = g0; base < g1; base += 64) {
    const int r = base + lane;
    const bool before = r < g1 && r != rs && prekey(pm.vposR[r]) < hk;
    cnt += __popcll(__ballot(before));
  }
  const int newr = g0 + cnt;
  {
    // the ranks between the old and the new place move by one: 64 at a time, every lane reads before any lane writes
    const unsigned sid = pm.idR[rs];
    const unsigned long long sc = pm.compR[rs];
    if (newr < rs) {
      for (int top = rs; top > newr; top -= 64) {            // r-1 -> r for r in (newr, top], highest block first
        const int r = top - lane;
        const bool mv = r > newr;
        const unsigned a = mv ? pm.vposR[r - 1] : 0u, b = mv ? pm.idR[r - 1] : 0u;
        const unsigned long long cc = mv ? pm.compR[r - 1] : 0ull;
        wave_sync();
        if (mv) { pm.vposR[r] = a; pm.idR[r] = b; pm.compR[r] = cc; }
        wave_sync();
      }
    } else {
      for (int bot = rs; bot < newr; bot += 64) {            // r+1 -> r for r in [bot, newr), lowest block first
        const int r = bot + lane;
        const bool mv = r < newr;
        const unsigned a = mv ? pm.vposR[r + 1] : 0u, b = mv ? pm.idR[r + 1] : 0u;
        const unsigned long long cc = mv ? pm.compR[r + 1] : 0ull;
        wave_sync();
        if (mv) { pm.vposR[r] = a; pm.idR[r] = b; pm.compR[r] = cc; }
        wave_sync();
      }
    }
    if (lane == 0) { pm.vposR[newr] = hole; pm.idR[newr] = sid; pm.compR[newr] = sc; }
  }
  __builtin_amdgcn_wave_barrier();
  // new rank | bit 31: an equal score is still in the heap || new position
  return ((unsigned long long)hole << 32) | (unsigned)newr | (g1 - g0 > 1 ? 0x80000000u : 0u);
}

// one tail candidate handled start to finish by one wave (the serial form: more than kMaxCand candidates)
// Returns the turn at which the re-inserted element sits on a tail position again IF it is tied with an element still
// in the heap (the replay must then reach that turn), else 0.
__device__ __noinline__ int replay_tail(const PruneMem &pm, int nB, int n, int k, int i) {
  const int occ = uni((int)(chain_scan(pm.vposR, nB, n, i, pm.takers + kMaxCand * (kTakers + 1)) >> 32));
  if (occ < 0) return 0;
  const unsigned long long ev = apply_event(pm.compR, pm.vposR, pm.idR, nB, n, k, i, occ);
  const unsigned hole = uni((unsigned)(ev >> 32));
  const bool tied = (uni((unsigned)ev) & 0x80000000u) != 0u;
  int again = 0;
  if (hole >= (unsigned)(n - k + 1)) {                               // it sits on a tail position again: its turn comes later
    if ((threadIdx.x & 63) == 0) atomicOr((unsigned *)&pm.tailmask[(n - (int)hole) >> 5], 1u << ((n - (int)hole) & 31));
    if (tied) again = n - (int)hole + 1;
  }
  __builtin_amdgcn_wave_barrier();
  return again;
}

// sort_token_no_order() (:1492): the visiting order of the next frame.  keys[i] = score bits of token i in
// creation order.  Writes the token ids into svid[0..return value).  Whole workgroup.
//
// WIDE (the wide-beam layout): the heap is laid over the list areas -- it is dead once the top elements are
// collected, so they travel through `G` (a scratch array in the utterance's slice) with their token ids, and the
// sorted list is built where the heap was; vposR lies over the sorting scratch.
// FULL (the multipath frame's mid-frame sort, beam_exact_mp.h): the caller wants tindex[] WHOLE -- arr_full[0..n) = the token
// ids at array positions 0..n-1 after the sort, residual heap and extracted part -- beside svid[] (the part the next step
// visits).  Both directions then run sweep replay + sift replay (the closed form of the downward sort, mirrored for the
// upward one), or, where that cannot run, the extraction loop itself.
template <bool WIDE, int NT, bool FULL = false>
__device__ __forceinline__ int exact_prune(XShared &sh, const unsigned *keys, int n, int k, lds_u64 *H, int heap_cap,
                           unsigned long long *Hglob, PruneMem pm, lds_i32 *svid, int mode, u32x4 *G,
                           unsigned long long *tp = nullptr, int *arr_full = nullptr) {
  const int tid = tid_now();
  unsigned long long tc_ = tp ? wall_clock64() : 0ull, tc3_ = tc_;
  (void)tc3_;
#define PTICK(i) do { if (tp && tid == 0 && ((JAMD_XBEAM_PROBE != 3 && JAMD_XBEAM_PROBE != 5 && JAMD_XBEAM_PROBE != 6) || (i) == 7)) { const unsigned long long n_ = wall_clock64(); tp[i] += n_ - tc_; tc_ = n_; tc3_ = n_; } } while (0)
#ifdef JAMD_DEV
#define PTICK5(i) do { if (JAMD_XBEAM_PROBE == 5 && tp && tid == 0) { const unsigned long long n_ = wall_clock64(); tp[i] += n_ - tc3_; tc3_ = n_; } } while (0)
#define PTICK3(i) do { if (JAMD_XBEAM_PROBE == 3 && tp && tid == 0) { const unsigned long long n_ = wall_clock64(); tp[i] += n_ - tc3_; tc3_ = n_; } } while (0)
#define PTICK6(i) do { if (JAMD_XBEAM_PROBE == 6 && tp && tid == 0) { const unsigned long long n_ = wall_clock64(); tp[i] += n_ - tc3_; tc3_ = n_; } } while (0)
#else
#define PTICK5(i) ((void)0)
#define PTICK3(i) ((void)0)
#define PTICK6(i) ((void)0)
#endif
  if (n <= k) {
    for (int j = tid; j < n; j += NT) svid[j] = j;
    if constexpr (FULL) { for (int j = tid; j < n; j += NT) arr_full[j] = j; }
    __syncthreads();
    return n;
  }
#define PSTAT(i, v) do { if (pm.pstat && tid == 0) pm.pstat[i] += (v); } while (0)
  PSTAT(0, 1);
  const bool upward = k < n - k;
  const bool in_lds = n <= heap_cap;
  auto run = [&](auto Hh) -> void {
    constexpr bool kLdsHeap = std::is_same<decltype(Hh), lds_u64 *>::value;
    auto build_heap = [&]() {                                      // first loop of sort_token_upward / _downward (:1354-1367)
      for (int i = tid; i < n; i += NT) Hh[i + 1] = ((unsigned long long)keys[i] << 32) | (unsigned)i;
      __syncthreads();
      PTICK5(4);
      bool heaped = false;
      if constexpr (kLdsHeap) heaped = upward ? heapify_overlapped<true, NT>(Hh, n) : heapify_overlapped<false, NT>(Hh, n);
      if (!heaped) { if (upward) heapify_levels<true, NT>(Hh, n); else heapify_levels<false, NT>(Hh, n); }
    };
    build_heap();
    PTICK5(5);
    PTICK(4);
    bool done = false;
    // sort_token_downward() (beam < tokens <= 2 beam) has a closed form too: the same lists over the n - k SMALLEST
    // elements of the min-heap (score bits complemented), the sweep replay for their moves, and a replay of the short
    // sifts below the extracted region for the residual heap (down_finish()).  Full shape with the sweep's scratch only.
    bool down_ok = false;
    // (wide layout, full shape only: the narrow layout's beams have a handful of tail candidates, and the mere presence of
    // this code in the kernel costs its steps 0-C 2.5 us each per frame at beam 800 -- profiles/r04_ab_sweep_code_presence.txt)
    // (round 5: the whole-array form also in the half shape -- the multipath frame's mid-frame sort needs it there; what does
    // not fit half a CU's LDS falls back to the extraction loop at run time)
    if constexpr (kLdsHeap && (WIDE || FULL) && (NT == jamdb::NT || FULL)) down_ok = (FULL || !upward) && pm.sw_glob != nullptr;
    // (FULL: down_ok = "the whole array can come out of the closed form", either direction)
    const int cnt = upward ? k : n - k;                            // extractions
    const unsigned xm = upward ? 0u : 0xffffffffu;
    if ((upward || down_ok) && (!FULL || down_ok) && mode != 1 && pm.b_cap > 0) {
      // closed form of the extraction loop
      const unsigned vk = kth_largest<NT>(sh, Hh, n, cnt, pm.hist, xm);
      // The top list sorted by (score descending, pre-order of the heap position ascending).  A bitonic network is 55
      // dependent steps at this size; the scores are spread well over their range, so the list is sorted by counting
      // instead: 2048 score bins between the k-th largest score and the maximum (monotone in the score, equal scores
      // in one bin), a prefix sum over the bins, a scatter by bin, and inside its bin (a handful of entries unless many
      // scores are equal) every entry counts the composites greater than its own.  The composites are distinct.
      const unsigned span = (upward ? uni(sh.maxbits) : ~uni(sh.minbits)) - vk;
      const int bshift = span ? max(0, 32 - __clz(span) - 11) : 0;
      // Bins over [k-th score, best]: linear in the score bits -- or, when the list crowds a few linear bins (peaked
      // scores: most of the beam sits just above the cut, a few tokens far above), on a LOG scale of the distance from
      // the cut: 32 octaves x 64 steps, fine where the list is dense.  Both are monotone in the score.
      bool logbins = false;
      auto bin_of = [&](unsigned scb) {
        const unsigned dlt = scb - vk;
        if (!logbins) return (int)min(2047u, dlt >> bshift);
        if (dlt == 0u) return 0;
        const int lz = __clz((int)dlt);
        return (int)((unsigned)(31 - lz) << 6 | ((lz == 31 ? 0u : (dlt << (lz + 1))) >> 26));
      };
      if (tid == 0) { sh.nB = 0; sh.i_last = 0; sh.sel_count = 0u; }
      for (int i = tid; i < (cnt + 31) / 32 + 1; i += NT) pm.tailmask[i] = 0u;
      __syncthreads();                                   // (kth_largest() left the histogram cleared)
      for (int p0 = 1; p0 <= n; p0 += NT) {
        const int p = p0 + tid;
        const unsigned long long hv = p <= n ? Hh[p] : 0ull;
        const unsigned hi = (unsigned)(hv >> 32) ^ xm;
        if ((FULL || !upward) && p <= n) Hglob[p] = hv;  // the heap itself: down_finish() replays the sifts below the extracted region on it
        const bool in = p <= n && hi >= vk;
        const int slot = wave_alloc(&sh.nB, in);
        if (in && slot < pm.b_cap) {
          const unsigned pk = 0xffffffffu - prekey((unsigned)p);
          if constexpr (WIDE) G[slot] = u32x4{pk, hi, (unsigned)hv, 0u};
          else pm.compT[slot] = ((unsigned long long)hi << 32) | pk;
          atomicAdd((unsigned *)&pm.hist[bin_of(hi)], 1u);
        }
      }
      __syncthreads();
      const int nB = uni(sh.nB);
      if (nB <= pm.b_cap) {
        // crowded bins (an entry counts the larger composites of its bin: quadratic in the bin) -> count again on the log scale
        constexpr int BPT0 = 2048 / NT;
        unsigned mx = 0u;
#pragma unroll
        for (int x = 0; x < BPT0; x++) mx = max(mx, pm.hist[BPT0 * tid + x]);
        if (mx > 48u) atomicMax(&sh.sel_count, mx);        // (cleared with nB above)
        __syncthreads();
        if (uni(sh.sel_count) > 48u) {
          logbins = true;
          for (int i = tid; i < 2048; i += NT) pm.hist[i] = 0u;
          __syncthreads();
          for (int e = tid; e < nB; e += NT) {
            unsigned hi;
            if constexpr (WIDE) hi = G[e].y; else hi = (unsigned)(pm.compT[e] >> 32);
            atomicAdd((unsigned *)&pm.hist[bin_of(hi)], 1u);
          }
          __syncthreads();
        }
      }
      PTICK(5);
      if (nB <= pm.b_cap) {
        {
          // exclusive prefix from the top bin down: thread t owns bins 2047 - BPT t ... 2048 - BPT (t + 1)
          constexpr int BPT = 2048 / NT;
          unsigned cb[BPT]; int tot = 0;
#pragma unroll
          for (int x = 0; x < BPT; x++) { cb[x] = pm.hist[2047 - BPT * tid - x]; tot += (int)cb[x]; }
          unsigned ex = (unsigned)block_excl_scan<NT>(sh, tot);
#pragma unroll
          for (int x = 0; x < BPT; x++) { pm.hist[2047 - BPT * tid - x] = ex; ex += cb[x]; }
          __syncthreads();
          for (int e = tid; e < nB; e += NT) {                  // by bin, any order inside; hist[b] ends as the END of bin b
            if constexpr (WIDE) {                               // (the heap is dead: every thread is past the barrier behind the collection)
              const u32x4 g = G[e];
              const unsigned at = atomicAdd((unsigned *)&pm.hist[bin_of(g.y)], 1u);
              pm.compR[at] = ((unsigned long long)g.y << 32) | g.x;
              pm.idT[at] = g.z;
            } else {
              const unsigned long long c = pm.compT[e];
              pm.compR[atomicAdd((unsigned *)&pm.hist[bin_of((unsigned)(c >> 32))], 1u)] = c;
            }
          }
          __syncthreads();
          for (int e = tid; e < nB; e += NT) {
            const unsigned long long c = pm.compR[e];
            const int b = bin_of((unsigned)(c >> 32));
            const int lo = b == 2047 ? 0 : (int)pm.hist[b + 1], hi = (int)pm.hist[b];
            int r = lo;
            for (int x = lo; x < hi; x++) r += pm.compR[x] > c ? 1 : 0;
            pm.compT[r] = c;
            if constexpr (WIDE) pm.idR[r] = pm.idT[e];
          }
          __syncthreads();
        }
        { lds_u64 *t_ = pm.compR; pm.compR = pm.compT; pm.compT = t_; }     // the sorted list is what the replay calls compR
        if constexpr (WIDE) pm.vposR = (lds_u32 *)pm.compT;                 // (the sorting scratch is free from here on)
        // An event re-inserts ONE element; the other elements keep their places in the order, and an element whose
        // score is unique in the list is ranked by its score wherever it sits.  So the replay can stop behind the last
        // turn at which a TIED element may sit on the tail position (sh.i_last; such an element is one that starts on a
        // tail position, possibly re-inserted on a later one): the events after it cannot change the order.
        for (int r = tid; r < nB; r += NT) {
          const unsigned long long cr = pm.compR[r];
          const unsigned p = prekey_pos(0xffffffffu - (unsigned)cr);
          pm.vposR[r] = p;
          if constexpr (!WIDE) pm.idR[r] = (unsigned)Hh[p];
          if (p >= (unsigned)(n - cnt + 1)) {
            atomicOr((unsigned *)&pm.tailmask[(n - (int)p) >> 5], 1u << ((n - (int)p) & 31));
            const unsigned sc = (unsigned)(cr >> 32);
            const bool tied = (r > 0 && (unsigned)(pm.compR[r - 1] >> 32) == sc) || (r + 1 < nB && (unsigned)(pm.compR[r + 1] >> 32) == sc);
            if (tied) atomicMax(&sh.i_last, n - (int)p + 1);
          }
        }
        __syncthreads();
        PTICK(6);
        if (FULL || !upward) {
          // the residual heap: every event matters (the survivors stay in heap layout), so the sweep runs over all turns
          bool ok = false;
          if constexpr (kLdsHeap && (WIDE || FULL) && (NT == jamdb::NT || FULL)) {
            const int tailb = sweep_down_bytes(cnt);
            // (the sift replay holds the whole heap in LDS, 8 bytes a token: a frame too large for it goes to the extraction loop at once)
            if (pm.sw_bytes > tailb + 1024 && 8 * (n + 2) + cnt + 80 <= ((pm.sw_bytes - tailb) & ~15) && n < 0xffff) {
              SweepDown dn;
              unsigned char JAMD_LDS *tl = pm.sw_region + ((pm.sw_bytes - tailb) & ~15);
              dn.fd = (lds_u32 *)tl; dn.posend = dn.fd + cnt + 1; dn.evbits = dn.posend + kSwLeft;
              dn.want_order = FULL ? 1 : 0;
              const int evmax = sweep_pick_evmax(nB, cnt, (pm.sw_bytes - tailb) & ~15);
              if (evmax) ok = sweep_replay<NT>(sh, pm.sw_region, (pm.sw_bytes - tailb) & ~15, pm.sw_glob, pm.compR, pm.vposR, pm.idR, pm.tailmask, nB, n, cnt,
                                               cnt, svid, evmax, &dn);
              __syncthreads();
              if constexpr (FULL) {                          // svid[] = the extracted elements, last extracted first: tindex[n - cnt ..)
                if (ok) for (int j = tid; j < cnt; j += NT) arr_full[n - cnt + j] = svid[j];
                __syncthreads();
              }
              if (ok) ok = upward ? down_finish<NT, false>(sh, pm.sw_region, (pm.sw_bytes - tailb) & ~15, Hglob, n, n - cnt, dn, sweep_ids(pm.sw_glob), nB, svid, FULL ? arr_full : nullptr)
                                  : down_finish<NT, true>(sh, pm.sw_region, (pm.sw_bytes - tailb) & ~15, Hglob, n, n - cnt, dn, sweep_ids(pm.sw_glob), nB, svid, FULL ? arr_full : nullptr);
              if constexpr (FULL) {                          // downward: what the next step visits is the residual heap
                if (ok && !upward) { __threadfence_block(); __syncthreads(); for (int j = tid; j < k; j += NT) svid[j] = arr_full[j]; }
              }
              if (!ok && tid == 0) sh.sw_info = -1;
              __syncthreads();
            }
          }
          if (ok) { done = true; PTICK(7); PSTAT(5, 1); PSTAT(7, sh.sw_info); }
          else build_heap();
        } else {
        // Tail positions holding a top element, in the order of their turns (bit b <-> extraction b + 1).  The chain
        // scans only READ the rank lists, so all candidates are scanned at once, one wave each; wave 0 then walks
        // the candidates in turn order and applies the events.  An event moves one element (and shifts the ranks
        // inside its tie group): a later candidate is scanned again only if that can change its chain.
        lds_i32 *ctl = pm.need + kMaxCand;                    // ncand, cursor, finished, last turn that matters
        if (tid < 64) {
          const int nw = (k + 31) / 32, lim = k;              // all of them: the last turn that matters can move back
          int nc = 0;
          for (int w0 = 0; w0 < nw; w0 += 64) {                // one mask word per lane
            const int w = w0 + tid, rem = lim - w * 32;        // turns i = w * 32 + b + 1 <= lim
            unsigned bits = w < nw ? pm.tailmask[w] : 0u;
            bits &= rem >= 32 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << rem) - 1u));
            const int c = __popc(bits);
            int incl = c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (tid >= off) incl += o; }
            int at = nc + incl - c;
            while (bits) {
              const int b = __ffs((int)bits) - 1;
              bits &= bits - 1u;
              if (at < kMaxCand) { pm.cand[at] = w * 32 + b + 1; pm.need[at] = 1; pm.ordv[at] = at; }
              at++;
            }
            nc += __shfl(incl, 63, 64);
          }
          if (tid == 0) { ctl[0] = nc; ctl[1] = 0; ctl[2] = 0; ctl[3] = sh.i_last; }
        }
        __syncthreads();
        // More live candidates (turn <= the last turn that matters) than the parallel replay holds: an event costs a
        // scan of the whole top list on one wave, hundreds of them cost more than the extraction loop itself run
        // pipelined -- give the closed form up for this frame.  (Wide beams over flat scores: a third of the top
        // elements sit on tail positions.)  The heap was overlaid by the lists in the wide layout: it is built again.
        // More candidates than the wave-serial replay below holds (wide beams: a tenth of the top elements sit on tail
        // positions, hundreds of candidates): the sweep replay resolves them together (beam_sweep.h).  What it cannot
        // hold -- or a work area without its scratch -- goes to the extraction loop itself: the heap is built again (the
        // sweep lays its own image over the whole overlay).
        bool give_up = false;
        if (uni(ctl[0]) > kMaxCand && uni(ctl[3]) > 0) {
          bool swept = false;
          if constexpr (WIDE && NT == jamdb::NT) {         // (the narrow layout and the half shape serve narrow beams: a handful of candidates)
           if (pm.sw_glob) {
            const int evmax = sweep_pick_evmax(nB, k, pm.sw_bytes);
            if (evmax) swept = sweep_replay<NT>(sh, pm.sw_region, pm.sw_bytes, pm.sw_glob, pm.compR, pm.vposR, pm.idR, pm.tailmask, nB, n, k,
                                                uni(ctl[3]), svid, evmax, nullptr);
            if (!swept && tid == 0) sh.sw_info = -1;
            __syncthreads();
           }
          }
          if (swept) { done = true; PTICK(7); PSTAT(3, 1); PSTAT(7, sh.sw_info); }
          else { give_up = true; PSTAT(4, 1); }
        }
        if (give_up) {
          build_heap();
        } else if (!done) {
#ifdef JAMD_DEV
        if (JAMD_XBEAM_PROBE == 3 && tp && tid == 0) tc3_ = wall_clock64();   // slot 7 - (4 + 5 + 6) = everything before the replay
#endif
        const int ncand0 = uni(ctl[0]);
        if (ncand0 > kMaxCand) {
          if (tid < 64) {                                     // serial form, straight off the mask, up to the last turn that matters
            const int nw = (k + 31) / 32;
            int ilast = uni(ctl[3]);
            for (int w = 0; w < nw && w * 32 + 1 <= ilast; w++) {
              unsigned donebits = 0u;
              for (;;) {
                const unsigned bits = ((volatile lds_u32 *)pm.tailmask)[w] & ~donebits;
                if (!bits) break;
                const int b = __ffs((int)bits) - 1;
                donebits |= (b == 31) ? 0xffffffffu : ((2u << b) - 1u);
                const int i = w * 32 + b + 1;
                if (i > ilast) break;
                if (i <= k) { const int again = uni(replay_tail(pm, nB, n, k, i)); if (again > ilast) ilast = again; }
              }
            }
          }
        } else if (ncand0 > 0 && uni(ctl[3]) > 0) {
          // A candidate keeps its slot (turn, occupant, chain occupants); ordv[] lists the slots in turn order, so a
          // candidate born of an event is one shifted int per later candidate.
          for (;;) {
            // (re)scan: the candidate at position c on wave c % 16
            {
              const int ncand = uni(ctl[0]), wv = uni(tid >> 6), ilast = uni(ctl[3]);
              for (int c = uni(ctl[1]) + wv; c < ncand; c += NT / 64) {
                const int sl = uni(pm.ordv[c]);
                const int turn = uni(pm.cand[sl]);
                if (!uni(pm.need[sl]) || turn > ilast) continue;
                lds_i32 *tk = pm.takers + sl * (kTakers + 1);
                const unsigned long long cs = chain_scan(pm.vposR, nB, n, turn, tk);
                if ((tid & 63) == 0) { pm.occ[sl] = (int)(cs >> 32); tk[kTakers] = (int)(unsigned)cs; pm.need[sl] = 0; }
              }
            }
            __syncthreads();
            PTICK3(4);
            if (tid < 64) {
              const int lane = tid;
              int ncand = uni(ctl[0]), c = uni(ctl[1]), ilast = uni(ctl[3]);
              for (; c < ncand; c++) {
                const int sl = uni(pm.ordv[c]);
                const int i = uni(pm.cand[sl]), nd = uni(pm.need[sl]), rs = uni(pm.occ[sl]);
                if (i > ilast) { c = ncand; break; }          // nothing behind this turn can change the order
                if (nd) break;                                // invalidated by an earlier event: next round
                if (rs < 0) continue;
                PTICK6(4);
                const unsigned long long ev = apply_event(pm.compR, pm.vposR, pm.idR, nB, n, k, i, rs);
                PTICK6(5);
                const unsigned hole = uni((unsigned)(ev >> 32));
                const int newr = uni((int)((unsigned)ev & 0x7fffffffu));
                const bool tied = (uni((unsigned)ev) & 0x80000000u) != 0u;
#ifdef JAMD_DEV
                if ((JAMD_XBEAM_PROBE == 3 || JAMD_XBEAM_PROBE == 6) && tp && tid == 0) tp[6] += 100;   // events (1 us each)
#endif
                const int lo = newr < rs ? newr : rs, hi = newr < rs ? rs : newr;
                // which later candidates can this change?  (ranks outside [lo, hi] keep their numbers)  One lane each;
                // the chain occupants are read with a fixed trip count so the loads go out together.
                const int c2 = c + 1 + lane;                  // ncand <= kMaxCand = 64: one pass
                int sl2 = 0, i2 = 0x7fffffff;
                if (c2 < ncand) { sl2 = pm.ordv[c2]; i2 = pm.cand[sl2]; }
                if (c2 < ncand && !pm.need[sl2] && hi >= i2 - 1) {        // (hi < i2 - 1: s is out before that turn)
                  const lds_i32 *tk = pm.takers + sl2 * (kTakers + 1);
                  const int nt = tk[kTakers], oc2 = pm.occ[sl2];
                  bool hit = false; int dat = 0;
#pragma unroll
                  for (int x = 0; x < kTakers; x++) {
                    const int tr = tk[x];
                    if (x < nt) { if (tr >= lo && tr <= hi) hit = true; if (tr < lo) dat++; }
                  }
                  if (!hit && !(oc2 >= 0 && oc2 < lo)) {
                    // would s, now at `hole`, be taken when the walk passes it?  It shares m levels with the chain.
                    const unsigned q2 = (unsigned)(n - i2 + 1);
                    const int Lq2 = 31 - __clz((int)q2), Lv = 31 - __clz((int)hole);
                    const int L = Lv < Lq2 ? Lv : Lq2;
                    const unsigned x = (hole >> (Lv - L)) ^ (q2 >> (Lq2 - L));
                    const int m = L - (x ? 32 - __clz((int)x) : 0);
                    hit = m >= dat;
                  }
                  if (hit) pm.need[sl2] = 1;
                }
                wave_sync();
                if (hole >= (unsigned)(n - k + 1)) {          // s sits on a tail position again: a candidate with a later turn
                  const int inew = n - (int)hole + 1;
                  if (tied && inew > ilast) ilast = inew;
                  const unsigned long long eqm = __ballot(c2 < ncand && i2 == inew);
                  if (eqm) {                                  // already a candidate: two elements share the position now
                    const int e = c + 1 + (__ffsll((long long)eqm) - 1);
                    if (lane == 0) pm.need[pm.ordv[e]] = 1;
                  } else {
                    if (ncand >= kMaxCand) { if (lane == 0) ctl[0] = kMaxCand + 1; ncand = kMaxCand + 1; break; }   // overflow: finish serially
                    const int at = c + 1 + __popcll(__ballot(c2 < ncand && i2 < inew));
                    const int mvslot = (c2 >= at && c2 < ncand) ? sl2 : -1;
                    wave_sync();
                    if (mvslot >= 0) pm.ordv[c2 + 1] = mvslot;
                    if (lane == 0) { pm.ordv[at] = ncand; pm.cand[ncand] = inew; pm.need[ncand] = 1; pm.occ[ncand] = -1; ctl[0] = ncand + 1; }
                    ncand++;
                  }
                  wave_sync();
                }
              }
              if (lane == 0) { ctl[1] = c; ctl[2] = (c >= ncand || ncand > kMaxCand) ? 1 : 0; ctl[3] = ilast; }
            }
            __syncthreads();
            PTICK3(5);
            if (uni(ctl[2])) break;
          }
          if (ctl[0] > kMaxCand && tid < 64) {                // candidate table overflowed mid-way: the rest serially
            int ilast = uni(ctl[3]);
            for (int i = pm.cand[pm.ordv[ctl[1]]]; i <= k && i <= ilast; i++) {
              bool any = false;
              for (int r0 = 0; r0 < nB; r0 += 64) { const int r = r0 + (tid & 63); if (__ballot(r < nB && pm.vposR[r] == (unsigned)(n - i + 1))) { any = true; break; } }
              if (any) { const int again = uni(replay_tail(pm, nB, n, k, i)); if (again > ilast) ilast = again; }
            }
          }
        }
        __syncthreads();
        PTICK(7);
        PSTAT(uni(ctl[3]) > 0 && uni(ctl[0]) > 0 ? 2 : 1, 1);
        for (int j = tid; j < k; j += NT) svid[j] = (int)pm.idR[k - 1 - j];    // tindex[n-k+j]: ascending
        done = true;
        }                                                        // (!give_up)
        }                                                        // (upward)
      }                                                          // (more ties on the cut than the lists hold: the heap is untouched)
    }
    if (!done) {
      PSTAT(6, 1);
      // the extraction loop itself: pipelined on one wave when the heap is in LDS, else (and in the cross-check
      // mode JAMD_ORDER_EXACT_SERIAL) sequentially on one lane
      bool piped = false;
      if constexpr (std::is_same<decltype(Hh), lds_u64 *>::value) {
        if (mode != 1) {
          if (tid < 64) { if (upward) heap_extract_pipelined<true>(Hh, n, k); else heap_extract_pipelined<false>(Hh, n, n - k); }
          piped = true;
        }
      }
      if (!piped && tid == 0) { if (upward) heap_extract_serial<true>(Hh, n, k); else heap_extract_serial<false>(Hh, n, n - k); }
      __syncthreads();
      for (int j = tid; j < k; j += NT) svid[j] = (int)(unsigned)(upward ? Hh[n - k + 1 + j] : Hh[1 + j]);
      if constexpr (FULL) { for (int p = tid; p < n; p += NT) arr_full[p] = (int)(unsigned)Hh[p + 1]; }
    }
    __syncthreads();
  };
  if (in_lds) run(H); else run(Hglob);
  return k;
#undef PSTAT
#undef PTICK
}

// sort_token_no_order() (beam.c:1492 over :1342-1480) carried out literally on (score bits << 32 | index) entries:
// H[1..n] ends as tindex[0..n-1].  The heap in LDS when it fits (pipelined extraction), else in the slice (one lane).
template <int NT>
__device__ __forceinline__ void literal_sort(const unsigned *keys, int n, int k, lds_u64 *Hl, int heap_cap, unsigned long long *Hg) {
  const int tid = tid_now();
  const bool upward = k < n - k;
  auto run = [&](auto Hh) -> void {
    constexpr bool kLds = std::is_same<decltype(Hh), lds_u64 *>::value;
    for (int i = tid; i < n; i += NT) Hh[i + 1] = ((unsigned long long)keys[i] << 32) | (unsigned)i;
    if (tid == 0) Hh[0] = 0ull;
    __syncthreads();
    bool heaped = false;
    if constexpr (kLds) heaped = upward ? heapify_overlapped<true, NT>(Hh, n) : heapify_overlapped<false, NT>(Hh, n);
    if (!heaped) { if (upward) heapify_levels<true, NT>(Hh, n); else heapify_levels<false, NT>(Hh, n); }
    if constexpr (kLds) {
      if (tid < 64) { if (upward) heap_extract_pipelined<true>(Hh, n, k); else heap_extract_pipelined<false>(Hh, n, n - k); }
    } else {
      if (tid == 0) { if (upward) heap_extract_serial<true>(Hh, n, k); else heap_extract_serial<false>(Hh, n, n - k); }
    }
    __syncthreads();
  };
  if (n <= heap_cap) run(Hl); else run(Hg);
}

}  // namespace
