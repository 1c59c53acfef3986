// gmm_outprob.hip -- GMM state-likelihood kernels for gfx950 (CDNA4).
//
// Replaces, for a whole block of frames at once, what the reference computes
// one (state, frame) at a time:
//   outprob_state() batch loop      libsent/src/phmm/outprob.c:230-242
//   calc_mix()                      libsent/src/phmm/calc_mix.c:41-81
//   gprune_none()/compute_g_base()  libsent/src/phmm/gprune_none.c:59-147
//   addlog_array()                  libsent/src/phmm/addlog.c:103-123
//
// Arithmetic contract (bit-exact with the reference's x86-64 object code):
//   * per Gaussian: tmp = gconst; for d ascending: x = o_d - mu_d;
//     tmp = tmp + (x*x)*ivar_d   -- four separately rounded fp32 operations,
//     this file is compiled with -ffp-contract=off so nothing is fused;
//     score = tmp * -0.5 ; score += ln w
//   * mixture log-sum: the table scan of addlog_array() from the LAST mixture
//     to the first, index (unsigned)((double)(-d) * 33333.3333 + 0.5)
//   * result (float)((double)lse * .434294482), LOG_ZERO if lse <= LOG_ZERO or
//     lse == 0 (calc_mix.c:78-80).
//
// Kernel "tile" (the batched hot kernel): ONE LANE = ONE FRAME (FPL frames per
// lane), so the feature vector lives in VGPRs, every Gaussian's (mean, ivar,
// gconst, ln w) record is wave-uniform and arrives through scalar loads into
// SGPRs (each VALU op takes it as its one SGPR operand), the D-loop is exactly
// 4 VALU ops per (frame, Gaussian, dim) with no LDS traffic, and the mixture
// log-sum is an in-lane scan in reference order -- no cross-lane reduction and
// no divergence except the (predicated) table gather.  Results are staged
// through a wave-private LDS tile so the [T][S] matrix is written in coalesced
// row segments.  See DESIGN.md "K1".
//
// This unit holds the kernels that visit every Gaussian of a plain state -- K1, its generic-D and narrow forms --
// and the per-Gaussian scores behind the plugin slot, each with its launcher, and the choice between the three
// forms of K1 (jamd_gmm_launch_plain).  The host layer that calls them is gmm_api.hip (see gmm_host.h).
#include "gmm_dev.h"
#include "gmm_host.h"
#include "gmm_deal.h"

namespace {
using namespace jamd;

constexpr int kWaves = 4;  // waves per workgroup

// FPL (frames per lane) is even: frames are held as packed pairs so that the
// D-loop compiles to v_pk_add_f32 / v_pk_mul_f32 with the Gaussian's scalar
// broadcast through op_sel from an SGPR pair.  Measured on MI355X
// (tools/ubench_valu.hip): a plain VOP2 with an SGPR operand issues at ~0.6x
// the VGPR-only rate, the packed forms do not pay that penalty.
// The mixture log-sum is software-pipelined: the table gather for entry e is
// issued after its D-loop and consumed after the D-loop of entry e-1, so its
// latency hides behind ~160 packed VALU ops.
// HAS_NULL: the model holds NULL densities (gconst stored as NaN, gprune_none.c:67) -- only then does the log-sum step
// carry the two selects that turn such a score into LOG_ZERO (jamd_gmm::has_null, set when the records are packed).
template <int D, int FPL, int NS, bool HAS_NULL>
__global__ void __launch_bounds__(64 * kWaves)
gmm_tile_kernel(const float *__restrict__ rec, const int *__restrict__ st_off,
                const float *__restrict__ frames, const float *__restrict__ tbl,
                float *__restrict__ out, int T, int S, int nsb, int nfb, int nstb,
                float addmin_f) {
  static_assert(FPL % 2 == 0, "frames are processed as packed pairs");
  constexpr int REC = ((2 * D + 2) + 3) & ~3;
  constexpr int FPW = 64 * FPL;
  constexpr int NP = FPL / 2;
  __shared__ float tile[kWaves][FPW][NS + 1];

  int fb, sb;
  if (!decode_block(nfb, nstb, fb, sb)) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int t0 = (fb * kWaves + wave) * FPW;
  if (t0 >= T) return;  // whole wave out of range (no block-level barriers below)

  f2 v[NP][D];
#pragma unroll
  for (int p = 0; p < NP; p++) load_frames<D>(v[p], nullptr, frames, t0 + p * 128, T, D, lane);

  // addlog table as a raw buffer (gfx9 dword 3: 32-bit data format); offsets past its JAMD_TBLSIZE + 1 entries read 0.
  // NaN inputs: a NaN |s - y| selects slot TBLSIZE (0.0f) and v_max_f32 drops a NaN operand -- scores are finite or
  // LOG_ZERO on this path (NULL densities are marked in gconst and handled before the log-sum), so no NaN reaches it.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "gmm_tile: the raw buffer descriptor below is the gfx9 (CDNA) format; this library is written for gfx950 only"
#endif
  const __amdgpu_buffer_rsrc_t tbl_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)tbl, 0, 4 * (JAMD_TBLSIZE + 1), 0x00020000);
  const int s_begin = sb * nsb;
  const int s_end = min(S, s_begin + nsb);
  for (int sg = s_begin; sg < s_end; sg += NS) {
    const int ns = min(NS, s_end - sg);
    for (int si = 0; si < ns; si++) {
      const int e0 = st_off[sg + si], e1 = st_off[sg + si + 1];
      f2 y2[NP], tv2[NP];            // running log-sum and pending table term, packed per frame pair
#pragma unroll
      for (int p = 0; p < NP; p++) { y2[p] = f2{JAMD_LOG_ZERO, JAMD_LOG_ZERO}; tv2[p] = f2{0.0f, 0.0f}; }
      for (int e = e1 - 1; e >= e0; e--) {
        const float *__restrict__ r = rec + (size_t)e * REC;
        const float gc = r[2 * D], lw = r[2 * D + 1];
        f2 acc[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) acc[p] = f2{gc, gc};
#pragma unroll
        for (int d = 0; d < D; d++) {
          const float mu = r[d], iv = r[D + d];
          const f2 mu2 = {mu, mu}, iv2 = {iv, iv};
#pragma unroll
          for (int p = 0; p < NP; p++) {
            f2 x = v[p][d] - mu2;
            x = x * x;
            x = x * iv2;
            acc[p] = acc[p] + x;
          }
        }
        const bool nulld = HAS_NULL && (gc != gc);  // NULL density marker (gprune_none.c:67)
        const float naddmin = -addmin_f;
#pragma unroll
        for (int p = 0; p < NP; p++) {
          // Packed form of addlog_step() for the two frames of a lane.  The table term of the
          // previous entry arrives in tv2 (0.0f from the extra table entry when none was due), so
          // finishing that step (addlog.c:119: y += tbl[idx]) is one packed add without a select.
          // The larger / smaller term of addlog.c:110-116 in the form with the fewest instructions (round 5: 29 -> 22
          // per Gaussian and frame pair): hi = max(s, y) (when they are equal either is the same float), and
          // -(lo - hi) = |s - y| exactly (a float subtraction commutes up to the sign), so the difference is ONE packed
          // subtraction whose absolute value enters the f32 -> f64 conversion as a source modifier; "d < LOG_ADDMIN"
          // becomes |s - y| > -LOG_ADDMIN on the same rounded values.  Index arithmetic in double as the reference.
          f2 s2 = acc[p] * f2{-0.5f, -0.5f};
          if (nulld) s2 = f2{JAMD_LOG_ZERO, JAMD_LOG_ZERO};
          s2 = s2 + f2{lw, lw};
          __builtin_amdgcn_sched_barrier(0);     // keep the wait for the gathered term behind the D-loop
          const f2 yy = y2[p] + tv2[p];
          const f2 hi = {__builtin_fmaxf(s2.x, yy.x), __builtin_fmaxf(s2.y, yy.y)};
          const f2 df = s2 - yy;
          const float a0 = __builtin_fabsf(df.x), a1 = __builtin_fabsf(df.y);
          // the gather is a raw buffer load: table descriptor in four SGPRs, a 32-bit byte offset per lane, no 64-bit
          // address arithmetic (slot JAMD_TBLSIZE of the table holds 0.0f: "no table term")
          unsigned o0 = ((unsigned)((double)a0 * JAMD_TMAG + 0.5)) << 2, o1 = ((unsigned)((double)a1 * JAMD_TMAG + 0.5)) << 2;
          o0 = (a0 <= naddmin) ? o0 : 4u * (unsigned)JAMD_TBLSIZE;
          o1 = (a1 <= naddmin) ? o1 : 4u * (unsigned)JAMD_TBLSIZE;
          tv2[p] = f2{__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(tbl_rsrc, (int)o0, 0, 0)),
                      __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(tbl_rsrc, (int)o1, 0, 0))};
          y2[p] = hi;
        }
      }
#pragma unroll
      for (int k = 0; k < FPL; k++) {
        const f2 fin = y2[k / 2] + tv2[k / 2];
        tile[wave][k * 64 + lane][si] = finish_state((k & 1) ? fin.y : fin.x);
      }
    }
    // (store_tile() in this kernel's own lines: inlined from the helper the loop's exit compare comes out inverted, and
    // the kernel's instruction text is pinned to profiles/gmm_split_kernel_diff.txt)
    wave_sync();
    constexpr int RPI = 64 / NS;  // rows per store instruction
    const int col = lane % NS, rsub = lane / NS;
#pragma unroll 4
    for (int it = 0; it < FPW / RPI; it++) {
      const int rr = it * RPI + rsub;
      const int t = t0 + rr;
      if (t < T && col < ns) out[(size_t)t * S + sg + col] = tile[wave][rr][col];
    }
    wave_release();
  }
}

// ---------------------------------------------------------------------------------------
// K1 at D = 39 with the RECORD RING.  Same lanes, frames, arithmetic, log-sum, tile and epilogue as gmm_tile_kernel;
// what differs is how a Gaussian's record reaches the SGPRs and the order in which the D-loop is written down.
//
// gmm_tile_kernel reads a record where it uses it: three s_load_dwordx16 at the top of a Gaussian and a wait in the
// next instruction, two more chunks waited for 12 and 2 packed operations after they are issued -- about 2.5 scalar
// load latencies per Gaussian that only the SIMD's other waves cover.  Here the records come from the chunk-ordered
// copy jamd_gmm::d_rec_ring (80 floats in five 64-byte chunks, gmm_host.h) into a ring of three 16-SGPR homes that is
// refilled in place ONE GAUSSIAN AHEAD; per Gaussian
//     chunk 0 from home 0 | load this record's chunk 3 -> home 0
//     chunk 1 from home 1 | load this record's chunk 4 -> home 1
//     chunk 2 from home 2 | WAIT
//     chunk 3 from home 0 | load the next record's chunks 0, 2 -> homes 0, 2
//     chunk 4 from home 1 | load the next record's chunk 1 -> home 1
//     log-sum step        | WAIT
// two waits: the first 32 packed operations behind the youngest load it retires, the second 36 behind the next record's
// chunks 0 and 2 and the log-sum step behind its chunk 1 (home 1 is free only once chunk 4 is used: three homes allow no
// better, and the kernel's 104 SGPRs leave no room for a fourth).  The "next record" of a state's
// first entry (the scan runs from the last mixture to the first) is the last entry of the block's next state; the
// block's last state reads its own last entry again, and a state that finds another record in the homes than its last
// (the first state of a block, the state after an empty one) loads it itself.
//
// The loads and waits are asm statements between sched_barrier(0)s: written as plain loads the scheduler sinks the
// next record's loads to the top of the loop, which is gmm_tile_kernel's schedule again.  The compiler does not know
// that an asm load's destination is written LATER than the statement, so it must be given no reason to touch a home
// between a load into it and the wait that retires it.  The one thing it does of its own accord is to copy a home
// (s_mov_b64 x 8) where control flow joins -- the loop's back edge, the end of an `if` --, and such a copy in front of
// the wait moves registers the load has not written yet: a result that is wrong only sometimes.  Hence THE RULE OF
// THIS KERNEL: every wait stands in the same basic block as the loads it retires, before any branch or join -- the
// second wait is the last statement of the loop body, the prologue's wait is inside its `if` -- and no statement
// between a load and its wait names the home.  profiles/gmm_ring_loop_isa.txt holds the loop of all four instantiations as
// compiled; check it again after any change here (no instruction between an s_load_dwordx16 and the next
// s_waitcnt lgkmcnt(0) may name the load's destination registers).
//
// The D-loop is skewed by one stage per dimension inside each chunk: a step issues sub(i), sq(i-1), mul_ivar(i-2),
// acc += (i-3), so every operand is three instructions old and the packed pipe is not held up by its own result.
// The additions are still ONE chain in ascending d from gconst: the same float sequence as gauss_pair().
typedef float f16v __attribute__((ext_vector_type(16)));
constexpr int kRingRec = 80;       // floats per entry of d_rec_ring (gmm_api.hip packs it)

template <int BYTE_OFF>
__device__ __forceinline__ void ring_load(f16v &home, const float *chunks) {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(home) : "s"(chunks), "i"(BYTE_OFF));
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void ring_wait(f16v &h0, f16v &h1, f16v &h2) {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(h0), "+s"(h1), "+s"(h2));
  __builtin_amdgcn_sched_barrier(0);
}
// N dimensions of the D-loop from one home: means at h[MU0 ..], inverse variances at h[IV0 ..], frames v[0 .. N - 1]
template <int N, int MU0, int IV0>
__device__ __forceinline__ void ring_chunk(f2 &acc, const f2 *v, const f16v &h) {
  f2 x[N], q[N], w[N];
#pragma unroll
  for (int i = 0; i < N + 3; i++) {
    if (i < N) { const float mu = h[MU0 + i]; x[i] = v[i] - f2{mu, mu}; }
    if (i >= 1 && i - 1 < N) q[i - 1] = x[i - 1] * x[i - 1];
    if (i >= 2 && i - 2 < N) { const float iv = h[IV0 + i - 2]; w[i - 2] = q[i - 2] * f2{iv, iv}; }
    if (i >= 3) acc = acc + w[i - 3];
    __builtin_amdgcn_sched_barrier(0);
  }
}

// PULL: the same kernel for a launch of as many blocks as the device holds at once (launch_tile).  What the other form
// takes from its block index -- one (state range, frames) tile per wave -- a wave here draws from a ticket counter, tile
// after tile until none is left (gmm_deal.h): everything from the state loop on is the body of that loop, the ring's
// `held` carries over tickets as it does over states, and nothing in a tile depends on which wave computes it or when.
// The four waves of a block share nothing but the LDS array (tile[wave] is private) and never wait for each other.
// A ticket names its states (s_begin, s_end): the last tail_q tiles of every share are drawn in pieces of tail_sub
// states, so that the launch ends on quarter tiles and not on whole ones (the block form ignores both arguments).
template <int NS, bool HAS_NULL, bool PULL>
__global__ void __launch_bounds__(64 * kWaves)
gmm_tile_ring_kernel(const float *__restrict__ ring, const int *__restrict__ st_off,
                     const float *__restrict__ frames, const float *__restrict__ tbl,
                     float *__restrict__ out, int T, int S, int nsb, int nfb, int nstb,
                     float addmin_f, int *__restrict__ heads, int tail_q, int tail_sub) {
  constexpr int D = 39, FPL = 2;
  constexpr int FPW = 64 * FPL;
  __shared__ float tile[kWaves][FPW][NS + 1];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  f2 v[D];
  int sb, t0, s_begin, s_end;
  if constexpr (!PULL) {
    int fb;
    if (!decode_block(nfb, nstb, fb, sb)) return;
    t0 = (fb * kWaves + wave) * FPW;
    if (t0 >= T) return;  // whole wave out of range (no block-level barriers below)
    load_frames<D>(v, nullptr, frames, t0, T, D, lane);
  }

  // (the addlog table as a raw buffer: see gmm_tile_kernel)
  const __amdgpu_buffer_rsrc_t tbl_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)tbl, 0, 4 * (JAMD_TBLSIZE + 1), 0x00020000);
  const float naddmin = -addmin_f;
  // PULL: the wave's share of the deal (gmm_deal.h; nfb holds the launch's groups of FPW frames) and the shares it has
  // found exhausted
  int share = blockIdx.x & (kGdShares - 1), spent = 0;
  f16v h0, h1, h2;             // the ring: chunks 0 / 1 / 2 of record `held` at the top of a Gaussian
  int held = -1;
  for (;;) {
    if constexpr (PULL) {
      // Take a ticket: lane 0 draws the next number of the wave's share (one returning add on the share's head, relaxed,
      // device scope: the number is all that is communicated); a number past the share's end sends the wave on to the
      // next share for good (a share never grows again), and after eight such finds there is no tile left anywhere.
      // Which wave computes a tile changes nothing in the tile: the result does not depend on the draw.
      // The last tail_q tiles of a share come in pieces of tail_sub states (gd_tail_ticket): the ticket names its states,
      // and a piece that begins behind the model's last state (a short last range) is an empty ticket -- the wave draws
      // again, before any frame is loaded.
      const GmmDeal deal = gd_make(nstb, nfb);
      const GmmTail tail = gd_tail_make(tail_q, nsb, tail_sub);
      int group = 0;
      bool got = false;
      while (spent < kGdShares) {
        int n = 0, s0 = 0, cnt = 0;
        if (lane == 0) n = __hip_atomic_fetch_add(heads + share * kGdHeadStride, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        n = __builtin_amdgcn_readfirstlane(n);
        if (gd_tail_ticket(deal, tail, share, n, sb, group, s0, cnt)) {
          s_begin = sb * nsb + s0;
          s_end = min(S, s_begin + cnt);
          got = s_begin < S;
          if (got) break;
          continue;
        }
        share = (share + 1) & (kGdShares - 1);
        spent++;
      }
      if (!got) return;
      t0 = group * FPW;
      // The frames are loaded for every ticket, as a block of the other form loads them for its one tile.  Keeping them
      // when the new ticket names the group already held would need `v` carried round this loop past a conditional
      // load: compiled, that is two copies of the 78 registers (183 VGPRs, or scratch under a 128-register bound), and
      // a share runs over a range's groups first (at least three in a pull launch), so a wave's next ticket names another group.
      load_frames<D>(v, nullptr, frames, t0, T, D, lane);
    } else {
      s_begin = sb * nsb;
      s_end = min(S, s_begin + nsb);
    }
    for (int sg = s_begin; sg < s_end; sg += NS) {
      const int ns = min(NS, s_end - sg);
      for (int si = 0; si < ns; si++) {
        const int s = sg + si;
        const int e0 = st_off[s], e1 = st_off[s + 1];
        // the record behind this state's first entry: the next state's last one (its own last one when that state is
        // empty: a valid record, and `held` sends the state after it through the prologue), or this state's last again
        const int e_over = (s + 1 < s_end ? st_off[s + 2] : e1) - 1;
        f2 y2 = {JAMD_LOG_ZERO, JAMD_LOG_ZERO}, tv2 = {0.0f, 0.0f};   // running log-sum and pending table term
        if (e1 > e0 && held != e1 - 1) {
          const float *r = ring + (size_t)(e1 - 1) * kRingRec;
          ring_load<0>(h0, r);
          ring_load<64>(h1, r);
          ring_load<128>(h2, r);
          ring_wait(h0, h1, h2);     // inside the `if`: see the rule above
        }
        for (int e = e1 - 1; e >= e0; e--) {
          const float *r = ring + (size_t)e * kRingRec;
          const float *rn = ring + (size_t)(e > e0 ? e - 1 : e_over) * kRingRec;
          const float gc = h0[0], lw = h0[1];
          const bool nulld = HAS_NULL && (gc != gc);  // NULL density marker (gprune_none.c:67)
          f2 acc = {gc, gc};
          ring_chunk<7, 2, 9>(acc, v, h0);
          ring_load<192>(h0, r);
          ring_chunk<8, 0, 8>(acc, v + 7, h1);
          ring_load<256>(h1, r);
          ring_chunk<8, 0, 8>(acc, v + 15, h2);
          ring_wait(h0, h1, h2);
          ring_chunk<8, 0, 8>(acc, v + 23, h0);
          ring_load<0>(h0, rn);
          ring_load<128>(h2, rn);
          ring_chunk<8, 0, 8>(acc, v + 31, h1);
          ring_load<64>(h1, rn);
          {
            // the log-sum step of gmm_tile_kernel (see the notes there), for the lane's one frame pair
            f2 s2 = acc * f2{-0.5f, -0.5f};
            if (nulld) s2 = f2{JAMD_LOG_ZERO, JAMD_LOG_ZERO};
            s2 = s2 + f2{lw, lw};
            __builtin_amdgcn_sched_barrier(0);     // keep the wait for the gathered term behind the D-loop
            const f2 yy = y2 + tv2;
            const f2 hi = {__builtin_fmaxf(s2.x, yy.x), __builtin_fmaxf(s2.y, yy.y)};
            const f2 df = s2 - yy;
            const float a0 = __builtin_fabsf(df.x), a1 = __builtin_fabsf(df.y);
            unsigned o0 = ((unsigned)((double)a0 * JAMD_TMAG + 0.5)) << 2, o1 = ((unsigned)((double)a1 * JAMD_TMAG + 0.5)) << 2;
            o0 = (a0 <= naddmin) ? o0 : 4u * (unsigned)JAMD_TBLSIZE;
            o1 = (a1 <= naddmin) ? o1 : 4u * (unsigned)JAMD_TBLSIZE;
            tv2 = f2{__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(tbl_rsrc, (int)o0, 0, 0)),
                     __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(tbl_rsrc, (int)o1, 0, 0))};
            y2 = hi;
          }
          ring_wait(h0, h1, h2);     // the last statement of the body: see the rule above
        }
        if (e1 > e0) held = e_over;
        const f2 fin = y2 + tv2;
        tile[wave][lane][si] = finish_state(fin.x);
        tile[wave][64 + lane][si] = finish_state(fin.y);
      }
      store_tile<NS, FPW>(tile[wave], out, t0, T, S, sg, ns, lane);
    }
    if constexpr (!PULL) break;
  }
}

// Generic-D variant: the frame vectors sit in LDS transposed [d][frame-in-wave] (load_frames<0>), a Gaussian is
// gauss_pair<0> on the lane's two frames and the log-sum the plain in-lane addlog_step() in the same order; blocks,
// tile and epilogue as above.
template <int FPL, int NS>
__global__ void __launch_bounds__(64 * kWaves)
gmm_tile_generic_kernel(const float *__restrict__ rec, const int *__restrict__ st_off,
                        const float *__restrict__ frames, const float *__restrict__ tbl,
                        float *__restrict__ out, int T, int S, int D, int REC, int nsb, int nfb,
                        int nstb, float addmin_f) {
  static_assert(FPL == 2, "load_frames / gauss_pair hold one packed pair of frames per lane");
  constexpr int FPW = 64 * FPL;
  __shared__ float tile[kWaves][FPW][NS + 1];
  extern __shared__ __align__(16) float dyn[];  // [kWaves][D][FPW]

  int fb, sb;
  if (!decode_block(nfb, nstb, fb, sb)) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int t0 = (fb * kWaves + wave) * FPW;
  if (t0 >= T) return;
  float *vt = dyn + (size_t)wave * D * FPW;
  load_frames<0>(nullptr, vt, frames, t0, T, D, lane);

  const int s_begin = sb * nsb;
  const int s_end = min(S, s_begin + nsb);
  for (int sg = s_begin; sg < s_end; sg += NS) {
    const int ns = min(NS, s_end - sg);
    for (int si = 0; si < ns; si++) {
      const int e0 = st_off[sg + si], e1 = st_off[sg + si + 1];
      float y0 = JAMD_LOG_ZERO, y1 = JAMD_LOG_ZERO;
      for (int e = e1 - 1; e >= e0; e--) {
        const float *__restrict__ r = rec + (size_t)e * REC;
        const float lw = r[2 * D + 1];
        const f2 g = gauss_pair<0>(nullptr, vt, lane, D, r);   // (LOG_ZERO for a NULL density, then the weight as K1)
        y0 = addlog_step(y0, g.x + lw, tbl, addmin_f);
        y1 = addlog_step(y1, g.y + lw, tbl, addmin_f);
      }
      tile[wave][lane][si] = finish_state(y0);
      tile[wave][64 + lane][si] = finish_state(y1);
    }
    store_tile<NS, FPW>(tile[wave], out, t0, T, S, sg, ns, lane);
  }
}

constexpr int kNarrowT = 256;      // calls of at most this many frames go to K1n (below; its scratch is kNarrowT x E floats)
constexpr int kPullNS = 16;        // the tile width K1 is launched with (jamd_gmm_launch_plain)
constexpr int kPullRounds = 5;     // rounds of blocks from which a call takes the pull form (jamd_gmm_pull_setup)

template <int D, int FPL, int NS>
int launch_tile(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st) {
  constexpr int FPB = kWaves * 64 * FPL;
  const int nfb = (T + FPB - 1) / FPB;
  // States per block: NS, the width of the output tile -- the smallest there is.  A block's fixed cost (its 128
  // frames per wave loaded into registers) is nothing against 16 states x 16 Gaussians of arithmetic, and short
  // blocks are what keeps the last wave of blocks of a launch short: at 64 000 frames a launch is four rounds of
  // 96-state blocks or twenty-three rounds of 16-state ones (23 500 blocks over 1 024 block slots: 22.95; the sweep
  // below was taken when the deal still left four XCDs a twenty-fourth), 10.97 vs 9.93 ms (sweep on MI355X: 16 / 32 /
  // 48 / 64 / 96 / 128 states -> 9.93 / 10.02 / 10.35 / 10.62 / 10.97 / 11.22 ms; 384 000 frames: 60.4 vs 61.8 ms;
  // 16 000: 2.63 vs 2.78 ms).  Block b runs on XCD b % 8; a state range of the full rounds of eight is pinned to one
  // XCD, so the blocks that share it share an L2, and the blocks of the leftover ranges (188 = 8 x 23 + 4 at 3 000
  // states) are dealt evenly over all eight (decode_block).
  const int nsb = NS;
  const int nstb = (g->S + nsb - 1) / nsb;
  const int grid = xcd_grid(nstb, nfb);
  if constexpr (D == 39 && FPL == 2) {
    // the record-ring form of the kernel (above); the suffix keeps measurements taken on the other form apart
    static_assert(NS == kPullNS, "jamd_gmm_pull_setup() asks the occupancy of this instantiation");
    // A call of many rounds of blocks (23 504 blocks against 1 024 resident at the bench shape) is served by the
    // PULL form: as many blocks as are resident together, whose waves draw (state range, 128-frame group) tiles from
    // the per-XCD ticket heads until none is left -- a wave slot is refilled when ITS tile ends, not when the slowest
    // of a block's four does, no block is dispatched after the first round, and the launch drains by quarter tiles
    // (when the heads run dry every slot is somewhere inside its last ticket; a whole tile lasts 400 us at the bench
    // shape).  Shorter calls keep the block form below as it is (the threshold: jamd_gmm_pull_setup).
    if (g->pull_min >= 0 && T > kNarrowT && (long long)nstb * nfb > g->pull_min) {
      const int nfw = (T + 64 * FPL - 1) / (64 * FPL);
      const int pgrid = gd_pull_grid(g->pull_cap, g->pull_grid);
      // the end of every share in pieces (gmm_deal.h): by default twice as many tiles as wave slots start on the share,
      // in quarters (profiles/ab_gmm_tail.txt)
      const GmmTail tail = gd_tail_make(g->pull_tail >= 0 ? g->pull_tail : gd_tail_default(pgrid), nsb, g->pull_sub);
      JAMD_HIP(hipMemsetAsync(g->d_pull_heads, 0, sizeof(int) * kGdShares * kGdHeadStride, st));
      if (g->has_null)
        hipLaunchKernelGGL((gmm_tile_ring_kernel<NS, true, true>), dim3(pgrid), dim3(64 * kWaves), 0, st,
                           g->d_rec_ring, g->d_st_off_plain, frames, g->eng->d_addlog, out, T, g->S, nsb, nfw,
                           nstb, g->eng->addmin_f, g->d_pull_heads, tail.q, tail.sub);
      else
        hipLaunchKernelGGL((gmm_tile_ring_kernel<NS, false, true>), dim3(pgrid), dim3(64 * kWaves), 0, st,
                           g->d_rec_ring, g->d_st_off_plain, frames, g->eng->d_addlog, out, T, g->S, nsb, nfw,
                           nstb, g->eng->addmin_f, g->d_pull_heads, tail.q, tail.sub);
      snprintf(g->last_kernel, sizeof(g->last_kernel), "gmm_tile<D=%d,FPL=%d,NS=%d,ring,pull> grid=%d nsb=%d tail=%dx%d", D, FPL, NS, pgrid, nsb, tail.q, tail.sub);
      return JAMD_OK;
    }
    if (g->has_null)
      hipLaunchKernelGGL((gmm_tile_ring_kernel<NS, true, false>), dim3(grid), dim3(64 * kWaves), 0, st,
                         g->d_rec_ring, g->d_st_off_plain, frames, g->eng->d_addlog, out, T, g->S, nsb, nfb,
                         nstb, g->eng->addmin_f, (int *)nullptr, 0, 0);
    else
      hipLaunchKernelGGL((gmm_tile_ring_kernel<NS, false, false>), dim3(grid), dim3(64 * kWaves), 0, st,
                         g->d_rec_ring, g->d_st_off_plain, frames, g->eng->d_addlog, out, T, g->S, nsb, nfb,
                         nstb, g->eng->addmin_f, (int *)nullptr, 0, 0);
    snprintf(g->last_kernel, sizeof(g->last_kernel), "gmm_tile<D=%d,FPL=%d,NS=%d,ring> grid=%d nsb=%d", D, FPL, NS, grid, nsb);
  } else {
    if (g->has_null)
      hipLaunchKernelGGL((gmm_tile_kernel<D, FPL, NS, true>), dim3(grid), dim3(64 * kWaves), 0, st,
                         g->d_rec, g->d_st_off_plain, frames, g->eng->d_addlog, out, T, g->S, nsb, nfb,
                         nstb, g->eng->addmin_f);
    else
      hipLaunchKernelGGL((gmm_tile_kernel<D, FPL, NS, false>), dim3(grid), dim3(64 * kWaves), 0, st,
                         g->d_rec, g->d_st_off_plain, frames, g->eng->d_addlog, out, T, g->S, nsb, nfb,
                         nstb, g->eng->addmin_f);
    snprintf(g->last_kernel, sizeof(g->last_kernel), "gmm_tile<D=%d,FPL=%d,NS=%d> grid=%d nsb=%d", D, FPL, NS, grid, nsb);
  }
  return JAMD_OK;
}

template <int FPL, int NS>
int launch_tile_generic(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st) {
  constexpr int FPB = kWaves * 64 * FPL;
  const int nfb = (T + FPB - 1) / FPB;
  const int nsb = NS;   // as launch_tile()
  const int nstb = (g->S + nsb - 1) / nsb;
  const int grid = xcd_grid(nstb, nfb);
  const size_t dyn = sizeof(float) * kWaves * g->D * 64 * FPL;
  const int rc = jamd_reserve_dyn_lds((const void *)gmm_tile_generic_kernel<FPL, NS>, dyn, "GMM outprob");
  if (rc != JAMD_OK) return rc;
  hipLaunchKernelGGL((gmm_tile_generic_kernel<FPL, NS>), dim3(grid), dim3(64 * kWaves), dyn, st,
                     g->d_rec, g->d_st_off_plain, frames, g->eng->d_addlog, out, T, g->S, g->D, g->rec,
                     nsb, nfb, nstb, g->eng->addmin_f);
  snprintf(g->last_kernel, sizeof(g->last_kernel), "gmm_tile_generic<FPL=%d,NS=%d> D=%d grid=%d",
           FPL, NS, g->D, grid);
  return JAMD_OK;
}

// ---------------------------------------------------------------------------------------
// K1n, the NARROW form of K1 (round 6): a call of a handful of frames -- live input, a streaming chunk
// (JAMD_STREAM_CHUNK = 25), the calcmix slot of a frame-synchronous caller.  K1 maps one lane to one frame (128 frame
// slots per wave): a 25-frame call fills a fifth of ONE wave per 16-state block, and every block still walks its 256
// Gaussians one after the other -- 250 us per call whatever T is, the 15.4 MB model streamed at 60 GB/s.  Here the
// mapping is turned round: one lane = one MIXTURE ENTRY (its record in 2 D + 2 registers, read once per call), the
// frames are wave-uniform and arrive by scalar load, two at a time as the packed pair of the D-loop; the weighted
// Gaussian scores go to a [T][E] scratch (coalesced), and a second kernel -- one lane per (frame, state) -- runs the
// table log-sum from the last mixture to the first (addlog_array(), addlog.c:103) and calc_mix()'s tail.  Same four
// separately rounded fp32 operations per dimension, same scan order: bit-identical to K1 (tests/test_gmm_gpu.py).
constexpr int kNarrowFB = 8;       // frames per block of the first kernel
template <int D, bool HAS_NULL>
__global__ void __launch_bounds__(64)
gmm_narrow_dens_kernel(const float *__restrict__ rec, const float *__restrict__ frames, float *__restrict__ dens, int T, int E,
                       int nfb, int neb) {
  constexpr int REC = (2 * D + 2 + 3) & ~3;
  // the frame blocks of one range of 64 entries run on ONE XCD (block b is placed on XCD b % 8): the range's records
  // come from HBM / Infinity Cache once and from that XCD's L2 for the other frame blocks; the ranges left over from
  // whole rounds of eight are spread over all XCDs, each on at most two (decode_block(), as K1)
  int fbk, ebk;
  if (!decode_block(nfb, neb, fbk, ebk)) return;
  const int e = ebk * 64 + threadIdx.x;
  const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(rec + (size_t)(e < E ? e : E - 1) * REC);
  float r[REC];
#pragma unroll
  for (int q = 0; q < REC / 4; q++) { const float4 v = r4[q]; r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w; }
  const float gc = r[2 * D], lw = r[2 * D + 1];
  const bool nulld = HAS_NULL && (gc != gc);      // NULL density marker (gprune_none.c:67)
  // a block takes kNarrowFB frames: with one wave per SIMD the scalar loads of a frame pair (a microsecond) were not
  // covered by anything (25 frames: 26 us); three or four waves per SIMD cover them (the record is read once per block: L2)
  const int t_end = min(T, (fbk + 1) * kNarrowFB);
  for (int t = fbk * kNarrowFB; t < t_end; t += 2) {
    const float *__restrict__ fa = frames + (size_t)t * D;
    const float *__restrict__ fb = frames + (size_t)(t + 1 < T ? t + 1 : t) * D;
    f2 acc = {gc, gc};
#pragma unroll
    for (int d = 0; d < D; d++) {
      f2 x = f2{fa[d], fb[d]} - f2{r[d], r[d]};
      x = x * x;
      x = x * f2{r[D + d], r[D + d]};
      acc = acc + x;
    }
    f2 s2 = acc * f2{-0.5f, -0.5f};
    if (nulld) s2 = f2{JAMD_LOG_ZERO, JAMD_LOG_ZERO};
    s2 = s2 + f2{lw, lw};
    if (e < E) {
      dens[(size_t)t * E + e] = s2.x;
      if (t + 1 < T) dens[(size_t)(t + 1) * E + e] = s2.y;
    }
  }
}

__global__ void __launch_bounds__(256)
gmm_narrow_lse_kernel(const float *__restrict__ dens, const int *__restrict__ st_off, const float *__restrict__ tbl,
                      float *__restrict__ out, int T, int S, int E, float addmin_f) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T * S) return;
  const int t = i / S, s = i - t * S;
  const int e0 = st_off[s], e1 = st_off[s + 1];
  const float *__restrict__ dr = dens + (size_t)t * E;
  float y = JAMD_LOG_ZERO;
  int e = e1 - 1;
  for (; e - 7 >= e0; e -= 8) {                    // eight terms in flight in front of the serial table scan
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = dr[e - q];
#pragma unroll
    for (int q = 0; q < 8; q++) y = addlog_step(y, v[q], tbl, addmin_f);
  }
  for (; e >= e0; e--) y = addlog_step(y, dr[e], tbl, addmin_f);
  out[(size_t)t * S + s] = finish_state(y);
}

template <int D>
int launch_narrow(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st) {
  const int E = g->E_plain;
  int rc = g->d_narrow.grow(sizeof(float) * (size_t)kNarrowT * (size_t)E);   // (first narrow call only)
  if (rc != JAMD_OK) return rc;
  const int grid = (E + 63) / 64;
  const int nfb = (T + kNarrowFB - 1) / kNarrowFB;
  const dim3 gr(xcd_grid(grid, nfb));
  if (g->has_null) hipLaunchKernelGGL((gmm_narrow_dens_kernel<D, true>), gr, dim3(64), 0, st, g->d_rec, frames, g->d_narrow, T, E, nfb, grid);
  else hipLaunchKernelGGL((gmm_narrow_dens_kernel<D, false>), gr, dim3(64), 0, st, g->d_rec, frames, g->d_narrow, T, E, nfb, grid);
  hipLaunchKernelGGL(gmm_narrow_lse_kernel, dim3((T * g->S + 255) / 256), dim3(256), 0, st, g->d_narrow, g->d_st_off_plain,
                     g->eng->d_addlog, out, T, g->S, E, g->eng->addmin_f);
  snprintf(g->last_kernel, sizeof(g->last_kernel), "gmm_narrow<D=%d> grid=%d + lse", D, grid);
  return JAMD_OK;
}

// ---------------------------------------------------------------------------------------
// Per-Gaussian scores for the reference's plugin slot (compute_gaussset / calcmix,
// plugin/calcmix.c:86-323): dens[t][e] = compute_g_base() of mixture entry e at frame t,
// (gconst + sum_d (o_d - mu_d)^2 * ivar_d) * -0.5, the same four fp32 operations per dimension as
// K1 and no weight, no log-sum (calc_mix() applies those to what the plugin returns).  One wave =
// 64 frames (their vectors transposed in LDS so any D fits), a block walks a chunk of entries,
// 16 at a time through a wave-private tile so that [T][E] is written in 64-byte row segments.
constexpr int kDensChunk = 1024;
__global__ void __launch_bounds__(64)
gmm_dens_kernel(const float *__restrict__ rec, const float *__restrict__ frames, float *__restrict__ out,
                int T, int E, int D, int REC) {
  extern __shared__ float xs[];                  // [D][64] then tile [64][17]
  float (*tile)[17] = reinterpret_cast<float (*)[17]>(xs + (size_t)D * 64);
  const int lane = threadIdx.x;
  const int t0 = blockIdx.x * 64, e_begin = blockIdx.y * kDensChunk;
  const int e_end = min(E, e_begin + kDensChunk);
  {
    int t = t0 + lane; if (t > T - 1) t = T - 1;
    const float *f = frames + (size_t)t * D;
    for (int d = 0; d < D; d++) xs[d * 64 + lane] = f[d];
  }
  wave_sync();
  for (int e0 = e_begin; e0 < e_end; e0 += 16) {
    const int ne = min(16, e_end - e0);
    for (int g = 0; g < ne; g++) {
      const float *__restrict__ r = rec + (size_t)(e0 + g) * REC;
      const float gc = r[2 * D];
      float acc = gc;
      for (int d = 0; d < D; d++) {
        float x = xs[d * 64 + lane] - r[d];
        x = x * x;
        x = x * r[D + d];
        acc = acc + x;
      }
      float sc = acc * -0.5f;
      if (gc != gc) sc = JAMD_LOG_ZERO;            // NULL density (gprune_none.c:67, plugin/calcmix.c:104)
      tile[lane][g] = sc;
    }
    // (store_tile() in this kernel's own lines: its tile is in dynamic LDS and its loop fully unrolled, and through
    // the helper the row multiply's operands trade places in the kernel's pinned instruction text)
    wave_sync();
    const int col = lane & 15, rsub = lane >> 4;
    for (int it = 0; it < 16; it++) {
      const int rr = it * 4 + rsub, t = t0 + rr;
      if (t < T && col < ne) out[(size_t)t * E + e0 + col] = tile[rr][col];
    }
    wave_release();
  }
}

}  // namespace


// entry points used by gmm_api.hip
int jamd_gmm_pull_setup(jamd_gmm *g) {
  if (g->D != 39) return JAMD_OK;      // the record-ring kernel alone has a pull form
  int rc, per_cu = 0;
  if ((rc = g->d_pull_heads.alloc(kGdShares * kGdHeadStride, true)) != JAMD_OK) return rc;
  if (g->has_null) JAMD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gmm_tile_ring_kernel<kPullNS, true, true>, 64 * kWaves, 0));
  else JAMD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gmm_tile_ring_kernel<kPullNS, false, true>, 64 * kWaves, 0));
  g->pull_cap = (per_cu * g->eng->num_cu) & ~7;       // (4 x 256 = 1 024 on MI355X)
  if (g->pull_cap < 8) g->pull_cap = 8;
  // A call takes the pull form from five rounds of blocks on.  With whole tiles to the end the form lost up to a few
  // rounds (the tiles of the last, partial round go to the waves that ask first: 2 048 frames 1.23, 8 000 frames 1.07,
  // profiles/ab_gmm_pull.txt); with the tail in quarters the last tickets are short and it mostly does not (single calls,
  // 3 000 states, pull / block: 2 048 frames, 0.73 rounds, 0.986; 4 000, 1.5 rounds, 0.995; 8 000, 2.9 rounds, 1.005;
  // 16 000, 5.9 rounds, 0.976; 32 000, 11.6 rounds, 0.956 -- profiles/ab_gmm_tail.txt).  8 000 frames is still slower
  // beyond the block form's spread, so the threshold lies between 2.9 and 5.9 rounds, on the side measured to win.
  g->pull_min = kPullRounds * g->pull_cap;
  // Development switches, read once per model: JAMD_GMM_PULL_MIN = the block count above which the pull form is used
  // (0: every call of more than kNarrowT frames; negative: never), JAMD_GMM_PULL_GRID = blocks of a pull launch.
  if (const char *s = getenv("JAMD_GMM_PULL_MIN")) g->pull_min = atoi(s);
  if (const char *s = getenv("JAMD_GMM_PULL_GRID")) g->pull_grid = atoi(s);
  // JAMD_GMM_PULL_TAIL = the tiles at the end of every share that are dealt in pieces (0: none, the deal of whole tiles;
  // unset: the default of launch_tile), JAMD_GMM_PULL_SUB = states of a piece (2, 4 or 8; measurement only).
  if (const char *s = getenv("JAMD_GMM_PULL_TAIL")) g->pull_tail = atoi(s) < 0 ? 0 : atoi(s);
  if (const char *s = getenv("JAMD_GMM_PULL_SUB")) { const int v = atoi(s); if (v == 2 || v == 4 || v == 8) g->pull_sub = v; }
  return JAMD_OK;
}

int jamd_gmm_launch_plain(jamd_gmm *g, const float *frames, int T, float *out, hipStream_t st) {
  // a handful of frames: one lane per mixture entry instead of one lane per frame (K1n above) -- where there is an
  // entry (a model whose plain states are all empty has none: K1 writes their LOG_ZERO) and a templated vector length
  const bool narrow = T <= kNarrowT && g->E_plain > 0;
  return dispatch_veclen(g->D, [&](auto dt) {
    constexpr int D = decltype(dt)::value;
    if constexpr (D == 0) return launch_tile_generic<2, 16>(g, frames, T, out, st);
    else return narrow ? launch_narrow<D>(g, frames, T, out, st) : launch_tile<D, 2, 16>(g, frames, T, out, st);
  });
}

int jamd_gmm_launch_dens(jamd_gmm *g, const float *rec, int E, const float *frames, int T, float *out, hipStream_t st) {
  const size_t lds = sizeof(float) * ((size_t)g->D * 64 + 64 * 17);
  if (lds > 64 * 1024) { jamd_set_error("jamd_gmm_dens_dev: vector length %d too large", g->D); return JAMD_EINVAL; }
  hipLaunchKernelGGL(gmm_dens_kernel, dim3((T + 63) / 64, (E + kDensChunk - 1) / kDensChunk), dim3(64), lds, st,
                     rec, frames, out, T, E, g->D, g->rec);
  return JAMD_OK;
}
