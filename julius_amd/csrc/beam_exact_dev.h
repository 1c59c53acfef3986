// beam_exact_dev.h -- what the two frame kernels of the exact-order first pass share on the device: K6x
// (beam_exact_kernel, beam_exact.hip) and K6m (beam_exact_mp_kernel, beam_exact_mp.h).  The workgroup's static LDS
// (XShared), the Viterbi cells and the candidate push, block scans, the survivors' two homes (XSv), the kernel
// arguments read where they are used (XKArgs / xargs_now()), the slice macros, and the parts of the kernel body both
// frames carry: the per-frame views of the launch constants, the kernel's entry, the score row request and the end
// (streaming park, find_1pass_result(), trace_backptr()).  Those parts are macros: each reads and writes a dozen of
// the kernel's locals, and as text they leave the instruction stream of either kernel as it was.
// Included by beam_prune.h (the pruning step is written on these helpers); everything sits in the anonymous namespace
// of the including translation unit.  Self-sufficient.
#pragma once
#include <type_traits>

#include "beam_common.h"
#include "beam_exact.h"

namespace {
using namespace jamdb;


#ifndef JAMD_XBEAM_CB
#define JAMD_XBEAM_CB 4                 // tokens per thread carried together through the finalize step
#endif
// The instrumented instantiation (JAMD_BEAM_TIMING=1) reports the four steps of a frame and the four parts of the
// pruning step in phase_us[0..7].  Finer probes exist only in development builds (-DJAMD_DEV, tools/build_variant.sh,
// tools/exact_probe.sh): JAMD_XBEAM_PROBE = 1 / 2 / 3 / 5 puts the sub-step clocks of steps 0-B / step C / the event
// replay / heap fill + heapify into phase_us[4..7] instead; 4 reports the shader clock (MHz) in phase_us[7].
#if !defined(JAMD_DEV) || !defined(JAMD_XBEAM_PROBE)
#undef JAMD_XBEAM_PROBE
#define JAMD_XBEAM_PROBE 0
#endif

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

struct XRowRef {                 // this frame's score row: its LDS copy or the row in global memory
  const float *g; const lds_f32 *l; bool lds;
  __device__ __forceinline__ float operator[](int i) const { return lds ? l[i] : g[i]; }
};

struct XShared {
  unsigned long long we_best;            // (ord(score + wordend_a), ~j): best word end, earliest visit
  int n_new, n_we, n_arc, n_atom, n_surv, best_atom, nB, i_last;
  unsigned maxbits, minbits;
  unsigned sel_digit, sel_need, sel_count;
  unsigned wsum[NT / 64], wsum2[NT / 64];
  int scan_total, scan_total2;
  int sw_nev, sw_limit, sw_fail, sw_changed, sw_ncl;     // the sweep replay (beam_sweep.h)
  int sw_ticks, sw_nev_out, sw_prof[8];
  int pst[16];                                   // this launch's share of jamd_beam_prune_stats(): kept here, added to the slice once at the end                      // its duration (100 MHz ticks), events held at the end
  int sw_info;                                   // last pruning step: rounds of the sweep replay, -1 = it gave up, 0 = not used
  int df_prof[4];                                // down_finish(): load, dependencies, sifts, output (100 MHz ticks; development)
  unsigned emaxbits;                             // multipath frame: best score among the tokens on emitting nodes (the score-pruning envelope)
  unsigned long long ph[8];                      // phase clocks of the instrumented instantiation (JAMD_BEAM_TIMING=1)
};

struct XCells {
  unsigned char *ub; unsigned o_nodekey, o_nodefirst, o_touched;
  lds_u64 *lkey; lds_i32 *lnode; lds_u32 *lfirst;
  int nslot;
};
#ifndef JAMD_XPROBES
#define JAMD_XPROBES 24
#endif
constexpr int kXProbes = JAMD_XPROBES;
// The probe loop of a cell insert is left to the compiler, which unrolls it fully into 24 nested conditionals: kept as ONE
// loop it saves 370 scalar spill slots and a sixth of the code but pays its mask bookkeeping on every insert -- 2.5 - 3 %
// slower on every configuration, measured in round 5 (profiles/r05b_ab_register_diet.txt) as in round 3.  Static spill
// counts are not run time.

// The thread index as a value the optimiser cannot carry from one frame to the next.  Everything derived from it (lane
// and wave numbers, per-thread addresses into a dozen arrays) is loop-invariant over the frame loop; hoisted, those
// values cost more registers than the kernel has and come back from scratch memory in the middle of serial sections.
// Recomputing them where they are used is a few VALU instructions.
__device__ __forceinline__ int tid_now() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  __builtin_assume(t >= 0 && t < 1024);
  return t;
}

// block-wide exclusive scan of one int per thread (two barriers); total in sh.scan_total
template <int NT>
__device__ __forceinline__ int block_excl_scan(XShared &sh, int v) {
  const int tx = tid_now(), lane = tx & 63, wv = tx >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) sh.wsum[wv] = (unsigned)incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wv; w++) base += (int)sh.wsum[w];
  if (tx == NT - 1) sh.scan_total = base + incl;
  __syncthreads();
  return base + incl - v;
}

// the same for two ints per thread (totals in sh.scan_total / sh.scan_total2)
template <int NT>
__device__ __forceinline__ void block_excl_scan2(XShared &sh, int a, int b, int &ea, int &eb) {
  const int tx = tid_now(), lane = tx & 63, wv = tx >> 6;
  int ia = a, ib = b;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int oa = __shfl_up(ia, off, 64), ob = __shfl_up(ib, off, 64);
    if (lane >= off) { ia += oa; ib += ob; }
  }
  if (lane == 63) { sh.wsum[wv] = (unsigned)ia; sh.wsum2[wv] = (unsigned)ib; }
  __syncthreads();
  int ba = 0, bb = 0;
  for (int w = 0; w < wv; w++) { ba += (int)sh.wsum[w]; bb += (int)sh.wsum2[w]; }
  if (tx == NT - 1) { sh.scan_total = ba + ia; sh.scan_total2 = bb + ib; }
  __syncthreads();
  ea = ba + ia - a; eb = bb + ib - b;
}

// A value every lane of the wave holds alike, moved to a scalar register: the compiler cannot know that a value read
// from LDS (or passed to a function that is not inlined) is uniform, and would run the loops it controls under
// execution masks.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
template <typename T>
__device__ __forceinline__ T JAMD_LDS *uni(T JAMD_LDS *p) {
  return (T JAMD_LDS *)(unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long)p);
}

__device__ __forceinline__ unsigned ordz(float f) { return ord(f + 0.0f); }   // -0.0 and +0.0 compare equal as floats

// Candidates for one node: key = the best of them (score bits || ~visiting index), nfirst = ~(their earliest
// visiting index).  propagate_token() :1945 with the visiting index as the tie breaker.
__device__ __forceinline__ void xpush_key(XShared &sh, const XCells &cl, int node, unsigned long long key, unsigned nfirst) {
  bool first = false;
  int slot = -1;
  if (cl.nslot > 0) {
    unsigned h = __umulhi((unsigned)node * 2654435761u, (unsigned)cl.nslot);
    for (int pr = 0; pr < kXProbes; pr++) {
      const int o = atomicCAS((int *)&cl.lnode[h], -1, node);
      if (o == -1 || o == node) { slot = (int)h; first = (o == -1); break; }
      h = (h + 1 == (unsigned)cl.nslot) ? 0u : h + 1;
    }
  }
  if (slot >= 0) {
    atomicMax((unsigned long long *)&cl.lkey[slot], key);
    atomicMax((unsigned *)&cl.lfirst[slot], nfirst);
  } else {
    const unsigned long long old =
        atomicMax(reinterpret_cast<unsigned long long *>(cl.ub + (unsigned)(cl.o_nodekey + 8u * (unsigned)node)), key);
    atomicMax(reinterpret_cast<unsigned *>(cl.ub + (unsigned)(cl.o_nodefirst + 4u * (unsigned)node)), nfirst);
    first = (old == 0ull);
  }
  const int s = wave_alloc(&sh.n_new, first);
  if (first) *reinterpret_cast<int2 *>(cl.ub + (unsigned)(cl.o_touched + 8u * (unsigned)s)) = make_int2(node, slot);
}
// one candidate
__device__ __forceinline__ void xpush(XShared &sh, const XCells &cl, int node, float score, unsigned vis) {
  if (score <= JAMD_LOG_ZERO) return;
  xpush_key(sh, cl, node, ((unsigned long long)ordz(score) << 32) | (unsigned)(~vis), ~vis);
}

// outprob_cd() with IWCD_NBEST (outprob.c:330-365): the mean of the K best member scores of a state set, `lps` lanes
// per set (a power of two, the lanes of a set adjacent).  Each lane keeps the K best of its members in descending
// order (insertion by max / min), the lanes merge in a butterfly; the sum runs from the best down as in the reference.
template <int K>
__device__ __forceinline__ float nbest_of_set(const LexDev &lx, const XRowRef &row, int a, int bnd, int sub, int lps) {
  float b[K];
#pragma unroll
  for (int i = 0; i < K; i++) b[i] = JAMD_LOG_ZERO;
  int n = 0;
  auto ins = [&](float p) {
#pragma unroll
    for (int i = 0; i < K; i++) { const float hi = __builtin_fmaxf(b[i], p); p = __builtin_fminf(b[i], p); b[i] = hi; }
  };
  for (int m = a + sub; m < bnd; m += 8 * lps) {
    int ix[8]; float pv[8];
#pragma unroll
    for (int jj = 0; jj < 8; jj++) ix[jj] = (m + lps * jj < bnd) ? lx.set_states(m + lps * jj) : -1;
#pragma unroll
    for (int jj = 0; jj < 8; jj++) pv[jj] = (ix[jj] >= 0) ? row[ix[jj]] : JAMD_LOG_ZERO;
#pragma unroll
    for (int jj = 0; jj < 8; jj++) { n += pv[jj] > JAMD_LOG_ZERO ? 1 : 0; ins(pv[jj]); }
  }
  for (int off = 1; off < lps; off <<= 1) {
    float c[K];
#pragma unroll
    for (int i = 0; i < K; i++) c[i] = __shfl_xor(b[i], off, 64);
    n += __shfl_xor(n, off, 64);
#pragma unroll
    for (int i = 0; i < K; i++) ins(c[i]);
  }
  if (n > lx.cdmax_num) n = lx.cdmax_num;
  float sum = 0.0f;
#pragma unroll
  for (int i = 0; i < K; i++) if (n > i) sum += b[i];
  return sum / (float)n;
}

// The survivors of the frame, in visiting order: in LDS (narrow layout) or in the utterance's slice (wide layout:
// steps 0 and A read them in order, only the winner look-ups of step C are gathers -- from L2).
template <bool WIDE> struct XSv;
template <> struct XSv<false> {
  lds_v4 *p;
  __device__ __forceinline__ Tok load(int j) const { return lds_tok_load(p, j); }
  __device__ __forceinline__ void store(int j, const Tok &t) const { lds_tok_store(p, j, t); }
  __device__ __forceinline__ void quads(int j, u32x4 &a, u32x4 &b) const { a = p[2 * j]; b = p[2 * j + 1]; }
};
template <> struct XSv<true> {
  u32x4 *p;
  __device__ __forceinline__ void quads(int j, u32x4 &a, u32x4 &b) const { a = p[2 * j]; b = p[2 * j + 1]; }
  __device__ __forceinline__ Tok load(int j) const {
    u32x4 a, b;
    quads(j, a, b);
    Tok t;
    t.node = (int)a.x; t.score = __uint_as_float(a.y); t.last_tre = (int)a.z; t.last_cword = (int)a.w;
    t.last_lscore = __uint_as_float(b.x); t.last_wid = (int)b.y; t.pad0 = (int)b.z; t.pad1 = (int)b.w;
    return t;
  }
  __device__ __forceinline__ void store(int j, const Tok &t) const {
    p[2 * j] = u32x4{(unsigned)t.node, __float_as_uint(t.score), (unsigned)t.last_tre, (unsigned)t.last_cword};
    p[2 * j + 1] = u32x4{__float_as_uint(t.last_lscore), (unsigned)t.last_wid, (unsigned)t.pad0, (unsigned)t.pad1};
  }
};

// ---- the kernel's arguments, read where they are used ------------------------------------------------------------
// LexDev + XWork are some 150 dwords of launch constants, and the frame loop derives another forty uniform addresses
// from them.  Taken as by-value parameters they are all loaded at the kernel's entry and stay live across the frame
// loop: the hardware has ~100 SGPRs, so the compiler parked a thousand of them in VGPR lanes (sgpr_spill_count 1 047 in
// round 4) and a sixth of the instruction stream was v_readlane / v_writelane.  They are constants of the KERNARG
// segment, which a wave can read at any time with a scalar load (scalar data cache): the first two parameters are one
// struct at offset 0 of that segment, and every frame re-derives its view of it from an address the compiler cannot see
// through (xargs_now(): the same device as tid_now() for the thread index), so that a value is loaded in the phase that
// uses it and dies there.  (The kernels' first parameter, ka_, is that struct: it is never named, it IS the segment.)
struct XKArgs { LexDev lx; XWork xw; };
__device__ __forceinline__ const XKArgs &xargs_now() {
  unsigned long long a = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return *(const XKArgs *)(const __attribute__((address_space(4))) XKArgs *)a;    // constant address space: scalar loads
}

// ---- the utterance's slice in global memory (ub = its base; wk / xw = the views below)
#define SLICE(T, off, i) (*reinterpret_cast<T *>(ub + (unsigned)((off) + (unsigned)sizeof(T) * (unsigned)(i))))
#define NODEKEY(i) SLICE(unsigned long long, wk.o_nodekey, i)
#define NODEFIRST(i) SLICE(unsigned, xw.o_nodefirst, i)
#define CUR(i) SLICE(Tok, wk.o_cur, i)
#define CURKEY(i) SLICE(unsigned, wk.o_cur_key, i)
#define REC(i) SLICE(u32x4, wk.o_cur + (unsigned)sizeof(Tok) * (unsigned)wk.tok_cap, i)   /* {node, visiting index of the winner, trellis word or -2, score bits} */
#define TOUCHED(i) SLICE(int2, wk.o_touched, i)
#define ARCQ(i) SLICE(int2, wk.o_arcq, i)
#define ATOM(i) SLICE(jamd_trellis_atom, wk.o_atoms, i)

// everything the frame loop derives from the launch constants (declares lx, xw, wk and the LDS / slice views): the part
// both kernels have; each adds its own lines (XBEAM_VIEWS in beam_exact.hip, XBEAM_MP_VIEWS in beam_exact_mp.h), two of
// them at the place they always had (AFTER_SV, AFTER_GCOL): the kernels sit on the register cliff, and the order of these
// declarations is the order in which the compiler first sees the loads (see PRUNE_MEM_FILL for what was tried).
// PruneMem / PRUNE_MEM_FILL: beam_prune.h.
#define XBEAM_VIEWS_COMMON(KA, LMT, AFTER_SV, AFTER_GCOL)                                                             \
  const LexDev &lx = (KA).lx; const XWork &xw = (KA).xw; const Work &wk = xw.w;                                       \
  XSv<WIDE> sv;                                            /* Tok[beam], two quads each */                            \
  if constexpr (WIDE) sv.p = reinterpret_cast<u32x4 *>(ub + wk.o_sv); else sv.p = (lds_v4 *)dyn_lds;                  \
  AFTER_SV                                                                                                            \
  lds_i32 *welist = (lds_i32 *)(dyn_lds + xw.off_we);      /* word ends of the frame; the pruning step returns its order here */ \
  lds_i32 *dbase = (lds_i32 *)(dyn_lds + xw.off_dbase);    /* [beam + 2] first dense visiting index of each source */ \
  lds_u32 *tpre = (lds_u32 *)(dyn_lds + xw.off_tpre);                                                                 \
  XCells cl;                                                                                                          \
  cl.ub = ub; cl.o_nodekey = wk.o_nodekey; cl.o_nodefirst = xw.o_nodefirst; cl.o_touched = wk.o_touched;              \
  cl.nslot = xw.nslot;                                                                                                \
  cl.lkey = (lds_u64 *)(dyn_lds + xw.off_cells);                                                                      \
  cl.lnode = (lds_i32 *)(dyn_lds + xw.off_lnode);                                                                     \
  cl.lfirst = (lds_u32 *)(dyn_lds + xw.off_lfirst);                                                                   \
  lds_f32 *rowc = (lds_f32 *)(dyn_lds + xw.off_row);                                                                  \
  PruneMem pm;                                                                                                        \
  PRUNE_MEM_FILL(pm, xw, dyn_lds, xw.o_sweep ? ub + xw.o_sweep : nullptr, xw.o_sweep ? sh.pst : nullptr);  /* (pstat: a generic pointer to LDS, a handful of accesses per frame) */ \
  lds_u64 *Hlds = (lds_u64 *)(dyn_lds + xw.off_heap);                                                                 \
  unsigned long long *Hglob = reinterpret_cast<unsigned long long *>(ub + xw.o_heap);                                 \
  u32x4 *Gcol = reinterpret_cast<u32x4 *>(ub + xw.o_collect);                                                         \
  AFTER_GCOL                                                                                                          \
  const float lmw = lx.lm_weight, pen = lx.lm_penalty;                                                                \
  const int lmt = (LMT);                                   /* K6m masks the multipath flag off */                     \
  const bool dfa = lmt != JAMD_LM_NGRAM;                                                                              \
  const bool wordmode = lmt == JAMD_LM_WORD;                                                                          \
  unsigned long long *memo = reinterpret_cast<unsigned long long *>(ub + wk.o_lmcache);                               \
  const int s1 = xw.s1, XW = xw.xw;                                                                                   \
  const unsigned submask = (1u << s1) - 1u;                                                                           \
  const int nroot_x = wordmode ? 0 : (dfa ? lx.startnum : lx.isolatenum);                                             \
  (void)welist; (void)dbase; (void)tpre; (void)rowc; (void)Hlds; (void)Hglob; (void)Gcol; (void)lmw; (void)pen;       \
  (void)memo; (void)XW; (void)submask; (void)nroot_x; (void)wordmode; (void)pm

// The kernel's entry: utterance pick (longest first, clamped), stream state, the slice, the views (the kernel's own
// macro), this launch's pruning statistics.  Declares sh, dyn_lds, ka0, u, tid, t_begin, nrows, ss, resume, base, T,
// finish, ub, res, pstat_glob.
#define XBEAM_ENTRY(VIEWS)                                                                                            \
  __shared__ XShared sh;                                                                                              \
  extern __shared__ __align__(16) unsigned char dyn_lds[];                                                            \
  const XKArgs &ka0 = xargs_now();                                                                                    \
  if (threadIdx.x == 0 && ka0.xw.w.resident) __hip_atomic_fetch_add(ka0.xw.w.resident, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  /* this workgroup holds its share of a CU now */ \
  const int u = min(max(utt_off[gridDim.x + 1 + blockIdx.x], 0), (int)gridDim.x - 1);  /* longest utterance first (upload_utt_off()); clamped: never outside the launch's slices */ \
  int tid = threadIdx.x;  /* refreshed every frame: see tid_now() */                                                  \
  const int t_begin = utt_off[u], nrows = utt_off[u + 1] - t_begin;                                                   \
  StreamState *ss = smode ? ka0.xw.w.stream + u : nullptr;                                                            \
  const bool resume = smode && ss->started;                                                                           \
  const int base = resume ? ss->frames_done : 0;                                                                      \
  const int T = base + nrows;                                                                                         \
  const bool finish = smode != 1;                                                                                     \
  unsigned char *const ub = ka0.xw.w.slices + (size_t)u * ka0.xw.w.utt_stride;                                        \
  jamd_pass1_result *res = ka0.xw.w.res + u;                                                                          \
  VIEWS(ka0);                                                                                                         \
  int *const pstat_glob = xw.o_sweep ? reinterpret_cast<int *>(ub + xw.o_pstat) : nullptr;                            \
  if (tid == 0) for (int i = 0; i < 16; i++) sh.pst[i] = 0;

// A later launch of a streaming session: nothing to do for an utterance that has stopped; else the parked survivors
// come back (narrow layout).  EXTRA: the kernel's own statement in front of the barrier.
#define XBEAM_RESUME(EXTRA)                                                                                           \
    if (!ss->active) return;                                                                                          \
    if constexpr (!WIDE) {                                                                                            \
      const u32x4 *src = (const u32x4 *)(ub + wk.o_sv);                                                               \
      for (int i = tid; i < wk.sv_bytes / 16; i += NT) sv.p[i] = src[i];                                              \
    }                                                                                                                 \
    if (tid == 0) { sh.n_atom = ss->n_atom; sh.n_surv = ss->n_surv; }                                                 \
    EXTRA;                                                                                                            \
    __syncthreads();

// A new utterance: result reset, LM memo clear, the kernel's own EXTRA, and the exit of an utterance without rows.
#define XBEAM_RESET(EXTRA)                                                                                            \
    if (tid == 0) {                                                                                                   \
      sh.n_atom = 0; sh.n_surv = 0;                                                                                   \
      res->status = JAMD_PASS1_OK; res->natom = 0; res->wnum = 0; res->score = JAMD_LOG_ZERO;                         \
      res->died_at = -1; res->ties = 0; res->ties_node = 0; res->ties_wordend = 0; res->ties_cut = 0;                 \
      res->frames = T; res->max_tokens = 0;                                                                           \
      for (int i = 0; i < 8; i++) res->phase_us[i] = 0;                                                               \
    }                                                                                                                 \
    for (int i = tid; i < wk.nscword; i += NT) memo[i] = 0xffffffff00000000ull;                                       \
    EXTRA;                                                                                                            \
    __syncthreads();                                                                                                  \
    if (nrows <= 0) {                                                                                                 \
      if (tid == 0) { if (smode != 1) res->status = JAMD_PASS1_FAIL; if (ss) { ss->started = 0; ss->active = 1; } }   \
      return;                                                                                                         \
    }

// the score envelope, the phase clocks (in LDS: eight 64-bit counters in registers cost 16 VGPRs the kernels do not have),
// the token high-water mark
#define XBEAM_LOOP_STATE()                                                                                            \
  float thr = resume ? ss->thr : JAMD_LOG_ZERO;                                                                       \
  unsigned long long *const ph = sh.ph;                                                                               \
  if (TIMED && threadIdx.x == 0) for (int i = 0; i < 8; i++) sh.ph[i] = 0ull;                                         \
  unsigned long long tc = wall_clock64(), tc2 = tc;                                                                   \
  (void)tc2;                                                                                                          \
  int max_tokens = resume ? ss->max_tokens : 1;                                                                       \
  bool stopped = false;

  // The frame's score row goes to LDS by LDS-DMA (no registers, nothing waits on it): the row of frame t + 1 is
  // requested when step C of frame t is done with the buffer, and has landed by the pruning step's first barrier.
#define XBEAM_ROW_REQUEST()                                                                                           \
  auto row_request = [&](int tt) {                                                                                    \
    if (!wk.row_cache || tt >= T) return;                                                                             \
    const float *rg = scores + (size_t)(t_begin + tt - base) * S;                                                     \
    const int ln = tid & 63;                                                                                          \
    for (int b = uni((int)(tid >> 6)) * 64; b < S; b += NT)                                                           \
      if (b + ln < S) __builtin_amdgcn_global_load_lds((glb_void *)(rg + b + ln), (lds_void *)(rowc + b), 4, 0, 0);   \
  }

// The end of the kernel.  A push of a streaming session that is not the last parks the survivors and the stream state
// (WIDE_PARK: what the wide layout has to do for that -- K6x moves its survivors home); otherwise find_1pass_result()
// :399-455 (grammar / word list: the best word on the latest frame that has one, the smaller id among equals as rw[t] is
// sorted by word id; N-gram: the tail-silence word ending latest) and trace_backptr() :294-340.  PROBE4: K6x's
// shader-clock probe (development builds).
#define XBEAM_END(WIDE_PARK, PROBE4)                                                                                  \
  if (smode == 1) {                                                                                                   \
    if constexpr (!WIDE) {                                                                                            \
      if (!stopped) {                                                                                                 \
        u32x4 *dst = (u32x4 *)(ub + wk.o_sv);                                                                         \
        for (int i = tid; i < wk.sv_bytes / 16; i += NT) dst[i] = sv.p[i];                                            \
      }                                                                                                               \
    } else {                                                                                                          \
      WIDE_PARK                                                                                                       \
    }                                                                                                                 \
    if (tid == 0) {                                                                                                   \
      ss->started = 1; ss->active = stopped ? 0 : 1; ss->frames_done = T; ss->n_surv = sh.n_surv; ss->thr = thr;      \
      ss->n_atom = sh.n_atom; ss->ties = 0; ss->ties_we = 0; ss->ties_cut = 0;                                        \
      ss->max_tokens = max_tokens;                                                                                    \
      res->natom = min(sh.n_atom, wk.atom_cap); res->frames = T; res->max_tokens = max_tokens;                        \
      res->ties = 0;                                                                                                  \
      if (TIMED) for (int i = 0; i < 8; i++) res->phase_us[i] += (int)(ph[i] / 100ull);                               \
      if (pstat_glob) for (int i = 0; i < 16; i++) pstat_glob[i] += sh.pst[i];                                        \
    }                                                                                                                 \
    return;                                                                                                           \
  }                                                                                                                   \
  if (ss && tid == 0) { ss->active = 0; ss->started = 1; ss->frames_done = T; }                                       \
                                                                                                                      \
  /* ---- find_1pass_result() :399-431 + trace_backptr() :294-340 */                                                  \
  const int natom = min(sh.n_atom, wk.atom_cap);                                                                      \
  if (tid == 0) sh.best_atom = -1;                                                                                    \
  __syncthreads();                                                                                                    \
  if (res->status == JAMD_PASS1_OK && dfa) {                                                                          \
    /* grammar / word list (:433-455): the best word on the latest frame that has one.  The reference walks rw[t], which */ \
    /* bt_sort_rw() has sorted by word id, with a strict <: of equally good words the smaller id wins -- the key below. */ \
    if (tid == 0) { sh.n_arc = -1; sh.we_best = 0ull; }                                                               \
    __syncthreads();                                                                                                  \
    int lt = -1;                                                                                                      \
    for (int i = tid; i < natom; i += NT)                                                                             \
      if (ATOM(i).backscore > JAMD_LOG_ZERO && ATOM(i).endtime > lt) lt = ATOM(i).endtime;                            \
    if (lt >= 0) atomicMax(&sh.n_arc, lt);                                                                            \
    __syncthreads();                                                                                                  \
    lt = sh.n_arc;                                                                                                    \
    for (int i = tid; i < natom; i += NT)                                                                             \
      if (ATOM(i).endtime == lt && ATOM(i).backscore > JAMD_LOG_ZERO)                                                 \
        atomicMax(&sh.we_best, ((unsigned long long)ord(ATOM(i).backscore) << 32) | (0xffffffffu - (unsigned)ATOM(i).wid)); \
    __syncthreads();                                                                                                  \
    const unsigned long long kb = sh.we_best;                                                                         \
    for (int i = tid; i < natom; i += NT)                                                                             \
      if (kb != 0ull && ATOM(i).endtime == lt && (unsigned)ATOM(i).wid == 0xffffffffu - (unsigned)kb &&               \
          ord(ATOM(i).backscore) == (unsigned)(kb >> 32)) sh.best_atom = i;                                           \
  } else if (res->status == JAMD_PASS1_OK) {                                                                          \
    /* the tail-silence word ending latest; atoms of one frame are emitted together, so "latest" is */                \
    /* decided on the end time, not on the index */                                                                   \
    int bt = -1;                                                                                                      \
    for (int i = tid; i < natom; i += NT)                                                                             \
      if (ATOM(i).wid == lx.tail_silwid && ATOM(i).backscore > JAMD_LOG_ZERO && ATOM(i).endtime > bt) bt = ATOM(i).endtime; \
    if (tid == 0) sh.n_arc = -1;                                                                                      \
    __syncthreads();                                                                                                  \
    if (bt >= 0) atomicMax(&sh.n_arc, bt);                                                                            \
    __syncthreads();                                                                                                  \
    bt = sh.n_arc;                                                                                                    \
    for (int i = tid; i < natom; i += NT)                                                                             \
      if (bt >= 0 && ATOM(i).wid == lx.tail_silwid && ATOM(i).backscore > JAMD_LOG_ZERO && ATOM(i).endtime == bt) sh.best_atom = i; \
  }                                                                                                                   \
  __syncthreads();                                                                                                    \
  if (tid == 0) {                                                                                                     \
    res->natom = natom; res->ties = 0; res->max_tokens = max_tokens;                                                  \
    res->ties_node = 0; res->ties_wordend = 0; res->ties_cut = 0;                                                     \
    if (pstat_glob) for (int i = 0; i < 16; i++) pstat_glob[i] += sh.pst[i];                                          \
    if (TIMED) for (int i = 0; i < 8; i++) res->phase_us[i] += (int)(ph[i] / 100ull);                                 \
    PROBE4                                                                                                            \
    res->frames = T;                                                                                                  \
    if (sh.n_atom > wk.atom_cap) res->status = JAMD_PASS1_OVERFLOW;                                                   \
    if (res->status == JAMD_PASS1_OK) {                                                                               \
      const int best = sh.best_atom;                                                                                  \
      if (best < 0) res->status = JAMD_PASS1_FAIL;                                                                    \
      else {                                                                                                          \
        int n = 0, a = best;                                                                                          \
        int rev[MAXSEQ];                                                                                              \
        rev[n++] = ATOM(a).wid;                                                                                       \
        while (ATOM(a).begintime > 0 && n < MAXSEQ) { a = ATOM(a).last_tre; rev[n++] = ATOM(a).wid; }                 \
        for (int k = 0; k < n; k++) res->wseq[k] = rev[n - 1 - k];                                                    \
        res->wnum = n; res->score = ATOM(best).backscore;                                                             \
      }                                                                                                               \
    }                                                                                                                 \
  }

}  // namespace
