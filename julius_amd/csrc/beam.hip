// beam.hip -- first-pass token passing over the tree lexicon (K6) for gfx950.
//
// Replaces, for a BATCH of utterances in one launch, the reference's
//   get_back_trellis_init()     libjulius/src/beam.c:1825  (+ init_nodescore :1552)
//   get_back_trellis_proceed()  beam.c:2663   (non-multipath branch :2832-2900)
//     beam_intra_word()/_core() beam.c:2154 / :2004
//     save_trellis()            beam.c:2209
//     beam_inter_word()         beam.c:2271
//     beam_inter_word_factoring beam.c:2549
//     sort_token_no_order()     beam.c:1492   (rank pruning)
//   get_back_trellis_end()      beam.c:3052
//   find_1pass_result()         beam.c:372    (+ trace_backptr :294)
// and their callees outprob_style() (outprob_style.c:354), max_successor_prob()
// / max_successor_prob_iw() (factoring_sub.c:942 / :1049) and the 2-gram access
// functions (libsent/src/ngram/ngram_access.c:225-403).
//
// Execution model: ONE WORKGROUP PER UTTERANCE, persistent over all frames of
// that utterance (the trellis is serial in t; utterances are independent, so a
// batch fills the chip).  Per frame:
//   A  every surviving token pushes its intra-word candidates, emits a trellis
//      atom if it sits on a word end and records itself in the word-end list;
//   B  word ends x isolated roots (2-gram) and best word end x shared roots
//      (1-gram factoring) push the cross-word candidates;
//   C  one thread per touched node takes the winner, rebuilds its payload from
//      the winning candidate id, adds the acoustic score, tracks the frame max;
//   D  rank pruning: radix select of the beam_width-th score + compaction.
// "push" is a 64-bit atomicMax on the node's Viterbi cell = (order-preserving score bits,
// candidate id): the Viterbi max of propagate_token() (beam.c:1945) without any
// ordering between candidates.  The cells of the frame being built live in an LDS hash
// table keyed by node (struct Cells; nodekey[] in global memory is its overflow).  The
// thread that claims a cell registers the node in the frame's touched list, step C
// empties the cell again, so both tables are clean after every frame without a clearing
// sweep (what clear_tokens(), beam.c:1122, does on the CPU).
// Grammar (per-category trees) and isolated-word recognition run through the same kernel
// (lx.lm_type): initial tokens enter through steps C and D of a pseudo frame 0, step B
// becomes word ends x all roots with the category-pair test, or nothing at all.
//
// Determinism / parity: every float is produced by the same sequence of fp32
// operations as the reference (this file is compiled with -ffp-contract=off).
// The only freedom is the visiting order, which matters only when two candidates
// for the same node, two word ends, or two tokens at the rank cut have EXACTLY
// equal scores; every such event is counted in jamd_pass1_result.ties.  With
// ties == 0 the trellis is the reference's trellis bit for bit.
//
// This file holds the kernel and the host functions that know its LDS image (fbeam_layout / fbeam_prepare /
// fbeam_launch, beam_host.h).  The work area and the C ABI are beam_api.hip's, the lexicon is beam_lexicon_api.hip's.
#include "jamd_device.h"
#include <type_traits>
#include <algorithm>

#include "beam_host.h"

namespace {
using namespace jamdb;
// candidate ids (low 32 bits of a node key) name the SOURCE of the transition, in
// terms that do not depend on any scheduling order, so that (score, id) is a
// canonical total order and the result is deterministic:
//   intra-word     bit31 = 0            [30:0] = source node
//   isolated root  bits[31:30] = 10     [29:0] = the word that ended (its end node is unique);
//                                       with a grammar every root is entered this way
//   shared root    bits[31:30] = 11     (the source is the frame's best word end);
//                                       with a grammar: [29:0] = index of an initial token
// The destination is the address of the key, so the arc is implied.
// Returns the previous key when it holds the SAME score as this candidate (an
// exact tie), else 0.
// Where the Viterbi cells of the frame being built live.  A frame touches a few thousand of the
// lexicon's 10^5..10^6 nodes; with hundreds of utterances in flight the direct-indexed nodekey[]
// tables (2 MB each) fall out of every cache and each push becomes a random DRAM read-modify-write.
// The cells therefore live in an LDS hash table keyed by node (open addressing, claimed with a CAS
// on the node word); a node whose probe window is full overflows to nodekey[] -- occupancy only
// grows within a frame, so every candidate of a node resolves to the same place.
struct Cells {
  unsigned char *ub;             // this utterance's slice: nodekey[] (overflow, and everything when nslot == 0), touched[]
  unsigned o_nodekey, o_touched;
  unsigned long long *lkey;      // [nslot] LDS cells (0 = empty)
  int *lnode;                    // [nslot] owning node (-1 = free)
  int nslot, shift;              // nslot = 1 << (32 - shift)
};
constexpr int kCellProbes = 24;

__device__ __forceinline__ unsigned long long push(Shared &sh, const Cells &cl, int node, float score, unsigned id) {
  if (score <= JAMD_LOG_ZERO) return 0ull;                    // propagate_token() :1951
  const unsigned long long key = ((unsigned long long)ord(score) << 32) | id;
  unsigned long long old;
  bool first;
  int slot = -1;
  if (cl.nslot > 0) {
    unsigned h = ((unsigned)node * 2654435761u) >> cl.shift;
    for (int pr = 0; pr < kCellProbes; pr++) {
      const int o = atomicCAS(&cl.lnode[h], -1, node);
      if (o == -1 || o == node) { slot = (int)h; first = (o == -1); break; }
      h = (h + 1) & (unsigned)(cl.nslot - 1);
    }
  }
  if (slot >= 0) {
    old = atomicMax(&cl.lkey[slot], key);
  } else {
    old = atomicMax(reinterpret_cast<unsigned long long *>(cl.ub + (unsigned)(cl.o_nodekey + 8u * (unsigned)node)), key);
    first = (old == 0ull);
  }
  const int s = wave_alloc(&sh.n_new, first);
  if (first) *reinterpret_cast<int2 *>(cl.ub + (unsigned)(cl.o_touched + 8u * (unsigned)s)) = make_int2(node, slot);
  // old == 0: nothing stored in the cell yet (the slot's claimer may still be on its way; it will
  // then see this key as its `old`, so no tie goes unnoticed)
  return (old != 0ull && (unsigned)(old >> 32) == (unsigned)(key >> 32) && old != key) ? old : 0ull;
}

// TIMED adds per-phase wall clocks (jamd_pass1_result.phase_us, thread 0; development aid selected
// with JAMD_BEAM_TIMING=1 when the work area is created) -- they cost some 20 VGPRs, so the
// production instantiation carries none.
#ifndef JAMD_BEAM_CB
#define JAMD_BEAM_CB 4                  // tokens per thread carried together through the finalize step
#endif
#ifndef JAMD_BEAM_WPE
#define JAMD_BEAM_WPE 4                 // waves per SIMD the register allocation targets (4 = one workgroup per CU)
#endif
template <bool TIMED, bool SVLDS>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(JAMD_BEAM_WPE, JAMD_BEAM_WPE)))
beam_pass1_kernel(LexDev lx, Work wk, const float *__restrict__ scores, int S,
                  const int *__restrict__ utt_off, int smode) {
  __shared__ Shared sh;
  extern __shared__ __align__(16) unsigned char dyn_lds[];
  const int u = blockIdx.x, tid = threadIdx.x;
  if (tid == 0 && wk.resident) __hip_atomic_fetch_add(wk.resident, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // this workgroup holds its CU now
  // smode 0: whole utterances.  smode 1 / 2: streaming -- this launch advances every utterance
  // by the rows utt_off[u]..utt_off[u+1]) of `scores`; 2 = also run get_back_trellis_end() and
  // the traceback.  The state between launches lives in wk.stream[u] and in the slice at o_sv.
  const int t_begin = utt_off[u], nrows = utt_off[u + 1] - t_begin;
  StreamState *ss = smode ? wk.stream + u : nullptr;
  const bool resume = smode && ss->started;
  const int base = resume ? ss->frames_done : 0;            // absolute index of this launch's first row
  const int T = base + nrows;                                // frames seen so far
  const bool finish = smode != 1;                            // run the end phase after the last row
  unsigned char *const ub = wk.slices + (size_t)u * wk.utt_stride;     // this utterance's slice
#define SLICE(T, off, i) (*reinterpret_cast<T *>(ub + (unsigned)((off) + (unsigned)sizeof(T) * (unsigned)(i))))
#define NODEKEY(i) SLICE(unsigned long long, wk.o_nodekey, i)
#define CUR(i) SLICE(Tok, wk.o_cur, i)
#define CURKEY(i) SLICE(unsigned, wk.o_cur_key, i)
#define TOUCHED(i) SLICE(int2, wk.o_touched, i)
#define ARCQ(i) SLICE(int2, wk.o_arcq, i)            /* extra arcs of this frame's survivors: (survivor, arc) */
#define ATOM(i) SLICE(jamd_trellis_atom, wk.o_atoms, i)
  jamd_pass1_result *res = wk.res + u;
  // survivor state of the previous frame (tokens, the atom each word end emitted, the
  // frame's word-end list, node -> survivor hash)
  SvImage<SVLDS> svi;                       // SVLDS == (wk.use_lds != 0): chosen at launch
  svi.bind(dyn_lds, ub + wk.o_sv, wk.beam, wk.hsize);
  const auto sv_atom = svi.atom;
  const auto welist = svi.we;
  const auto hkey = svi.hkey;
  const auto hval = svi.hval;
  const int hmask = wk.hsize - 1;
  // the frame's Viterbi cells: LDS table behind the survivor image (16-byte aligned), see Cells
  Cells cl;
  cl.ub = ub; cl.o_nodekey = wk.o_nodekey; cl.o_touched = wk.o_touched; cl.nslot = SVLDS ? wk.cell_slots : 0;
  cl.lkey = (unsigned long long *)(dyn_lds + wk.cell_off);
  cl.lnode = (int *)(dyn_lds + wk.node_off);
  unsigned *hist = (unsigned *)(dyn_lds + wk.cell_off);    // step D only: the cells are all empty then
  float *rowc = (float *)(dyn_lds + wk.row_off);           // this frame's score row when wk.row_cache
  cl.shift = cl.nslot > 0 ? 32 - (31 - __clz(cl.nslot)) : 0;
  for (int i = tid; i < cl.nslot; i += NT) { cl.lkey[i] = 0ull; cl.lnode[i] = -1; }
  const float lmw = lx.lm_weight, pen = lx.lm_penalty;
  const bool dfa = lx.lm_type != JAMD_LM_NGRAM;          // grammar or word list: initial-token frame, no factoring
  const bool wordmode = lx.lm_type == JAMD_LM_WORD;      // isolated words: no cross-word transition at all
  unsigned long long *memo = reinterpret_cast<unsigned long long *>(ub + wk.o_lmcache);

  if (resume) {
    if (!ss->active) return;                                 // died / overflowed / finished earlier
    if (SVLDS) {                                             // survivor image back into LDS
      const u32x4 *src = (const u32x4 *)(ub + wk.o_sv);
      lds_v4 *dst = (lds_v4 *)dyn_lds;
      for (int i = tid; i < wk.sv_bytes / 16; i += NT) dst[i] = src[i];
    }
    if (tid == 0) {
      sh.n_atom = ss->n_atom; sh.ties = ss->ties; sh.ties_we = ss->ties_we; sh.ties_cut = ss->ties_cut;
      sh.n_surv = ss->n_surv;
    }
    __syncthreads();
  } else {
    if (tid == 0) {
      sh.n_atom = 0; sh.ties = 0; sh.ties_we = 0; sh.ties_cut = 0; sh.n_surv = 0;
      res->status = JAMD_PASS1_OK; res->natom = 0; res->wnum = 0; res->score = JAMD_LOG_ZERO;
      res->died_at = -1; res->ties = 0; res->frames = T; res->max_tokens = 0;
      for (int i = 0; i < 8; i++) res->phase_us[i] = 0;
    }
    for (int i = tid; i < wk.hsize; i += NT) hkey[i] = -1;
    for (int i = tid; i < wk.nscword; i += NT) memo[i] = 0xffffffff00000000ull;   // context -1: never matches
    __syncthreads();
    if (nrows <= 0) {                                        // nothing to start from yet
      if (tid == 0) { if (smode != 1) res->status = JAMD_PASS1_FAIL; if (ss) { ss->started = 0; ss->active = 1; } }
      return;
    }
    // ---- get_back_trellis_init(): the silB head token (init_nodescore, beam.c:1622-1665).
    // With a grammar the initial tokens (one per word that may start a sentence, :1669-1757)
    // enter through the finalize and rank-pruning steps of a pseudo frame 0 below.
    if (tid == 0 && !dfa) {
      const int node = lx.word_head(lx.head_silwid);
      const int4 nr = lx.node_b(node);                 // {stend, scid, out_id, out_kind}
      Tok nw;
      float ls = (nr.y != 0) ? max_successor_prob(lx, -1, nr.y) : 0.0f;
      ls = ls * lmw + pen;
      nw.node = node; nw.last_tre = -1; nw.last_cword = -1; nw.last_wid = -1; nw.last_lscore = ls;
      nw.score = node_outprob(lx, scores + (size_t)t_begin * S, nr.w, nr.z, -1) + ls;
      nw.pad0 = nw.pad1 = 0;
      svi.store(0, nw);
      hash_put(hkey, hval, hmask, node, 0);
      sh.n_surv = 1;
    }
  }
  float thr = resume ? ss->thr : JAMD_LOG_ZERO;        // d->score_pruning_threshold (beam.c:1935)
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tc = wall_clock64(), tq = 0;   // phase clocks (100 MHz), thread 0 only
#define PHASE(i) do { if (TIMED && tid == 0) { const unsigned long long n_ = wall_clock64(); ph[i] += n_ - tc; tc = n_; } } while (0)
  int max_tokens = resume ? ss->max_tokens : 1;
  bool stopped = false;
  __syncthreads();

  // frames base+1 .. T-1 of this launch are propagated into (frame `base` itself when resuming);
  // t == T is the end phase and only runs when finishing
  for (int t = resume ? base : (dfa ? 0 : 1); t <= (finish ? T : T - 1); t++) {
    // tl/tn swap (beam.c:2697-2698): sv[] holds last frame's survivors
    const int n_surv = sh.n_surv;
    __syncthreads();
    if (tid == 0) { sh.n_new = 0; sh.n_we = 0; sh.n_arc = 0; sh.we_best = 0ull; sh.maxbits = ord(JAMD_LOG_ZERO); sh.minbits = 0xffffffffu; }
    __syncthreads();
    const bool last = (t == T);     // get_back_trellis_end(): word ends only, no pruning test
    if (wk.row_cache && !last) {    // readers: step C of this frame, two barriers from here
      const float *__restrict__ rg = scores + (size_t)(t_begin + t - base) * S;
      for (int i = tid; i < S; i += NT) rowc[i] = rg[i];
    }

    // one intra-word candidate of token tk: score, LM factoring update, push, tie accounting
    auto intra_candidate = [&](const Tok &tk, int next_node, float a) {
      const int node = tk.node;
      float tmpsum = tk.score + a;
      const int nscid = (next_node != node) ? lx.scid(next_node) : 0;
      const bool fac = nscid != 0;
      if (fac) {
        const float ng = max_successor_prob(lx, tk.last_cword, nscid, memo) * lmw + pen;
        tmpsum -= tk.last_lscore;
        tmpsum += ng;
      }
      const unsigned long long tie = push(sh, cl, next_node, tmpsum, (unsigned)node);
      if (tie != 0ull) {
        // two different sources reach next_node with exactly the same score.
        // Harmless when both carry the same history (same predecessor atom, context
        // word and LM score) -- merging tree branches produce that; anything else is
        // a genuine tie, resolved by the larger source id and counted.
        bool same = false;
        if (((unsigned)tie >> 31) == 0u) {
          const Tok o = svi.load(hash_get(hkey, hval, hmask, (int)(unsigned)tie));
          // the LM score is recomputed from last_cword on entering a factoring
          // node from another node (see step C); otherwise it is inherited
          const bool re_o = next_node != o.node && lx.scid(next_node) != 0;
          same = o.last_tre == tk.last_tre && o.last_cword == tk.last_cword &&
                 (fac == re_o) && (fac || o.last_lscore == tk.last_lscore);
        }
        if (!same) atomicAdd(&sh.ties, 1);
      }
    };
    // ---- A: intra-word transitions + word-end atoms (main loop, beam.c:2838-2900)
    for (int j = tid; j < n_surv; j += NT) {
      const Tok tk = svi.load(j);
      const int node = tk.node;
      const int4 na = lx.node_a(node);               // {self_a, next_a, ac_off, ac_end}
      const int sword = lx.node_b(node).x;           // stend
      if (!last) {
        if (tk.score <= JAMD_LOG_ZERO) continue;
        if (tk.score < thr) continue;
        // beam_intra_word() :2154-2180 -> beam_intra_word_core() :2004-2135.  The self loop and
        // the `next` arc are handled here; the extra arcs of branching nodes (up to tens per
        // node) go to a work queue so that no lane walks them alone.
        const int e0 = na.z, e1 = na.w;
        if (e1 > e0) {
          const int base = atomicAdd(&sh.n_arc, e1 - e0);
          for (int e = e0; e < e1; e++) ARCQ(base + e - e0) = make_int2(j, e);
        }
        for (int k = 0; k < 2; k++) {
          int next_node; float a;
          if (k == 0) { next_node = node; a = __int_as_float(na.x); if (a == JAMD_LOG_ZERO) continue; }
          else { next_node = node + 1; a = __int_as_float(na.y); if (a == JAMD_LOG_ZERO) continue; }
          intra_candidate(tk, next_node, a);
        }
      }
      if (sword >= 0) {
        // save_trellis() :2209-2247
        const int ai = wave_alloc(&sh.n_atom, true);
        if (ai < wk.atom_cap) {
          jamd_trellis_atom a;
          a.wid = sword; a.last_tre = tk.last_tre; a.backscore = tk.score; a.lscore = tk.last_lscore;
          a.begintime = (short)((tk.last_tre < 0 ? -1 : ATOM(tk.last_tre).endtime) + 1);
          a.endtime = (short)(t - 1);
          ATOM(ai) = a;
        }
        sv_atom[j] = ai;
        if (!last && !wordmode && sword != lx.tail_silwid) {   // beam_inter_word() :2296-2313
          welist[atomicAdd(&sh.n_we, 1)] = j;
          const float tmpprob = tk.score + lx.wordend_a(sword);
          if (!dfa && tmpprob > JAMD_LOG_ZERO) {
            const unsigned long long key = ((unsigned long long)ord(tmpprob) << 32) | (unsigned)sword;
            const unsigned long long old = atomicMax(&sh.we_best, key);
            if (old != 0ull && (unsigned)(old >> 32) == (unsigned)(key >> 32)) atomicAdd(&sh.ties_we, 1);
          }
        }
      }
    }
    __syncthreads();
    if (!last) {                                   // drain the extra-arc queue, one arc per thread
      const int n_arc = sh.n_arc;
      for (int q = tid; q < n_arc; q += NT) {
        const int2 it = ARCQ(q);
        intra_candidate(svi.load(it.x), lx.ac_to(it.y), lx.ac_a(it.y));
      }
      __syncthreads();
    }
    PHASE(0);
    if (last) break;

    // ---- B1: word ends -> isolated roots with the 2-gram (beam_inter_word() :2334-2516)
    if (dfa) {
      // grammar: every word end x every root whose category may follow (category-pair
      // constraint, beam_inter_word() :2404-2412), word insertion penalty + the ended word's
      // in-class score as the LM score (:2452-2461)
      const int n_we = sh.n_we, nroot = lx.startnum;
      const int total = n_we * nroot;
      for (int x = tid; x < total; x += NT) {
        const int w = x / nroot, r = x - w * nroot;
        const Tok tk = svi.load(welist[w]);
        const int sword = lx.node_b(tk.node).x;
        if (!lx.cat_pair(lx.wton(sword) * lx.ncat + lx.root_cat(r))) continue;
        const int last_word = lx.is_transparent(sword) ? tk.last_cword : sword;
        float tmpsum = tk.score;
        tmpsum += lx.wordend_a(sword);
        float ng = lx.penalty1;
        ng += (last_word >= 0) ? lx.cprob(last_word) : 0.0f;
        tmpsum += ng;
        if (push(sh, cl, lx.startnode(r), tmpsum, 0x80000000u | (unsigned)sword) != 0ull)
          atomicAdd(&sh.ties, 1);
      }
      if (t == 0)          // pseudo frame 0: the initial tokens (init_nodescore(), beam.c:1669-1757)
        for (int e = tid; e < lx.ninit; e += NT)
          push(sh, cl, lx.init_node(e), lx.init_lscore(e), 0xC0000000u | (unsigned)e);
    } else {
      const int n_we = sh.n_we, niso = lx.isolatenum;
      const int total = n_we * niso;
      for (int x = tid; x < total; x += NT) {
        const int w = x / niso, i = x - w * niso;
        const Tok tk = svi.load(welist[w]);
        const int sword = lx.node_b(tk.node).x;
        const bool tr = lx.is_transparent(sword) != 0;
        const int last_word = tr ? tk.last_cword : sword;
        const int2 ir = lx.iso_root(i);                    // {root node, successor word}
        // one entry of max_successor_prob_iw()'s array (factoring_sub.c:1119-1143)
        const float p = (last_word < 0) ? 0.0f
                        : lx.iwtab ? lx.iwtab[(size_t)lx.wton(last_word) * niso + i]
                        : bigram_prob(lx, lx.wton(last_word), lx.wton(ir.y)) + lx.cprob(ir.y);
        float tmpsum = tk.score;
        tmpsum += lx.wordend_a(sword);
        const float ng = p * lmw + pen;
        tmpsum += ng;
        if (tr && tk.last_cword >= 0 && lx.is_transparent(tk.last_cword)) tmpsum += lx.lm_penalty_trans;
        if (push(sh, cl, ir.x, tmpsum, 0x80000000u | (unsigned)sword) != 0ull)
          atomicAdd(&sh.ties, 1);
      }
    }
    // ---- B2: best word end -> shared roots with the 1-gram factoring value
    //          (beam_inter_word_factoring() :2549-2637)
    if (!dfa && sh.we_best != 0ull) {
      const unsigned long long kb = sh.we_best;
      const float best_score = unord((unsigned)(kb >> 32));
      const int sword = (int)(unsigned)kb;
      const Tok tk = svi.load(hash_get(hkey, hval, hmask, lx.word_end(sword)));
      const bool trans2 = lx.is_transparent(sword) && tk.last_cword >= 0 && lx.is_transparent(tk.last_cword);
      for (int r = tid; r < lx.nshared; r += NT) {
        const float2 sr = lx.shared_root(r);               // {root node (bits), fscore}
        const float ng = sr.y * lmw + pen;
        float tmpsum = best_score;
        tmpsum += ng;
        if (trans2) tmpsum += lx.lm_penalty_trans;
        if (tmpsum < thr) continue;                               // :2580
        if (push(sh, cl, __float_as_int(sr.x), tmpsum, 0xC0000000u) != 0ull) atomicAdd(&sh.ties, 1);
      }
    }
    __syncthreads();
    if (tid == 0) sh.n_arc = 0;                    // the queue now collects state-set reductions
    PHASE(1);

    // ---- C: finalize the touched nodes: winner's payload + acoustic score (:2944-2951)
    const int n_new = sh.n_new;
    if (n_new > max_tokens) max_tokens = n_new;
    {
      const RowRef row{scores + (size_t)(t_begin + t - base) * S, rowc, wk.row_cache != 0};
      unsigned mymax = ord(JAMD_LOG_ZERO), mymin = 0xffffffffu;
      // CB tokens per thread are carried through the steps together: every step's loads (node
      // record, LM memo, context table, score row) are issued for all of them before any is used, so
      // one thread has up to CB independent gathers in flight instead of one dependent chain per token.
      constexpr int CB = JAMD_BEAM_CB;
      for (int s0 = tid; s0 < n_new; s0 += CB * NT) {
        bool ok[CB]; int node[CB], slot[CB]; int4 nr[CB]; unsigned long long key[CB];
        int l_tre[CB], l_cword[CB], l_wid[CB], lmreq[CB], ent[CB];
        float l_ls[CB];
#pragma unroll
        for (int k = 0; k < CB; k++) {
          const int s = s0 + k * NT;
          ok[k] = s < n_new;
          const int2 t2 = ok[k] ? TOUCHED(s) : make_int2(0, -1);     // {node, LDS slot or -1}
          node[k] = t2.x; slot[k] = t2.y;
        }
#pragma unroll
        for (int k = 0; k < CB; k++) nr[k] = lx.node_b(node[k]);     // {stend, scid, out_id, out_kind}
#pragma unroll
        for (int k = 0; k < CB; k++) {
          key[k] = 0ull;
          if (ok[k]) {
            if (slot[k] >= 0) { key[k] = cl.lkey[slot[k]]; cl.lkey[slot[k]] = 0ull; cl.lnode[slot[k]] = -1; }   // back to empty
            else key[k] = atomicExch(&NODEKEY(node[k]), 0ull);
          }
        }
        // winner's payload.  lmreq != 0: the LM factoring value has to be looked up (next step)
#pragma unroll
        for (int k = 0; k < CB; k++) {
          const unsigned id = (unsigned)key[k];
          lmreq[k] = 0; l_tre[k] = -1; l_cword[k] = -1; l_wid[k] = -1; l_ls[k] = 0.0f;
          if (!ok[k]) continue;
          if ((id >> 31) == 0u) {                      // intra-word, id = source node
            const Tok tk = svi.load(hash_get(hkey, hval, hmask, (int)id));
            l_tre[k] = tk.last_tre; l_cword[k] = tk.last_cword; l_wid[k] = tk.last_wid;
            if (node[k] != tk.node && nr[k].y != 0) lmreq[k] = nr[k].y;   // beam_intra_word_core() :2069-2082
            else l_ls[k] = tk.last_lscore;
          } else if (dfa && (id >> 30) == 3u) {        // an initial token of the grammar
            l_ls[k] = lx.init_lscore(id & 0x3fffffffu);
          } else {
            const bool iso = (id >> 30) == 2u;
            const int sword = iso ? (int)(id & 0x3fffffffu) : (int)(unsigned)sh.we_best;
            const int j = hash_get(hkey, hval, hmask, lx.word_end(sword));
            const Tok tk = svi.load(j);
            const int last_word = lx.is_transparent(sword) ? tk.last_cword : sword;
            l_tre[k] = sv_atom[j]; l_cword[k] = last_word; l_wid[k] = sword;
            if (dfa) {                                       // beam_inter_word() :2452-2461
              float ng = lx.penalty1;
              ng += (last_word >= 0) ? lx.cprob(last_word) : 0.0f;
              l_ls[k] = ng;
            } else if (iso) {                                // beam_inter_word() :2430-2438
              const int wn = lx.scword(nr[k].y);
              const float p = (last_word < 0) ? 0.0f
                              : bigram_prob(lx, lx.wton(last_word), lx.wton(wn)) + lx.cprob(wn);
              l_ls[k] = p * lmw + pen;
            } else {                                         // beam_inter_word_factoring() :2572-2573
              l_ls[k] = lx.fscore(-nr[k].y) * lmw + pen;
            }
          }
        }
        // LM factoring value on entering a branch node: max_successor_prob(), its memo read issued
        // for all CB tokens first (factoring_sub.c:942-1008)
        {
          int ctx[CB]; unsigned long long mm[CB]; float fs[CB];
#pragma unroll
          for (int k = 0; k < CB; k++) {
            ctx[k] = -1; mm[k] = 0ull; fs[k] = 0.0f;
            if (lmreq[k] != 0 && l_cword[k] >= 0) {
              if (lmreq[k] < 0) fs[k] = lx.fscore(-lmreq[k]);
              else { ctx[k] = lx.wton(l_cword[k]); mm[k] = memo[lmreq[k]]; }
            }
          }
#pragma unroll
          for (int k = 0; k < CB; k++) {
            if (lmreq[k] == 0) continue;
            float p = 0.0f;                                   // lastword < 0: no LM context yet
            if (l_cword[k] >= 0) {
              if (lmreq[k] < 0) p = fs[k];
              else if ((int)(unsigned)(mm[k] >> 32) == ctx[k]) p = __uint_as_float((unsigned)mm[k]);
              else p = max_successor_prob(lx, l_cword[k], lmreq[k], memo);     // memo miss: 2-gram search, refill
            }
            l_ls[k] = p * lmw + pen;
          }
        }
        // outprob_style(), outprob_style.c:354-486: a plain state score is added here; a
        // state-set reduction (tens of gathers) is deferred to the cooperative drain below
        {
          int col[CB];
#pragma unroll
          for (int k = 0; k < CB; k++) {
            col[k] = lx.nlc;
            if (ok[k] && nr[k].w >= JAMD_AS_RSET && l_wid[k] >= 0) col[k] = lx.word_lc(l_wid[k]);
          }
#pragma unroll
          for (int k = 0; k < CB; k++) {
            if (nr[k].w == JAMD_AS_STATE) ent[k] = nr[k].z;
            else if (nr[k].w == JAMD_AS_LSET) ent[k] = ~nr[k].z;
            else ent[k] = ok[k] ? lx.lc_tab((size_t)nr[k].z * (lx.nlc + 1) + col[k]) : 0;
          }
        }
        float ac[CB];
#pragma unroll
        for (int k = 0; k < CB; k++) ac[k] = (ok[k] && ent[k] >= 0) ? row[ent[k]] : 0.0f;
#pragma unroll
        for (int k = 0; k < CB; k++) {
          if (!ok[k]) continue;
          const int s = s0 + k * NT;
          const float score = unord((unsigned)(key[k] >> 32));
          Tok nw;
          nw.node = node[k]; nw.pad0 = nw.pad1 = 0;
          nw.last_tre = l_tre[k]; nw.last_cword = l_cword[k]; nw.last_wid = l_wid[k]; nw.last_lscore = l_ls[k];
          if (ent[k] >= 0) {
            nw.score = score + ac[k];
            const unsigned b = ord(nw.score);
            CURKEY(s) = b;
            if (b > mymax) mymax = b;
            if (b < mymin) mymin = b;
          } else {
            nw.score = score;
            ARCQ(atomicAdd(&sh.n_arc, 1)) = make_int2(s, ~ent[k]);     // (token, state set); arcq is free again
          }
          CUR(s) = nw;
        }
      }
      __syncthreads();
      if (TIMED && tid == 0) { const unsigned long long n_ = wall_clock64(); ph[4] += n_ - tc; tq = n_; }   // token loop
      // drain: four lanes per (token, set) item, each reduces every fourth member, then the
      // partial results are merged through shuffles (outprob_cd(), outprob.c:287-400)
      const int n_set = sh.n_arc;
      const int sub = tid & 3, lane = tid & 63;
      for (int q0 = 0; q0 < n_set; q0 += NT / 4) {
        const int q = q0 + (tid >> 2);
        const bool act = q < n_set;
        const int2 it = act ? ARCQ(q) : make_int2(0, 0);
        const int a = act ? lx.set_off(it.y) : 0, bnd = act ? lx.set_off(it.y + 1) : 0;
        float r;
        if (lx.cdset_method == JAMD_IWCD_NBEST && lx.cdmax_num <= 4) {
          float b0 = JAMD_LOG_ZERO, b1 = JAMD_LOG_ZERO, b2 = JAMD_LOG_ZERO, b3 = JAMD_LOG_ZERO;
          int n = 0;
          auto ins = [&](float p) {
            float t_;
            if (p > b0) { t_ = b0; b0 = p; p = t_; }
            if (p > b1) { t_ = b1; b1 = p; p = t_; }
            if (p > b2) { t_ = b2; b2 = p; p = t_; }
            if (p > b3) { b3 = p; }
          };
          for (int m = a + sub; m < bnd; m += 16) {          // four members per lane in flight
            int ix[4]; float pv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) ix[j] = (m + 4 * j < bnd) ? lx.set_states(m + 4 * j) : -1;
#pragma unroll
            for (int j = 0; j < 4; j++) pv[j] = (ix[j] >= 0) ? row[ix[j]] : JAMD_LOG_ZERO;
#pragma unroll
            for (int j = 0; j < 4; j++) if (pv[j] > JAMD_LOG_ZERO) { n++; ins(pv[j]); }
          }
          // merge the four partial top lists into the group's first lane (values <= LOG_ZERO are
          // padding and never displace anything)
#pragma unroll
          for (int src = 1; src < 4; src++) {
            const int from = (lane & ~3) + src;
            const float c0 = __shfl(b0, from, 64), c1 = __shfl(b1, from, 64), c2 = __shfl(b2, from, 64),
                        c3 = __shfl(b3, from, 64);
            const int cn = __shfl(n, from, 64);
            if (sub == 0) { ins(c0); ins(c1); ins(c2); ins(c3); n += cn; }
          }
          if (n > lx.cdmax_num) n = lx.cdmax_num;
          float sum = 0.0f;
          if (n > 0) sum += b0;
          if (n > 1) sum += b1;
          if (n > 2) sum += b2;
          if (n > 3) sum += b3;
          r = sum / (float)n;
        } else if (lx.cdset_method == JAMD_IWCD_MAX) {
          float m_ = JAMD_LOG_ZERO;
          for (int m = a + sub; m < bnd; m += 16) {
            int ix[4]; float pv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) ix[j] = (m + 4 * j < bnd) ? lx.set_states(m + 4 * j) : -1;
#pragma unroll
            for (int j = 0; j < 4; j++) pv[j] = (ix[j] >= 0) ? row[ix[j]] : JAMD_LOG_ZERO;
#pragma unroll
            for (int j = 0; j < 4; j++) if (m_ < pv[j]) m_ = pv[j];
          }
#pragma unroll
          for (int src = 1; src < 4; src++) { const float c = __shfl(m_, (lane & ~3) + src, 64); if (m_ < c) m_ = c; }
          r = m_;
        } else {
          // average (member-order float sum) and long N-best lists: one lane, reference order
          r = (act && sub == 0) ? cd_reduce(row, lx.set_states_ptr(), a, bnd, lx.cdset_method, lx.cdmax_num) : 0.0f;
        }
        if (act && sub == 0) {
          const float sc = CUR(it.x).score + r;
          CUR(it.x).score = sc;
          const unsigned b = ord(sc);
          CURKEY(it.x) = b;
          if (b > mymax) mymax = b;
          if (b < mymin) mymin = b;
        }
      }
      if (TIMED && tid == 0) { ph[5] += wall_clock64() - tq; ph[6] += sh.n_arc; }     // set drain; number of set reductions
      atomicMax(&sh.maxbits, mymax);
      atomicMin(&sh.minbits, mymin);
    }
    __syncthreads();
    PHASE(2);
    {
      const float mx = unord(sh.maxbits);                          // score_pruning_max :2948
      thr = (wk.width >= 0.0f) ? (mx - wk.width) : JAMD_LOG_ZERO;  // :2954-2960
      if (t == 0) thr = JAMD_LOG_ZERO;                             // get_back_trellis_init() sets no score threshold
    }
    if (n_new == 0) {                                              // :3012-3015
      if (tid == 0) { res->status = JAMD_PASS1_DIED; res->died_at = t; }
      stopped = true;
      __syncthreads();
      break;
    }
    if (sh.n_atom > wk.atom_cap) {
      if (tid == 0) res->status = JAMD_PASS1_OVERFLOW;
      stopped = true;
      __syncthreads();
      break;
    }

    // ---- D: rank pruning, sort_token_no_order() :1492 -> the top beam_width tokens become
    //         the next frame's survivors (copied into sv[], hashed by node)
    unsigned prefix = 0, need = 0, count_eq = 0;
    const bool prune = n_new > wk.beam;
    if (prune) {
      // radix select of the beam_width-th largest key.  All keys of a frame share their
      // high bits (scores lie within a few hundred log units), so only the bits below the
      // highest bit in which the frame's max and min differ are selected on, 11 at a time
      // (typically 2-3 passes).
      need = (unsigned)wk.beam;
      const unsigned diff = sh.maxbits ^ sh.minbits;
      int remaining = diff ? 32 - __clz(diff) : 0;       // number of varying low bits
      prefix = remaining < 32 ? (sh.maxbits >> remaining) : 0u;
      count_eq = (unsigned)n_new;
      while (remaining > 0) {
        const int w = remaining < 11 ? remaining : 11;
        const int shift = remaining - w;
        const unsigned dmask = (1u << w) - 1u;
        for (int i = tid; i < 2048; i += NT) hist[i] = 0;
        __syncthreads();
        for (int s = tid; s < n_new; s += NT) {
          const unsigned b = CURKEY(s);
          const unsigned hi = (shift + w < 32) ? (b >> (shift + w)) : 0u;
          if (hi == prefix) atomicAdd(&hist[(b >> shift) & dmask], 1u);
        }
        __syncthreads();
        {
          // suffix scan over the 2048 digits with the whole workgroup: thread i owns digits 2i, 2i+1;
          // `above` = tokens with a larger digit
          const unsigned h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
          const unsigned pair = h0 + h1;
          unsigned incl = pair;                          // inclusive suffix sum over the lanes >= this one
          const int ln = tid & 63;
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_down(incl, off, 64);
            if (ln + off < 64) incl += o;
          }
          if (ln == 0) sh.wsum[tid >> 6] = incl;         // this wave's total
          __syncthreads();
          unsigned above = incl - pair;                  // larger digits inside the wave ...
          for (int wv = (tid >> 6) + 1; wv < NT / 64; wv++) above += sh.wsum[wv];   // ... and in the waves above
          // digit 2i+1 first (the larger one)
          if (above < need && need <= above + h1) { sh.sel_digit = 2u * tid + 1u; sh.sel_need = need - above; sh.sel_count = h1; }
          above += h1;
          if (above < need && need <= above + h0) { sh.sel_digit = 2u * tid; sh.sel_need = need - above; sh.sel_count = h0; }
        }
        __syncthreads();
        prefix = (prefix << w) | sh.sel_digit;
        need = sh.sel_need;
        count_eq = sh.sel_count;
        remaining -= w;
      }
      // prefix = score bits of the beam_width-th token; keep everything above it and
      // `need` of the count_eq tokens equal to it
      for (int i = tid; i < 2048; i += NT) hist[i] = 0;   // the histogram sat on the first cells: empty them again
    }
    for (int i = tid; i < wk.hsize; i += NT) hkey[i] = -1;
    const bool cut_tie = prune && count_eq > need;
    if (tid == 0) { sh.n_surv = 0; sh.eq_n = 0; if (cut_tie) sh.ties_cut += 1; }
    __syncthreads();
    if (cut_tie) {
      // several tokens share the cut score: collect their nodes (a handful), then keep
      // those on the smallest nodes (canonical; the reference keeps whichever its heap
      // order left inside)
      for (int s = tid; s < n_new; s += NT)
        if (CURKEY(s) == prefix) {
          const int q = atomicAdd(&sh.eq_n, 1);
          if (q < 128) sh.eq_node[q] = CUR(s).node;
        }
      __syncthreads();
    }
    for (int s = tid; s < n_new; s += NT) {
      bool keep = true;
      if (prune) {
        const unsigned b = CURKEY(s);
        keep = b > prefix;
        if (b == prefix) {
          if (!cut_tie) keep = true;
          else {
            const int mynode = CUR(s).node;
            unsigned rank = 0;
            if (sh.eq_n <= 128) {
              for (int q = 0; q < sh.eq_n; q++) rank += (sh.eq_node[q] < mynode) ? 1u : 0u;
            } else {
              for (int q = 0; q < n_new; q++) rank += (CURKEY(q) == prefix && CUR(q).node < mynode) ? 1u : 0u;
            }
            keep = rank < need;
          }
        }
      }
      if (keep) {
        const Tok me = CUR(s);
        const int j = wave_alloc(&sh.n_surv, true);
        svi.store(j, me);
        hash_put(hkey, hval, hmask, me.node, j);
      }
    }
    __syncthreads();
    PHASE(3);
  }
  __syncthreads();

  if (smode == 1) {            // not finished: park the state for the next launch
    if (SVLDS && !stopped) {
      u32x4 *dst = (u32x4 *)(ub + wk.o_sv);
      const lds_v4 *src = (const lds_v4 *)dyn_lds;
      for (int i = tid; i < wk.sv_bytes / 16; i += NT) dst[i] = src[i];
    }
    if (tid == 0) {
      ss->started = 1; ss->active = stopped ? 0 : 1; ss->frames_done = T; ss->n_surv = sh.n_surv; ss->thr = thr;
      ss->n_atom = sh.n_atom; ss->ties = sh.ties; ss->ties_we = sh.ties_we; ss->ties_cut = sh.ties_cut;
      ss->max_tokens = max_tokens;
      res->natom = min(sh.n_atom, wk.atom_cap); res->frames = T; res->max_tokens = max_tokens;
      res->ties = sh.ties + sh.ties_we + sh.ties_cut;
      if (TIMED) for (int i = 0; i < 8; i++) res->phase_us[i] += (int)(ph[i] / 100ull);
    }
    return;
  }
  if (ss && tid == 0) { ss->active = 0; ss->started = 1; ss->frames_done = T; }

  // ---- find_1pass_result() :399-431 + trace_backptr() :294-340
  const int natom = min(sh.n_atom, wk.atom_cap);
  if (tid == 0) sh.best_atom = -1;
  __syncthreads();
  if (res->status == JAMD_PASS1_OK && dfa) {
    // grammar (:433-455): the best word on the latest frame where a word survived; equal scores
    // go to the smaller word id (rw[t] is sorted by word id and the test is a strict <)
    if (tid == 0) { sh.n_arc = -1; sh.we_best = 0ull; }
    __syncthreads();
    int lt = -1;
    for (int i = tid; i < natom; i += NT)
      if (ATOM(i).backscore > JAMD_LOG_ZERO && ATOM(i).endtime > lt) lt = ATOM(i).endtime;
    if (lt >= 0) atomicMax(&sh.n_arc, lt);
    __syncthreads();
    lt = sh.n_arc;
    for (int i = tid; i < natom; i += NT)
      if (ATOM(i).endtime == lt && ATOM(i).backscore > JAMD_LOG_ZERO)
        atomicMax(&sh.we_best, ((unsigned long long)ord(ATOM(i).backscore) << 32) | (0xffffffffu - (unsigned)ATOM(i).wid));
    __syncthreads();
    const unsigned long long kb = sh.we_best;
    for (int i = tid; i < natom; i += NT)      // (frame, word) names one atom: a word has one end node
      if (kb != 0ull && ATOM(i).endtime == lt && (unsigned)ATOM(i).wid == 0xffffffffu - (unsigned)kb &&
          ord(ATOM(i).backscore) == (unsigned)(kb >> 32)) sh.best_atom = i;
  } else if (res->status == JAMD_PASS1_OK) {
    int best = -1;
    for (int i = tid; i < natom; i += NT)
      if (ATOM(i).wid == lx.tail_silwid && ATOM(i).backscore > JAMD_LOG_ZERO) best = i;  // ascending i
    if (best >= 0) atomicMax(&sh.best_atom, best);
  }
  __syncthreads();
  if (tid == 0) {
    res->natom = natom; res->ties = sh.ties + sh.ties_we + sh.ties_cut; res->max_tokens = max_tokens;
    res->ties_node = sh.ties; res->ties_wordend = sh.ties_we; res->ties_cut = sh.ties_cut;
    if (TIMED) for (int i = 0; i < 8; i++) res->phase_us[i] += (int)(ph[i] / 100ull);
    res->frames = T;
    if (sh.n_atom > wk.atom_cap) res->status = JAMD_PASS1_OVERFLOW;
    if (res->status == JAMD_PASS1_OK) {
      const int best = sh.best_atom;
      if (best < 0) res->status = JAMD_PASS1_FAIL;
      else {
        int n = 0, a = best;
        int rev[MAXSEQ];
        rev[n++] = ATOM(a).wid;
        while (ATOM(a).begintime > 0 && n < MAXSEQ) { a = ATOM(a).last_tre; rev[n++] = ATOM(a).wid; }
        for (int k = 0; k < n; k++) res->wseq[k] = rev[n - 1 - k];
        res->wnum = n; res->score = ATOM(best).backscore;
      }
    }
  }
}


#undef SLICE
#undef NODEKEY
#undef CUR
#undef CURKEY
#undef TOUCHED
#undef ARCQ
#undef ATOM

}  // namespace

// ---- the host functions that know this kernel's LDS image (beam_host.h)
namespace jamdb {

void fbeam_layout(Work *wp) {
  Work &w = *wp;
  const int beam_width = w.beam;
  // survivor state: Tok[beam] + atom[beam] + welist[beam] + hash keys/values[hsize]
  w.hsize = 64; while (w.hsize < 2 * beam_width) w.hsize <<= 1;
  w.sv_bytes = (int)(beam_width * (sizeof(Tok) + 2 * sizeof(int)) + (size_t)w.hsize * 2 * sizeof(int));
  w.sv_bytes = (w.sv_bytes + 15) & ~15;
  w.use_lds = w.sv_bytes + kHistBytes <= kMaxDynLds ? 1 : 0;
  // what is left of the LDS budget holds the frame's Viterbi cells (12 bytes per slot), if that is
  // at least 4096 slots; a frame that outgrows the table overflows into nodekey[]
  w.cell_slots = 0;
  if (w.use_lds) {
    int slots = 4096;
    while ((size_t)w.sv_bytes + (size_t)slots * 2 * 12 <= (size_t)kMaxDynLds && slots < 65536) slots *= 2;
    if ((size_t)w.sv_bytes + (size_t)slots * 12 <= (size_t)kMaxDynLds) w.cell_slots = slots;
    // a frame creates about five tokens per survivor; a table that would run above ~2/3 load
    // costs more in failed probes than it saves, so narrower-than-needed tables are not used
    if (w.cell_slots < 8 * beam_width) w.cell_slots = 0;
#ifdef JAMD_DEV
    if (getenv("JAMD_BEAM_NO_LDS_CELLS") != nullptr) w.cell_slots = 0;      // development switch (timing comparison)
#endif
  }
  w.cell_off = w.use_lds ? w.sv_bytes : 0;
  w.node_off = w.cell_off + (8 * w.cell_slots > kHistBytes ? 8 * w.cell_slots : kHistBytes);
  w.row_off = w.node_off + 4 * w.cell_slots;
  w.lds_bytes = w.row_off;
  w.row_cache = 0;
}

hipError_t fbeam_prepare() {
  // the attribute is per kernel, not per work area: always ask for the whole budget
  const void *fn[] = {(const void *)beam_pass1_kernel<false, true>, (const void *)beam_pass1_kernel<true, true>,
                      (const void *)beam_pass1_kernel<false, false>, (const void *)beam_pass1_kernel<true, false>};
  for (const void *f : fn) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// instantiation by where the survivor image lives and by instrumentation
void fbeam_launch(const LexDev &lx, const Work &w0, const float *scores, int nstate, const int *d_utt_off, int nutt,
                  int smode, bool timed, hipStream_t st) {
  Work w = w0;                                       // the score row joins the LDS image when it still fits
  w.row_cache = w.lds_bytes + 4 * nstate <= kMaxDynLds;
#ifdef JAMD_DEV
  if (getenv("JAMD_BEAM_NO_ROW_CACHE") != nullptr) w.row_cache = 0;
#endif
  const int lds = w.lds_bytes + (w.row_cache ? 4 * nstate : 0);
  const dim3 grid(nutt), block(NT);
  if (w.use_lds) {
    if (timed) hipLaunchKernelGGL((beam_pass1_kernel<true, true>), grid, block, lds, st, lx, w, scores, nstate, d_utt_off, smode);
    else hipLaunchKernelGGL((beam_pass1_kernel<false, true>), grid, block, lds, st, lx, w, scores, nstate, d_utt_off, smode);
  } else {
    if (timed) hipLaunchKernelGGL((beam_pass1_kernel<true, false>), grid, block, lds, st, lx, w, scores, nstate, d_utt_off, smode);
    else hipLaunchKernelGGL((beam_pass1_kernel<false, false>), grid, block, lds, st, lx, w, scores, nstate, d_utt_off, smode);
  }
}

}  // namespace jamdb
