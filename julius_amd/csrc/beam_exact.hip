// beam_exact.hip -- first-pass token passing with the REFERENCE'S TIE SEMANTICS, frame-parallel: the kernel for
// ordinary lexicons (K6x, here), the one for multipath lexicons (K6m, beam_exact_mp.h, compiled in this unit), the
// prune_order_kernel diagnostic, and their launches.  The pruning step is beam_prune.h, what K6x and K6m share
// beam_exact_dev.h, the LDS layout beam_exact_layout.hip.
//
// beam.hip's beam_pass1_kernel resolves exact score ties canonically (larger source id, smaller node on
// the rank cut); the reference resolves them by its visiting order:
//   * propagate_token() (libjulius/src/beam.c:1945-1980) replaces a token only on a STRICTLY better score,
//     so among equal candidates the one visited first wins;
//   * beam_inter_word() keeps the first of equally good word ends as wordend_best (:2308);
//   * the visiting order of a frame is tindex[n_start..n_end] as sort_token_no_order() (:1492) left it:
//     creation order when nothing is pruned, else the output of a partial heap sort
//     (sort_token_upward / _downward, :1342-1480) over the tokens in creation order;
//   * creation order is the order of first visits (create_token(), :1148).
// The kernels reproduce all of that with the whole workgroup:
//   1. every candidate carries its visiting index vis = (position j of the source in the visiting order,
//      transition number within the source: self, next, extra arcs in wchmm order, then the roots from
//      startnum-1 down to 0; the factoring pass of beam_inter_word_factoring() counts as source n_surv).
//      The Viterbi cell is atomicMax(score bits || ~vis): best score, earliest visit -- first-writer-wins.
//      A second atomicMax(~vis) per cell keeps the node's FIRST visit.
//   2. creation order = rank of the first visit: one bit per visiting index in a bitmap, prefix popcount.
//   3. rank pruning = the reference's heap, exactly (beam_prune.h):
//        - heapify runs level-parallel (the sift-downs of one tree level touch disjoint subtrees and the
//          reference runs the levels bottom-up, so the result is the sequential one), with the levels
//          overlapped inside a wave (heapify_overlapped());
//        - the extraction loop of sort_token_upward() (tokens > 2 beam) is replaced by its closed form.  While
//          the element taken from the tail is smaller than every element still to be extracted, an extraction is
//          a hole running down the path of larger children (left on ties): the heap is a tree of stable merges,
//          and the extraction order is (score descending, PRE-ORDER index of the heap position ascending).  The
//          exceptions ("events": the tail element is itself among the top k) re-insert that element at the end of
//          the current max path.  A few per frame are found and replayed one by one by a single wave with range
//          queries over the top-k list (sorted by counting over score bins), only up to the last turn that can
//          still change the order; hundreds per frame (wide beams) are resolved together by the sweep replay
//          (beam_sweep.h).  The equivalence was fuzzed against the sequential code (tests/test_prune_order.py does
//          it on the device; HISTORY.md part II section 3 "K6x" has the argument);
//        - sort_token_downward() (beam < tokens <= 2 beam) has the same closed form over the n - k SMALLEST
//          elements of the min-heap: the sorted list, the sweep replay for their moves, and a replay of the short
//          sifts below the extracted region for the residual heap (down_finish(), beam_sweep.h) -- wide layout,
//          full shape;
//        - the same lists + sweep replay + sift replay deliver the WHOLE array, residual heap and extracted part,
//          in either direction (exact_prune<FULL>): the multipath frame's mid-frame sort, whose result is the
//          input of that frame's final cut;
//        - whatever that machinery cannot hold (heap outside LDS, too many events, a layout without the sweep's
//          scratch) runs the extraction loop itself, pipelined on one wave when the heap is in LDS, else on one lane.
// Everything else -- LM factoring, outprob_style(), trellis atoms, score pruning -- is the arithmetic of
// beam_pass1_kernel.  The word trellis equals the reference's bit for bit, ties included
// (tests/test_beam_gpu.py::test_exact_*, tests/test_multipath_exact_gpu.py).  N-gram, grammar and word-list
// lexicons, with and without multipath.
#include "beam_prune.h"

namespace {

// K6x's per-frame views: the common part and the trellis word of each survivor (step 0 numbers them, steps A and C read them)
#define XBEAM_VIEWS(KA)                                                                                               \
  XBEAM_VIEWS_COMMON(KA, lx.lm_type, lds_i32 *sv_atom = (lds_i32 *)(dyn_lds + xw.off_atom);, );                       \
  (void)sv_atom

// Four waves per SIMD (128 VGPRs) in both shapes.  The half shape at five (96 VGPRs, a fifth of the register file left to a
// co-resident scoring wave) worked but did not pay: HISTORY.md part II section 5, "K1 beside K6x".
template <bool TIMED, bool WIDE, int NT>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4, 4)))
beam_exact_kernel(XKArgs ka_, const float *__restrict__ scores, int S, const int *__restrict__ utt_off, int smode) {
  // LDS image: survivors in VISITING ORDER (no node hash: a candidate names its source by position)
  XBEAM_ENTRY(XBEAM_VIEWS);
  for (int i = tid; i < cl.nslot; i += NT) { cl.lkey[i] = 0ull; cl.lnode[i] = -1; cl.lfirst[i] = 0u; }

  if (resume) {
    XBEAM_RESUME();
  } else {
    XBEAM_RESET();
    // get_back_trellis_init(): the silB head token (init_nodescore, beam.c:1622-1665); grammar / word list:
    // the initial tokens enter through the finalize and pruning steps of a pseudo frame 0
    if (tid == 0 && !dfa) {
      const int node = lx.word_head(lx.head_silwid);
      const int4 nr = lx.node_b(node);
      Tok nw;
      float ls = (nr.y != 0) ? max_successor_prob(lx, -1, nr.y) : 0.0f;
      ls = ls * lmw + pen;
      nw.node = node; nw.last_tre = -1; nw.last_cword = -1; nw.last_wid = -1; nw.last_lscore = ls;
      nw.score = node_outprob(lx, scores + (size_t)t_begin * S, nr.w, nr.z, -1) + ls;
      nw.pad0 = nr.x; nw.pad1 = 0;
      sv.store(0, nw);
      sh.n_surv = 1;
    }
  }
  XBEAM_LOOP_STATE();
#ifdef JAMD_DEV
  const unsigned long long cyc0 = clock64(), wall0 = tc;   // JAMD_XBEAM_PROBE == 4: shader clock under this kernel
#endif
#define PHASE(i) do { if (TIMED && tid == 0) { const unsigned long long n_ = wall_clock64(); ph[i] += n_ - tc; tc = n_; tc2 = n_; } } while (0)
#ifdef JAMD_DEV
#define PROBE(g, i) do { if (TIMED && JAMD_XBEAM_PROBE == (g) && tid == 0) { const unsigned long long n_ = wall_clock64(); ph[i] += n_ - tc2; tc2 = n_; } } while (0)
#else
#define PROBE(g, i) ((void)0)
#endif
  __syncthreads();

  XBEAM_ROW_REQUEST();
  row_request(resume ? base : (dfa ? 0 : 1));
  int par = 0;      // wide layout: the survivors live at o_sv (0) or at the head of the CUR() area (1), in turns: step E writes the next frame's where this frame's are not
  (void)par;
  for (int t = resume ? base : (dfa ? 0 : 1); t <= (finish ? T : T - 1); t++) {
    tid = tid_now();
    XBEAM_VIEWS(xargs_now());                              // this frame's view of the launch constants (see xargs_now())
    if constexpr (WIDE) sv.p = reinterpret_cast<u32x4 *>(ub + (par ? wk.o_cur : wk.o_sv));   // (the survivors' two homes: step E)
    const int n_surv = uni(sh.n_surv);
    __syncthreads();
    if (tid == 0) { sh.n_new = 0; sh.n_we = 0; sh.n_arc = 0; sh.we_best = 0ull; sh.maxbits = ord(JAMD_LOG_ZERO); sh.minbits = 0xffffffffu; }
    const bool last = (t == T);
    // ---- 0: dense visiting indices.  Source j owns XW slots for its word-internal transitions and, when it
    //         is a word end that may be followed by a word, one slot per root; sources pruned by score own none.
    //         The same scan numbers the trellis words of the frame in visiting order (save_trellis() is called in
    //         that order, beam.c:2209: the atom array comes out in the reference's creation order).
    int nbits = 0;
    {
      int carry = 0, acarry = sh.n_atom;
      for (int j0 = 0; j0 < n_surv; j0 += NT) {
        const int j = j0 + tid;
        int cnt = 0, isend = 0;
        if (j < n_surv) {
          u32x4 a_, b_;
          sv.quads(j, a_, b_);
          const float sc = __uint_as_float(a_.y); const int sw = (int)b_.z;
          const bool alive = last || (sc > JAMD_LOG_ZERO && !(sc < thr));
          if (alive && !last) cnt = XW + ((sw >= 0 && !wordmode && sw != lx.tail_silwid) ? nroot_x : 0);
          isend = (alive && sw >= 0) ? 1 : 0;
        }
        int ex, ea;
        block_excl_scan2<NT>(sh, cnt, isend, ex, ea);
        if (j < n_surv) { dbase[j] = carry + ex; sv_atom[j] = isend ? acarry + ea : -1; }
        carry += sh.scan_total; acarry += sh.scan_total2;
        __syncthreads();
      }
      if (tid == 0) { dbase[n_surv] = carry; sh.n_atom = acarry; }
      nbits = last ? 0 : carry + (dfa ? (t == 0 ? lx.ninit : 0) : XW + lx.nshared);
    }
    PROBE(1, 4);
    const int nwords = (nbits + 31) >> 5;
    const bool bm_in_lds = nwords <= xw.bm_words;
    // the creation-order bitmap: in LDS, or (a frame with more visiting indices than fit) in the utterance's slice
    lds_u32 *bm_l = (lds_u32 *)(dyn_lds + xw.off_bm);
    unsigned *bm_g = reinterpret_cast<unsigned *>(ub + xw.o_bitmap);
    auto bm_get = [&](int w) -> unsigned { return bm_in_lds ? bm_l[w] : bm_g[w]; };
    __syncthreads();

    // nscid = successor id of next_node (0 for the self loop): the caller loads it beside the transition record
    auto intra_candidate = [&](const Tok &tk, int j, int next_node, float a, int sub, int nscid) {
      float tmpsum = tk.score + a;
      if (nscid != 0) {
        const float ng = max_successor_prob(lx, tk.last_cword, nscid, memo) * lmw + pen;
        tmpsum -= tk.last_lscore;
        tmpsum += ng;
      }
      xpush(sh, cl, next_node, tmpsum, ((unsigned)j << s1) | (unsigned)sub);
    };
    // ---- A: intra-word transitions + word-end atoms (beam.c:2838-2900)
    for (int j = tid; j < n_surv; j += NT) {
      const Tok tk = sv.load(j);
      const int node = tk.node;
      const int sword = tk.pad0;                       // stend
      if (!last) {
        if (tk.score <= JAMD_LOG_ZERO) continue;
        if (tk.score < thr) continue;
        const int4 na = lx.node_a(node);
        const int nscid1 = (node + 1 < lx.nnode) ? lx.scid(node + 1) : 0;   // independent of na: both loads in flight together
        const int e0 = na.z, e1 = na.w;
        if (e1 > e0) {
          const int b0 = atomicAdd(&sh.n_arc, e1 - e0);
          for (int e = e0; e < e1; e++) ARCQ(b0 + e - e0) = make_int2(j | ((2 + e - e0) << 16), e);   // (source | transition number, arc)
        }
        { const float a = __int_as_float(na.x); if (a != JAMD_LOG_ZERO) intra_candidate(tk, j, node, a, 0, 0); }
        { const float a = __int_as_float(na.y); if (a != JAMD_LOG_ZERO) intra_candidate(tk, j, node + 1, a, 1, nscid1); }
      }
      if (sword >= 0) {
        const int ai = sv_atom[j];                         // save_trellis() :2209-2247, numbered in step 0
        if (ai < wk.atom_cap) {
          jamd_trellis_atom a;
          a.wid = sword; a.last_tre = tk.last_tre; a.backscore = tk.score; a.lscore = tk.last_lscore;
          a.begintime = (short)((tk.last_tre < 0 ? -1 : ATOM(tk.last_tre).endtime) + 1);
          a.endtime = (short)(t - 1);
          ATOM(ai) = a;
        }
        if (!last && !wordmode && sword != lx.tail_silwid) {   // beam_inter_word() :2296-2313
          welist[atomicAdd(&sh.n_we, 1)] = j;
          const float tmpprob = tk.score + lx.wordend_a(sword);
          if (!dfa && tmpprob > JAMD_LOG_ZERO)                 // strict < in the reference: the earliest of the best
            atomicMax(&sh.we_best, ((unsigned long long)ordz(tmpprob) << 32) | (unsigned)(~(unsigned)j));
        }
      }
    }
    __syncthreads();
    PROBE(1, 5);
    if (!last) {
      const int n_arc = uni(sh.n_arc);
      for (int q = tid; q < n_arc; q += NT) {
        const int2 it = ARCQ(q);
        const int j = it.x & 0xffff;
        const int to = lx.ac_to(it.y);
        const Tok tk = sv.load(j);
        intra_candidate(tk, j, to, lx.ac_a(it.y), it.x >> 16, to != tk.node ? lx.scid(to) : 0);
      }
      __syncthreads();
    }
    PHASE(0);
    if (last) break;

    // ---- B: cross-word transitions.  Roots are visited from startnum-1 down to 0 (beam.c:2334, :2562); the
    //         root lists of the lexicon image are stored in that order.
    if (dfa) {
      const int n_we = sh.n_we, nroot = lx.startnum;
      const int total = n_we * nroot;
      for (int x = tid; x < total; x += NT) {
        const int w = x / nroot, rv = x - w * nroot;
        const int r = nroot - 1 - rv;
        const int j = welist[w];
        const Tok tk = sv.load(j);
        const int sword = tk.pad0;
        if (!lx.cat_pair(lx.wton(sword) * lx.ncat + lx.root_cat(r))) continue;
        if (lx.nfwd && fwd_next(lx, tk.pad1, lx.root_cat(r)) < 0) continue;     // forward DFA: no arc for this category (:2412-2422)
        const int last_word = lx.is_transparent(sword) ? tk.last_cword : sword;
        float tmpsum = tk.score;
        tmpsum += lx.wordend_a(sword);
        float ng = lx.penalty1;
        ng += (last_word >= 0) ? lx.cprob(last_word) : 0.0f;
        tmpsum += ng;
        xpush(sh, cl, lx.startnode(r), tmpsum, ((unsigned)j << s1) | (unsigned)(XW + rv));
      }
      if (t == 0)
        for (int e = tid; e < lx.ninit; e += NT) xpush(sh, cl, lx.init_node(e), lx.init_lscore(e), (unsigned)e);
    } else {
      // beam_inter_word() :2296-2440, root by root: a word end is reduced to (score + exit transition, LM context,
      // source position) once, then every isolated root takes the best candidate and the earliest visit over the
      // word ends with independent, coalesced reads of the cross-word LM table -- one cell update per root
      // instead of one per (word end, root).  The result is the one of pushing the candidates one by one
      // (a cell keeps a maximum and the first visit a minimum).
      const int n_we = uni(sh.n_we), niso = lx.isolatenum;
      lds_v4 *werec = (lds_v4 *)tpre;                           // [kWeChunk] (tpre is free until step C0)
      constexpr int kWeChunk = NT / 4;
      for (int w0 = 0; w0 < n_we; w0 += kWeChunk) {
        const int nrec = min(kWeChunk, n_we - w0);
        if (tid < nrec) {
          const int j = welist[w0 + tid];
          const Tok tk = sv.load(j);
          const int sword = tk.pad0;
          const bool tr = lx.is_transparent(sword) != 0;
          const int last_word = tr ? tk.last_cword : sword;
          float bs = tk.score;
          bs += lx.wordend_a(sword);
          const bool trans2 = tr && tk.last_cword >= 0 && lx.is_transparent(tk.last_cword);
          u32x4 rec;
          rec.x = __float_as_uint(bs); rec.y = (unsigned)(last_word < 0 ? -1 : lx.wton(last_word));
          rec.z = (unsigned)j | (trans2 ? 0x80000000u : 0u); rec.w = (unsigned)last_word;
          werec[tid] = rec;
        }
        __syncthreads();
        int parts = NT / (niso > 0 ? niso : 1);
        if (parts < 1) parts = 1;
        if (parts > nrec) parts = nrec;
        const int total = niso * parts;
        for (int x = tid; x < total; x += NT) {
          const int part = x / niso, i = x - part * niso;
          const int2 ir = lx.iso_root(i);
          unsigned long long best = 0ull; unsigned nfirst = 0u;
          // four word ends at a time: the table reads of a group go out together (one memory latency per group, not
          // per word end; a maximum and a minimum do not care about the order)
          constexpr int G = 4;
          for (int w0g = part; w0g < nrec; w0g += G * parts) {
            u32x4 rec[G]; float p[G]; bool live[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
              const int w = w0g + g * parts;
              live[g] = w < nrec;
              rec[g] = werec[live[g] ? w : part];
              const int ctx = (int)rec[g].y;
              p[g] = (!live[g] || ctx < 0) ? 0.0f
                     : lx.iwtab ? lx.iwtab[(size_t)ctx * niso + i]
                     : bigram_prob(lx, ctx, lx.wton(ir.y)) + lx.cprob(ir.y);
            }
#pragma unroll
            for (int g = 0; g < G; g++) {
              if (!live[g]) continue;
              float tmpsum = __uint_as_float(rec[g].x);
              const float ng = p[g] * lmw + pen;
              tmpsum += ng;
              if (rec[g].z & 0x80000000u) tmpsum += lx.lm_penalty_trans;
              if (tmpsum <= JAMD_LOG_ZERO) continue;
              const unsigned nv = ~(((rec[g].z & 0x7fffffffu) << s1) | (unsigned)(XW + i));
              const unsigned long long key = ((unsigned long long)ordz(tmpsum) << 32) | nv;
              if (key > best) best = key;
              if (nv > nfirst) nfirst = nv;
            }
          }
          if (best != 0ull) xpush_key(sh, cl, ir.x, best, nfirst);
        }
        __syncthreads();
      }
      PROBE(1, 7);
      if (sh.we_best != 0ull) {                       // beam_inter_word_factoring() :2549-2637
        const unsigned long long kb = sh.we_best;
        const float best_score = unord((unsigned)(kb >> 32));
        const Tok tk = sv.load((int)(~(unsigned)kb));
        const int sword = tk.pad0;
        const bool trans2 = lx.is_transparent(sword) && tk.last_cword >= 0 && lx.is_transparent(tk.last_cword);
        for (int r = tid; r < lx.nshared; r += NT) {
          const float2 sr = lx.shared_root(r);
          const float ng = sr.y * lmw + pen;
          float tmpsum = best_score;
          tmpsum += ng;
          if (trans2) tmpsum += lx.lm_penalty_trans;
          if (tmpsum < thr) continue;                               // :2580
          xpush(sh, cl, __float_as_int(sr.x), tmpsum, ((unsigned)n_surv << s1) | (unsigned)(XW + r));
        }
      }
    }
    __syncthreads();
    if (tid == 0) sh.n_arc = 0;
    PHASE(1);

    // ---- C0: creation order = rank of the node's first visit (create_token() :1148)
    const int n_new = uni(sh.n_new);
    if (n_new > max_tokens) max_tokens = n_new;
    if (pm.pstat && tid == 0) { pm.pstat[8] += n_new; pm.pstat[9] += n_surv; pm.pstat[10] += sh.n_we; pm.pstat[11] += 1; }   // work counters (jamd_beam_prune_stats())
    if (n_new > wk.tok_cap) {              // cannot happen (tok_cap bounds the reachable nodes); never write past the arrays
      if (tid == 0) res->status = JAMD_PASS1_OVERFLOW;
      stopped = true;
      __syncthreads();
      break;
    }
    int Wsh = 0;                                      // bitmap words per thread in the prefix scan: a power of two
    while ((NT << Wsh) < nwords) Wsh++;
    const int W = 1 << Wsh;
    {
      for (int i = tid; i < nwords; i += NT) { if (bm_in_lds) bm_l[i] = 0u; else bm_g[i] = 0u; }
      __syncthreads();
      for (int s = tid; s < n_new; s += NT) {
        const int2 t2 = TOUCHED(s);
        const unsigned fv = ~(t2.y >= 0 ? cl.lfirst[t2.y] : NODEFIRST(t2.x));
        const int dense = ((dfa && t == 0) ? 0 : dbase[fv >> s1]) + (int)(fv & submask);
        if (bm_in_lds) atomicOr((unsigned *)&bm_l[dense >> 5], 1u << (dense & 31)); else atomicOr(&bm_g[dense >> 5], 1u << (dense & 31));
      }
      __syncthreads();
      PROBE(2, 4);
      int cnt = 0;
      for (int x = 0; x < W; x++) { const int w = tid * W + x; if (w < nwords) cnt += __popc(bm_get(w)); }
      const int ex = block_excl_scan<NT>(sh, cnt);
      tpre[tid] = (unsigned)ex;
      __syncthreads();
      PROBE(2, 5);
    }
    // ---- C: finalize the touched nodes: winner's payload + acoustic score (:2944-2951), stored at the
    //         token's creation index
    {
      const XRowRef row{scores + (size_t)(t_begin + t - base) * S, rowc, wk.row_cache != 0};
      unsigned mymax = ord(JAMD_LOG_ZERO), mymin = 0xffffffffu;
      constexpr int CB = JAMD_XBEAM_CB;
      for (int s0 = tid; s0 < n_new; s0 += CB * NT) {
        bool ok[CB]; int node[CB], slot[CB], tokid[CB]; int4 nr[CB]; unsigned long long key[CB]; unsigned fvis[CB];
        int l_tre[CB], l_wid[CB], ent[CB];
#pragma unroll
        for (int k = 0; k < CB; k++) {
          const int s = s0 + k * NT;
          ok[k] = s < n_new;
          const int2 t2 = ok[k] ? TOUCHED(s) : make_int2(0, -1);
          node[k] = t2.x; slot[k] = t2.y;
        }
#pragma unroll
        for (int k = 0; k < CB; k++) nr[k] = lx.node_b(node[k]);
#pragma unroll
        for (int k = 0; k < CB; k++) {
          key[k] = 0ull; fvis[k] = 0u;
          if (ok[k]) {
            if (slot[k] >= 0) {
              key[k] = cl.lkey[slot[k]]; fvis[k] = ~cl.lfirst[slot[k]];
              cl.lkey[slot[k]] = 0ull; cl.lnode[slot[k]] = -1; cl.lfirst[slot[k]] = 0u;
            } else {
              key[k] = atomicExch(&NODEKEY(node[k]), 0ull);
              fvis[k] = ~atomicExch(&NODEFIRST(node[k]), 0u);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < CB; k++) {
          tokid[k] = 0;
          if (!ok[k]) continue;
          const int dense = ((dfa && t == 0) ? 0 : dbase[fvis[k] >> s1]) + (int)(fvis[k] & submask);
          const int w = dense >> 5, tw = w >> Wsh;
          int r = (int)tpre[tw];
          for (int x = tw * W; x < w; x++) r += __popc(bm_get(x));
          r += __popc(bm_get(w) & ((1u << (dense & 31)) - 1u));
          tokid[k] = r;
        }
        // of the winner's payload only what the score needs (the word whose last phone selects the state of a word-head
        // node) and what the pruning step overwrites (the trellis word a cross-word winner comes from); the rest is built
        // for the SURVIVORS after the pruning step, from the record {node, visiting index, trellis word, score} (round 6)
#pragma unroll
        for (int k = 0; k < CB; k++) {
          const unsigned vis = ~(unsigned)key[k];
          l_tre[k] = -2; l_wid[k] = -1;
          if (!ok[k]) continue;
          int j = (int)(vis >> s1);
          const int sub = (int)(vis & submask);
          if (dfa && t == 0) { l_tre[k] = -1; continue; }
          if (j < n_surv && sub < XW) {                          // intra-word: inherited
            if (nr[k].w >= JAMD_AS_RSET) l_wid[k] = sv.load(j).last_wid;
          } else {
            if (!(j < n_surv)) j = (int)(~(unsigned)sh.we_best);  // the factoring pass: from the best word end
            l_tre[k] = sv_atom[j];
            if (nr[k].w >= JAMD_AS_RSET) l_wid[k] = sv.load(j).pad0;
          }
        }
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
          const int s = tokid[k];
          const float score = unord((unsigned)(key[k] >> 32));
          float sc = score;
          if (ent[k] >= 0) {
            sc = score + ac[k];
            const unsigned b = ordz(sc);
            CURKEY(s) = b;
            if (b > mymax) mymax = b;
            if (b < mymin) mymin = b;
          } else {
            ARCQ(atomicAdd(&sh.n_arc, 1)) = make_int2(s, ~ent[k]);
          }
          REC(s) = u32x4{(unsigned)node[k], ~(unsigned)key[k], (unsigned)l_tre[k], __float_as_uint(sc)};
        }
      }
      __syncthreads();
      PROBE(2, 6);
      // state-set reductions (outprob_cd(), outprob.c:287-400): four, two or one lane per (token, set), so that the
      // frame's sets go through in one round when they can; eight member loads in flight per lane
      const int n_set = uni(sh.n_arc);
      const int lps = n_set <= NT / 4 ? 4 : (n_set <= NT / 2 ? 2 : 1), lsh = lps == 4 ? 2 : (lps == 2 ? 1 : 0);
      const int sub = tid & (lps - 1), lane = tid & 63;
      // the lane split (jamd_beam_prune_stats() [13..15]): LDS adds that return nothing, from the thread whose wave has the
      // fewest items below (thread 0's has the most, and the other [8..11] updates)
      if (tid == NT - 1) { atomicAdd(&sh.pst[15], n_set); if (lps != 4) atomicAdd(&sh.pst[lps == 2 ? 13 : 14], 1); }
      for (int q0 = 0; q0 < n_set; q0 += NT >> lsh) {
        const int q = q0 + (tid >> lsh);
        const bool act = q < n_set;
        const int2 it = act ? ARCQ(q) : make_int2(0, 0);
        const int a = act ? lx.set_off(it.y) : 0, bnd = act ? lx.set_off(it.y + 1) : 0;
        const float sc0 = (act && sub == 0) ? __uint_as_float(REC(it.x).w) : 0.0f;      // in flight beside the member loads
        float r;
        if (lx.cdset_method == JAMD_IWCD_NBEST && lx.cdmax_num <= 4) {
          r = lx.cdmax_num <= 3 ? nbest_of_set<3>(lx, row, a, bnd, sub, lps) : nbest_of_set<4>(lx, row, a, bnd, sub, lps);
        } else if (lx.cdset_method == JAMD_IWCD_MAX) {
          float m_ = JAMD_LOG_ZERO;
          for (int m = a + sub; m < bnd; m += 8 * lps) {
            int ix[8]; float pv[8];
#pragma unroll
            for (int jj = 0; jj < 8; jj++) ix[jj] = (m + lps * jj < bnd) ? lx.set_states(m + lps * jj) : -1;
#pragma unroll
            for (int jj = 0; jj < 8; jj++) pv[jj] = (ix[jj] >= 0) ? row[ix[jj]] : JAMD_LOG_ZERO;
#pragma unroll
            for (int jj = 0; jj < 8; jj++) if (m_ < pv[jj]) m_ = pv[jj];
          }
          for (int src = 1; src < lps; src++) { const float c = __shfl(m_, (lane & ~(lps - 1)) + src, 64); if (m_ < c) m_ = c; }
          r = m_;
        } else {
          r = (act && sub == 0) ? cd_reduce(row, lx.set_states_ptr(), a, bnd, lx.cdset_method, lx.cdmax_num) : 0.0f;
        }
        if (act && sub == 0) {
          const float sc = sc0 + r;
          REC(it.x).w = __float_as_uint(sc);
          const unsigned b = ordz(sc);
          CURKEY(it.x) = b;
          if (b > mymax) mymax = b;
          if (b < mymin) mymin = b;
        }
      }
      atomicMax(&sh.maxbits, mymax);
      atomicMin(&sh.minbits, mymin);
    }
    __syncthreads();
    row_request(t + 1);
    PHASE(2);
    {
      const float mx = unord(sh.maxbits);
      thr = (wk.width >= 0.0f) ? (mx - wk.width) : JAMD_LOG_ZERO;
      if (t == 0) thr = JAMD_LOG_ZERO;
    }
    if (n_new == 0) {
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
    // ---- D: rank pruning with the reference's heap; the next frame visits sv[0..n_keep) in this order
    const int n_keep = exact_prune<WIDE, NT>(sh, &CURKEY(0), n_new, wk.beam, Hlds, xw.heap_cap, Hglob, pm, welist, xw.prune_mode, Gcol, (TIMED && (JAMD_XBEAM_PROBE == 0 || JAMD_XBEAM_PROBE == 3 || JAMD_XBEAM_PROBE == 5 || JAMD_XBEAM_PROBE == 6)) ? ph : nullptr);
    // ---- E: the survivors' records (create_token() / propagate_token(): TOKEN2's last_tre, last_cword, last_lscore ...).
    //         Only the <= beam tokens that are kept get one: step C left {node, visiting index, trellis word, score} for every
    //         token (16 bytes instead of 32), and the sources' records and the LM look-ups are read for the survivors only.
    {
      constexpr int CB = JAMD_XBEAM_CB;
      for (int s0 = tid; s0 < n_keep; s0 += CB * NT) {
        bool ok[CB]; int node[CB]; int4 nr[CB]; u32x4 rec[CB];
        int l_tre[CB], l_cword[CB], l_wid[CB], lmreq[CB], l_to[CB];       // l_to: forward-DFA state (TOKEN2.to_state), 0 without one
        float l_ls[CB];
#pragma unroll
        for (int k = 0; k < CB; k++) {
          const int jn = s0 + k * NT;
          ok[k] = jn < n_keep;
          rec[k] = ok[k] ? REC(welist[jn]) : u32x4{0u, 0u, 0u, 0u};
          node[k] = (int)rec[k].x;
        }
#pragma unroll
        for (int k = 0; k < CB; k++) nr[k] = lx.node_b(node[k]);
        // the winner's payload from its visiting index (the sources are the OLD survivors: the new ones go through CUR())
#pragma unroll
        for (int k = 0; k < CB; k++) {
          const unsigned vis = rec[k].y;
          lmreq[k] = 0; l_tre[k] = -1; l_cword[k] = -1; l_wid[k] = -1; l_ls[k] = 0.0f; l_to[k] = 0;
          if (!ok[k]) continue;
          int j = (int)(vis >> s1);
          const int sub = (int)(vis & submask);
          if (dfa && t == 0) {                                 // an initial token of the grammar
            l_ls[k] = lx.init_lscore(sub);
            if (lx.nfwd) l_to[k] = lx.init_to_state(sub);      // :1739-1747
          } else if (j < n_surv && sub < XW) {                 // intra-word
            const Tok tk = sv.load(j);
            l_tre[k] = tk.last_tre; l_cword[k] = tk.last_cword; l_wid[k] = tk.last_wid; l_to[k] = tk.pad1;   // (:2120: the state is inherited)
            if (node[k] != tk.node && nr[k].y != 0) lmreq[k] = nr[k].y;   // beam_intra_word_core() :2069-2082
            else l_ls[k] = tk.last_lscore;
          } else {
            const bool iso = j < n_surv;
            if (!iso) j = (int)(~(unsigned)sh.we_best);        // the factoring pass: from the best word end
            const Tok tk = sv.load(j);
            const int sword = tk.pad0;
            const int last_word = lx.is_transparent(sword) ? tk.last_cword : sword;
            l_tre[k] = (int)rec[k].z; l_cword[k] = last_word; l_wid[k] = sword;
            if (dfa) {                                       // beam_inter_word() :2452-2461
              float ng = lx.penalty1;
              ng += (last_word >= 0) ? lx.cprob(last_word) : 0.0f;
              l_ls[k] = ng;
              if (lx.nfwd) l_to[k] = fwd_next(lx, tk.pad1, lx.root_cat(lx.startnum - 1 - (sub - XW)));   // the arc step B found (:2415-2420)
            } else if (iso) {                                // beam_inter_word() :2430-2438
              float p = 0.0f;
              if (last_word >= 0) {
                if (lx.iwtab) p = lx.iwtab[(size_t)lx.wton(last_word) * lx.isolatenum + (sub - XW)];
                else { const int wn = lx.scword(nr[k].y); p = bigram_prob(lx, lx.wton(last_word), lx.wton(wn)) + lx.cprob(wn); }
              }
              l_ls[k] = p * lmw + pen;
            } else {                                         // beam_inter_word_factoring() :2572-2573
              l_ls[k] = lx.fscore(-nr[k].y) * lmw + pen;
            }
          }
        }
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
            float p = 0.0f;
            if (l_cword[k] >= 0) {
              if (lmreq[k] < 0) p = fs[k];
              else if ((int)(unsigned)(mm[k] >> 32) == ctx[k]) p = __uint_as_float((unsigned)mm[k]);
              else p = max_successor_prob(lx, l_cword[k], lmreq[k], memo);
            }
            l_ls[k] = p * lmw + pen;
          }
        }
#pragma unroll
        for (int k = 0; k < CB; k++) {
          if (!ok[k]) continue;
          Tok nw;
          nw.node = node[k]; nw.score = __uint_as_float(rec[k].w); nw.pad0 = nr[k].x; nw.pad1 = l_to[k];
          nw.last_tre = l_tre[k]; nw.last_cword = l_cword[k]; nw.last_wid = l_wid[k]; nw.last_lscore = l_ls[k];
          if constexpr (WIDE) { XSv<true> svn; svn.p = reinterpret_cast<u32x4 *>(ub + (par ? wk.o_sv : wk.o_cur)); svn.store(s0 + k * NT, nw); }
          else CUR(s0 + k * NT) = nw;
        }
      }
    }
    __syncthreads();
    if constexpr (WIDE) par ^= 1;
    else { for (int j = tid; j < n_keep; j += NT) sv.store(j, CUR(j)); }   // (LDS: the sources had to be read first)
    if (tid == 0) sh.n_surv = n_keep;
    // the pruning step used the cell area: empty it again
    for (int i = tid; i < cl.nslot; i += NT) { cl.lkey[i] = 0ull; cl.lnode[i] = -1; cl.lfirst[i] = 0u; }
    __syncthreads();
    PHASE(3);
  }
  __syncthreads();

#ifdef JAMD_DEV
#define XBEAM_PROBE4 if (TIMED && JAMD_XBEAM_PROBE == 4) res->phase_us[7] = (int)((clock64() - cyc0) * 100ull / (wall_clock64() - wall0));   /* MHz */
#else
#define XBEAM_PROBE4
#endif
  // (wide layout, survivors at the head of the CUR() area: the next launch finds them at o_sv)
  XBEAM_END(if (!stopped && par) {
              const u32x4 *src = (const u32x4 *)(ub + wk.o_cur);
              u32x4 *dst = (u32x4 *)(ub + wk.o_sv);
              for (int i = tid; i < 2 * sh.n_surv; i += NT) dst[i] = src[i];
            }, XBEAM_PROBE4);
#undef XBEAM_PROBE4
}

}  // namespace

#include "beam_exact_mp.h"

namespace {

// diagnostic: the pruning step alone on given score bits (tests/test_prune_order.py fuzzes it against the
// sequential heap)
template <bool WIDE, int NT, bool FULL>
__global__ void __launch_bounds__(NT) prune_order_kernel(XWork xw, const unsigned *keys, int n, int k, int *out, int *nout,
                                                         unsigned long long *hglob, u32x4 *gcol, unsigned char *gsweep, int *arr) {
  __shared__ XShared sh;
  extern __shared__ __align__(16) unsigned char dyn_lds[];
  PruneMem pm;
  PRUNE_MEM_FILL(pm, xw, dyn_lds, gsweep, nullptr);
  lds_i32 *svid = (lds_i32 *)(dyn_lds + xw.off_we);
  unsigned mx = 0u, mn = 0xffffffffu;
  for (int i = threadIdx.x; i < n; i += NT) { const unsigned b = keys[i]; if (b > mx) mx = b; if (b < mn) mn = b; }
  if (threadIdx.x == 0) { sh.maxbits = 0u; sh.minbits = 0xffffffffu; sh.sw_info = 0; sh.sw_ticks = 0; sh.sw_nev_out = 0; for (int i = 0; i < 8; i++) sh.sw_prof[i] = 0; for (int i = 0; i < 4; i++) sh.df_prof[i] = 0; }
  __syncthreads();
  atomicMax(&sh.maxbits, mx); atomicMin(&sh.minbits, mn);
  __syncthreads();
  const int nk = exact_prune<WIDE, NT, FULL>(sh, keys, n, k, (lds_u64 *)(dyn_lds + xw.off_heap), xw.heap_cap, hglob, pm, svid,
                                         xw.prune_mode, gcol, nullptr, arr);
  for (int j = threadIdx.x; j < nk; j += NT) out[j] = svid[j];
  if (threadIdx.x == 0) { nout[0] = nk; nout[1] = sh.sw_info; nout[2] = sh.sw_ticks; nout[3] = sh.sw_nev_out; for (int i = 0; i < 8; i++) nout[4 + i] = sh.sw_prof[i]; for (int i = 0; i < 4; i++) nout[12 + i] = sh.df_prof[i]; }
}

}  // namespace

namespace jamdb {

hipError_t xbeam_prepare() {
  const void *fn[] = {(const void *)beam_exact_kernel<false, false, NT>, (const void *)beam_exact_kernel<true, false, NT>,
                      (const void *)beam_exact_kernel<false, true, NT>, (const void *)beam_exact_kernel<true, true, NT>,
                      (const void *)beam_exact_mp_kernel<false, false, NT>, (const void *)beam_exact_mp_kernel<true, false, NT>,
                      (const void *)beam_exact_mp_kernel<false, true, NT>, (const void *)beam_exact_mp_kernel<true, true, NT>,
                      (const void *)prune_order_kernel<false, NT, false>, (const void *)prune_order_kernel<true, NT, false>,
                      (const void *)prune_order_kernel<false, NT, true>, (const void *)prune_order_kernel<true, NT, true>};
  for (const void *f : fn) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds);
    if (e != hipSuccess) return e;
  }
  // the half shape is always the wide layout (xbeam_layout())
  const void *fh[] = {(const void *)beam_exact_kernel<false, true, kHalfNT>, (const void *)beam_exact_kernel<true, true, kHalfNT>,
                      (const void *)beam_exact_mp_kernel<false, true, kHalfNT>, (const void *)beam_exact_mp_kernel<true, true, kHalfNT>,
                      (const void *)prune_order_kernel<true, kHalfNT, false>};
  for (const void *f : fh) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kHalfDynLds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

void xbeam_launch(const LexDev &lx, const XWork &xw0, const float *scores, int nstate, const int *d_utt_off, int nutt,
                  int smode, bool timed, hipStream_t st) {
  XWork xw = xw0;
  xbeam_place(&xw, nstate);
  const int lds = xw.lds_bytes + (xw.w.row_cache ? 4 * nstate : 0);
  const dim3 grid(nutt), block(xw.nt);
  // the shape dispatch, once for every kernel of this file: the half shape is always the wide layout (xbeam_layout())
#define XBEAM_BY_SHAPE(LAUNCH) do { if (xw.nt == kHalfNT) LAUNCH(true, kHalfNT); else if (xw.wide) LAUNCH(true, NT); else LAUNCH(false, NT); } while (0)
#define XBEAM_LAUNCH(KERNEL, W, N)                                                                                           \
  do {                                                                                                                       \
    if (timed) hipLaunchKernelGGL((KERNEL<true, W, N>), grid, block, lds, st, XKArgs{lx, xw}, scores, nstate, d_utt_off, smode); \
    else hipLaunchKernelGGL((KERNEL<false, W, N>), grid, block, lds, st, XKArgs{lx, xw}, scores, nstate, d_utt_off, smode);      \
  } while (0)
#define XBEAM_LAUNCH_X(W, N) XBEAM_LAUNCH(beam_exact_kernel, W, N)
#define XBEAM_LAUNCH_MP(W, N) XBEAM_LAUNCH(beam_exact_mp_kernel, W, N)      /* multipath lexicons: their own frame (beam_exact_mp.h) */
  if (xw.mp) XBEAM_BY_SHAPE(XBEAM_LAUNCH_MP);
  else XBEAM_BY_SHAPE(XBEAM_LAUNCH_X);
#undef XBEAM_LAUNCH_MP
#undef XBEAM_LAUNCH_X
#undef XBEAM_LAUNCH
}

void xbeam_prune_order_launch(const XWork &xw, const unsigned *d_keys, int n, int k, int *d_out, int *d_nout,
                              unsigned long long *d_hglob, u32x4 *d_collect, unsigned char *d_sweep, int *d_arr, hipStream_t st) {
#define XBEAM_LAUNCH_P(W, N) hipLaunchKernelGGL((prune_order_kernel<W, N, false>), dim3(1), dim3(N), xw.lds_bytes, st, xw, d_keys, n, k, d_out, d_nout, d_hglob, d_collect, d_sweep, nullptr)
  if (d_arr) {                                          // the whole array (exact_prune<FULL>: full shape only)
    if (xw.wide) hipLaunchKernelGGL((prune_order_kernel<true, NT, true>), dim3(1), dim3(NT), xw.lds_bytes, st, xw, d_keys, n, k, d_out, d_nout, d_hglob, d_collect, d_sweep, d_arr);
    else hipLaunchKernelGGL((prune_order_kernel<false, NT, true>), dim3(1), dim3(NT), xw.lds_bytes, st, xw, d_keys, n, k, d_out, d_nout, d_hglob, d_collect, d_sweep, d_arr);
  }
  else XBEAM_BY_SHAPE(XBEAM_LAUNCH_P);
#undef XBEAM_LAUNCH_P
#undef XBEAM_BY_SHAPE
}

size_t xbeam_sweep_bytes(int beam) { return sweep_global_bytes(beam + 256); }

}  // namespace jamdb
