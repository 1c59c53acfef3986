// beam_strict.hip -- STRICT-ORDER first pass (verification mode, JAMD_ORDER_STRICT / jamd_beam_set_strict_order()).
//
// The reference resolves exact score ties by its visiting order, which is the output of
// a partial heap sort over token indices (beam.c:1342-1516) applied frame after frame; no
// parallel schedule can reproduce that.  This kernel therefore runs the reference's
// SEQUENTIAL algorithm -- same token creation order, same heap permutation, same
// first-writer-wins propagation -- with ONE LANE PER UTTERANCE (parallel only across the
// utterances of a batch).  It is two to three orders of magnitude slower per utterance
// than beam_pass1_kernel and exists so that the word trellis can be checked bit for bit
// against the reference in every case, ties included.  Same inputs, same result records.
#include "jamd_device.h"

#include "beam_host.h"

namespace jamdb {
struct STok { int last_tre, last_cword; float last_lscore, score; int node; int to_state; };   // to_state: forward-DFA state (TOKEN2.to_state), 0 without one

}  // namespace jamdb

namespace {
using namespace jamdb;

struct SBeam {
  const LexDev *lx; const float *sc; int S;
  STok *tl[2]; int *ti[2]; int tnum[2]; int *token; int cap;
  int tn, tlx, n_start, n_end;
  float thr, we_best_score; int we_best_node, we_best_tre, we_best_cword;
  jamd_trellis_atom *atoms; int natom, atom_cap; bool overflow;
};

__device__ int s_create_token(SBeam &b) {                       // create_token() beam.c:1148
  const int id = b.tnum[b.tn];
  if (id + 1 >= b.cap) { b.overflow = true; return id > 0 ? id - 1 : 0; }
  b.tnum[b.tn]++;
  b.ti[b.tn][id] = id;
  return id;
}

// sort_token_upward / _downward (beam.c:1342 / :1414): 1-based heap over tindex
__device__ void s_sort(SBeam &b, int neednum, int totalnum, bool upward) {
  STok *tl = b.tl[b.tn]; int *ti = b.ti[b.tn];
#define SD_(A) ti[(A) - 1]
#define SV_(A) (tl[ti[(A) - 1]].score)
#define BEFORE_(x, y) (upward ? ((x) < (y)) : ((x) > (y)))
#define STOP_(x, y) (upward ? ((x) >= (y)) : ((x) <= (y)))
  int n, root, child, parent, s;
  for (root = totalnum / 2; root >= 1; root--) {
    s = SD_(root); parent = root;
    while ((child = parent * 2) <= totalnum) {
      if (child < totalnum && BEFORE_(SV_(child), SV_(child + 1))) child++;
      if (STOP_(tl[s].score, SV_(child))) break;
      SD_(parent) = SD_(child); parent = child;
    }
    SD_(parent) = s;
  }
  n = totalnum;
  while (n > totalnum - neednum) {
    s = SD_(n); SD_(n) = SD_(1); n--; parent = 1;
    while ((child = parent * 2) <= n) {
      if (child < n && BEFORE_(SV_(child), SV_(child + 1))) child++;
      if (STOP_(tl[s].score, SV_(child))) break;
      SD_(parent) = SD_(child); parent = child;
    }
    SD_(parent) = s;
  }
#undef SD_
#undef SV_
#undef BEFORE_
#undef STOP_
}
__device__ void s_sort_no_order(SBeam &b, int neednum) {         // sort_token_no_order() :1492
  const int totalnum = b.tnum[b.tn], restnum = totalnum - neednum;
  if (neednum >= totalnum) { b.n_start = 0; b.n_end = totalnum - 1; }
  else if (neednum < restnum) { s_sort(b, neednum, totalnum, true); b.n_start = totalnum - neednum; b.n_end = totalnum - 1; }
  else { s_sort(b, restnum, totalnum, false); b.n_start = 0; b.n_end = neednum - 1; }
}

__device__ void s_propagate(SBeam &b, int next_node, float next_score, int last_tre, int last_cword,
                            float last_lscore, int to_state = 0) {   // propagate_token() :1945
  if (next_score <= JAMD_LOG_ZERO) return;
  int id = b.token[next_node];
  if (id >= 0) {
    STok &tk = b.tl[b.tn][id];
    if (tk.score < next_score) { tk.last_tre = last_tre; tk.last_cword = last_cword; tk.last_lscore = last_lscore; tk.score = next_score; tk.to_state = to_state; }
  } else {
    id = s_create_token(b);
    STok &tk = b.tl[b.tn][id];
    tk.last_tre = last_tre; tk.last_cword = last_cword; tk.last_lscore = last_lscore; tk.score = next_score;
    tk.node = next_node; tk.to_state = to_state; b.token[next_node] = id;
  }
}

__device__ void s_intra_core(SBeam &b, const STok &tk, int next_node, float next_a) {   // :2004
  const LexDev &lx = *b.lx;
  float tmpsum = tk.score + next_a, ng = JAMD_LOG_ZERO;
  const int nscid = (next_node != tk.node) ? lx.scid(next_node) : 0;
  if (nscid != 0) {
    ng = max_successor_prob(lx, tk.last_cword, nscid) * lx.lm_weight + lx.lm_penalty;
    tmpsum -= tk.last_lscore;
    tmpsum += ng;
  }
  if (ng == JAMD_LOG_ZERO) ng = tk.last_lscore;
  s_propagate(b, next_node, tmpsum, tk.last_tre, tk.last_cword, ng, tk.to_state);     // :2120
}

__device__ int s_save_trellis(SBeam &b, const STok &tk, int sword, int t) {            // :2209
  if (b.natom >= b.atom_cap) { b.overflow = true; return b.natom - 1; }
  jamd_trellis_atom a;
  a.wid = sword; a.backscore = tk.score; a.last_tre = tk.last_tre; a.lscore = tk.last_lscore;
  a.begintime = (short)((tk.last_tre < 0 ? -1 : b.atoms[tk.last_tre].endtime) + 1);
  a.endtime = (short)(t - 1);
  b.atoms[b.natom] = a;
  return b.natom++;
}

// ---- multipath lexicons (hmminfo->multipath) ----------------------------------------------------------
// A multipath model (model-skip / state-skip transitions) builds a lexicon whose word-begin and
// word-end nodes have no output, and beam.c runs a different frame for it (:2747-2836): word-internal
// transitions of every survivor, THEN the beam over the new tokens, THEN trellis words and cross-word
// transitions from the word ends among those (the root has no output, so the token is passed on along
// the root's own arcs within the frame, :2467-2510), output probabilities only on emitting nodes
// (:2930-2943); frame 0 already goes through this (pass1.c:239) and one transition-only call ends the
// input (:3066-3073).  The kernel below is instantiated for both frames (MP): same helpers, same records,
// `if constexpr (MP)` at the points where the reference tests its multipath flag.
// Exact by construction; the CPU restatement of the same frame is pinned to the reference on
// multipath tasks (tests/test_beam_oracle.py), the kernel against both (tests/test_beam_gpu.py::test_multipath_*).
__device__ void s_enter_word_mp(SBeam &b, const LexDev &lx, int root, float tmpsum, int tre, int last_word, float ng, int to_state = 0) {
  const int4 na = lx.node_a(root);
  const float a_self = __int_as_float(na.x), a_next = __int_as_float(na.y);
  if (a_self != JAMD_LOG_ZERO) s_propagate(b, root, tmpsum + a_self, tre, last_word, ng, to_state);
  if (a_next != JAMD_LOG_ZERO) s_propagate(b, root + 1, tmpsum + a_next, tre, last_word, ng, to_state);
  for (int e = na.z; e < na.w; e++) s_propagate(b, lx.ac_to(e), tmpsum + lx.ac_a(e), tre, last_word, ng, to_state);
}

// a cross-word candidate arrives at a root: the root takes it (s_propagate()), or -- multipath, the root has no
// output -- passes it on along its own arcs
template <bool MP>
__device__ void s_enter_word(SBeam &b, int root, float tmpsum, int tre, int last_word, float ng, int to_state = 0) {
  if constexpr (MP) s_enter_word_mp(b, *b.lx, root, tmpsum, tre, last_word, ng, to_state);
  else s_propagate(b, root, tmpsum, tre, last_word, ng, to_state);
}

// Binds this lane's utterance and resets its result record.  Returns the utterance's frame count; <= 0: nothing to
// decode (the record says JAMD_PASS1_FAIL).
__device__ int s_setup(SBeam &b, const LexDev &lx, const Work &wk, const StrictWork &sw, const float *scores, int S,
                       const int *utt_off, int u, jamd_pass1_result *res) {
  const int t_begin = utt_off[u], T = utt_off[u + 1] - t_begin;
  b.lx = &lx; b.sc = scores + (size_t)t_begin * S; b.S = S;
  for (int i = 0; i < 2; i++) { b.tl[i] = sw.tl[i] + (size_t)u * sw.cap; b.ti[i] = sw.ti[i] + (size_t)u * sw.cap; b.tnum[i] = 0; }
  b.token = sw.token + (size_t)u * wk.nnode; b.cap = sw.cap;
  b.atoms = reinterpret_cast<jamd_trellis_atom *>(wk.slices + (size_t)u * wk.utt_stride + wk.o_atoms); b.natom = 0; b.atom_cap = wk.atom_cap; b.overflow = false;
  res->status = JAMD_PASS1_OK; res->natom = 0; res->wnum = 0; res->score = JAMD_LOG_ZERO; res->died_at = -1;
  res->ties = res->ties_node = res->ties_wordend = res->ties_cut = 0; res->frames = T; res->max_tokens = 0;
  for (int i = 0; i < 8; i++) res->phase_us[i] = 0;
  if (T <= 0) { res->status = JAMD_PASS1_FAIL; return T; }
  for (int i = 0; i < wk.nnode; i++) b.token[i] = -1;               // init_nodescore() :1587-1590
  b.tn = 0; b.tlx = 1;
  return T;
}

// word-internal transitions of one survivor: beam_intra_word() :2154
__device__ void s_intra_word(SBeam &b, const STok &tk) {
  const LexDev &lx = *b.lx;
  const int node = tk.node;
  const int4 na = lx.node_a(node);
  const float a_self = __int_as_float(na.x), a_next = __int_as_float(na.y);
  if (a_self != JAMD_LOG_ZERO) s_intra_core(b, tk, node, a_self);
  if (a_next != JAMD_LOG_ZERO) s_intra_core(b, tk, node + 1, a_next);
  for (int e = na.z; e < na.w; e++) s_intra_core(b, tk, lx.ac_to(e), lx.ac_a(e));
}

// A token on a word-end node at frame t: its trellis word, then the cross-word transitions (none after the last
// frame and for isolated words).  head_root: multipath N-gram only, the root no word is followed by (else -1).
template <bool MP>
__device__ void s_word_end(SBeam &b, const STok &tk, int sword, int t, bool final, int head_root) {
  const LexDev &lx = *b.lx;
  const float lmw = lx.lm_weight, pen = lx.lm_penalty;
  const int node = tk.node;
  const int tre = s_save_trellis(b, tk, sword, t);
  if (final || lx.lm_type == JAMD_LM_WORD) return;                        // :2875: isolated words stop here
  if (lx.lm_type != JAMD_LM_NGRAM) {                                      // beam_inter_word(), grammar branch
    const int last_word = lx.is_transparent(sword) ? tk.last_cword : sword;
    for (int stid = lx.startnum - 1; stid >= 0; stid--) {
      if (!lx.cat_pair(lx.wton(sword) * lx.ncat + lx.root_cat(stid))) continue;      // :2404-2412
      int next_state = 0;
      if (lx.nfwd) { next_state = fwd_next(lx, tk.to_state, lx.root_cat(stid)); if (next_state < 0) continue; }   // :2412-2422
      float tmpsum = tk.score;
      if constexpr (!MP) tmpsum += lx.wordend_a(sword);
      float ng = lx.penalty1;                                             // :2452-2461
      ng += (last_word >= 0) ? lx.cprob(last_word) : 0.0f;
      tmpsum += ng;
      s_enter_word<MP>(b, lx.startnode(stid), tmpsum, tre, last_word, ng, next_state);
    }
  } else if (sword != lx.tail_silwid) {                                   // beam_inter_word() :2271
    const bool tr = lx.is_transparent(sword) != 0;
    const int last_word = tr ? tk.last_cword : sword;
    float tmpprob = tk.score;
    if constexpr (!MP) tmpprob += lx.wordend_a(sword);                    // no wordend_a in multipath (:2307)
    if (b.we_best_score < tmpprob) {
      b.we_best_score = tmpprob; b.we_best_node = node; b.we_best_tre = tre; b.we_best_cword = tk.last_cword;
    }
    for (int stid = lx.startnum - 1; stid >= 0; stid--) {
      const int next_node = lx.startnode(stid);
      if (MP && next_node == head_root) continue;                         // :2336-2341
      if (lx.start2isolate(stid) == -1) continue;
      const int wn = lx.scword(lx.scid(next_node));
      const float p = (last_word < 0) ? 0.0f
                      : bigram_prob(lx, lx.wton(last_word), lx.wton(wn)) + lx.cprob(wn);
      float tmpsum = tk.score;
      if constexpr (!MP) tmpsum += lx.wordend_a(sword);
      const float ng = p * lmw + pen;
      tmpsum += ng;
      if (tr && tk.last_cword >= 0 && lx.is_transparent(tk.last_cword)) tmpsum += lx.lm_penalty_trans;
      s_enter_word<MP>(b, next_node, tmpsum, tre, last_word, ng);
    }
  }
}

// find_1pass_result() :399 + trace_backptr() :294-340.  False: no sentence ends in the trellis.
__device__ bool s_result(const SBeam &b, jamd_pass1_result *res) {
  const LexDev &lx = *b.lx;
  int best = -1;
  if (lx.lm_type != JAMD_LM_NGRAM) {                                             // :433-455
    int lt = -1;
    for (int i = b.natom - 1; i >= 0 && lt < 0; i--) if (b.atoms[i].backscore > JAMD_LOG_ZERO) lt = b.atoms[i].endtime;
    for (int i = 0; i < b.natom; i++) {        // atoms are emitted in time order
      const jamd_trellis_atom &a = b.atoms[i];
      if (a.endtime != lt || !(a.backscore > JAMD_LOG_ZERO)) continue;
      if (best < 0 || b.atoms[best].backscore < a.backscore ||
          (b.atoms[best].backscore == a.backscore && a.wid < b.atoms[best].wid)) best = i;
    }
  } else {
    // atoms are emitted in time order: the first hit from the back is the tail word ending latest
    for (int i = b.natom - 1; i >= 0; i--)
      if (b.atoms[i].wid == lx.tail_silwid && b.atoms[i].backscore > JAMD_LOG_ZERO) { best = i; break; }
  }
  if (best < 0) return false;
  int n = 0, a = best;
  int rev[MAXSEQ];
  rev[n++] = b.atoms[a].wid;
  while (b.atoms[a].begintime > 0 && n < MAXSEQ) { a = b.atoms[a].last_tre; rev[n++] = b.atoms[a].wid; }
  for (int k = 0; k < n; k++) res->wseq[k] = rev[n - 1 - k];
  res->wnum = n; res->score = b.atoms[best].backscore;
  return true;
}

template <bool MP>
__global__ void __launch_bounds__(64)
beam_strict_kernel(LexDev lx, Work wk, StrictWork sw, const float *__restrict__ scores, int S,
                   const int *__restrict__ utt_off, int nutt) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= nutt) return;
  jamd_pass1_result *res = wk.res + u;
  SBeam b;
  const int T = s_setup(b, lx, wk, sw, scores, S, utt_off, u, res);
  if (T <= 0) return;
  const float lmw = lx.lm_weight, pen = lx.lm_penalty;
  int status = JAMD_PASS1_OK, died_at = -1, max_tokens = 1;
  const bool dfa = lx.lm_type != JAMD_LM_NGRAM;
  const int head_root = (MP && !dfa) ? lx.word_head(lx.head_silwid) : -1;
  // the initial tokens; multipath: score = LM score only (:1733), the first output probability is frame 0's
  if (dfa) {                                                         // init_nodescore() :1669-1757, :1762-1788
    for (int e = 0; e < lx.ninit; e++) {
      const int id = s_create_token(b);
      STok &nw = b.tl[b.tn][id];
      const int node = lx.init_node(e);
      nw.last_lscore = lx.init_lscore(e); nw.last_tre = -1; nw.last_cword = -1;
      if constexpr (MP) nw.score = nw.last_lscore;
      else { const int4 nr = lx.node_b(node); nw.score = node_outprob(lx, b.sc, nr.w, nr.z, -1) + nw.last_lscore; }
      nw.node = node; nw.to_state = lx.nfwd ? lx.init_to_state(e) : 0; b.token[node] = id;       // :1739-1747
    }
  } else {                                                           // init_nodescore() :1622-1665
    const int id = s_create_token(b);
    STok &nw = b.tl[b.tn][id];
    const int node = lx.word_head(lx.head_silwid);
    const int4 nr = lx.node_b(node);
    float ls = (nr.y != 0) ? max_successor_prob(lx, -1, nr.y) : 0.0f;
    ls = ls * lmw + pen;
    nw.last_lscore = ls; nw.last_tre = -1; nw.last_cword = -1;
    if constexpr (MP) nw.score = ls;
    else nw.score = node_outprob(lx, b.sc, nr.w, nr.z, -1) + ls;
    nw.node = node; nw.to_state = 0; b.token[node] = id;
  }
  s_sort_no_order(b, wk.beam);
  b.thr = JAMD_LOG_ZERO;

  // get_back_trellis_proceed() :2663.  Multipath: frame 0 goes through it too, and t == T is get_back_trellis_end()'s
  // final, transition-only call
  for (int t = MP ? 0 : 1; MP ? t <= T : t < T; t++) {
    const bool final = MP && t == T;
    b.tlx = b.tn; b.tn = b.tn ? 0 : 1;
    const int tl = b.tlx, tn = b.tn;
    b.we_best_score = JAMD_LOG_ZERO;
    for (int j = 0; j < b.tnum[tl]; j++) b.token[b.tl[tl][j].node] = -1;        // clear_tokens() :1122
    for (int j = b.n_start; j <= b.n_end; j++) {                     // multipath: :2752-2769
      const STok tk = b.tl[tl][b.ti[tl][j]];
      if (tk.score <= JAMD_LOG_ZERO) continue;
      if (tk.score < b.thr) continue;
      s_intra_word(b, tk);
      if constexpr (!MP) {                                           // the survivors' own word ends, in the same visit
        const int sword = lx.node_b(tk.node).x;
        if (sword >= 0) s_word_end<false>(b, tk, sword, t, false, -1);
      }
    }
    if constexpr (MP) {
      s_sort_no_order(b, wk.beam);                                   // :2774, over the new tokens
      for (int j = b.n_start; j <= b.n_end; j++) {                   // :2779-2825: the word ends among those
        const STok tk = b.tl[tn][b.ti[tn][j]];
        if (tk.score < b.thr) continue;
        const int sword = lx.node_b(tk.node).x;
        if (sword >= 0) s_word_end<true>(b, tk, sword, t, final, head_root);
      }
    }
    if (!dfa && b.we_best_score > JAMD_LOG_ZERO) {                               // beam_inter_word_factoring() :2549
      const int sword = lx.node_b(b.we_best_node).x;
      const int last_word = lx.is_transparent(sword) ? b.we_best_cword : sword;
      for (int stid = lx.startnum - 1; stid >= 0; stid--) {
        const int next_node = lx.startnode(stid);
        if (MP && next_node == head_root) continue;                              // :2566-2571
        if (lx.start2isolate(stid) != -1) continue;
        const float ng = lx.fscore(-lx.scid(next_node)) * lmw + pen;
        float tmpsum = b.we_best_score;
        tmpsum += ng;
        if (lx.is_transparent(sword) && b.we_best_cword >= 0 && lx.is_transparent(b.we_best_cword)) tmpsum += lx.lm_penalty_trans;
        if (tmpsum < b.thr) continue;
        s_enter_word<MP>(b, next_node, tmpsum, b.we_best_tre, last_word, ng);
      }
    }
    float pmax = JAMD_LOG_ZERO;
    if (!final) {                                                                // :2944-2951; multipath :2930-2943
      const float *row = b.sc + (size_t)t * S;
      for (int j = 0; j < b.tnum[tn]; j++) {
        STok &tk = b.tl[tn][b.ti[tn][j]];
        const int4 nr = lx.node_b(tk.node);
        if (MP && nr.w == JAMD_AS_NONE) continue;                                // non-output node
        const int lw = tk.last_tre < 0 ? -1 : b.atoms[tk.last_tre].wid;
        tk.score += node_outprob(lx, row, nr.w, nr.z, lw);
        if (pmax < tk.score) pmax = tk.score;
      }
    }
    b.thr = (wk.width >= 0.0f) ? (pmax - wk.width) : JAMD_LOG_ZERO;
    if (b.tnum[tn] > max_tokens) max_tokens = b.tnum[tn];
    b.tnum[tl] = 0;
    s_sort_no_order(b, wk.beam);
    if (b.tnum[tn] == 0) { if (!final) { status = JAMD_PASS1_DIED; died_at = t; } break; }
    if (b.overflow) break;
  }
  if (status == JAMD_PASS1_OK && !b.overflow) {
    if constexpr (!MP) {                                                         // get_back_trellis_end() :3076
      b.tlx = b.tn; b.tn = b.tn ? 0 : 1;
      for (int j = b.n_start; j <= b.n_end; j++) {
        const STok tk = b.tl[b.tlx][b.ti[b.tlx][j]];
        const int sword = lx.node_b(tk.node).x;
        if (sword >= 0) s_save_trellis(b, tk, sword, T);
      }
    }
    if (!s_result(b, res)) status = JAMD_PASS1_FAIL;
  }
  if (b.overflow) status = JAMD_PASS1_OVERFLOW;
  res->status = status; res->died_at = died_at; res->natom = b.natom; res->max_tokens = max_tokens;
}

}  // namespace

namespace jamdb {

int sbeam_prepare(StrictMem *sm, const Work &w, bool multipath, int max_utts) {
  if (sm->view.token != nullptr) return JAMD_OK;
  const size_t U = (size_t)max_utts;
  // a node holds at most one token per frame; multipath frames also create tokens behind every root
  const int cap = multipath ? w.nnode + 2 : w.tok_cap + 2;
  int rc;
  for (int i = 0; i < 2; i++) {
    if ((rc = sm->tl[i].alloc(U * cap)) != JAMD_OK || (rc = sm->ti[i].alloc(U * cap)) != JAMD_OK) return rc;
  }
  if ((rc = sm->token.alloc(U * w.nnode)) != JAMD_OK) return rc;
  sm->view = StrictWork{{sm->tl[0], sm->tl[1]}, {sm->ti[0], sm->ti[1]}, sm->token, cap};   // (token last: set = all of it is there)
  return JAMD_OK;
}

void sbeam_launch(const LexDev &lx, const Work &w, const StrictWork &sw, bool multipath, const float *scores, int nstate,
                  const int *d_utt_off, int nutt, hipStream_t st) {
  const dim3 grid((nutt + 63) / 64), block(64);
  if (multipath) hipLaunchKernelGGL(beam_strict_kernel<true>, grid, block, 0, st, lx, w, sw, scores, nstate, d_utt_off, nutt);
  else hipLaunchKernelGGL(beam_strict_kernel<false>, grid, block, 0, st, lx, w, sw, scores, nstate, d_utt_off, nutt);
}

}  // namespace jamdb
