// beam_lexicon_image.h -- the part of the tree lexicon that needs no device: lexicon_check() range-checks every index a
// first-pass kernel will follow (a truncated or corrupt blob must be refused, not read out of bounds on the host or the
// device), lexicon_image() packs all arrays into the one arena LexDev (beam_common.h) addresses by 32-bit offsets and
// flattens the multipath roots.  Plain C++ without a HIP header: csrc/beam_lexicon_api.hip wraps it in the C ABI, and
// tests/lexicon_image_check.cpp compiles it alone under the host sanitizers.  A refusal returns false with the whole
// message, the caller's name included, in `err`.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "beam_lex_arrays.h"
#include "julius_amd.h"

namespace jamdb {

constexpr int kLexNbestMax = 16;             // jamd::kNbestMax (jamd_device.h; beam_lexicon_api.hip asserts they agree)

// The arena's records, as the kernels read them (int4 + int4, int2, float2, int4)
struct LexNode { int self_a, next_a, ac_off, ac_end, stend, scid, out_id, out_kind; };   // self_a / next_a: float bits
struct LexIsoRoot { int node, word; };                  // LexDev::iso_root: {root node, successor word scword[scid[root]]}
struct LexSharedRoot { int node; float fscore; };       // LexDev::shared_root: {root node (its bits in a float), fscore[-scid[root]]}
struct LexMpArc { int to, a, slot, tag; };              // see LexHost::o_mp_iso
static_assert(sizeof(LexNode) == 32 && sizeof(LexIsoRoot) == 8 && sizeof(LexSharedRoot) == 8 && sizeof(LexMpArc) == 16,
              "the records of the lexicon arena");

// What the host keeps of a lexicon beside LexDev (jamd_lexicon is one of these)
struct LexHost {
  int maxfan = 2, nscword = 0;
  bool multipath = false;          // JAMD_LM_MULTIPATH lexicon: its own frame (beam_exact_mp.h; strict order: beam_strict_kernel<true>)
  bool mp_parallel = false;        // ... and no root reaches a word-end node along its own arcs: the frame-parallel kernel can decode it
  // multipath: where a token entering a word goes (the root has no output: beam.c:2467-2510) -- one int4 {target node,
  // transition bits, root number * maxfan + transition number, root number / fscore bits} per transition a root really has,
  // in visiting order; byte offsets into the lexicon arena + entry counts (XWork carries them to the kernel)
  unsigned o_mp_iso = 0, o_mp_shared = 0, o_mp_start = 0;
  int n_mp_iso = 0, n_mp_shared = 0, n_mp_start = 0;
  // ... and the nodes those transitions lead to, numbered densely: int [nnode], -1 = never entered from a root.  Only such a
  // node can meet a token of the frame's second half, so the per-utterance "which token sits on this node" table of the
  // multipath frame (XWork::o_nodetok) has n_mp_tgt entries instead of nnode (a few KB that stay in L2 instead of a
  // megabyte per utterance written four bytes at a time).
  unsigned o_mp_tgt = 0;
  int n_mp_tgt = 0;
};

// LexDev's scalar fields, by name
#define JAMD_LEX_SCALARS(X)                                                                                        \
  X(int, nnode) X(int, nword) X(int, startnum) X(int, isolatenum) X(int, nshared) X(int, nlc) X(int, cdset_method)  \
  X(int, cdmax_num) X(int, head_silwid) X(int, tail_silwid) X(int, ng_mode) X(int, ng_unk_id)                       \
  X(float, ng_unk_num_log) X(float, lm_weight) X(float, lm_penalty) X(float, lm_penalty_trans)                      \
  X(int, lm_type) X(int, ncat) X(int, ninit) X(float, penalty1) X(int, nfwd)

struct LexImage : LexHost {
  std::vector<unsigned char> arena;      // every array 16-byte aligned, an empty one as 16 bytes of zeros
  size_t bytes = 0;                      // the arena's size (also where only the size was asked for)
#define X(T, name) T name = 0;
  JAMD_LEX_SCALARS(X)
#undef X
#define X(T, name) unsigned o_##name = 0;
  JAMD_LEX_ARRAYS(X)
#undef X
  unsigned o_node_a = 0, o_node_b = 0, o_scid = 0;
};

__attribute__((format(printf, 2, 3))) static inline bool lex_errf(std::string &err, const char *fmt, ...) {
  char b[512];                               // (what jamd_last_error() keeps)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  err = b;
  return false;
}

struct LexKind {
  int lmt; bool multipath, wordmode, dfa;    // dfa: the two LM_DFA variants share everything but the word boundary
  explicit LexKind(const jamd_lexicon_desc &h)
      : lmt(h.lm_type & 0xff), multipath((h.lm_type & JAMD_LM_MULTIPATH) != 0), wordmode(lmt == JAMD_LM_WORD),
        dfa(lmt == JAMD_LM_DFA || wordmode) {}
};

static inline void lexicon_image(const jamd_lexicon_desc &h, LexImage *im, bool size_only);

// Every index a kernel or lexicon_image() will follow is range-checked here, every array they read is there.
// `max_bytes`: what 32-bit offsets can address (a test asks for less).
static inline bool lexicon_check(const jamd_lexicon_desc &h, std::string &err, size_t max_bytes = (size_t)1 << 32) {
  const LexKind k(h);
  const bool wordmode = k.wordmode, dfa = k.dfa;
  if ((h.lm_type & ~(0xff | JAMD_LM_MULTIPATH)) != 0 || (k.lmt != JAMD_LM_NGRAM && !dfa))
    return lex_errf(err, "jamd_lexicon_create: lm_type=%d", h.lm_type);
  if (dfa && (h.ninit < 0 || (h.ninit > 0 && (!h.init_node || !h.init_lscore)) ||
              (!wordmode && (h.ncat <= 0 || !h.cat_pair || !h.start2wid))))
    return lex_errf(err, "jamd_lexicon_create: grammar descriptor incomplete (ncat=%d ninit=%d)", h.ncat, h.ninit);
  if (h.nnode <= 0 || h.nword <= 0 || h.startnum < 0 || (!dfa && (h.head_silwid < 0 || h.head_silwid >= h.nword)))
    return lex_errf(err, "jamd_lexicon_create: bad sizes (nnode=%d nword=%d head_silwid=%d)", h.nnode, h.nword, h.head_silwid);
  if (h.isolatenum < 0 || (dfa && h.isolatenum != 0) || h.nlc < 0 || h.nlcrow < 0 || h.nset < 0 || h.nfscore < 0 || h.nscword < 0 ||
      h.ng_nword < 0 || h.ng_nbigram < 0 || h.nfwd < 0)
    return lex_errf(err, "jamd_lexicon_create: bad table sizes (isolatenum=%d nlc=%d nlcrow=%d nset=%d nfscore=%d nscword=%d ng_nword=%d ng_nbigram=%d nfwd=%d)",
                    h.isolatenum, h.nlc, h.nlcrow, h.nset, h.nfscore, h.nscword, h.ng_nword, h.ng_nbigram, h.nfwd);
  if (h.cdset_method == JAMD_IWCD_NBEST && (h.cdmax_num < 1 || h.cdmax_num > kLexNbestMax))
    return lex_errf(err, "jamd_lexicon_create: cdmax_num=%d outside [1,%d]", h.cdmax_num, kLexNbestMax);
  if (!h.ac_off || !h.self_a || !h.next_a || !h.stend || !h.scid || !h.out_id || !h.out_kind ||
      (h.startnum > 0 && !h.startnode) || !h.word_head || !h.wton || h.ac_off[0] != 0)
    return lex_errf(err, "jamd_lexicon_create: NULL or malformed node arrays");
  if ((h.startnum > 0 && !h.start2isolate) || !h.word_lc || !h.wordend_a || !h.cprob || !h.is_transparent ||
      (h.nlcrow > 0 && !h.lc_tab) || (h.nfscore > 0 && !h.fscore) || (h.nscword > 0 && !h.scword))
    return lex_errf(err, "jamd_lexicon_create: NULL root, word or successor arrays");
  if ((h.ng_nword > 0 && (!h.ng_uni_prob || !h.ng_uni_bo || !h.ng_bi_bgn || !h.ng_bi_num)) ||
      (h.ng_nbigram > 0 && (!h.ng_bi_wid || !h.ng_bi_prob)))
    return lex_errf(err, "jamd_lexicon_create: NULL N-gram arrays");
  for (int i = 0; i < h.nnode; i++) {
    if (h.ac_off[i + 1] < h.ac_off[i]) return lex_errf(err, "jamd_lexicon_create: ac_off not monotone at node %d", i);
    if (h.stend[i] >= h.nword) return lex_errf(err, "jamd_lexicon_create: node %d ends word %d of %d", i, h.stend[i], h.nword);
    if (h.scid[i] >= h.nscword || (h.scid[i] < 0 && -(long long)h.scid[i] >= h.nfscore))
      return lex_errf(err, "jamd_lexicon_create: node %d has successor id %d outside the tables", i, h.scid[i]);
    if (h.scid[i] > 0 && (h.scword[h.scid[i]] < 0 || h.scword[h.scid[i]] >= h.nword))
      return lex_errf(err, "jamd_lexicon_create: successor id %d names word %d of %d", h.scid[i], h.scword[h.scid[i]], h.nword);
    // what node_outprob() (beam_common.h) follows: a state id, a state set, a row of lc_tab
    const int kind = h.out_kind[i], id = h.out_id[i];
    if (kind > JAMD_AS_NONE || (kind == JAMD_AS_STATE && id < 0) || (kind == JAMD_AS_LSET && (id < 0 || id >= h.nset)) ||
        ((kind == JAMD_AS_RSET || kind == JAMD_AS_LRSET) && (id < 0 || id >= h.nlcrow)))
      return lex_errf(err, "jamd_lexicon_create: node %d has output %d of kind %d outside the tables", i, id, kind);
  }
  if (h.next_a[h.nnode - 1] != JAMD_LOG_ZERO) return lex_errf(err, "jamd_lexicon_create: the last node has a next node");
  const int nac = h.ac_off[h.nnode];
  if (nac > 0 && (!h.ac_to || !h.ac_a)) return lex_errf(err, "jamd_lexicon_create: arc arrays missing");
  for (int a = 0; a < nac; a++)
    if (h.ac_to[a] < 0 || h.ac_to[a] >= h.nnode) return lex_errf(err, "jamd_lexicon_create: arc %d leads to node %d of %d", a, h.ac_to[a], h.nnode);
  for (int s = 0; s < h.startnum; s++)
    if (h.startnode[s] < 0 || h.startnode[s] >= h.nnode) return lex_errf(err, "jamd_lexicon_create: root %d is node %d of %d", s, h.startnode[s], h.nnode);
  for (int w = 0; w < h.nword; w++)
    if (h.word_head[w] < -1 || h.word_head[w] >= h.nnode) return lex_errf(err, "jamd_lexicon_create: word %d starts at node %d of %d", w, h.word_head[w], h.nnode);
  if (h.nset > 0) {
    if (!h.set_off || !h.set_states || h.set_off[0] != 0) return lex_errf(err, "jamd_lexicon_create: state-set table missing");
    for (int i = 0; i < h.nset; i++)
      if (h.set_off[i + 1] < h.set_off[i]) return lex_errf(err, "jamd_lexicon_create: set_off not monotone at %d", i);
    for (int s = 0; s < h.set_off[h.nset]; s++)
      if (h.set_states[s] < 0) return lex_errf(err, "jamd_lexicon_create: negative state in set table");
  }
  // the left-context table: a state id, or ~(state set); the column a word selects
  for (size_t x = 0; x < (size_t)h.nlcrow * ((size_t)h.nlc + 1); x++)
    if (h.lc_tab[x] < 0 && ~h.lc_tab[x] >= h.nset) return lex_errf(err, "jamd_lexicon_create: lc_tab entry %zu names state set %d of %d", x, ~h.lc_tab[x], h.nset);
  for (int w = 0; w < h.nword && h.nlcrow > 0; w++)
    if (h.word_lc[w] < 0 || h.word_lc[w] > h.nlc) return lex_errf(err, "jamd_lexicon_create: word %d selects left context %d of %d", w, h.word_lc[w], h.nlc);
  if (!dfa) {
    // the 2-gram as bigram_prob() / search_bigram() (beam_common.h) read it
    for (int w = 0; w < h.nword; w++)
      if (h.wton[w] < 0 || h.wton[w] >= h.ng_nword) return lex_errf(err, "jamd_lexicon_create: word %d is N-gram entry %d of %d", w, h.wton[w], h.ng_nword);
    for (int c = 0; c < h.ng_nword; c++)
      if (h.ng_bi_bgn[c] >= 0 && (h.ng_bi_num[c] < 0 || h.ng_bi_bgn[c] >= h.ng_nbigram || h.ng_bi_num[c] > h.ng_nbigram - h.ng_bi_bgn[c]))
        return lex_errf(err, "jamd_lexicon_create: 2-grams of entry %d leave the table", c);
  }
  std::vector<int> iso((size_t)h.isolatenum, -1);
  for (int s = 0; s < h.startnum && !dfa; s++) {
    const int i = h.start2isolate[s], sc = h.scid[h.startnode[s]];
    if (i >= 0) {
      if (i >= h.isolatenum || iso[(size_t)i] >= 0) return lex_errf(err, "jamd_lexicon_create: start2isolate out of range or repeated");
      iso[(size_t)i] = s;
      if (sc <= 0 || sc >= h.nscword) return lex_errf(err, "jamd_lexicon_create: isolated root without a successor word");
    } else if (sc >= 0 || -sc >= h.nfscore) return lex_errf(err, "jamd_lexicon_create: shared root without a factoring value");
  }
  if (h.nword >= (1 << 30)) return lex_errf(err, "jamd_lexicon_create: nword=%d too large", h.nword);
  for (size_t i = 0; i < iso.size(); i++)
    if (iso[i] < 0) return lex_errf(err, "jamd_lexicon_create: isolated root %d is not assigned", (int)i);
  if (dfa) {
    for (int s = 0; s < h.startnum && !wordmode; s++) {
      const int w = h.start2wid[s];
      if (w < 0 || w >= h.nword || h.wton[w] < 0 || h.wton[w] >= h.ncat) return lex_errf(err, "jamd_lexicon_create: root %d has no valid category", s);
    }
    for (int w = 0; w < h.nword && !wordmode; w++)
      if (h.wton[w] < 0 || h.wton[w] >= h.ncat) return lex_errf(err, "jamd_lexicon_create: word %d outside the categories", w);
    for (int e = 0; e < h.ninit; e++)
      if (h.init_node[e] < 0 || h.init_node[e] >= h.nnode) return lex_errf(err, "jamd_lexicon_create: bad initial node");
    if (h.nfwd > 0) {
      // forward DFA: every index the kernels will follow is checked here
      if (wordmode || !h.fwd_off || !h.fwd_label || !h.fwd_to || !h.init_to_state || h.fwd_off[0] != 0)
        return lex_errf(err, "jamd_lexicon_create: forward DFA descriptor incomplete");
      for (int s = 0; s < h.nfwd; s++)
        if (h.fwd_off[s + 1] < h.fwd_off[s]) return lex_errf(err, "jamd_lexicon_create: forward DFA offsets not monotone");
      for (int a = 0; a < h.fwd_off[h.nfwd]; a++)
        if (h.fwd_to[a] < 0 || h.fwd_to[a] >= h.nfwd) return lex_errf(err, "jamd_lexicon_create: forward DFA arc %d leaves the automaton", a);
      for (int e = 0; e < h.ninit; e++)
        if (h.init_to_state[e] < -1 || h.init_to_state[e] >= h.nfwd) return lex_errf(err, "jamd_lexicon_create: bad initial forward-DFA state");
    }
  }
  LexImage size;
  lexicon_image(h, &size, true);
  if (size.bytes >= max_bytes) return lex_errf(err, "jamd_lexicon_create: lexicon image exceeds 4 GB");
  return true;
}

// The image of a descriptor that lexicon_check() accepts.  Every array is appended (16-byte aligned) to one host image
// that is uploaded once; the kernel sees the base pointer and 32-bit byte offsets (see LexDev).  With size_only the
// arena stays empty and only im->bytes is told (the offsets are then those of the image, truncated to 32 bits).
static inline void lexicon_image(const jamd_lexicon_desc &h, LexImage *im, bool size_only = false) {
  const LexKind k(h);
  const bool multipath = k.multipath, wordmode = k.wordmode, dfa = k.dfa;
  *im = LexImage();
  std::vector<unsigned char> &arena = im->arena;
  size_t size = 0;
  auto put = [&](const void *src, size_t bytes) {
    const size_t at = (size + 15) & ~(size_t)15;
    size = at + (bytes ? bytes : 16);
    if (!size_only) {
      arena.resize(size);
      if (bytes) memcpy(arena.data() + at, src, bytes);
    }
    return (unsigned)at;
  };
#define UP(field, src, n) im->o_##field = put((src), sizeof(*(src)) * (size_t)(n))
  im->nnode = h.nnode; im->nword = h.nword; im->startnum = h.startnum; im->isolatenum = h.isolatenum;
  im->nlc = h.nlc; im->cdset_method = h.cdset_method; im->cdmax_num = h.cdmax_num;
  im->head_silwid = h.head_silwid; im->tail_silwid = h.tail_silwid; im->ng_mode = h.ng_mode; im->ng_unk_id = h.ng_unk_id;
  im->ng_unk_num_log = h.ng_unk_num_log; im->lm_weight = h.lm_weight; im->lm_penalty = h.lm_penalty;
  im->lm_penalty_trans = h.lm_penalty_trans;
  im->nscword = h.nscword; im->multipath = multipath;
  const int nac = h.ac_off[h.nnode], nset_states = h.nset ? h.set_off[h.nset] : 0;
  auto bits = [](float f) { int b; memcpy(&b, &f, 4); return b; };
  int maxfan = 2;
  std::vector<LexNode> node((size_t)h.nnode);          // one 32-byte record per node (LexDev::node_a / node_b / scid)
  std::vector<int> word_end((size_t)h.nword, -1);
  for (int i = 0; i < h.nnode; i++) {
    maxfan = std::max(maxfan, 2 + h.ac_off[i + 1] - h.ac_off[i]);
    node[(size_t)i] = {bits(h.self_a[i]), bits(h.next_a[i]), h.ac_off[i], h.ac_off[i + 1],
                       h.stend[i], h.scid[i], h.out_id[i], (int)h.out_kind[i]};
    if (h.stend[i] >= 0) word_end[(size_t)h.stend[i]] = i;
  }
  im->maxfan = maxfan;
  if (multipath) {
    // A root that reaches a word-end node along its own arcs (a word of tee models only): a cross-word transition would
    // improve a word end inside the loop that visits the word ends (beam.c:2779-2825), and the result depends on the loop's
    // position -- strict order only.  Roots are non-emitting; so is every word end of a multipath lexicon.
    bool ok = true;
    for (int s = 0; s < h.startnum && ok; s++) {
      const int r = h.startnode[s];
      if (h.self_a[r] != JAMD_LOG_ZERO && h.stend[r] >= 0) ok = false;
      if (h.next_a[r] != JAMD_LOG_ZERO && h.stend[r + 1] >= 0) ok = false;
      for (int a = h.ac_off[r]; a < h.ac_off[r + 1]; a++) if (h.stend[h.ac_to[a]] >= 0) ok = false;
    }
    im->mp_parallel = ok;
  }
  // both root lists in the order beam_inter_word() / beam_inter_word_factoring() visit them (stid from
  // startnum-1 down to 0, beam.c:2334 / :2562): the exact-order kernel numbers its candidates by list index
  std::vector<LexIsoRoot> iso_root;
  std::vector<LexSharedRoot> shared_root;
  for (int s = h.startnum - 1; s >= 0 && !dfa; s--) {
    const int nd = h.startnode[s], sc = h.scid[nd];
    if (h.start2isolate[s] >= 0) iso_root.push_back({nd, h.scword[sc]});
    else shared_root.push_back({nd, h.fscore[-sc]});
  }
  im->nshared = (int)shared_root.size();
  im->o_node_a = put(node.data(), node.size() * sizeof(LexNode));
  im->o_node_b = im->o_node_a + 16u; im->o_scid = im->o_node_a + 20u;
  UP(ac_to, h.ac_to, nac); UP(ac_a, h.ac_a, nac);
  UP(iso_root, iso_root.data(), iso_root.size()); UP(shared_root, shared_root.data(), shared_root.size());
  UP(word_end, word_end.data(), word_end.size());
  if (multipath) {
    // the roots' own transitions, flattened once (csrc/beam_exact_mp.h, step B')
    auto expand = [&](int root, int rootno, int tag, std::vector<LexMpArc> &out) {
      if (h.self_a[root] != JAMD_LOG_ZERO) out.push_back({root, bits(h.self_a[root]), rootno * maxfan + 0, tag});
      if (h.next_a[root] != JAMD_LOG_ZERO) out.push_back({root + 1, bits(h.next_a[root]), rootno * maxfan + 1, tag});
      for (int a = h.ac_off[root]; a < h.ac_off[root + 1]; a++)
        out.push_back({h.ac_to[a], bits(h.ac_a[a]), rootno * maxfan + 2 + (a - h.ac_off[root]), tag});
    };
    std::vector<LexMpArc> e_iso, e_shared, e_start;
    const int head_root = dfa ? -1 : h.word_head[h.head_silwid];
    for (size_t i = 0; i < iso_root.size(); i++)
      if (iso_root[i].node != head_root) expand(iso_root[i].node, (int)i, (int)i, e_iso);                            // :2336-2341
    for (size_t r = 0; r < shared_root.size(); r++)
      if (shared_root[r].node != head_root) expand(shared_root[r].node, (int)r, bits(shared_root[r].fscore), e_shared);   // :2566-2571
    for (int rv = 0; rv < h.startnum && dfa && !wordmode; rv++) {
      const int r = h.startnum - 1 - rv;                                                                              // roots from startnum-1 down (:2334)
      expand(h.startnode[r], rv, r, e_start);
    }
    im->o_mp_iso = put(e_iso.data(), e_iso.size() * sizeof(LexMpArc)); im->n_mp_iso = (int)e_iso.size();
    im->o_mp_shared = put(e_shared.data(), e_shared.size() * sizeof(LexMpArc)); im->n_mp_shared = (int)e_shared.size();
    im->o_mp_start = put(e_start.data(), e_start.size() * sizeof(LexMpArc)); im->n_mp_start = (int)e_start.size();
    std::vector<int> tgt((size_t)h.nnode, -1);
    for (const std::vector<LexMpArc> *v : {&e_iso, &e_shared, &e_start})
      for (const LexMpArc &ent : *v) if (tgt[(size_t)ent.to] < 0) tgt[(size_t)ent.to] = im->n_mp_tgt++;
    im->o_mp_tgt = put(tgt.data(), tgt.size() * sizeof(int));
  }
  UP(startnode, h.startnode, h.startnum); UP(start2isolate, h.start2isolate, h.startnum);
  UP(lc_tab, h.lc_tab, (size_t)h.nlcrow * (h.nlc + 1)); UP(word_lc, h.word_lc, h.nword);
  UP(set_off, h.set_off, h.nset ? h.nset + 1 : 0); UP(set_states, h.set_states, nset_states);
  UP(wordend_a, h.wordend_a, h.nword); UP(wton, h.wton, h.nword); UP(cprob, h.cprob, h.nword);
  UP(is_transparent, h.is_transparent, h.nword); UP(word_head, h.word_head, h.nword);
  UP(fscore, h.fscore, h.nfscore); UP(scword, h.scword, h.nscword);
  UP(ng_uni_prob, h.ng_uni_prob, h.ng_nword); UP(ng_uni_bo, h.ng_uni_bo, h.ng_nword);
  UP(ng_bi_bgn, h.ng_bi_bgn, h.ng_nword); UP(ng_bi_num, h.ng_bi_num, h.ng_nword);
  UP(ng_bi_wid, h.ng_bi_wid, h.ng_nbigram); UP(ng_bi_prob, h.ng_bi_prob, h.ng_nbigram);
  im->lm_type = k.lmt; im->ncat = dfa ? h.ncat : 0; im->ninit = dfa ? h.ninit : 0; im->penalty1 = dfa ? h.penalty1 : 0.0f;
  if (dfa) {
    std::vector<int> root_cat((size_t)h.startnum, 0);
    for (int s = 0; s < h.startnum && !wordmode; s++) root_cat[(size_t)s] = h.wton[h.start2wid[s]];
    UP(cat_pair, h.cat_pair, wordmode ? 0 : (size_t)h.ncat * h.ncat); UP(root_cat, root_cat.data(), root_cat.size());
    UP(init_node, h.init_node, h.ninit); UP(init_lscore, h.init_lscore, h.ninit);
    if (h.nfwd > 0) {
      UP(fwd_off, h.fwd_off, (size_t)h.nfwd + 1); UP(fwd_label, h.fwd_label, (size_t)h.fwd_off[h.nfwd]);
      UP(fwd_to, h.fwd_to, (size_t)h.fwd_off[h.nfwd]); UP(init_to_state, h.init_to_state, h.ninit);
      im->nfwd = h.nfwd;
    }
  }
#undef UP
  im->bytes = size;
}

}  // namespace jamdb
