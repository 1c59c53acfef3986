// lexicon_image_check.cpp -- the device-free part of the tree lexicon (julius_amd/csrc/beam_lexicon_image.h: the check of
// every index a first-pass kernel follows, the arena image, the flattened multipath roots) as a program of its own, so
// that tests/test_lexicon_host.py can build it with -fsanitize=address,undefined and run it over the smallest
// descriptors that still have every part -- each array a heap block of exactly its length, so an overread is seen --
// and over every refusal of lexicon_check(), one corrupted field per case.
//
//   lexicon_image_check HEADER     HEADER: path of beam_lexicon_image.h, whose refusals are counted against the cases;
//                                  prints one line per case; exit 0 when every case behaved
#include "beam_lexicon_image.h"

#include <fstream>
#include <functional>
#include <set>
#include <sstream>

using namespace jamdb;

static int failures = 0;
static void expect(bool ok, const std::string &what) {
  printf("%s: %s\n", ok ? "ok" : "FAILED", what.c_str());
  if (!ok) failures++;
}

static const float LZ = JAMD_LOG_ZERO;
static int bits(float f) { int b; memcpy(&b, &f, 4); return b; }

// A descriptor whose arrays are vectors: an empty one is passed as NULL.
struct Lex {
  jamd_lexicon_desc s{};               // the scalar fields (the pointers are set by desc())
  std::vector<float> self_a, next_a, ac_a, wordend_a, cprob, fscore, ng_uni_prob, ng_uni_bo, ng_bi_prob, init_lscore;
  std::vector<int> ac_off, ac_to, stend, scid, out_id, lc_tab, word_lc, set_off, set_states, startnode, start2isolate, wton,
      word_head, scword, ng_bi_bgn, ng_bi_num, ng_bi_wid, start2wid, init_node, fwd_off, fwd_label, fwd_to, init_to_state;
  std::vector<unsigned char> out_kind, is_transparent, cat_pair;
  jamd_lexicon_desc desc() const {
    jamd_lexicon_desc d = s;
#define P(name) d.name = name.empty() ? nullptr : name.data();
    P(self_a) P(next_a) P(ac_a) P(wordend_a) P(cprob) P(fscore) P(ng_uni_prob) P(ng_uni_bo) P(ng_bi_prob) P(init_lscore)
    P(ac_off) P(ac_to) P(stend) P(scid) P(out_id) P(lc_tab) P(word_lc) P(set_off) P(set_states) P(startnode) P(start2isolate)
    P(wton) P(word_head) P(scword) P(ng_bi_bgn) P(ng_bi_num) P(ng_bi_wid) P(start2wid) P(init_node) P(fwd_off) P(fwd_label)
    P(fwd_to) P(init_to_state) P(out_kind) P(is_transparent) P(cat_pair)
#undef P
    return d;
  }
};

// Three words under an N-gram: roots 0 (isolated 0, word 0 = the head silence), 3 (shared, word 2, one extra arc) and 6
// (isolated 1, word 1), each followed by one inner node and the word end; one state set, a 2 x 2 left-context table, one 2-gram.
static Lex ngram_lex() {
  Lex l;
  l.s.nnode = 9; l.s.nword = 3; l.s.startnum = 3; l.s.isolatenum = 2;
  l.self_a = {LZ, -0.5f, -0.5f, -0.6f, -0.5f, -0.5f, -0.4f, -0.5f, -0.5f};
  l.next_a = {-0.9f, -0.9f, LZ, -0.8f, -0.9f, LZ, -1.1f, -0.9f, LZ};
  l.ac_off = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1}; l.ac_to = {4}; l.ac_a = {-0.7f};
  l.stend = {-1, -1, 0, -1, -1, 2, -1, -1, 1};
  l.scid = {1, 0, 0, -1, 0, 0, 2, 0, 0};
  l.out_kind = {JAMD_AS_STATE, JAMD_AS_LSET, JAMD_AS_STATE, JAMD_AS_RSET, JAMD_AS_STATE, JAMD_AS_LRSET, JAMD_AS_STATE, JAMD_AS_STATE, JAMD_AS_STATE};
  l.out_id = {3, 0, 1, 0, 2, 1, 0, 4, 5};
  l.s.nlc = 1; l.s.nlcrow = 2; l.lc_tab = {0, ~0, 3, 1}; l.word_lc = {0, 1, 0};
  l.s.nset = 1; l.set_off = {0, 2}; l.set_states = {1, 2}; l.s.cdset_method = JAMD_IWCD_AVG; l.s.cdmax_num = 3;
  l.startnode = {0, 3, 6}; l.start2isolate = {0, -1, 1};
  l.wordend_a = {-0.3f, -0.3f, -0.3f}; l.wton = {0, 1, 2}; l.cprob = {0.f, -0.1f, -0.2f}; l.is_transparent = {1, 0, 0};
  l.word_head = {0, 6, 3}; l.s.head_silwid = 0; l.s.tail_silwid = 1;
  l.s.nfscore = 2; l.s.nscword = 3; l.fscore = {0.f, -2.5f}; l.scword = {0, 0, 1};
  l.s.ng_mode = JAMD_NG_NORMAL; l.s.ng_nword = 3; l.s.ng_nbigram = 1; l.s.ng_unk_id = 2; l.s.ng_unk_num_log = 0.5f;
  l.ng_uni_prob = {-1.f, -2.f, -3.f}; l.ng_uni_bo = {-0.1f, -0.2f, -0.3f};
  l.ng_bi_bgn = {0, -1, -1}; l.ng_bi_num = {1, 0, 0}; l.ng_bi_wid = {1}; l.ng_bi_prob = {-1.5f};
  l.s.lm_weight = 8.f; l.s.lm_penalty = -2.f; l.s.lm_penalty_trans = -1.f;
  l.s.lm_type = JAMD_LM_NGRAM;
  return l;
}

// Two words, one per category, each a root and its word end; two initial tokens; a forward DFA of two states.
static Lex grammar_lex() {
  Lex l;
  l.s.nnode = 4; l.s.nword = 2; l.s.startnum = 2; l.s.isolatenum = 0;
  l.self_a = {-0.5f, -0.5f, LZ, -0.5f}; l.next_a = {-0.9f, LZ, -0.8f, LZ};
  l.ac_off = {0, 0, 0, 0, 0};
  l.stend = {-1, 0, -1, 1}; l.scid = {0, 0, 0, 0}; l.s.nscword = 1; l.scword = {0};
  l.out_kind = {JAMD_AS_STATE, JAMD_AS_STATE, JAMD_AS_STATE, JAMD_AS_STATE}; l.out_id = {0, 1, 2, 3};
  l.word_lc = {0, 0};
  l.startnode = {0, 2}; l.start2isolate = {-1, -1};
  l.wordend_a = {-0.3f, -0.3f}; l.wton = {0, 1}; l.cprob = {0.f, 0.f}; l.is_transparent = {0, 0}; l.word_head = {0, 2};
  l.s.lm_weight = 1.f; l.s.lm_type = JAMD_LM_DFA;
  l.s.ncat = 2; l.cat_pair = {0, 1, 1, 0}; l.start2wid = {0, 1};
  l.s.ninit = 2; l.init_node = {0, 2}; l.init_lscore = {-1.f, -2.f}; l.s.penalty1 = -0.5f;
  l.s.nfwd = 2; l.fwd_off = {0, 1, 2}; l.fwd_label = {0, 1}; l.fwd_to = {1, 0}; l.init_to_state = {1, -1};
  return l;
}

static Lex word_lex() {
  Lex l = grammar_lex();
  l.s.lm_type = JAMD_LM_WORD; l.s.ncat = 0; l.cat_pair.clear(); l.start2wid.clear();
  l.s.nfwd = 0; l.fwd_off.clear(); l.fwd_label.clear(); l.fwd_to.clear(); l.init_to_state.clear();
  return l;
}

struct Span { std::string name; unsigned off; const void *src; size_t bytes; };

struct Want {                          // what the flattening rule gives, written out by hand
  int maxfan; bool mp_parallel;
  std::vector<LexIsoRoot> iso; std::vector<int> shared;        // iso_root; the nodes of shared_root
  std::vector<LexMpArc> mp_iso, mp_shared, mp_start; std::vector<int> tgt;
};

static void check_valid(const char *what, const Lex &l, const Want &want) {
  const jamd_lexicon_desc d = l.desc();
  const bool dfa = (d.lm_type & 0xff) != JAMD_LM_NGRAM, mp = (d.lm_type & JAMD_LM_MULTIPATH) != 0;
  std::string err;
  const bool ok = lexicon_check(d, err);
  expect(ok, std::string(what) + ": accepted" + (ok ? "" : " (" + err + ")"));
  if (!ok) return;
  LexImage im, sz;
  lexicon_image(d, &im);
  lexicon_image(d, &sz, true);
  const unsigned char *A = im.arena.data();
  expect(im.bytes == im.arena.size() && sz.bytes == im.bytes && sz.arena.empty() && sz.o_scword == im.o_scword, std::string(what) + ": size alone");
  // the root lists, in descending root order
  std::vector<LexSharedRoot> shared;
  for (int n : want.shared) shared.push_back({n, l.fscore[(size_t)-l.scid[(size_t)n]]});
  std::vector<int> word_end((size_t)d.nword, -1), root_cat;
  for (int i = 0; i < d.nnode; i++) if (l.stend[(size_t)i] >= 0) word_end[(size_t)l.stend[(size_t)i]] = i;
  for (int s = 0; s < d.startnum && dfa; s++) root_cat.push_back(l.start2wid.empty() ? 0 : l.wton[(size_t)l.start2wid[(size_t)s]]);
  std::vector<Span> sp;
#define SRC(name, v) sp.push_back({#name, im.o_##name, (v).data(), (v).size() * sizeof((v)[0])});
  SRC(ac_to, l.ac_to) SRC(ac_a, l.ac_a) SRC(iso_root, want.iso) SRC(shared_root, shared) SRC(word_end, word_end)
  SRC(startnode, l.startnode) SRC(start2isolate, l.start2isolate) SRC(lc_tab, l.lc_tab) SRC(word_lc, l.word_lc)
  SRC(set_off, l.set_off) SRC(set_states, l.set_states) SRC(wordend_a, l.wordend_a) SRC(wton, l.wton) SRC(cprob, l.cprob)
  SRC(is_transparent, l.is_transparent) SRC(word_head, l.word_head) SRC(fscore, l.fscore) SRC(scword, l.scword)
  SRC(ng_uni_prob, l.ng_uni_prob) SRC(ng_uni_bo, l.ng_uni_bo) SRC(ng_bi_bgn, l.ng_bi_bgn) SRC(ng_bi_num, l.ng_bi_num)
  SRC(ng_bi_wid, l.ng_bi_wid) SRC(ng_bi_prob, l.ng_bi_prob)
  if (dfa) { SRC(cat_pair, l.cat_pair) SRC(root_cat, root_cat) SRC(init_node, l.init_node) SRC(init_lscore, l.init_lscore) }
  if (d.nfwd > 0) { SRC(fwd_off, l.fwd_off) SRC(fwd_label, l.fwd_label) SRC(fwd_to, l.fwd_to) SRC(init_to_state, l.init_to_state) }
#undef SRC
  std::vector<LexNode> node;
  for (size_t i = 0; i < (size_t)d.nnode; i++)
    node.push_back({bits(l.self_a[i]), bits(l.next_a[i]), l.ac_off[i], l.ac_off[i + 1], l.stend[i], l.scid[i], l.out_id[i], (int)l.out_kind[i]});
  sp.push_back({"node", im.o_node_a, node.data(), node.size() * sizeof(LexNode)});
  if (mp) {
    sp.push_back({"mp_iso", im.o_mp_iso, want.mp_iso.data(), want.mp_iso.size() * sizeof(LexMpArc)});
    sp.push_back({"mp_shared", im.o_mp_shared, want.mp_shared.data(), want.mp_shared.size() * sizeof(LexMpArc)});
    sp.push_back({"mp_start", im.o_mp_start, want.mp_start.data(), want.mp_start.size() * sizeof(LexMpArc)});
    sp.push_back({"mp_tgt", im.o_mp_tgt, want.tgt.data(), want.tgt.size() * sizeof(int)});
  }
  bool placed = im.o_node_b == im.o_node_a + 16 && im.o_scid == im.o_node_a + 20, equal = true;
  std::sort(sp.begin(), sp.end(), [](const Span &a, const Span &b) { return a.off < b.off; });
  for (size_t i = 0; i < sp.size(); i++) {
    const size_t end = sp[i].off + (sp[i].bytes ? sp[i].bytes : 16);
    placed = placed && sp[i].off % 16 == 0 && end <= im.arena.size() && (i + 1 == sp.size() || end <= sp[i + 1].off);
    if (placed && sp[i].src && sp[i].bytes && memcmp(A + sp[i].off, sp[i].src, sp[i].bytes) != 0) {
      equal = false;
      printf("  %s differs from its source\n", sp[i].name.c_str());
    }
  }
  expect(placed, std::string(what) + ": every offset 16-byte aligned, in bounds, no overlap");
  expect(placed && equal, std::string(what) + ": every array, the node records and the root lists equal their source");
  expect(im.maxfan == want.maxfan && im.nshared == (int)want.shared.size() && im.nscword == d.nscword && im.multipath == mp &&
             im.mp_parallel == want.mp_parallel && im.lm_type == (d.lm_type & 0xff) && im.nfwd == d.nfwd &&
             im.ncat == (dfa ? d.ncat : 0) && im.ninit == (dfa ? d.ninit : 0) && im.nnode == d.nnode && im.nword == d.nword &&
             im.startnum == d.startnum && im.isolatenum == d.isolatenum && im.head_silwid == d.head_silwid && im.lm_weight == d.lm_weight,
         std::string(what) + ": maxfan, nshared, the multipath verdict and the scalar fields");
  if (mp)
    expect(im.n_mp_iso == (int)want.mp_iso.size() && im.n_mp_shared == (int)want.mp_shared.size() &&
               im.n_mp_start == (int)want.mp_start.size() && im.n_mp_tgt == 1 + *std::max_element(want.tgt.begin(), want.tgt.end()),
           std::string(what) + ": the multipath lists' counts");
}

static void check_all_valid() {
  const Lex n = ngram_lex();
  const int fs = bits(-2.5f);
  Want w{3, false, {{6, 1}, {0, 0}}, {3}, {}, {}, {}, {}};
  check_valid("N-gram", n, w);
  // multipath: root 6 (list index 0) has both transitions, root 0 is the head silence's and is left out; the shared
  // root's next node and its extra arc both lead to node 4
  Lex m = n;
  m.s.lm_type |= JAMD_LM_MULTIPATH;
  m.out_kind[0] = m.out_kind[3] = m.out_kind[6] = JAMD_AS_NONE;
  w.mp_parallel = true;
  w.mp_iso = {{6, bits(-0.4f), 0, 0}, {7, bits(-1.1f), 1, 0}};
  w.mp_shared = {{3, bits(-0.6f), 0, fs}, {4, bits(-0.8f), 1, fs}, {4, bits(-0.7f), 2, fs}};
  w.tgt = {-1, -1, -1, 2, 3, -1, 0, 1, -1};
  check_valid("multipath N-gram", m, w);
  m.ac_to[0] = 5;                        // the shared root's extra arc reaches the end of word 2
  w.mp_parallel = false;
  w.mp_shared[2].to = 5;
  w.tgt = {-1, -1, -1, 2, 3, 4, 0, 1, -1};
  check_valid("multipath N-gram, a root reaches a word end", m, w);
  const Lex g = grammar_lex();
  check_valid("grammar", g, Want{2, false, {}, {}, {}, {}, {}, {}});
  check_valid("word mode", word_lex(), Want{2, false, {}, {}, {}, {}, {}, {}});
  // multipath grammar: the roots from the last down, root 1 (node 2) has no self transition; both reach their word ends
  Lex gm = g;
  gm.s.lm_type |= JAMD_LM_MULTIPATH;
  Want gw{2, false, {}, {}, {}, {}, {{3, bits(-0.8f), 1, 1}, {0, bits(-0.5f), 2, 0}, {1, bits(-0.9f), 3, 0}}, {1, 2, -1, 0}};
  check_valid("multipath grammar", gm, gw);
}

// ---- every refusal once: (case, base descriptor, the one corruption, the text)
struct Refusal { const char *what; Lex (*base)(); std::function<void(Lex &)> corrupt; const char *text; size_t max_bytes; };
static const size_t k4G = (size_t)1 << 32;
static const std::vector<Refusal> kRefusals = {
  {"unknown flag bits", ngram_lex, [](Lex &l) { l.s.lm_type = 0x200; }, "jamd_lexicon_create: lm_type=512", k4G},
  {"unknown LM type", ngram_lex, [](Lex &l) { l.s.lm_type = 3; }, "jamd_lexicon_create: lm_type=3", k4G},
  {"negative ninit", grammar_lex, [](Lex &l) { l.s.ninit = -1; }, "jamd_lexicon_create: grammar descriptor incomplete (ncat=2 ninit=-1)", k4G},
  {"grammar without cat_pair", grammar_lex, [](Lex &l) { l.cat_pair.clear(); }, "jamd_lexicon_create: grammar descriptor incomplete (ncat=2 ninit=2)", k4G},
  {"word mode without init_lscore", word_lex, [](Lex &l) { l.init_lscore.clear(); }, "jamd_lexicon_create: grammar descriptor incomplete (ncat=0 ninit=2)", k4G},
  {"no nodes", ngram_lex, [](Lex &l) { l.s.nnode = 0; }, "jamd_lexicon_create: bad sizes (nnode=0 nword=3 head_silwid=0)", k4G},
  {"head silence past the words", ngram_lex, [](Lex &l) { l.s.head_silwid = 3; }, "jamd_lexicon_create: bad sizes (nnode=9 nword=3 head_silwid=3)", k4G},
  {"negative nset", ngram_lex, [](Lex &l) { l.s.nset = -1; }, "jamd_lexicon_create: bad table sizes (isolatenum=2 nlc=1 nlcrow=2 nset=-1 nfscore=2 nscword=3 ng_nword=3 ng_nbigram=1 nfwd=0)", k4G},
  {"grammar with isolated roots", grammar_lex, [](Lex &l) { l.s.isolatenum = 1; }, "jamd_lexicon_create: bad table sizes (isolatenum=1 nlc=0 nlcrow=0 nset=0 nfscore=0 nscword=1 ng_nword=0 ng_nbigram=0 nfwd=2)", k4G},
  {"cdmax_num", ngram_lex, [](Lex &l) { l.s.cdset_method = JAMD_IWCD_NBEST; l.s.cdmax_num = 17; }, "jamd_lexicon_create: cdmax_num=17 outside [1,16]", k4G},
  {"scid NULL", ngram_lex, [](Lex &l) { l.scid.clear(); }, "jamd_lexicon_create: NULL or malformed node arrays", k4G},
  {"ac_off starts at 1", ngram_lex, [](Lex &l) { l.ac_off[0] = 1; }, "jamd_lexicon_create: NULL or malformed node arrays", k4G},
  {"word_lc NULL", ngram_lex, [](Lex &l) { l.word_lc.clear(); }, "jamd_lexicon_create: NULL root, word or successor arrays", k4G},
  {"start2isolate NULL", grammar_lex, [](Lex &l) { l.start2isolate.clear(); }, "jamd_lexicon_create: NULL root, word or successor arrays", k4G},
  {"scword NULL", ngram_lex, [](Lex &l) { l.scword.clear(); }, "jamd_lexicon_create: NULL root, word or successor arrays", k4G},
  {"fscore NULL", ngram_lex, [](Lex &l) { l.fscore.clear(); }, "jamd_lexicon_create: NULL root, word or successor arrays", k4G},
  {"lc_tab NULL", ngram_lex, [](Lex &l) { l.lc_tab.clear(); }, "jamd_lexicon_create: NULL root, word or successor arrays", k4G},
  {"cprob NULL", ngram_lex, [](Lex &l) { l.cprob.clear(); }, "jamd_lexicon_create: NULL root, word or successor arrays", k4G},
  {"ng_bi_wid NULL", ngram_lex, [](Lex &l) { l.ng_bi_wid.clear(); }, "jamd_lexicon_create: NULL N-gram arrays", k4G},
  {"ng_uni_bo NULL", ngram_lex, [](Lex &l) { l.ng_uni_bo.clear(); }, "jamd_lexicon_create: NULL N-gram arrays", k4G},
  {"ac_off descends", ngram_lex, [](Lex &l) { l.ac_off[2] = -1; }, "jamd_lexicon_create: ac_off not monotone at node 1", k4G},
  {"word end past the words", ngram_lex, [](Lex &l) { l.stend[2] = 3; }, "jamd_lexicon_create: node 2 ends word 3 of 3", k4G},
  {"successor id past scword", ngram_lex, [](Lex &l) { l.scid[1] = 3; }, "jamd_lexicon_create: node 1 has successor id 3 outside the tables", k4G},
  {"factoring id past fscore", ngram_lex, [](Lex &l) { l.scid[4] = -2; }, "jamd_lexicon_create: node 4 has successor id -2 outside the tables", k4G},
  {"scword one element short", ngram_lex, [](Lex &l) { l.s.nscword = 2; l.scword.pop_back(); }, "jamd_lexicon_create: node 6 has successor id 2 outside the tables", k4G},
  {"fscore one element short", ngram_lex, [](Lex &l) { l.s.nfscore = 1; l.fscore.pop_back(); }, "jamd_lexicon_create: node 3 has successor id -1 outside the tables", k4G},
  {"successor word past the words", ngram_lex, [](Lex &l) { l.scword[1] = 3; }, "jamd_lexicon_create: successor id 1 names word 3 of 3", k4G},
  {"negative successor word", ngram_lex, [](Lex &l) { l.scword[2] = -1; }, "jamd_lexicon_create: successor id 2 names word -1 of 3", k4G},
  {"state set past the table", ngram_lex, [](Lex &l) { l.out_id[1] = 1; }, "jamd_lexicon_create: node 1 has output 1 of kind 1 outside the tables", k4G},
  {"lc_tab row past the table", ngram_lex, [](Lex &l) { l.out_id[5] = 2; }, "jamd_lexicon_create: node 5 has output 2 of kind 3 outside the tables", k4G},
  {"lc_tab one row short", ngram_lex, [](Lex &l) { l.s.nlcrow = 1; l.lc_tab.resize(2); }, "jamd_lexicon_create: node 5 has output 1 of kind 3 outside the tables", k4G},
  {"negative state", ngram_lex, [](Lex &l) { l.out_id[0] = -1; }, "jamd_lexicon_create: node 0 has output -1 of kind 0 outside the tables", k4G},
  {"unknown output kind", ngram_lex, [](Lex &l) { l.out_kind[8] = 5; }, "jamd_lexicon_create: node 8 has output 5 of kind 5 outside the tables", k4G},
  {"last node goes on", ngram_lex, [](Lex &l) { l.next_a[8] = -0.5f; }, "jamd_lexicon_create: the last node has a next node", k4G},
  {"ac_to NULL", ngram_lex, [](Lex &l) { l.ac_to.clear(); }, "jamd_lexicon_create: arc arrays missing", k4G},
  {"ac_a NULL", ngram_lex, [](Lex &l) { l.ac_a.clear(); }, "jamd_lexicon_create: arc arrays missing", k4G},
  {"arc past the nodes", ngram_lex, [](Lex &l) { l.ac_to[0] = 9; }, "jamd_lexicon_create: arc 0 leads to node 9 of 9", k4G},
  {"arc to a negative node", ngram_lex, [](Lex &l) { l.ac_to[0] = -1; }, "jamd_lexicon_create: arc 0 leads to node -1 of 9", k4G},
  {"root past the nodes", ngram_lex, [](Lex &l) { l.startnode[1] = 9; }, "jamd_lexicon_create: root 1 is node 9 of 9", k4G},
  {"word head below -1", ngram_lex, [](Lex &l) { l.word_head[0] = -2; }, "jamd_lexicon_create: word 0 starts at node -2 of 9", k4G},
  {"word head past the nodes", ngram_lex, [](Lex &l) { l.word_head[2] = 9; }, "jamd_lexicon_create: word 2 starts at node 9 of 9", k4G},
  {"set_off NULL", ngram_lex, [](Lex &l) { l.set_off.clear(); }, "jamd_lexicon_create: state-set table missing", k4G},
  {"set_off descends", ngram_lex, [](Lex &l) { l.set_off[1] = -1; }, "jamd_lexicon_create: set_off not monotone at 0", k4G},
  {"negative set member", ngram_lex, [](Lex &l) { l.set_states[1] = -1; }, "jamd_lexicon_create: negative state in set table", k4G},
  {"lc_tab names a set past the table", ngram_lex, [](Lex &l) { l.lc_tab[1] = ~1; }, "jamd_lexicon_create: lc_tab entry 1 names state set 1 of 1", k4G},
  {"state sets one short", ngram_lex, [](Lex &l) { l.s.nset = 0; l.out_kind[1] = JAMD_AS_STATE; }, "jamd_lexicon_create: lc_tab entry 1 names state set 0 of 0", k4G},
  {"left context past the columns", ngram_lex, [](Lex &l) { l.word_lc[0] = 2; }, "jamd_lexicon_create: word 0 selects left context 2 of 1", k4G},
  {"negative left context", ngram_lex, [](Lex &l) { l.word_lc[2] = -1; }, "jamd_lexicon_create: word 2 selects left context -1 of 1", k4G},
  {"N-gram entry past the table", ngram_lex, [](Lex &l) { l.wton[2] = 3; }, "jamd_lexicon_create: word 2 is N-gram entry 3 of 3", k4G},
  {"1-grams one short", ngram_lex, [](Lex &l) { l.s.ng_nword = 2; }, "jamd_lexicon_create: word 2 is N-gram entry 2 of 2", k4G},
  {"2-grams past the table", ngram_lex, [](Lex &l) { l.ng_bi_num[0] = 2; }, "jamd_lexicon_create: 2-grams of entry 0 leave the table", k4G},
  {"2-grams begin past the table", ngram_lex, [](Lex &l) { l.ng_bi_bgn[2] = 1; }, "jamd_lexicon_create: 2-grams of entry 2 leave the table", k4G},
  {"negative 2-gram count", ngram_lex, [](Lex &l) { l.ng_bi_num[0] = -1; }, "jamd_lexicon_create: 2-grams of entry 0 leave the table", k4G},
  {"isolated number repeated", ngram_lex, [](Lex &l) { l.start2isolate[2] = 0; }, "jamd_lexicon_create: start2isolate out of range or repeated", k4G},
  {"isolated number past isolatenum", ngram_lex, [](Lex &l) { l.start2isolate[2] = 2; }, "jamd_lexicon_create: start2isolate out of range or repeated", k4G},
  {"isolatenum one short", ngram_lex, [](Lex &l) { l.s.isolatenum = 1; }, "jamd_lexicon_create: start2isolate out of range or repeated", k4G},
  {"isolated root without a word", ngram_lex, [](Lex &l) { l.scid[0] = 0; }, "jamd_lexicon_create: isolated root without a successor word", k4G},
  {"shared root without a value", ngram_lex, [](Lex &l) { l.scid[3] = 0; }, "jamd_lexicon_create: shared root without a factoring value", k4G},
  {"isolated root unassigned", ngram_lex, [](Lex &l) { l.s.isolatenum = 3; }, "jamd_lexicon_create: isolated root 2 is not assigned", k4G},
  {"root's word past the words", grammar_lex, [](Lex &l) { l.start2wid[0] = 2; }, "jamd_lexicon_create: root 0 has no valid category", k4G},
  {"root's category past ncat", grammar_lex, [](Lex &l) { l.wton[1] = 2; }, "jamd_lexicon_create: root 1 has no valid category", k4G},
  {"word's category past ncat", grammar_lex, [](Lex &l) { l.start2wid[1] = 0; l.wton[1] = 2; }, "jamd_lexicon_create: word 1 outside the categories", k4G},
  {"initial node past the nodes", grammar_lex, [](Lex &l) { l.init_node[1] = 4; }, "jamd_lexicon_create: bad initial node", k4G},
  {"initial node in word mode", word_lex, [](Lex &l) { l.init_node[0] = -1; }, "jamd_lexicon_create: bad initial node", k4G},
  {"forward DFA without fwd_to", grammar_lex, [](Lex &l) { l.fwd_to.clear(); }, "jamd_lexicon_create: forward DFA descriptor incomplete", k4G},
  {"forward DFA in word mode", word_lex, [](Lex &l) { l.s.nfwd = 1; }, "jamd_lexicon_create: forward DFA descriptor incomplete", k4G},
  {"forward DFA offsets descend", grammar_lex, [](Lex &l) { l.fwd_off[1] = 3; }, "jamd_lexicon_create: forward DFA offsets not monotone", k4G},
  {"forward DFA arc past the states", grammar_lex, [](Lex &l) { l.fwd_to[1] = 2; }, "jamd_lexicon_create: forward DFA arc 1 leaves the automaton", k4G},
  {"forward DFA one state short", grammar_lex, [](Lex &l) { l.s.nfwd = 1; }, "jamd_lexicon_create: forward DFA arc 0 leaves the automaton", k4G},
  {"initial state past the states", grammar_lex, [](Lex &l) { l.init_to_state[0] = 2; }, "jamd_lexicon_create: bad initial forward-DFA state", k4G},
  {"initial state below -1", grammar_lex, [](Lex &l) { l.init_to_state[1] = -2; }, "jamd_lexicon_create: bad initial forward-DFA state", k4G},
  {"image at the limit of its offsets", ngram_lex, [](Lex &) {}, "jamd_lexicon_create: lexicon image exceeds 4 GB", 0},   // (0: the image's own size)
};
// nword >= 2^30 is refused behind loops over the word arrays: a descriptor that gets there needs 4 GB of them
static const std::set<std::string> kNotReached = {"jamd_lexicon_create: nword=%d too large"};

// A message is what a format gives: every conversion (%d, %zu) stands for one integer, the rest is literal.
static bool made_by(const std::string &fmt, const std::string &msg) {
  size_t f = 0, m = 0;
  while (f < fmt.size()) {
    if (fmt[f] == '%') {
      f = fmt.find_first_of("du", f);
      if (f == std::string::npos) return false;
      f++;
      if (m < msg.size() && msg[m] == '-') m++;
      const size_t digits = m;
      while (m < msg.size() && msg[m] >= '0' && msg[m] <= '9') m++;
      if (m == digits) return false;
    } else if (m >= msg.size() || fmt[f++] != msg[m++]) return false;
  }
  return m == msg.size();
}

static void check_refusals(const char *header) {
  std::set<std::string> reached;
  for (const Refusal &r : kRefusals) {
    Lex l = r.base();
    r.corrupt(l);
    const jamd_lexicon_desc d = l.desc();
    size_t limit = r.max_bytes;
    if (limit == 0) { LexImage im; lexicon_image(d, &im, true); limit = im.bytes; }
    std::string err;
    const bool ok = lexicon_check(d, err, limit);
    expect(!ok && err == r.text, std::string("refused: ") + r.what + (ok ? " (accepted)" : err == r.text ? "" : " (" + err + ")"));
    if (!ok) reached.insert(err);
  }
  { // one byte below the limit the same descriptor is accepted
    const Lex l = ngram_lex();
    const jamd_lexicon_desc d = l.desc();
    LexImage im; lexicon_image(d, &im, true);
    std::string err;
    expect(lexicon_check(d, err, im.bytes + 1), "accepted: image one byte below the limit");
  }
  // every refusal the header holds is reached by a case: a reached message is what its format gives, whole
  std::ifstream in(header);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string text = ss.str(), key = "lex_errf(err, \"";
  int refusals = 0, missed = 0;
  std::set<std::string> formats;
  for (size_t at = text.find(key); at != std::string::npos; at = text.find(key, at + 1)) {
    const size_t from = at + key.size();
    const std::string fmt = text.substr(from, text.find('"', from) - from);
    refusals++;
    formats.insert(fmt);
    bool hit = kNotReached.count(fmt) != 0;
    for (const std::string &e : reached) hit = hit || made_by(fmt, e);
    if (!hit) { missed++; printf("  no case reaches: %s\n", fmt.c_str()); }
  }
  // ... and no two refusals share a format, so none hides behind another's case
  expect((int)formats.size() == refusals, "the header's refusals have " + std::to_string(formats.size()) + " distinct texts");
  expect(refusals >= 30 && missed == 0, "every one of the header's " + std::to_string(refusals) + " refusals is reached (" +
                                            std::to_string(kNotReached.size()) + " listed as out of reach)");
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: lexicon_image_check path/to/beam_lexicon_image.h\n"); return 2; }
  check_all_valid();
  check_refusals(argv[1]);
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
