// beam_lex_arrays.h -- the arrays of the lexicon arena, by name: LexDev (beam_common.h) makes its offsets and accessors
// of the list, the host image (beam_lexicon_image.h) its offsets.  No include, no type of its own: the element types are
// the device's and matter to LexDev only.
#pragma once

// All lexicon / LM arrays live in ONE device allocation and are addressed as base + 32-bit byte
// offset: a kernel that carries some forty 64-bit array pointers next to its per-utterance work
// pointers needs twice the scalar registers the hardware has, and the spilled ones come back
// through v_readlane -- a third of the first-pass kernel's instructions before this layout.  With a
// uniform base the loads also take the `global_load v, voffset32, s[base]` form (no 64-bit address
// arithmetic per access).
#define JAMD_LEX_ARRAYS(X)                                                                       \
  X(int, ac_to) X(float, ac_a)                                                                               \
  X(int2, iso_root)        /* [isolatenum] {root node, successor word scword[scid[root]]}                  */ \
  X(float2, shared_root)   /* [nshared]    {root node bits, fscore[-scid[root]]}                           */ \
  X(int, word_end)         /* [nword] node whose stend is the word                                         */ \
  X(int, startnode) X(int, start2isolate)   /* [startnum] as in wchmm (the strict-order kernel walks them like beam.c) */ \
  X(int, lc_tab) X(int, word_lc) X(int, set_off) X(int, set_states)                                          \
  X(float, wordend_a) X(int, wton) X(float, cprob) X(unsigned char, is_transparent)                          \
  X(int, word_head) X(float, fscore) X(int, scword)                                                          \
  X(float, ng_uni_prob) X(float, ng_uni_bo) X(int, ng_bi_bgn) X(int, ng_bi_num) X(int, ng_bi_wid) X(float, ng_bi_prob) \
  /* grammar (per-category trees): category-pair matrix [ncat][ncat] (dfa_cp()), each root's category         \
     wton[start2wid[root]], the initial tokens [ninit] */                                                      \
  X(unsigned char, cat_pair) X(int, root_cat) X(int, init_node) X(float, init_lscore)                         \
  /* forward DFA (nfwd > 0; libjulius/src/beam.c:1739-1747, :2412-2422): arcs of a state in list order, the initial tokens' states */ \
  X(int, fwd_off) X(int, fwd_label) X(int, fwd_to) X(int, init_to_state)
