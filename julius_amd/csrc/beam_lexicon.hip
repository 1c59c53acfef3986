// beam_lexicon.hip -- the tree lexicon and its language model on the device: jamd_lexicon_create() checks every index a
// first-pass kernel will follow, packs all arrays into one arena (LexDev, beam_common.h) and builds the cross-word LM table.
#include "jamd_device.h"
#include <algorithm>

#include "beam_host.h"

namespace {
using namespace jamdb;
// the cross-word LM table (LexDev::iwtab): one thread per (context, isolated root)
constexpr size_t kIwTabMaxBytes = (size_t)2 << 30;
__global__ void __launch_bounds__(256) iwtab_build_kernel(LexDev lx, float *tab, int nctx, int niso) {
  const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= (size_t)nctx * niso) return;
  const int ctx = (int)(x / niso), i = (int)(x - (size_t)ctx * niso);
  const int w = lx.iso_root(i).y;
  tab[x] = bigram_prob(lx, ctx, lx.wton(w)) + lx.cprob(w);
}

template <typename T>
int upload(T **dst, const T *src, size_t n) {
  JAMD_HIP(hipMalloc((void **)dst, sizeof(T) * (n ? n : 1)));
  if (n) JAMD_HIP(hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
  return JAMD_OK;
}

}  // namespace

extern "C" {

int jamd_lexicon_create(jamd_engine *e, const jamd_lexicon_desc *h, jamd_lexicon **out) {
  if (!e || !h || !out) { jamd_set_error("jamd_lexicon_create: NULL argument"); return JAMD_EINVAL; }
  *out = nullptr;
  const int lmt = h->lm_type & 0xff;
  const bool multipath = (h->lm_type & JAMD_LM_MULTIPATH) != 0;
  const bool wordmode = lmt == JAMD_LM_WORD;
  const bool dfa = lmt == JAMD_LM_DFA || wordmode;             // the two LM_DFA variants share everything but the word boundary
  if ((h->lm_type & ~(0xff | JAMD_LM_MULTIPATH)) != 0 || (lmt != JAMD_LM_NGRAM && !dfa)) {
    jamd_set_error("jamd_lexicon_create: lm_type=%d", h->lm_type); return JAMD_EINVAL;
  }
  if (dfa && (h->ninit < 0 || (h->ninit > 0 && (!h->init_node || !h->init_lscore)) ||
              (!wordmode && (h->ncat <= 0 || !h->cat_pair || !h->start2wid)))) {
    jamd_set_error("jamd_lexicon_create: grammar descriptor incomplete (ncat=%d ninit=%d)", h->ncat, h->ninit);
    return JAMD_EINVAL;
  }
  if (h->nnode <= 0 || h->nword <= 0 || h->startnum < 0 || (!dfa && (h->head_silwid < 0 || h->head_silwid >= h->nword))) {
    jamd_set_error("jamd_lexicon_create: bad sizes (nnode=%d nword=%d head_silwid=%d)", h->nnode, h->nword,
                   h->head_silwid);
    return JAMD_EINVAL;
  }
  if (h->cdset_method == JAMD_IWCD_NBEST && (h->cdmax_num < 1 || h->cdmax_num > jamd::kNbestMax)) {
    jamd_set_error("jamd_lexicon_create: cdmax_num=%d outside [1,%d]", h->cdmax_num, jamd::kNbestMax);
    return JAMD_EINVAL;
  }
  // every index a kernel will follow is range-checked here: a truncated or corrupt blob (jamd_lexicon_load)
  // must fail with JAMD_EINVAL, not read out of bounds on the host or the device
  if (!h->ac_off || !h->self_a || !h->next_a || !h->stend || !h->scid || !h->out_id || !h->out_kind ||
      (h->startnum > 0 && !h->startnode) || !h->word_head || !h->wton || h->ac_off[0] != 0) {
    jamd_set_error("jamd_lexicon_create: NULL or malformed node arrays"); return JAMD_EINVAL;
  }
  int maxfan = 2;
  for (int i = 0; i < h->nnode; i++) {
    const int x = h->ac_off[i + 1] - h->ac_off[i];
    if (x < 0) { jamd_set_error("jamd_lexicon_create: ac_off not monotone at node %d", i); return JAMD_EINVAL; }
    if (2 + x > maxfan) maxfan = 2 + x;
    if (h->stend[i] >= h->nword) { jamd_set_error("jamd_lexicon_create: node %d ends word %d of %d", i, h->stend[i], h->nword); return JAMD_EINVAL; }
    if (h->scid[i] >= h->nscword || (h->scid[i] < 0 && -h->scid[i] >= h->nfscore)) {
      jamd_set_error("jamd_lexicon_create: node %d has successor id %d outside the tables", i, h->scid[i]); return JAMD_EINVAL;
    }
  }
  for (int k = 0; k < h->ac_off[h->nnode]; k++)
    if (h->ac_to[k] < 0 || h->ac_to[k] >= h->nnode) { jamd_set_error("jamd_lexicon_create: arc %d leads to node %d of %d", k, h->ac_to[k], h->nnode); return JAMD_EINVAL; }
  for (int s = 0; s < h->startnum; s++)
    if (h->startnode[s] < 0 || h->startnode[s] >= h->nnode) { jamd_set_error("jamd_lexicon_create: root %d is node %d of %d", s, h->startnode[s], h->nnode); return JAMD_EINVAL; }
  for (int w = 0; w < h->nword; w++)
    if (h->word_head[w] < -1 || h->word_head[w] >= h->nnode) { jamd_set_error("jamd_lexicon_create: word %d starts at node %d of %d", w, h->word_head[w], h->nnode); return JAMD_EINVAL; }
  if (h->nset > 0) {
    if (!h->set_off || !h->set_states || h->set_off[0] != 0) { jamd_set_error("jamd_lexicon_create: state-set table missing"); return JAMD_EINVAL; }
    for (int i = 0; i < h->nset; i++)
      if (h->set_off[i + 1] < h->set_off[i]) { jamd_set_error("jamd_lexicon_create: set_off not monotone at %d", i); return JAMD_EINVAL; }
    for (int k = 0; k < h->set_off[h->nset]; k++)
      if (h->set_states[k] < 0) { jamd_set_error("jamd_lexicon_create: negative state in set table"); return JAMD_EINVAL; }
  }
  std::vector<int> iso(h->isolatenum > 0 ? h->isolatenum : 0, -1), shared;
  for (int s = 0; s < h->startnum && !dfa; s++) {
    const int i = h->start2isolate[s];
    if (i >= 0) {
      if (i >= h->isolatenum || iso[i] >= 0) { jamd_set_error("jamd_lexicon_create: start2isolate out of range or repeated"); return JAMD_EINVAL; }
      iso[i] = s;
      const int sc = h->scid[h->startnode[s]];
      if (sc <= 0 || sc >= h->nscword) { jamd_set_error("jamd_lexicon_create: isolated root without a successor word"); return JAMD_EINVAL; }
    } else {
      const int sc = h->scid[h->startnode[s]];
      if (sc >= 0 || -sc >= h->nfscore) { jamd_set_error("jamd_lexicon_create: shared root without a factoring value"); return JAMD_EINVAL; }
      shared.push_back(s);
    }
  }
  if (h->nword >= (1 << 30)) { jamd_set_error("jamd_lexicon_create: nword=%d too large", h->nword); return JAMD_EINVAL; }
  JAMD_HIP(hipSetDevice(e->device));
  jamd_lexicon *l = new jamd_lexicon();
  l->eng = e; l->maxfan = maxfan; l->nscword = h->nscword; l->multipath = multipath;
  if (multipath) {
    // A root that reaches a word-end node along its own arcs (a word of tee models only): a cross-word transition would
    // improve a word end inside the loop that visits the word ends (beam.c:2779-2825), and the result depends on the loop's
    // position -- strict order only.  Roots are non-emitting; so is every word end of a multipath lexicon.
    bool ok = true;
    for (int s = 0; s < h->startnum && ok; s++) {
      const int r = h->startnode[s];
      if (h->self_a[r] != JAMD_LOG_ZERO && h->stend[r] >= 0) ok = false;
      if (h->next_a[r] != JAMD_LOG_ZERO && r + 1 < h->nnode && h->stend[r + 1] >= 0) ok = false;
      for (int k = h->ac_off[r]; k < h->ac_off[r + 1]; k++) if (h->stend[h->ac_to[k]] >= 0) ok = false;
    }
    l->mp_parallel = ok;
  }
  LexDev &d = l->d;
  d.nnode = h->nnode; d.nword = h->nword; d.startnum = h->startnum; d.isolatenum = h->isolatenum;
  d.nshared = (int)shared.size(); d.nlc = h->nlc; d.cdset_method = h->cdset_method; d.cdmax_num = h->cdmax_num;
  d.head_silwid = h->head_silwid; d.tail_silwid = h->tail_silwid; d.ng_mode = h->ng_mode; d.ng_unk_id = h->ng_unk_id;
  d.ng_unk_num_log = h->ng_unk_num_log; d.lm_weight = h->lm_weight; d.lm_penalty = h->lm_penalty;
  d.lm_penalty_trans = h->lm_penalty_trans;
  const int nac = h->ac_off[h->nnode], nset_states = h->nset ? h->set_off[h->nset] : 0;
  int rc = JAMD_OK;
  // every array is appended (16-byte aligned) to one host image that is uploaded once; the kernel
  // sees the base pointer and 32-bit byte offsets (see LexDev)
  std::vector<unsigned char> arena;
#define UP(field, src, n)                                                              \
  do {                                                                                 \
    const size_t bytes_ = sizeof(*(src)) * (size_t)(n), at_ = (arena.size() + 15) & ~(size_t)15;   \
    arena.resize(at_ + (bytes_ ? bytes_ : 16));                                        \
    if (bytes_) memcpy(arena.data() + at_, (src), bytes_);                             \
    d.o_##field = (unsigned)at_;                                                       \
  } while (0)
  std::vector<int4> na(h->nnode), nb(h->nnode);
  std::vector<int> word_end(h->nword, -1);
  for (int i = 0; i < h->nnode; i++) {
    int sa, nx;
    memcpy(&sa, &h->self_a[i], 4); memcpy(&nx, &h->next_a[i], 4);
    na[i] = make_int4(sa, nx, h->ac_off[i], h->ac_off[i + 1]);
    nb[i] = make_int4(h->stend[i], h->scid[i], h->out_id[i], (int)h->out_kind[i]);
    if (h->stend[i] >= 0 && h->stend[i] < h->nword) word_end[h->stend[i]] = i;
  }
  // both root lists in the order beam_inter_word() / beam_inter_word_factoring() visit them (stid from
  // startnum-1 down to 0, beam.c:2334 / :2562): the exact-order kernel numbers its candidates by list index
  for (size_t i = 0; i < iso.size() && !dfa; i++)
    if (iso[i] < 0) { jamd_set_error("jamd_lexicon_create: isolated root %d is not assigned", (int)i); return JAMD_EINVAL; }
  std::sort(iso.begin(), iso.end(), [](int a, int b) { return a > b; });
  std::sort(shared.begin(), shared.end(), [](int a, int b) { return a > b; });
  std::vector<int2> iso_root(iso.size());
  for (size_t i = 0; i < iso.size(); i++) {
    const int node = h->startnode[iso[i]];
    iso_root[i] = make_int2(node, h->scword[h->scid[node]]);
  }
  std::vector<float2> shared_root(shared.size());
  for (size_t i = 0; i < shared.size(); i++) {
    const int node = h->startnode[shared[i]];
    float nf; memcpy(&nf, &node, 4);
    shared_root[i] = make_float2(nf, h->fscore[-h->scid[node]]);
  }
  {
    std::vector<int4> nab(2 * (size_t)h->nnode);       // one 32-byte record per node (LexDev::node_a / node_b / scid)
    for (int i = 0; i < h->nnode; i++) { nab[2 * (size_t)i] = na[i]; nab[2 * (size_t)i + 1] = nb[i]; }
    UP(node_a, nab.data(), nab.size());
    d.o_node_b = d.o_node_a + 16u; d.o_scid = d.o_node_a + 20u;
  }
  UP(ac_to, h->ac_to, nac); UP(ac_a, h->ac_a, nac);
  UP(iso_root, iso_root.data(), iso_root.size()); UP(shared_root, shared_root.data(), shared_root.size());
  UP(word_end, word_end.data(), word_end.size());
  if (multipath) {
    // the roots' own transitions, flattened once (csrc/beam_exact_mp.h, step B')
    auto expand = [&](int root, int rootno, int tag, std::vector<int4> &out) {
      auto bits = [](float f) { int b; memcpy(&b, &f, 4); return b; };
      if (h->self_a[root] != JAMD_LOG_ZERO) out.push_back(make_int4(root, bits(h->self_a[root]), rootno * maxfan + 0, tag));
      if (h->next_a[root] != JAMD_LOG_ZERO) out.push_back(make_int4(root + 1, bits(h->next_a[root]), rootno * maxfan + 1, tag));
      for (int k = h->ac_off[root]; k < h->ac_off[root + 1]; k++)
        out.push_back(make_int4(h->ac_to[k], bits(h->ac_a[k]), rootno * maxfan + 2 + (k - h->ac_off[root]), tag));
    };
    std::vector<int4> e_iso, e_shared, e_start;
    const int head_root = dfa ? -1 : h->word_head[h->head_silwid];
    for (size_t i = 0; i < iso_root.size() && !dfa; i++)
      if (iso_root[i].x != head_root) expand(iso_root[i].x, (int)i, (int)i, e_iso);                       // :2336-2341
    for (size_t r = 0; r < shared_root.size() && !dfa; r++) {
      int node; memcpy(&node, &shared_root[r].x, 4);
      int fs; memcpy(&fs, &shared_root[r].y, 4);
      if (node != head_root) expand(node, (int)r, fs, e_shared);                                          // :2566-2571
    }
    for (int rv = 0; rv < h->startnum && dfa && !wordmode; rv++) {
      const int r = h->startnum - 1 - rv;                                                                 // roots from startnum-1 down (:2334)
      expand(h->startnode[r], rv, r, e_start);
    }
    auto put = [&](const std::vector<int4> &v, unsigned *off, int *cnt) {
      const size_t at = (arena.size() + 15) & ~(size_t)15;
      arena.resize(at + (v.empty() ? 16 : v.size() * sizeof(int4)));
      if (!v.empty()) memcpy(arena.data() + at, v.data(), v.size() * sizeof(int4));
      *off = (unsigned)at; *cnt = (int)v.size();
    };
    put(e_iso, &l->o_mp_iso, &l->n_mp_iso); put(e_shared, &l->o_mp_shared, &l->n_mp_shared); put(e_start, &l->o_mp_start, &l->n_mp_start);
    {
      std::vector<int> tgt((size_t)h->nnode, -1);
      int ntgt = 0;
      for (const std::vector<int4> *v : {&e_iso, &e_shared, &e_start})
        for (const int4 &ent : *v) if (tgt[(size_t)ent.x] < 0) tgt[(size_t)ent.x] = ntgt++;
      const size_t at = (arena.size() + 15) & ~(size_t)15;
      arena.resize(at + tgt.size() * sizeof(int));
      memcpy(arena.data() + at, tgt.data(), tgt.size() * sizeof(int));
      l->o_mp_tgt = (unsigned)at; l->n_mp_tgt = ntgt;
    }
  }
  UP(startnode, h->startnode, h->startnum); UP(start2isolate, h->start2isolate, h->startnum);
  UP(lc_tab, h->lc_tab, (size_t)h->nlcrow * (h->nlc + 1)); UP(word_lc, h->word_lc, h->nword);
  UP(set_off, h->set_off, h->nset + 1); UP(set_states, h->set_states, nset_states);
  UP(wordend_a, h->wordend_a, h->nword); UP(wton, h->wton, h->nword); UP(cprob, h->cprob, h->nword);
  UP(is_transparent, h->is_transparent, h->nword); UP(word_head, h->word_head, h->nword);
  UP(fscore, h->fscore, h->nfscore); UP(scword, h->scword, h->nscword);
  UP(ng_uni_prob, h->ng_uni_prob, h->ng_nword); UP(ng_uni_bo, h->ng_uni_bo, h->ng_nword);
  UP(ng_bi_bgn, h->ng_bi_bgn, h->ng_nword); UP(ng_bi_num, h->ng_bi_num, h->ng_nword);
  UP(ng_bi_wid, h->ng_bi_wid, h->ng_nbigram); UP(ng_bi_prob, h->ng_bi_prob, h->ng_nbigram);
  d.lm_type = lmt; d.ncat = dfa ? h->ncat : 0; d.ninit = dfa ? h->ninit : 0; d.penalty1 = dfa ? h->penalty1 : 0.0f;
  if (dfa) {
    std::vector<int> root_cat(h->startnum, 0);
    for (int s = 0; s < h->startnum && !wordmode; s++) {
      const int w = h->start2wid[s];
      if (w < 0 || w >= h->nword || h->wton[w] < 0 || h->wton[w] >= h->ncat) {
        jamd_set_error("jamd_lexicon_create: root %d has no valid category", s); rc = JAMD_EINVAL; break;
      }
      root_cat[s] = h->wton[w];
    }
    for (int w = 0; w < h->nword && rc == JAMD_OK && !wordmode; w++)
      if (h->wton[w] < 0 || h->wton[w] >= h->ncat) { jamd_set_error("jamd_lexicon_create: word %d outside the categories", w); rc = JAMD_EINVAL; }
    for (int e = 0; e < h->ninit && rc == JAMD_OK; e++)
      if (h->init_node[e] < 0 || h->init_node[e] >= h->nnode) { jamd_set_error("jamd_lexicon_create: bad initial node"); rc = JAMD_EINVAL; }
    UP(cat_pair, h->cat_pair, wordmode ? 0 : (size_t)h->ncat * h->ncat); UP(root_cat, root_cat.data(), root_cat.size());
    UP(init_node, h->init_node, h->ninit); UP(init_lscore, h->init_lscore, h->ninit);
    if (h->nfwd > 0 && rc == JAMD_OK) {
      // forward DFA: every index the kernels will follow is checked here
      if (wordmode || !h->fwd_off || !h->fwd_label || !h->fwd_to || !h->init_to_state || h->fwd_off[0] != 0) {
        jamd_set_error("jamd_lexicon_create: forward DFA descriptor incomplete"); rc = JAMD_EINVAL;
      }
      for (int s2 = 0; s2 < h->nfwd && rc == JAMD_OK; s2++)
        if (h->fwd_off[s2 + 1] < h->fwd_off[s2]) { jamd_set_error("jamd_lexicon_create: forward DFA offsets not monotone"); rc = JAMD_EINVAL; }
      for (int a = 0; rc == JAMD_OK && a < h->fwd_off[h->nfwd]; a++)
        if (h->fwd_to[a] < 0 || h->fwd_to[a] >= h->nfwd) { jamd_set_error("jamd_lexicon_create: forward DFA arc %d leaves the automaton", a); rc = JAMD_EINVAL; }
      for (int e2 = 0; rc == JAMD_OK && e2 < h->ninit; e2++)
        if (h->init_to_state[e2] < -1 || h->init_to_state[e2] >= h->nfwd) { jamd_set_error("jamd_lexicon_create: bad initial forward-DFA state"); rc = JAMD_EINVAL; }
      if (rc == JAMD_OK) {
        UP(fwd_off, h->fwd_off, (size_t)h->nfwd + 1); UP(fwd_label, h->fwd_label, (size_t)h->fwd_off[h->nfwd]);
        UP(fwd_to, h->fwd_to, (size_t)h->fwd_off[h->nfwd]); UP(init_to_state, h->init_to_state, h->ninit);
        d.nfwd = h->nfwd;
      }
    }
  }
#undef UP
  if (rc == JAMD_OK && arena.size() >= ((size_t)1 << 32)) { jamd_set_error("jamd_lexicon_create: lexicon image exceeds 4 GB"); rc = JAMD_EINVAL; }
  if (rc == JAMD_OK) {
    unsigned char *dev = nullptr;
    rc = upload(&dev, arena.data(), arena.size());
    d.base = dev;
    if (dev) l->owned.push_back((void *)dev);
  }
  if (rc == JAMD_OK && !dfa && h->isolatenum > 0 && h->ng_nword > 0 &&
      (size_t)h->ng_nword * h->isolatenum * sizeof(float) <= kIwTabMaxBytes) {
    const size_t cells = (size_t)h->ng_nword * h->isolatenum;
    float *tab = nullptr;
    if (hipMalloc((void **)&tab, cells * sizeof(float)) == hipSuccess) {
      l->owned.push_back((void *)tab);
      hipLaunchKernelGGL(iwtab_build_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream, d, tab, h->ng_nword, h->isolatenum);
      if (hipGetLastError() == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess) d.iwtab = tab;
    } else (void)hipGetLastError();             // no room: the kernels compute the entries on the fly
  }
  if (rc != JAMD_OK) { jamd_lexicon_destroy(l); return rc; }
  *out = l;
  return JAMD_OK;
}

void jamd_lexicon_destroy(jamd_lexicon *l) {
  if (!l) return;
  (void)hipSetDevice(l->eng->device);
  for (void *p : l->owned) (void)hipFree(p);
  delete l;
}

}  // extern "C"
