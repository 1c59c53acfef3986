// beam_lexicon_api.hip -- the tree lexicon and its language model as an object of the C ABI: jamd_lexicon_create() has the
// descriptor checked and packed into one arena without a device (beam_lexicon_image.h), uploads that arena once and asks
// for the cross-word LM table (beam_lexicon.hip).  No kernel lives here.
#include "beam_host.h"

using namespace jamdb;

static_assert(kLexNbestMax == jamd::kNbestMax, "beam_lexicon_image.h repeats jamd::kNbestMax");
constexpr size_t kIwTabMaxBytes = (size_t)2 << 30;

extern "C" {

int jamd_lexicon_create(jamd_engine *e, const jamd_lexicon_desc *h, jamd_lexicon **out) {
  if (!e || !h || !out) return jamd_refuse("jamd_lexicon_create: NULL argument");
  *out = nullptr;
  std::string err;
  if (!lexicon_check(*h, err)) return jamd_refuse("%s", err.c_str());
  LexImage im;
  lexicon_image(*h, &im);
  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_lexicon> l(new jamd_lexicon());
  l->device = e->device;
  static_cast<LexHost &>(*l) = im;
  LexDev &d = l->d;
#define X(T, name) d.name = im.name;
  JAMD_LEX_SCALARS(X)
#undef X
#define X(T, name) d.o_##name = im.o_##name;
  JAMD_LEX_ARRAYS(X)
#undef X
  d.o_node_a = im.o_node_a; d.o_node_b = im.o_node_b; d.o_scid = im.o_scid;
  { const int rc = l->arena.upload(im.arena.data(), im.arena.size()); if (rc != JAMD_OK) return rc; }
  d.base = l->arena;
  const size_t cells = (size_t)h->ng_nword * h->isolatenum;
  const char *no_tab = getenv("JAMD_NO_IWTAB");    // (development: the table-less LM path at any size)
  const bool want_tab = !(no_tab && atoi(no_tab) != 0);
  if (want_tab && d.lm_type == JAMD_LM_NGRAM && cells > 0 && cells * sizeof(float) <= kIwTabMaxBytes) {
    // no room, or a build that failed: the kernels compute the entries on the fly, and the call has not failed, so
    // jamd_last_error() keeps what it said before
    const std::string said = jamd_last_error();
    if (l->iwtab.grow(cells * sizeof(float)) != JAMD_OK) { (void)hipGetLastError(); jamd_set_error("%s", said.c_str()); }
    else if (iwtab_build(d, l->iwtab, h->ng_nword, h->isolatenum, e->stream) == hipSuccess) d.iwtab = l->iwtab;
  }
  *out = l.release();
  return JAMD_OK;
}

int jamd_lexicon_lm_table(const jamd_lexicon *l) {
  if (!l) return -1;
  return l->d.iwtab != nullptr ? 1 : 0;
}

void jamd_lexicon_destroy(jamd_lexicon *l) {
  if (!l) return;
  (void)hipSetDevice(l->device);
  delete l;
}

}  // extern "C"
