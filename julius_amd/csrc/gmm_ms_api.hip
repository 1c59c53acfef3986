// gmm_ms_api.hip -- the host layer of multi-stream GMM scoring: everything of jamd_gmm_ms that is not a kernel or
// its launcher.
//
// jamd_gmm_ms_create() / jamd_gmm_ms_create_opt() check the caller's description completely BEFORE the first device
// call (a refusal names the field and costs no upload), pack every mixture pdf's Gaussians in the order the kernel reads
// them -- a pdf shared by several states (a `~p` macro) is packed once, a codebook once for all its pdfs -- and upload
// once.  The entry points check their arguments.  Nothing is launched from here: see gmm_ms_host.h.
#include "gmm_ms_host.h"

#include <cmath>

namespace {

constexpr int kDefaultChunk = 2048;                    // frames of scratch: the header's jamd_gmm_ms_opt
constexpr size_t kDefaultScratch = 256u << 20;         // ... unless that passes this many bytes

// opt == nullptr: jamd_gmm_ms_create(), `-gprune none` over plain mixtures.
int ms_build(const char *who, jamd_engine *e, const jamd_gmm_ms_desc *d, const jamd_gmm_ms_opt *opt, jamd_gmm_ms **out) {
  const int ns = d->nstream;
  if (ns < 1 || ns > 50) return jamd_refuse("%s: nstream=%d; 1 .. 50 streams (MAXSTREAMNUM) are supported", who, ns);
  if (d->nstate <= 0 || d->veclen <= 0 || d->npdf <= 0 || d->nentry < 0 || d->ndens < 0)
    return jamd_refuse("%s: bad dimensions nstate=%d veclen=%d npdf=%d nentry=%d ndens=%d", who, d->nstate,
                       d->veclen, d->npdf, d->nentry, d->ndens);
  if (!d->vsize || !d->pdf_stream || !d->pdf_off || !d->st_pdf || !d->dens_off || (d->nentry && (!d->ent_dens || !d->ent_logw)) ||
      (d->ndens && (!d->mean || !d->ivar || !d->gconst)))
    return jamd_refuse("%s: NULL model array", who);
  if (opt) {
    if (opt->gprune == JAMD_GPRUNE_HEU || opt->gprune == JAMD_GPRUNE_BEAM)
      return jamd_refuse("%s: gprune %s is not served for a multi-stream object (none and safe are)", who,
                         opt->gprune == JAMD_GPRUNE_HEU ? "heu" : "beam");
    if (opt->gprune != JAMD_GPRUNE_NONE && opt->gprune != JAMD_GPRUNE_SAFE)
      return jamd_refuse("%s: gprune=%d is not a JAMD_GPRUNE_* value", who, opt->gprune);
    if (opt->gprune == JAMD_GPRUNE_SAFE && opt->gprune_num < 1) return jamd_refuse("%s: gprune safe needs gprune_num >= 1", who);
    if (opt->gprune == JAMD_GPRUNE_SAFE && opt->gprune_num > 64)
      return jamd_refuse("%s: gprune_num %d > 64 is not supported on the device", who, opt->gprune_num);
    if (opt->chunk_frames < 0) return jamd_refuse("%s: chunk_frames=%d is negative", who, opt->chunk_frames);
  }
  std::vector<JamdMsStream> strm((size_t)ns);
  long long sum = 0;
  for (int s = 0; s < ns; s++) {
    if (d->vsize[s] <= 0) return jamd_refuse("%s: vsize[%d]=%d is not positive", who, s, d->vsize[s]);
    strm[(size_t)s].off = (int)sum; strm[(size_t)s].len = d->vsize[s];
    sum += d->vsize[s];
    if (sum > d->veclen) break;
  }
  if (sum != d->veclen) return jamd_refuse("%s: vsize sums to %lld, veclen is %d", who, sum, d->veclen);
  if (d->dens_off[0] != 0) return jamd_refuse("%s: dens_off must start at 0", who);
  for (int g = 0; g < d->ndens; g++)
    if (d->dens_off[g + 1] < d->dens_off[g]) return jamd_refuse("%s: dens_off not monotone at %d", who, g);
  if (d->pdf_off[0] != 0 || d->pdf_off[d->npdf] != d->nentry) return jamd_refuse("%s: pdf_off must run from 0 to nentry", who);
  // the pdfs: stream ids, entry ranges, and every density as long as its pdf's stream
  const bool safe = opt && opt->gprune == JAMD_GPRUNE_SAFE;
  int nbook = 0, ntied = 0;
  for (int p = 0; p < d->npdf; p++) {
    const int n = d->pdf_off[p + 1] - d->pdf_off[p], sid = d->pdf_stream[p];
    if (n < 0) return jamd_refuse("%s: pdf_off not monotone at %d", who, p);
    if (sid < 0 || sid >= ns) return jamd_refuse("%s: pdf_stream[%d]=%d out of range (nstream=%d)", who, p, sid, ns);
    if (d->pdf_book && d->pdf_book[p] >= 0) {
      if (!opt)
        return jamd_refuse("%s: pdf %d is a tied-mixture pdf (pdf_book=%d); tied-mixture streams are not served", who, p, d->pdf_book[p]);
      ntied++;
      if (d->pdf_book[p] >= nbook) nbook = d->pdf_book[p] + 1;
    }
    const int len = d->vsize[sid];
    for (int i = 0; i < n; i++) {
      const int en = d->pdf_off[p] + i, dn = d->ent_dens[en];
      if (dn >= d->ndens) return jamd_refuse("%s: ent_dens[%d]=%d out of range (ndens=%d)", who, en, dn, d->ndens);
      if (dn >= 0 && d->dens_off[dn + 1] - d->dens_off[dn] != len)
        return jamd_refuse("%s: density %d has length %d, the vsize of stream %d (pdf %d) is %d", who, dn,
                           d->dens_off[dn + 1] - d->dens_off[dn], sid, p, len);
    }
  }
  // the codebooks: dense ids, one member list and one stream for all the pdfs of a book
  if (nbook > d->npdf) return jamd_refuse("%s: pdf_book: codebook ids are not dense (%d is named, there are %d pdfs)", who, nbook - 1, d->npdf);
  std::vector<int> book_first((size_t)nbook, -1);
  for (int p = 0; p < d->npdf && ntied; p++) {
    const int b = d->pdf_book[p];
    if (b < 0) continue;
    const int q = book_first[(size_t)b];
    if (q < 0) { book_first[(size_t)b] = p; continue; }
    if (d->pdf_stream[p] != d->pdf_stream[q])
      return jamd_refuse("%s: pdf_stream: codebook %d spans streams %d (pdf %d) and %d (pdf %d)", who, b, d->pdf_stream[q], q,
                         d->pdf_stream[p], p);
    const int n = d->pdf_off[p + 1] - d->pdf_off[p];
    if (n != d->pdf_off[q + 1] - d->pdf_off[q] ||
        (n && memcmp(d->ent_dens + d->pdf_off[p], d->ent_dens + d->pdf_off[q], sizeof(int) * (size_t)n) != 0))
      return jamd_refuse("%s: ent_dens: pdfs %d and %d of codebook %d do not list the same densities", who, q, p, b);
  }
  for (int b = 0; b < nbook; b++)
    if (book_first[(size_t)b] < 0)
      return jamd_refuse("%s: pdf_book: codebook ids are not dense (no pdf names book %d of 0 .. %d)", who, b, nbook - 1);
  const bool cached = ntied > 0 || safe;        // K1mt; otherwise K1m as jamd_gmm_ms_create() builds it
  // the states: one pdf of the right stream per slot, finite weights
  const size_t nslot = (size_t)d->nstate * ns;
  std::vector<float> st_w(nslot, 1.0f);
  for (size_t q = 0; q < nslot; q++) {
    const int s = (int)(q / ns), k = (int)(q % ns), p = d->st_pdf[q];
    if (p < 0 || p >= d->npdf) return jamd_refuse("%s: st_pdf[%d][%d]=%d out of range (npdf=%d)", who, s, k, p, d->npdf);
    if (d->pdf_stream[p] != k)
      return jamd_refuse("%s: st_pdf[%d][%d] names pdf %d, whose pdf_stream is %d", who, s, k, p, d->pdf_stream[p]);
    if (d->st_weight) {
      st_w[q] = d->st_weight[q];
      if (!std::isfinite(st_w[q])) return jamd_refuse("%s: st_weight[%d][%d] is not finite", who, s, k);
    }
  }

  // what is packed where: a plain pdf's records for K1m's loop (none), the books' members for the cache
  std::vector<JamdMsPdf> pdf((size_t)d->npdf);
  std::vector<JamdMsTpdf> tpdf(cached ? (size_t)d->npdf : 0);
  std::vector<JamdMsBook> book;
  std::vector<int> book_pdf;                      // the pdf whose entries are the book's members
  size_t nfloat = 0;
  bool has_plain = false;
  for (int b = 0; b < nbook; b++) book_pdf.push_back(book_first[(size_t)b]);
  for (int p = 0; p < d->npdf; p++) {
    const int n = d->pdf_off[p + 1] - d->pdf_off[p], len = d->vsize[d->pdf_stream[p]];
    const bool tied = ntied && d->pdf_book[p] >= 0;
    pdf[(size_t)p].rec = 0; pdf[(size_t)p].n = 0;
    if (cached) tpdf[(size_t)p] = JamdMsTpdf{-1, d->pdf_off[p], 0, 0};
    if (tied) tpdf[(size_t)p].book = d->pdf_book[p];
    else if (safe) { tpdf[(size_t)p].book = (int)book_pdf.size(); book_pdf.push_back(p); }   // a column of its own
    else {
      pdf[(size_t)p].rec = (int)nfloat; pdf[(size_t)p].n = n;
      nfloat += (size_t)n * jamd_ms_rec(len);
      has_plain = true;
    }
    if (nfloat > 0x7fffffffu) return jamd_refuse("%s: the model's records exceed 2^31 floats", who);
  }
  int maxall = 1, maxbook = 0, maxlen = 1;
  for (size_t b = 0; b < book_pdf.size(); b++) {
    const int p = book_pdf[b], n = d->pdf_off[p + 1] - d->pdf_off[p], sid = d->pdf_stream[p];
    book.push_back(JamdMsBook{(int)nfloat, n, strm[(size_t)sid].off, strm[(size_t)sid].len});
    nfloat += (size_t)n * jamd_ms_rec(d->vsize[sid]);
    if (nfloat > 0x7fffffffu) return jamd_refuse("%s: the model's records exceed 2^31 floats", who);
    if (n > maxall) maxall = n;
    if ((int)b < nbook && n > maxbook) maxbook = n;
    if (d->vsize[sid] > maxlen) maxlen = d->vsize[sid];
  }
  const int cap = safe ? (opt->gprune_num < maxall ? opt->gprune_num : maxall) : maxall;
  for (int p = 0; p < d->npdf && cached; p++)
    if (tpdf[(size_t)p].book >= 0) {
      const int n = book[(size_t)tpdf[(size_t)p].book].n;
      tpdf[(size_t)p].nmax = n < cap ? n : cap;
    }
  int chunk = 0;
  if (cached) {
    const size_t row = book.size() * ((size_t)cap * (sizeof(float) + sizeof(int)) + 2 * sizeof(int));
    chunk = opt->chunk_frames;
    if (chunk == 0) {
      chunk = kDefaultChunk;
      while (chunk > 128 && (size_t)(chunk + 1) * row > kDefaultScratch) chunk -= 128;
    }
  }

  // records, in the order the kernels load them
  std::vector<float> rec(nfloat, 0.0f);
  auto fill = [&](float *r, int p, int len, bool weights) {
    const int R = jamd_ms_rec(len), n = d->pdf_off[p + 1] - d->pdf_off[p];
    for (int i = 0; i < n; i++, r += R) {
      const int en = d->pdf_off[p] + i, dn = d->ent_dens[en];
      if (dn >= 0) {
        memcpy(r, d->mean + d->dens_off[dn], sizeof(float) * (size_t)len);
        memcpy(r + len, d->ivar + d->dens_off[dn], sizeof(float) * (size_t)len);
        r[2 * len] = d->gconst[dn];
      } else {
        r[2 * len] = __builtin_nanf("");   // NULL density (gprune_none.c:67)
      }
      r[2 * len + 1] = weights ? d->ent_logw[en] : 0.0f;
    }
  };
  for (int p = 0; p < d->npdf; p++)
    if (pdf[(size_t)p].n) fill(rec.data() + (size_t)pdf[(size_t)p].rec, p, d->vsize[d->pdf_stream[p]], true);
  for (size_t b = 0; b < book.size(); b++) fill(rec.data() + (size_t)book[b].rec, book_pdf[b], book[b].len, false);

  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_gmm_ms> g(new jamd_gmm_ms());   // (its members own what they hold)
  int rc;
  g->eng = e; g->S = d->nstate; g->D = d->veclen; g->nstream = ns; g->npdf = d->npdf;
  g->cached = cached;
  if (cached) {
    g->gprune = opt->gprune; g->cap = cap; g->chunk = chunk;
    g->nbook = nbook; g->nbook_all = (int)book.size(); g->maxbook = maxbook; g->maxlen = maxlen; g->has_plain = has_plain;
    if ((rc = jamd_gmm_ms_tied_setup(g.get())) != JAMD_OK) return rc;
    const size_t rows = (size_t)chunk + 1, nb = book.size();
    if ((rc = g->d_book.upload(book.data(), nb)) != JAMD_OK) return rc;
    if ((rc = g->d_tpdf.upload(tpdf.data(), tpdf.size())) != JAMD_OK) return rc;
    if ((rc = g->d_ent_logw.upload(d->ent_logw, (size_t)d->nentry)) != JAMD_OK) return rc;
    if ((rc = g->d_c_score.alloc(rows * nb * cap)) != JAMD_OK) return rc;
    if ((rc = g->d_c_id.alloc(rows * nb * cap)) != JAMD_OK) return rc;
    if ((rc = g->d_c_num.alloc(rows * nb, true)) != JAMD_OK) return rc;
    if ((rc = g->d_c_flag.alloc(rows * nb, true)) != JAMD_OK) return rc;
  } else if ((rc = jamd_gmm_ms_setup(g.get())) != JAMD_OK) return rc;
  if ((rc = g->d_rec.upload(rec.data(), rec.size())) != JAMD_OK) return rc;
  if ((rc = g->d_pdf.upload(pdf.data(), pdf.size())) != JAMD_OK) return rc;
  if ((rc = g->d_stream.upload(strm.data(), strm.size())) != JAMD_OK) return rc;
  if ((rc = g->d_st_pdf.upload(d->st_pdf, nslot)) != JAMD_OK) return rc;
  if ((rc = g->d_st_w.upload(st_w.data(), nslot)) != JAMD_OK) return rc;
  *out = g.release();
  return JAMD_OK;
}

int check_utts(const char *who, const jamd_gmm_ms *g, const void *in, const void *outp, const int *utt_off, int nutt) {
  if (!g || !in || !outp || !utt_off || nutt < 1 || utt_off[0] != 0) return jamd_refuse("%s: bad argument", who);
  for (int u = 0; u < nutt; u++)
    if (utt_off[u + 1] < utt_off[u]) return jamd_refuse("%s: utt_off must be non-decreasing", who);
  return JAMD_OK;
}

}  // namespace

extern "C" {

int jamd_gmm_ms_create(jamd_engine *e, const jamd_gmm_ms_desc *d, jamd_gmm_ms **out) {
  if (!e || !d || !out) return jamd_refuse("jamd_gmm_ms_create: NULL argument");
  *out = nullptr;
  return ms_build("jamd_gmm_ms_create", e, d, nullptr, out);
}

int jamd_gmm_ms_create_opt(jamd_engine *e, const jamd_gmm_ms_desc *d, const jamd_gmm_ms_opt *opt, jamd_gmm_ms **out) {
  if (out) *out = nullptr;
  if (!opt) return jamd_refuse("jamd_gmm_ms_create_opt: opt is NULL");
  if (!e || !d || !out) return jamd_refuse("jamd_gmm_ms_create_opt: NULL argument");
  return ms_build("jamd_gmm_ms_create_opt", e, d, opt, out);
}

void jamd_gmm_ms_destroy(jamd_gmm_ms *g) {
  if (!g) return;
  (void)hipSetDevice(g->eng->device);
  delete g;
}

int jamd_gmm_ms_nstate(const jamd_gmm_ms *g) { return g ? g->S : -1; }
int jamd_gmm_ms_veclen(const jamd_gmm_ms *g) { return g ? g->D : -1; }
int jamd_gmm_ms_nstream(const jamd_gmm_ms *g) { return g ? g->nstream : -1; }
int jamd_gmm_ms_tmix_cap(const jamd_gmm_ms *g) { return g ? (g->nbook ? g->cap : 0) : -1; }
int jamd_gmm_ms_nbook(const jamd_gmm_ms *g) { return g ? g->nbook : -1; }
const char *jamd_gmm_ms_last_kernel(const jamd_gmm_ms *g) { return g ? g->last_kernel : ""; }

int jamd_gmm_ms_outprob_utts_dev(jamd_gmm_ms *g, const float *dev_frames, const int *utt_off, int nutt, float *dev_out, void *stream) {
  int rc = check_utts("jamd_gmm_ms_outprob_utts_dev", g, dev_frames, dev_out, utt_off, nutt);
  if (rc != JAMD_OK) return rc;
  const int T = utt_off[nutt];
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(g->eng->device));
  hipStream_t st = jamd_stream(g->eng, stream);
  rc = g->cached ? jamd_gmm_ms_tied_launch(g, dev_frames, utt_off, nutt, dev_out, nullptr, nullptr, nullptr, st)
                 : jamd_gmm_ms_launch(g, dev_frames, T, dev_out, st);
  if (rc != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_gmm_ms_outprob_dev: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  return JAMD_OK;
}

int jamd_gmm_ms_outprob_dev(jamd_gmm_ms *g, const float *dev_frames, int T, float *dev_out, void *stream) {
  if (!g || !dev_frames || !dev_out || T < 0) return jamd_refuse("jamd_gmm_ms_outprob_dev: bad argument");
  const int off[2] = {0, T};
  return jamd_gmm_ms_outprob_utts_dev(g, dev_frames, off, 1, dev_out, stream);
}

int jamd_gmm_ms_outprob_utts_host(jamd_gmm_ms *g, const float *host_frames, const int *utt_off, int nutt, float *host_out) {
  const int rc = check_utts("jamd_gmm_ms_outprob_utts_host", g, host_frames, host_out, utt_off, nutt);
  if (rc != JAMD_OK) return rc;
  const int T = utt_off[nutt];
  if (T == 0) return JAMD_OK;
  return jamd_host_call(&g->stage, g->eng, host_frames, (size_t)T * g->D, host_out, (size_t)T * g->S,
                        [&](const float *in, float *o, hipStream_t st) -> long long {
                          const int rc = jamd_gmm_ms_outprob_utts_dev(g, in, utt_off, nutt, o, st);
                          return rc != JAMD_OK ? rc : (long long)T * g->S;
                        }, JAMD_ELAUNCH);
}

int jamd_gmm_ms_outprob_host(jamd_gmm_ms *g, const float *host_frames, int T, float *host_out) {
  if (!g || !host_frames || !host_out || T < 0) return jamd_refuse("jamd_gmm_ms_outprob_host: bad argument");
  const int off[2] = {0, T};
  return jamd_gmm_ms_outprob_utts_host(g, host_frames, off, 1, host_out);
}

int jamd_gmm_ms_tmix_cache_dev(jamd_gmm_ms *g, const float *dev_frames, int T, float *dev_score, int *dev_id, int *dev_num,
                               void *stream) {
  if (!g || !dev_frames || !dev_score || !dev_id || !dev_num || T < 0) return jamd_refuse("jamd_gmm_ms_tmix_cache_dev: bad argument");
  if (!g->cached || !g->nbook) { jamd_set_error("jamd_gmm_ms_tmix_cache_dev: model has no tied-mixture pdf"); return JAMD_ESTATE; }
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(g->eng->device));
  const int off[2] = {0, T};
  const int rc = jamd_gmm_ms_tied_launch(g, dev_frames, off, 1, nullptr, dev_score, dev_id, dev_num, jamd_stream(g->eng, stream));
  if (rc != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_gmm_ms_tmix_cache_dev: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  return JAMD_OK;
}

}  // extern "C"
