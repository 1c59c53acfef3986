// gmm_ms_api.hip -- the host layer of multi-stream GMM scoring: everything of jamd_gmm_ms that is not the kernel or
// its launcher.
//
// jamd_gmm_ms_create() checks the caller's description completely BEFORE the first device call (a refusal names the
// field and costs no upload), packs every mixture pdf's Gaussians in the order the kernel reads them -- a pdf shared
// by several states (a `~p` macro) is packed once -- and uploads once.  The entry points check their arguments.
// Nothing is launched from here: see gmm_ms_host.h.
#include "gmm_ms_host.h"

#include <cmath>

extern "C" {

int jamd_gmm_ms_create(jamd_engine *e, const jamd_gmm_ms_desc *d, jamd_gmm_ms **out) {
  if (!e || !d || !out) return jamd_refuse("jamd_gmm_ms_create: NULL argument");
  *out = nullptr;
  const int ns = d->nstream;
  if (ns < 1 || ns > 50) return jamd_refuse("jamd_gmm_ms_create: nstream=%d; 1 .. 50 streams (MAXSTREAMNUM) are supported", ns);
  if (d->nstate <= 0 || d->veclen <= 0 || d->npdf <= 0 || d->nentry < 0 || d->ndens < 0)
    return jamd_refuse("jamd_gmm_ms_create: bad dimensions nstate=%d veclen=%d npdf=%d nentry=%d ndens=%d", d->nstate,
                       d->veclen, d->npdf, d->nentry, d->ndens);
  if (!d->vsize || !d->pdf_stream || !d->pdf_off || !d->st_pdf || !d->dens_off || (d->nentry && (!d->ent_dens || !d->ent_logw)) ||
      (d->ndens && (!d->mean || !d->ivar || !d->gconst)))
    return jamd_refuse("jamd_gmm_ms_create: NULL model array");
  std::vector<JamdMsStream> strm((size_t)ns);
  long long sum = 0;
  for (int s = 0; s < ns; s++) {
    if (d->vsize[s] <= 0) return jamd_refuse("jamd_gmm_ms_create: vsize[%d]=%d is not positive", s, d->vsize[s]);
    strm[(size_t)s].off = (int)sum; strm[(size_t)s].len = d->vsize[s];
    sum += d->vsize[s];
    if (sum > d->veclen) break;
  }
  if (sum != d->veclen) return jamd_refuse("jamd_gmm_ms_create: vsize sums to %lld, veclen is %d", sum, d->veclen);
  if (d->dens_off[0] != 0) return jamd_refuse("jamd_gmm_ms_create: dens_off must start at 0");
  for (int g = 0; g < d->ndens; g++)
    if (d->dens_off[g + 1] < d->dens_off[g]) return jamd_refuse("jamd_gmm_ms_create: dens_off not monotone at %d", g);
  if (d->pdf_off[0] != 0 || d->pdf_off[d->npdf] != d->nentry) return jamd_refuse("jamd_gmm_ms_create: pdf_off must run from 0 to nentry");
  // the pdfs: stream ids, entry ranges, and every density as long as its pdf's stream
  std::vector<JamdMsPdf> pdf((size_t)d->npdf);
  size_t nfloat = 0;
  for (int p = 0; p < d->npdf; p++) {
    const int n = d->pdf_off[p + 1] - d->pdf_off[p], sid = d->pdf_stream[p];
    if (n < 0) return jamd_refuse("jamd_gmm_ms_create: pdf_off not monotone at %d", p);
    if (sid < 0 || sid >= ns) return jamd_refuse("jamd_gmm_ms_create: pdf_stream[%d]=%d out of range (nstream=%d)", p, sid, ns);
    if (d->pdf_book && d->pdf_book[p] >= 0)
      return jamd_refuse("jamd_gmm_ms_create: pdf %d is a tied-mixture pdf (pdf_book=%d); tied-mixture streams are not served", p, d->pdf_book[p]);
    const int len = d->vsize[sid];
    for (int i = 0; i < n; i++) {
      const int en = d->pdf_off[p] + i, dn = d->ent_dens[en];
      if (dn >= d->ndens) return jamd_refuse("jamd_gmm_ms_create: ent_dens[%d]=%d out of range (ndens=%d)", en, dn, d->ndens);
      if (dn >= 0 && d->dens_off[dn + 1] - d->dens_off[dn] != len)
        return jamd_refuse("jamd_gmm_ms_create: density %d has length %d, the vsize of stream %d (pdf %d) is %d", dn,
                           d->dens_off[dn + 1] - d->dens_off[dn], sid, p, len);
    }
    pdf[(size_t)p].rec = (int)nfloat; pdf[(size_t)p].n = n;
    nfloat += (size_t)n * jamd_ms_rec(len);
    if (nfloat > 0x7fffffffu) return jamd_refuse("jamd_gmm_ms_create: the model's records exceed 2^31 floats");
  }
  // the states: one pdf of the right stream per slot, finite weights
  const size_t nslot = (size_t)d->nstate * ns;
  std::vector<float> st_w(nslot, 1.0f);
  for (size_t q = 0; q < nslot; q++) {
    const int s = (int)(q / ns), k = (int)(q % ns), p = d->st_pdf[q];
    if (p < 0 || p >= d->npdf) return jamd_refuse("jamd_gmm_ms_create: st_pdf[%d][%d]=%d out of range (npdf=%d)", s, k, p, d->npdf);
    if (d->pdf_stream[p] != k)
      return jamd_refuse("jamd_gmm_ms_create: st_pdf[%d][%d] names pdf %d, whose pdf_stream is %d", s, k, p, d->pdf_stream[p]);
    if (d->st_weight) {
      st_w[q] = d->st_weight[q];
      if (!std::isfinite(st_w[q])) return jamd_refuse("jamd_gmm_ms_create: st_weight[%d][%d] is not finite", s, k);
    }
  }

  // records per pdf, in the order the kernel loads them
  std::vector<float> rec(nfloat, 0.0f);
  for (int p = 0; p < d->npdf; p++) {
    const int len = d->vsize[d->pdf_stream[p]], R = jamd_ms_rec(len);
    for (int i = 0; i < pdf[(size_t)p].n; i++) {
      const int en = d->pdf_off[p] + i, dn = d->ent_dens[en];
      float *r = rec.data() + (size_t)pdf[(size_t)p].rec + (size_t)i * R;
      if (dn >= 0) {
        memcpy(r, d->mean + d->dens_off[dn], sizeof(float) * (size_t)len);
        memcpy(r + len, d->ivar + d->dens_off[dn], sizeof(float) * (size_t)len);
        r[2 * len] = d->gconst[dn];
      } else {
        r[2 * len] = __builtin_nanf("");   // NULL density (gprune_none.c:67)
      }
      r[2 * len + 1] = d->ent_logw[en];
    }
  }

  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_gmm_ms> g(new jamd_gmm_ms());   // (its members own what they hold)
  int rc;
  g->eng = e; g->S = d->nstate; g->D = d->veclen; g->nstream = ns; g->npdf = d->npdf;
  if ((rc = jamd_gmm_ms_setup(g.get())) != JAMD_OK) return rc;
  if ((rc = g->d_rec.upload(rec.data(), rec.size())) != JAMD_OK) return rc;
  if ((rc = g->d_pdf.upload(pdf.data(), pdf.size())) != JAMD_OK) return rc;
  if ((rc = g->d_stream.upload(strm.data(), strm.size())) != JAMD_OK) return rc;
  if ((rc = g->d_st_pdf.upload(d->st_pdf, nslot)) != JAMD_OK) return rc;
  if ((rc = g->d_st_w.upload(st_w.data(), nslot)) != JAMD_OK) return rc;
  *out = g.release();
  return JAMD_OK;
}

void jamd_gmm_ms_destroy(jamd_gmm_ms *g) {
  if (!g) return;
  (void)hipSetDevice(g->eng->device);
  delete g;
}

int jamd_gmm_ms_nstate(const jamd_gmm_ms *g) { return g ? g->S : -1; }
int jamd_gmm_ms_veclen(const jamd_gmm_ms *g) { return g ? g->D : -1; }
int jamd_gmm_ms_nstream(const jamd_gmm_ms *g) { return g ? g->nstream : -1; }
const char *jamd_gmm_ms_last_kernel(const jamd_gmm_ms *g) { return g ? g->last_kernel : ""; }

int jamd_gmm_ms_outprob_dev(jamd_gmm_ms *g, const float *dev_frames, int T, float *dev_out, void *stream) {
  if (!g || !dev_frames || !dev_out || T < 0) return jamd_refuse("jamd_gmm_ms_outprob_dev: bad argument");
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(g->eng->device));
  const int rc = jamd_gmm_ms_launch(g, dev_frames, T, dev_out, jamd_stream(g->eng, stream));
  if (rc != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_gmm_ms_outprob_dev: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  return JAMD_OK;
}

int jamd_gmm_ms_outprob_host(jamd_gmm_ms *g, const float *host_frames, int T, float *host_out) {
  if (!g || !host_frames || !host_out || T < 0) return jamd_refuse("jamd_gmm_ms_outprob_host: bad argument");
  if (T == 0) return JAMD_OK;
  return jamd_host_call(&g->stage, g->eng, host_frames, (size_t)T * g->D, host_out, (size_t)T * g->S,
                        [&](const float *in, float *o, hipStream_t st) -> long long {
                          const int rc = jamd_gmm_ms_outprob_dev(g, in, T, o, st);
                          return rc != JAMD_OK ? rc : (long long)T * g->S;
                        }, JAMD_ELAUNCH);
}

}  // extern "C"
