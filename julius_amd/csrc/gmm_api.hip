// gmm_api.hip -- the host layer of GMM scoring: everything of jamd_gmm that is not a kernel or a launcher.
//
// jamd_gmm_create() validates the caller's model and packs it into the records the kernels stream, the entry points check their arguments, keep the model's scratch and the utterance
// boundaries of the running call, and pick the scoring path by what the MODEL is (plain / gprune safe /
// tied-mixture); which kernel serves a plain call of a given length and vector length is the launcher's
// business (gmm_outprob.hip).  Nothing is launched from here: see gmm_host.h.
#include "gmm_host.h"

extern "C" {

int jamd_gmm_create(jamd_engine *e, const jamd_gmm_desc *d, int gprune, int gprune_num, jamd_gmm **out) {
  if (!e || !d || !out) { jamd_set_error("jamd_gmm_create: NULL argument"); return JAMD_EINVAL; }
  *out = nullptr;
  if (d->nstream != 1) {
    jamd_set_error("jamd_gmm_create: nstream=%d; only single-stream models are supported", d->nstream);
    return JAMD_EINVAL;
  }
  if (d->nstate <= 0 || d->veclen <= 0 || d->veclen > 1024 || d->nentry < 0 || d->ndens < 0) {
    jamd_set_error("jamd_gmm_create: bad dimensions S=%d D=%d G=%d E=%d", d->nstate, d->veclen,
                   d->ndens, d->nentry);
    return JAMD_EINVAL;
  }
  if (gprune != JAMD_GPRUNE_NONE && gprune != JAMD_GPRUNE_SAFE && gprune != JAMD_GPRUNE_HEU && gprune != JAMD_GPRUNE_BEAM) {
    jamd_set_error("jamd_gmm_create: unknown gprune method %d", gprune);
    return JAMD_EINVAL;
  }
  const bool history_pruning = gprune == JAMD_GPRUNE_HEU || gprune == JAMD_GPRUNE_BEAM;
  const int requested_gprune = gprune;
  // heu / beam on plain mixture states: calc_mix() passes last_id == NULL, the branch that is safe pruning
  // (gprune_heu.c:337-350, gprune_beam.c:337-350) -- same kernel, same numbers.  Checked below once the
  // states are classified.
  if (history_pruning) gprune = JAMD_GPRUNE_SAFE;
  if (!d->mean || !d->ivar || !d->gconst || !d->st_off || (d->nentry && (!d->ent_dens || !d->ent_logw))) {
    jamd_set_error("jamd_gmm_create: NULL model array");
    return JAMD_EINVAL;
  }
  if (d->st_off[0] != 0 || d->st_off[d->nstate] != d->nentry) {
    jamd_set_error("jamd_gmm_create: st_off must run from 0 to nentry");
    return JAMD_EINVAL;
  }
  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_gmm> g(new jamd_gmm());   // (its members own what they hold)
  int rc;
  g->eng = e; g->S = d->nstate; g->D = d->veclen; g->E = d->nentry;
  g->gprune = gprune; g->gprune_num = gprune_num;
  const int D = g->D;
  g->rec = ((2 * D + 2) + 3) & ~3;
  const bool have_books = d->nbook > 0 && d->st_book;
  std::vector<int> st_off_plain(g->S + 1, 0), tied;
  std::vector<int> book_first(d->nbook > 0 ? d->nbook : 0, -1);
  for (int s = 0; s < g->S; s++) {
    const int n = d->st_off[s + 1] - d->st_off[s];
    if (n < 0) { jamd_set_error("jamd_gmm_create: st_off not monotone at %d", s); return JAMD_EINVAL; }
    const int b = have_books ? d->st_book[s] : -1;
    if (b >= d->nbook) { jamd_set_error("jamd_gmm_create: codebook id %d out of range", b); return JAMD_EINVAL; }
    if (b >= 0) {
      tied.push_back(s);
      if (book_first[b] < 0) book_first[b] = s;
      else if (n != d->st_off[book_first[b] + 1] - d->st_off[book_first[b]]) {
        jamd_set_error("jamd_gmm_create: states of codebook %d disagree on its size", b); return JAMD_EINVAL;
      }
      st_off_plain[s + 1] = st_off_plain[s];
    } else {
      if (n > g->maxmix) g->maxmix = n;
      st_off_plain[s + 1] = st_off_plain[s] + n;
    }
  }
  g->E_plain = st_off_plain[g->S];
  g->ntied = (int)tied.size();
  // heu / beam over tied-mixture codebooks: frame t's thresholds come from the codebook's cached winners of frame
  // t - 1 (calc_tied_mix.c:203-215).  The device scores every state of every frame, so that history is the previous
  // frame of the same utterance: parity is defined against the reference under eager scoring
  // (outprob_set_batch_computation, outprob.c:230-242); see tmix_book_hist_kernel.
  if (history_pruning && g->ntied > 0) g->hist_method = requested_gprune;
  g->nbook = g->ntied ? d->nbook : 0;
  if (gprune == JAMD_GPRUNE_SAFE && gprune_num < 1) {
    jamd_set_error("jamd_gmm_create: gprune safe needs gprune_num >= 1"); return JAMD_EINVAL;
  }
  if (gprune == JAMD_GPRUNE_SAFE && gprune_num > 64) {
    jamd_set_error("jamd_gmm_create: gprune_num %d > 64 is not supported on the device", gprune_num);
    return JAMD_EINVAL;
  }
  auto fill_rec = [&](float *r, int dn, float lw) -> bool {
    if (dn >= d->ndens) return false;
    if (dn >= 0) {
      memcpy(r, d->mean + (size_t)dn * D, sizeof(float) * D);
      memcpy(r + D, d->ivar + (size_t)dn * D, sizeof(float) * D);
      r[2 * D] = d->gconst[dn];
      if (r[2 * D] != r[2 * D]) g->has_null = true;   // (a NaN gconst keeps the meaning it always had here)
    } else {
      r[2 * D] = __builtin_nanf("");   // NULL density (gprune_none.c:67)
      g->has_null = true;
    }
    r[2 * D + 1] = lw;
    return true;
  };
  // entry records of the plain states, contiguous in state order so the scalar
  // stream of a state range is one linear read (shared ~m/~v macros are
  // duplicated -- 288 GB of HBM makes that free).
  std::vector<float> rec((size_t)g->E_plain * g->rec, 0.0f);
  for (int s = 0; s < g->S; s++) {
    if (have_books && d->st_book[s] >= 0) continue;
    for (int k = 0; k < d->st_off[s + 1] - d->st_off[s]; k++) {
      const int en = d->st_off[s] + k;
      if (!fill_rec(rec.data() + (size_t)(st_off_plain[s] + k) * g->rec, d->ent_dens[en], d->ent_logw[en])) {
        jamd_set_error("jamd_gmm_create: density index %d out of range", d->ent_dens[en]); return JAMD_EINVAL;
      }
    }
  }
  if ((rc = g->d_rec.upload(rec.data(), rec.size())) != JAMD_OK) return rc;
  if (D == 39) {
    // the same records once more in the order K1's record ring loads them (jamd_gmm::d_rec_ring, gmm_host.h): packed
    // here, once per model -- 15.4 MB at 3000 states x 16 mixtures
    constexpr int kRing = 80;
    std::vector<float> ring((size_t)g->E_plain * kRing, 0.0f);
    for (int en = 0; en < g->E_plain; en++) {
      const float *r = rec.data() + (size_t)en * g->rec;
      float *q = ring.data() + (size_t)en * kRing;
      q[0] = r[2 * D]; q[1] = r[2 * D + 1];
      for (int k = 0; k < 7; k++) { q[2 + k] = r[k]; q[9 + k] = r[D + k]; }
      for (int c = 1; c < 5; c++)
        for (int k = 0; k < 8; k++) { q[16 * c + k] = r[8 * c - 1 + k]; q[16 * c + 8 + k] = r[D + 8 * c - 1 + k]; }
    }
    if ((rc = g->d_rec_ring.upload(ring.data(), ring.size())) != JAMD_OK) return rc;
    if ((rc = jamd_gmm_pull_setup(g.get())) != JAMD_OK) return rc;
  }
  if ((rc = g->d_st_off.upload(d->st_off, g->S + 1)) != JAMD_OK) return rc;
  if ((rc = g->d_st_off_plain.upload(st_off_plain.data(), g->S + 1)) != JAMD_OK) return rc;
  if (g->ntied) {
    // codebooks: the densities of book b in codebook order are the entries of any
    // state tied to it (GCODEBOOK.d[], htk_hmm.h:196-201)
    std::vector<int> book_off(g->nbook + 1, 0);
    for (int b = 0; b < g->nbook; b++) {
      const int n = book_first[b] >= 0 ? d->st_off[book_first[b] + 1] - d->st_off[book_first[b]] : 0;
      book_off[b + 1] = book_off[b] + n;
      if (n > g->maxbook) g->maxbook = n;
    }
    std::vector<float> brec((size_t)book_off[g->nbook] * g->rec, 0.0f);
    for (int b = 0; b < g->nbook; b++) {
      if (book_first[b] < 0) continue;
      for (int k = 0; k < book_off[b + 1] - book_off[b]; k++) {
        if (!fill_rec(brec.data() + (size_t)(book_off[b] + k) * g->rec,
                      d->ent_dens[d->st_off[book_first[b]] + k], 0.0f)) {
          jamd_set_error("jamd_gmm_create: codebook density index out of range"); return JAMD_EINVAL;
        }
      }
    }
    g->tm_cap = (gprune == JAMD_GPRUNE_NONE) ? g->maxbook : (gprune_num < g->maxbook ? gprune_num : g->maxbook);
    g->h_book_off = book_off;
    if ((rc = g->d_book_rec.upload(brec.data(), brec.size())) != JAMD_OK) return rc;
    if ((rc = g->d_book_off.upload(book_off.data(), g->nbook + 1)) != JAMD_OK) return rc;
    if ((rc = g->d_st_book.upload(d->st_book, g->S)) != JAMD_OK) return rc;
    if ((rc = g->d_ent_logw.upload(d->ent_logw, g->E)) != JAMD_OK) return rc;
    if ((rc = g->d_tied_states.upload(tied.data(), g->ntied)) != JAMD_OK) return rc;
  }
  *out = g.release();
  return JAMD_OK;
}

void jamd_gmm_destroy(jamd_gmm *g) {
  if (!g) return;
  (void)hipSetDevice(g->eng->device);
  delete g;
}

int jamd_gmm_nstate(const jamd_gmm *g) { return g ? g->S : -1; }
int jamd_gmm_veclen(const jamd_gmm *g) { return g ? g->D : -1; }
const char *jamd_gmm_last_kernel(const jamd_gmm *g) { return g ? g->last_kernel : ""; }

// number of per-Gaussian score columns: the mixture entries of a plain model in state order, the
// codebook Gaussians of a tied-mixture model in codebook order; 0 for a model that mixes both
int jamd_gmm_nentry(const jamd_gmm *g) {
  if (!g) return 0;
  if (g->ntied == 0) return g->E;
  if (g->ntied == g->S && !g->h_book_off.empty()) return g->h_book_off[g->nbook];
  return 0;
}

int jamd_gmm_book_offsets(const jamd_gmm *g, int *off, int cap) {
  if (!g || !off || g->ntied != g->S || (int)g->h_book_off.size() != g->nbook + 1 || cap < g->nbook + 1) {
    jamd_set_error("jamd_gmm_book_offsets: not an all-tied-mixture model, or buffer too small"); return JAMD_EINVAL;
  }
  memcpy(off, g->h_book_off.data(), sizeof(int) * (size_t)(g->nbook + 1));
  return JAMD_OK;
}

int jamd_gmm_dens_dev(jamd_gmm *g, const float *dev_frames, int T, float *dev_out, void *stream) {
  if (!g || !dev_frames || !dev_out || T < 0) { jamd_set_error("jamd_gmm_dens_dev: bad argument"); return JAMD_EINVAL; }
  const int E = jamd_gmm_nentry(g);
  if (E <= 0) {
    jamd_set_error("jamd_gmm_dens_dev: models mixing plain and tied-mixture states have no single column order");
    return JAMD_EINVAL;
  }
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(g->eng->device));
  hipStream_t st = jamd_stream(g->eng, stream);
  const int rc = jamd_gmm_launch_dens(g, g->ntied ? g->d_book_rec : g->d_rec, E, dev_frames, T, dev_out, st);
  if (rc != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_gmm_dens_dev: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  return JAMD_OK;
}

int jamd_gmm_dens_host(jamd_gmm *g, const float *host_frames, int T, float *host_out) {
  if (!g || !host_frames || !host_out || T < 0) { jamd_set_error("jamd_gmm_dens_host: bad argument"); return JAMD_EINVAL; }
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(g->eng->device));
  const int E = jamd_gmm_nentry(g);
  if (E <= 0) { jamd_set_error("jamd_gmm_dens_host: no single column order for this model"); return JAMD_EINVAL; }
  return jamd_host_call(&g->dens_stage, g->eng, host_frames, (size_t)T * g->D, host_out, (size_t)T * E,
                        [&](const float *in, float *o, hipStream_t st) -> long long {
                          const int rc = jamd_gmm_dens_dev(g, in, T, o, st);
                          return rc != JAMD_OK ? rc : (long long)T * E;
                        }, JAMD_ELAUNCH);
}

// utterance boundaries of the running call, for the one scoring path that cares where an input begins
static int set_utterances(jamd_gmm *g, const int *utt_off, int nutt, hipStream_t st) {
  if (g->ntied == 0 || g->gprune == JAMD_GPRUNE_NONE) return JAMD_OK;   // (heu / beam arrive here as safe + hist_method)
  // utt_off is the caller's memory: staged in a PINNED buffer the model owns, so that the copy is truly asynchronous (a
  // pipelining host keeps its scoring stream free of host waits; from pageable memory the runtime would either block or
  // stage).  The next call on this model waits for the copy before it rewrites the staging buffer (normally long done);
  // utt.d itself is ordered by the stream.
  const size_t bytes = sizeof(int) * ((size_t)nutt + 1);
  int rc;
  if ((rc = g->utt.begin(bytes < 4096 ? 4096 : bytes)) != JAMD_OK) return rc;
  memcpy(g->utt.h.p, utt_off, bytes);
  if ((rc = g->utt.send(bytes, st)) != JAMD_OK) return rc;
  g->cur_nutt = nutt;
  return JAMD_OK;
}

int jamd_gmm_outprob_dev(jamd_gmm *g, const float *dev_frames, int T, float *dev_out, void *stream) {
  const int off[2] = {0, T};
  if (T < 0) { jamd_set_error("jamd_gmm_outprob_dev: bad argument"); return JAMD_EINVAL; }
  return jamd_gmm_outprob_utts_dev(g, dev_frames, off, 1, dev_out, stream);
}

int jamd_gmm_outprob_utts_dev(jamd_gmm *g, const float *dev_frames, const int *utt_off, int nutt, float *dev_out, void *stream) {
  if (!g || !dev_frames || !dev_out || !utt_off || nutt < 1 || utt_off[0] != 0) {
    jamd_set_error("jamd_gmm_outprob_utts_dev: bad argument");
    return JAMD_EINVAL;
  }
  for (int u = 0; u < nutt; u++)
    if (utt_off[u + 1] < utt_off[u]) { jamd_set_error("jamd_gmm_outprob_utts_dev: utt_off must be non-decreasing"); return JAMD_EINVAL; }
  const int T = utt_off[nutt];
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(g->eng->device));
  hipStream_t st = jamd_stream(g->eng, stream);
  int rc = JAMD_OK;
  if ((rc = set_utterances(g, utt_off, nutt, st)) != JAMD_OK) return rc;
  if (g->E_plain == 0 && g->ntied == g->S) {
    // all states tied-mixture: nothing for the plain-state kernels to do
  } else if (g->gprune == JAMD_GPRUNE_SAFE) {
    // (gprune safe with N >= the largest mixture keeps every Gaussian but in descending-score order,
    // gprune_common.c:88; that order changes the table log-sum, so it goes through the sorted kernel like any N)
    rc = jamd_gmm_launch_safe(g, dev_frames, T, dev_out, st);
  } else {
    rc = jamd_gmm_launch_plain(g, dev_frames, T, dev_out, st);
  }
  if (rc != JAMD_OK) return rc;
  if (g->ntied) {
    // calc_tied_mix(): codebook top-N cache per (frame, book), then the states
    const size_t n = (size_t)T * g->nbook * g->tm_cap;
    if ((rc = g->d_tm_score.grow(sizeof(float) * n)) != JAMD_OK) return rc;
    if ((rc = g->d_tm_id.grow(sizeof(int) * n)) != JAMD_OK) return rc;
    if ((rc = g->d_tm_num.grow(sizeof(int) * (size_t)T * g->nbook)) != JAMD_OK) return rc;
    if ((rc = jamd_gmm_launch_tmix(g, dev_frames, T, dev_out, g->d_tm_score, g->d_tm_id, g->d_tm_num, st)) != JAMD_OK) return rc;
  }
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    jamd_set_error("jamd_gmm_outprob_dev: launch failed: %s", hipGetErrorString(le));
    return JAMD_ELAUNCH;
  }
  return JAMD_OK;
}

int jamd_gmm_outprob_host(jamd_gmm *g, const float *host_frames, int T, float *host_out) {
  if (!g || !host_frames || !host_out || T < 0) {
    jamd_set_error("jamd_gmm_outprob_host: bad argument");
    return JAMD_EINVAL;
  }
  if (T == 0) return JAMD_OK;
  return jamd_host_call(&g->stage, g->eng, host_frames, (size_t)T * g->D, host_out, (size_t)T * g->S,
                        [&](const float *in, float *o, hipStream_t st) -> long long {
                          const int rc = jamd_gmm_outprob_dev(g, in, T, o, st);
                          return rc != JAMD_OK ? rc : (long long)T * g->S;
                        }, JAMD_ELAUNCH);
}

int jamd_gmm_tmix_cap(const jamd_gmm *g) { return g ? g->tm_cap : -1; }
int jamd_gmm_nbook(const jamd_gmm *g) { return g ? g->nbook : -1; }

int jamd_gmm_tmix_cache_dev(jamd_gmm *g, const float *dev_frames, int T, float *dev_score,
                            int *dev_id, int *dev_num, void *stream) {
  if (!g || !dev_frames || !dev_score || !dev_id || !dev_num || T < 0) {
    jamd_set_error("jamd_gmm_tmix_cache_dev: bad argument");
    return JAMD_EINVAL;
  }
  if (!g->ntied) { jamd_set_error("jamd_gmm_tmix_cache_dev: model has no tied-mixture states"); return JAMD_ESTATE; }
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(g->eng->device));
  const int off[2] = {0, T};
  int rc = set_utterances(g, off, 1, jamd_stream(g->eng, stream));
  if (rc == JAMD_OK) rc = jamd_gmm_launch_tmix(g, dev_frames, T, nullptr, dev_score, dev_id, dev_num, jamd_stream(g->eng, stream));
  if (rc != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    jamd_set_error("jamd_gmm_tmix_cache_dev: launch failed: %s", hipGetErrorString(le));
    return JAMD_ELAUNCH;
  }
  return JAMD_OK;
}

}  // extern "C"
