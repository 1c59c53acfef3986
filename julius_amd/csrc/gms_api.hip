// gms_api.hip -- the C ABI of Gaussian mixture selection (jamd_gms_*): validation, the object with the selection model it
// scores through jamd_gmm_dens_dev(), scratch.  It launches nothing: the kernels and their launcher are in gms.hip
// (gms_host.h).
#include "gms_host.h"

extern "C" {

int jamd_gms_create(jamd_engine *e, const jamd_gmm_desc *gs, const int *state2gs, int nstate, int nbest,
                    jamd_gms **out) {
  if (!e || !gs || !state2gs || !out || nstate <= 0 || nbest < 1) { jamd_set_error("jamd_gms_create: bad argument"); return JAMD_EINVAL; }
  *out = nullptr;
  if (gs->nbook > 0 || gs->nstream != 1) { jamd_set_error("jamd_gms_create: the selection model must be a plain single-stream GMM"); return JAMD_EINVAL; }
  for (int s = 0; s < nstate; s++)
    if (state2gs[s] >= gs->nstate) { jamd_set_error("jamd_gms_create: state2gs[%d] out of range", s); return JAMD_EINVAL; }
  // compute_g_max() starts from a state's last entry: the reference's reader cannot produce a state without one
  for (int i = 0; gs->st_off && i < gs->nstate; i++)
    if (gs->st_off[i + 1] - gs->st_off[i] < 1) { jamd_set_error("jamd_gms_create: selection state %d has no Gaussians", i); return JAMD_EINVAL; }
  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_gms> m(new jamd_gms());   // (its members own what they hold, the selection model included)
  m->eng = e; m->Sgs = gs->nstate; m->Egs = gs->nentry; m->S = nstate; m->nbest = nbest;
  int rc;
  if ((rc = jamd_gmm_create(e, gs, JAMD_GPRUNE_NONE, 0, &m->gs)) != JAMD_OK) return rc;
  if ((rc = m->d_st_off.upload(gs->st_off, gs->nstate + 1)) != JAMD_OK) return rc;
  if ((rc = m->d_logw.upload(gs->ent_logw, gs->nentry)) != JAMD_OK) return rc;
  if ((rc = m->d_state2gs.upload(state2gs, nstate)) != JAMD_OK) return rc;
  *out = m.release();
  return JAMD_OK;
}

int jamd_gms_nstate(const jamd_gms *m) { return m ? m->S : 0; }

int jamd_gms_set_strict_order(jamd_gms *m, int on) {
  if (!m) { jamd_set_error("jamd_gms_set_strict_order: NULL"); return JAMD_EINVAL; }
  m->strict = on != 0;
  return JAMD_OK;
}

void jamd_gms_destroy(jamd_gms *m) {
  if (!m) return;
  (void)hipSetDevice(m->eng->device);
  delete m;
}

int jamd_gms_apply_dev(jamd_gms *m, const float *dev_frames, int T, const int *utt_off, int nutt,
                       float *dev_scores, void *stream) {
  if (!m || !dev_frames || !dev_scores || T < 0 || (utt_off && nutt < 1)) { jamd_set_error("jamd_gms_apply_dev: bad argument"); return JAMD_EINVAL; }
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(m->eng->device));
  hipStream_t st = jamd_stream(m->eng, stream);
  const int one[2] = {0, T};
  if (!utt_off) { utt_off = one; nutt = 1; }
  if (utt_off[0] != 0 || utt_off[nutt] != T) { jamd_set_error("jamd_gms_apply_dev: utt_off must run from 0 to T"); return JAMD_EINVAL; }
  int rc;
  if ((rc = m->d_utt_off.grow(sizeof(int) * ((size_t)nutt + 1))) != JAMD_OK) return rc;
  if ((rc = m->d_dens.grow(sizeof(float) * ((size_t)T * m->Egs + 64))) != JAMD_OK) return rc;
  if ((rc = m->d_fs.grow(sizeof(float) * (size_t)T * m->Sgs)) != JAMD_OK) return rc;
  JAMD_HIP(hipMemcpyAsync(m->d_utt_off, utt_off, sizeof(int) * (nutt + 1), hipMemcpyHostToDevice, st));
  if ((rc = jamd_gmm_dens_dev(m->gs, dev_frames, T, m->d_dens, st)) != JAMD_OK) return rc;
  if (gms_lds_bytes(m->Sgs, m->Egs) > 159 * 1024) { jamd_set_error("jamd_gms_apply_dev: a selection model of %d states / %d Gaussians does not fit in LDS", m->Sgs, m->Egs); return JAMD_EINVAL; }
  if ((rc = gms_launch(m, st, T, nutt, dev_scores)) != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_gms_apply_dev: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  return JAMD_OK;
}

int jamd_gms_apply_host(jamd_gms *m, const float *host_frames, int T, const int *utt_off, int nutt,
                        float *host_scores) {
  if (!m || !host_frames || !host_scores || T < 0) { jamd_set_error("jamd_gms_apply_host: bad argument"); return JAMD_EINVAL; }
  if (T == 0) return JAMD_OK;
  const size_t nfr = (size_t)T * jamd_gmm_veclen(m->gs), nsc = (size_t)T * m->S;
  return jamd_host_call(&m->stage, m->eng, host_frames, nfr, host_scores, nsc,
                        [&](const float *in, float *o, hipStream_t st) -> long long {
                          JAMD_HIP(hipMemcpyAsync(o, host_scores, sizeof(float) * nsc, hipMemcpyHostToDevice, st));
                          const int rc = jamd_gms_apply_dev(m, in, T, utt_off, nutt, o, st);
                          return rc != JAMD_OK ? rc : (long long)nsc;
                        }, JAMD_ELAUNCH);
}

}  // extern "C"
