// rejgmm_api.hip -- the C ABI of GMM-based input rejection (jamd_rejgmm_*): validation, the object and its tables,
// scratch, gmm_end()'s verdict.  It launches nothing: the kernels and their launchers are in rejgmm.hip (rejgmm_host.h).
#include "rejgmm_host.h"

#include <cmath>

extern "C" {

int jamd_rejgmm_create(jamd_engine *e, const jamd_gmm_desc *gmm, const int *model_state, int nmodel, int gprune_num,
                       jamd_rejgmm **out) {
  if (!e || !gmm || !model_state || !out || nmodel < 1 || gprune_num < 1) { jamd_set_error("jamd_rejgmm_create: bad argument"); return JAMD_EINVAL; }
  *out = nullptr;
  if (gmm->nbook > 0 || gmm->nstream != 1) { jamd_set_error("jamd_rejgmm_create: tied-mixture and multi-stream GMMs are not supported (gmm_init(), gmm.c:431-434)"); return JAMD_EINVAL; }
  int maxmix = 1;
  for (int k = 0; k < nmodel; k++) {
    if (model_state[k] < 0 || model_state[k] >= gmm->nstate) { jamd_set_error("jamd_rejgmm_create: model_state[%d] out of range", k); return JAMD_EINVAL; }
    const int n = gmm->st_off[model_state[k] + 1] - gmm->st_off[model_state[k]];
    if (n > maxmix) maxmix = n;
  }
  const int need = gprune_num < maxmix ? gprune_num : maxmix;
  if (need > 64) { jamd_set_error("jamd_rejgmm_create: more than 64 Gaussians kept per model (-gmmnum %d, %d mixtures)", gprune_num, maxmix); return JAMD_EINVAL; }
  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_rejgmm> m(new jamd_rejgmm());   // (its members own what they hold)
  m->eng = e; m->D = gmm->veclen; m->nmodel = nmodel; m->gprune_num = gprune_num; m->maxmix = maxmix;
  int rc;
  if ((rc = m->d_mean.upload(gmm->mean, (size_t)gmm->ndens * gmm->veclen)) != JAMD_OK) return rc;
  if ((rc = m->d_ivar.upload(gmm->ivar, (size_t)gmm->ndens * gmm->veclen)) != JAMD_OK) return rc;
  if ((rc = m->d_gconst.upload(gmm->gconst, (size_t)gmm->ndens)) != JAMD_OK) return rc;
  if ((rc = m->d_logw.upload(gmm->ent_logw, (size_t)gmm->nentry)) != JAMD_OK) return rc;
  if ((rc = m->d_st_off.upload(gmm->st_off, (size_t)gmm->nstate + 1)) != JAMD_OK) return rc;
  if ((rc = m->d_ent_dens.upload(gmm->ent_dens, (size_t)gmm->nentry)) != JAMD_OK) return rc;
  if ((rc = m->d_model_state.upload(model_state, (size_t)nmodel)) != JAMD_OK) return rc;
  *out = m.release();
  return JAMD_OK;
}

void jamd_rejgmm_destroy(jamd_rejgmm *m) {
  if (!m) return;
  (void)hipSetDevice(m->eng->device);
  delete m;
}

int jamd_rejgmm_nmodel(const jamd_rejgmm *m) { return m ? m->nmodel : 0; }

int jamd_rejgmm_set_models(jamd_rejgmm *m, const char *const *names, const unsigned char *is_voice) {
  if (!m || !names || !is_voice) { jamd_set_error("jamd_rejgmm_set_models: NULL argument"); return JAMD_EINVAL; }
  m->names.assign(names, names + m->nmodel);
  m->is_voice.assign(is_voice, is_voice + m->nmodel);
  return JAMD_OK;
}

const char *jamd_rejgmm_model_name(const jamd_rejgmm *m, int k) {
  return (m && k >= 0 && k < (int)m->names.size()) ? m->names[k].c_str() : "";
}

// gmm_end() (gmm.c:614-660) + gmm_valid_input() (:672-679) on one row of utterance sums
int jamd_rejgmm_verdict(const jamd_rejgmm *m, const float *utt_scores, int *winner, float *cm, int *accepted) {
  if (!m || !utt_scores || !winner || !cm || !accepted) { jamd_set_error("jamd_rejgmm_verdict: NULL argument"); return JAMD_EINVAL; }
  float maxprob = JAMD_LOG_ZERO; int maxid = 0; bool found = false;
  for (int i = 0; i < m->nmodel; i++) if (maxprob < utt_scores[i]) { maxprob = utt_scores[i]; maxid = i; found = true; }
  float sum = 0.0f;
  for (int i = 0; i < m->nmodel; i++) sum += (float)pow(10.0, 0.05 * (double)(utt_scores[i] - maxprob));
  *winner = maxid; *cm = (float)(1.0 / sum);
  *accepted = found && (m->is_voice.empty() || m->is_voice[maxid]) ? 1 : 0;
  return JAMD_OK;
}
int jamd_rejgmm_veclen(const jamd_rejgmm *m) { return m ? m->D : 0; }

int jamd_rejgmm_frame_scores_dev(jamd_rejgmm *m, const float *dev_frames, int T, float *dev_out, void *stream) {
  if (!m || !dev_frames || !dev_out || T < 0) { jamd_set_error("jamd_rejgmm_frame_scores_dev: bad argument"); return JAMD_EINVAL; }
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(m->eng->device));
  hipStream_t st = jamd_stream(m->eng, stream);
  const int rc = rejgmm_launch_frames(m, st, dev_frames, T, dev_out);
  if (rc != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_rejgmm_frame_scores_dev: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  return JAMD_OK;
}

int jamd_rejgmm_utt_scores_dev(jamd_rejgmm *m, const float *dev_frame_scores, int T, const int *utt_off, int nutt,
                               float *dev_out, void *stream) {
  if (!m || !dev_frame_scores || !dev_out || !utt_off || nutt < 1 || T < 0) { jamd_set_error("jamd_rejgmm_utt_scores_dev: bad argument"); return JAMD_EINVAL; }
  if (utt_off[0] != 0 || utt_off[nutt] != T) { jamd_set_error("jamd_rejgmm_utt_scores_dev: utt_off must run from 0 to T"); return JAMD_EINVAL; }
  JAMD_HIP(hipSetDevice(m->eng->device));
  hipStream_t st = jamd_stream(m->eng, stream);
  int rc;
  if ((rc = m->d_utt_off.grow(sizeof(int) * ((size_t)nutt + 1))) != JAMD_OK) return rc;
  JAMD_HIP(hipMemcpyAsync(m->d_utt_off, utt_off, sizeof(int) * (nutt + 1), hipMemcpyHostToDevice, st));
  if ((rc = rejgmm_launch_sums(m, st, dev_frame_scores, nutt, dev_out)) != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_rejgmm_utt_scores_dev: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  return JAMD_OK;
}

int jamd_rejgmm_scores_host(jamd_rejgmm *m, const float *host_frames, int T, const int *utt_off, int nutt,
                            float *host_frame_scores, float *host_utt_scores) {
  if (!m || !host_frames || T < 0 || (!host_frame_scores && !host_utt_scores) || (host_utt_scores && (!utt_off || nutt < 1))) {
    jamd_set_error("jamd_rejgmm_scores_host: bad argument"); return JAMD_EINVAL;
  }
  if (T == 0) {
    if (host_utt_scores) for (int i = 0; i < nutt * m->nmodel; i++) host_utt_scores[i] = 0.0f;
    return JAMD_OK;
  }
  const size_t nfs = (size_t)T * m->nmodel, nus = host_utt_scores ? (size_t)nutt * m->nmodel : 0;
  return jamd_host_call(&m->stage, m->eng, host_frames, (size_t)T * m->D, host_frame_scores, nfs + nus,
                        [&](const float *in, float *o, hipStream_t st) -> long long {
                          int rc;
                          if ((rc = jamd_rejgmm_frame_scores_dev(m, in, T, o, st)) != JAMD_OK) return rc;
                          if (host_utt_scores) {   // the sums lie behind the frame scores and come down here
                            if ((rc = jamd_rejgmm_utt_scores_dev(m, o, T, utt_off, nutt, o + nfs, st)) != JAMD_OK) return rc;
                            JAMD_HIP(hipMemcpyAsync(host_utt_scores, o + nfs, sizeof(float) * nus, hipMemcpyDeviceToHost, st));
                          }
                          return host_frame_scores ? (long long)nfs : 0;
                        }, JAMD_ELAUNCH);
}

}  // extern "C"
