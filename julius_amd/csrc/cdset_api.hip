// cdset_api.hip -- the C ABI of the pseudo-phone state-set scores (jamd_cdset_*): validation, the object and its set
// tables.  It launches nothing: the kernel and its launcher are in cdset.hip (cdset_host.h).
#include "jamd_device.h"
#include "cdset_host.h"

extern "C" {

int jamd_cdset_create(jamd_engine *e, int nset, const int *set_off, const int *states, int method,
                      int nbest, jamd_cdset **out) {
  if (!e || !out || nset < 0 || (nset && (!set_off || !states))) {
    jamd_set_error("jamd_cdset_create: bad argument");
    return JAMD_EINVAL;
  }
  *out = nullptr;
  if (method != JAMD_IWCD_MAX && method != JAMD_IWCD_AVG && method != JAMD_IWCD_NBEST) {
    jamd_set_error("jamd_cdset_create: unknown method %d", method);
    return JAMD_EINVAL;
  }
  if (method == JAMD_IWCD_NBEST && (nbest < 1 || nbest > jamd::kNbestMax)) {
    jamd_set_error("jamd_cdset_create: nbest=%d outside [1,%d]", nbest, jamd::kNbestMax);
    return JAMD_EINVAL;
  }
  if (nset && set_off[0] != 0) { jamd_set_error("jamd_cdset_create: set_off[0] != 0"); return JAMD_EINVAL; }
  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_cdset> c(new jamd_cdset());   // (its members own what they hold)
  c->eng = e; c->nset = nset; c->method = method; c->nbest = nbest;
  c->nstates = nset ? set_off[nset] : 0;
  int rc;
  if ((rc = c->d_off.upload(set_off, nset ? nset + 1 : 0)) != JAMD_OK) return rc;   // (no set: tables of nothing)
  if ((rc = c->d_states.upload(states, c->nstates)) != JAMD_OK) return rc;
  *out = c.release();
  return JAMD_OK;
}

void jamd_cdset_destroy(jamd_cdset *c) {
  if (!c) return;
  (void)hipSetDevice(c->eng->device);
  delete c;
}

int jamd_cdset_nset(const jamd_cdset *c) { return c ? c->nset : -1; }

int jamd_cdset_outprob_dev(jamd_cdset *c, const float *dev_scores, int T, int nstate, float *dev_cd,
                           void *stream) {
  if (!c || !dev_scores || !dev_cd || T < 0 || nstate <= 0) {
    jamd_set_error("jamd_cdset_outprob_dev: bad argument");
    return JAMD_EINVAL;
  }
  if (T == 0 || c->nset == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(c->eng->device));
  const int rc = cdset_launch(c, jamd_stream(c->eng, stream), dev_scores, T, nstate, dev_cd);
  if (rc != JAMD_OK) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    jamd_set_error("jamd_cdset_outprob_dev: launch failed: %s", hipGetErrorString(le));
    return JAMD_ELAUNCH;
  }
  return JAMD_OK;
}

}  // extern "C"
