// dnn_api.hip -- the C ABI of DNN scoring (jamd_dnn_*): validation, the object with its weights packed into the rows the
// layer kernel streams, scratch, and how a very long batch is cut into chunks whose softmax tails run on a side stream.
// It launches nothing: the kernels and their launchers are in dnn.hip (dnn_host.h).
#include "dnn_host.h"

extern "C" {

int jamd_dnn_create(jamd_engine *e, const jamd_dnn_desc *d, jamd_dnn **out) {
  if (!e || !d || !out || d->nlayer < 1 || !d->dims || !d->w || !d->b || !d->state_prior) {
    jamd_set_error("jamd_dnn_create: bad argument");
    return JAMD_EINVAL;
  }
  *out = nullptr;
  for (int l = 0; l <= d->nlayer; l++) {
    if (d->dims[l] <= 0) { jamd_set_error("jamd_dnn_create: dims[%d]=%d", l, d->dims[l]); return JAMD_EINVAL; }
    // dnn_layer_load() insists on 8-element aligned inputs on AVX/FMA hosts
    // (calc_dnn.c:395) and calc_dnn_fma() would silently drop a tail
    if (l < d->nlayer && d->dims[l] % 8 != 0) {
      jamd_set_error("jamd_dnn_create: layer %d input length %d is not a multiple of 8 "
                     "(same restriction as the reference's SIMD path)", l, d->dims[l]);
      return JAMD_EINVAL;
    }
  }
  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_dnn> n(new jamd_dnn());   // (its members own what they hold)
  n->eng = e; n->nlayer = d->nlayer;
  n->dims.assign(d->dims, d->dims + d->nlayer + 1);
  for (int v : n->dims) if (v > n->maxdim) n->maxdim = v;
  n->d_b = std::vector<JamdDev<float>>(d->nlayer);
  n->d_wr = std::vector<JamdDev<float>>(d->nlayer);
  int rc;
  for (int l = 0; l < d->nlayer; l++) {
    if ((rc = n->d_b[l].upload(d->b[l], n->dims[l + 1])) != JAMD_OK) return rc;
    // the weights as residue-major rows (dnn_layer_rs_kernel)
    const int K = n->dims[l], N = n->dims[l + 1], kmp = ((K / 8 + 7) / 8) * 8;
    std::vector<float> wr((size_t)N * 8 * kmp, 0.0f);
    for (int o = 0; o < N; o++)
      for (int k = 0; k < K; k++)
        wr[(size_t)o * 8 * kmp + (size_t)(k & 7) * kmp + dnn_rm_pos(k >> 3)] = d->w[l][(size_t)o * K + k];
    if ((rc = n->d_wr[l].upload(wr.data(), wr.size())) != JAMD_OK) return rc;
    n->kmp.push_back(kmp);
  }
  if ((rc = n->d_prior.upload(d->state_prior, n->dims[d->nlayer])) != JAMD_OK) return rc;
  if ((rc = n->d_zero.alloc(16, true)) != JAMD_OK) return rc;
  *out = n.release();
  return JAMD_OK;
}

void jamd_dnn_destroy(jamd_dnn *n) {
  if (!n) return;
  (void)hipSetDevice(n->eng->device);
  if (n->side) {                           // before the memory goes: what still runs on the side stream
    (void)hipStreamSynchronize(n->side);
    for (int i = 0; i < 8; i++) (void)hipEventDestroy(n->ev_gemm[i]);
    (void)hipEventDestroy(n->ev_tail); (void)hipEventDestroy(n->ev_start);
    (void)hipStreamDestroy(n->side);
  }
  delete n;
}

int jamd_dnn_nstate(const jamd_dnn *n) { return n ? n->dims[n->nlayer] : -1; }
int jamd_dnn_veclen(const jamd_dnn *n) { return n ? n->dims[0] : -1; }

int jamd_dnn_outprob_dev(jamd_dnn *n, const float *dev_frames, int T, float *dev_out, void *stream) {
  if (!n || !dev_frames || !dev_out || T < 0) {
    jamd_set_error("jamd_dnn_outprob_dev: bad argument");
    return JAMD_EINVAL;
  }
  if (T == 0) return JAMD_OK;
  JAMD_HIP(hipSetDevice(n->eng->device));
  hipStream_t st = jamd_stream(n->eng, stream);
  int rc;
  // hidden activations ping-pong between two [T][maxhidden] buffers
  int maxh = 1;
  for (int l = 1; l < n->nlayer; l++) if (8 * n->kmp[l] > maxh) maxh = 8 * n->kmp[l];
  if ((rc = n->d_xr.grow(sizeof(float) * (size_t)T * 8 * n->kmp[0])) != JAMD_OK) return rc;
  for (int k = 0; k < 2; k++)
    if ((rc = n->d_act[k].grow(sizeof(float) * (size_t)T * maxh)) != JAMD_OK) return rc;
  if ((rc = n->d_lse.grow(sizeof(float) * (size_t)T)) != JAMD_OK) return rc;
  // The output layer is followed by the serial row log-sum (dnn_lse: one lane per frame, a
  // latency-bound chain of table gathers that keeps ~1 wave per CU busy) and the
  // normalisation.  For very long batches (>= 131072 frames) the frames are cut into up to 8 chunks of 32768+ frames; chunk c's tail
  // runs on a side stream and overlaps chunk c+1's GEMMs, whose blocks leave registers and
  // issue slots free for it.
  int nchunk = T >= 131072 ? (T + 32767) / 32768 : 1;  // measured: pays (+4.5 %) only for very long batches
  if (nchunk > 8) nchunk = 8;
#ifdef JAMD_DEV
  if (getenv("JAMD_DNN_NOCHUNK")) nchunk = 1;
#endif
  int per = ((T + nchunk - 1) / nchunk + kDnnRowBlock - 1) / kDnnRowBlock * kDnnRowBlock;
  if (nchunk > 1 && n->side == nullptr) {
    JAMD_HIP(hipStreamCreateWithFlags(&n->side, hipStreamNonBlocking));
    for (int i = 0; i < 8; i++) JAMD_HIP(hipEventCreateWithFlags(&n->ev_gemm[i], hipEventDisableTiming));
    JAMD_HIP(hipEventCreateWithFlags(&n->ev_tail, hipEventDisableTiming));
    JAMD_HIP(hipEventCreateWithFlags(&n->ev_start, hipEventDisableTiming));
  }
  if (nchunk > 1) {     // the side stream must not start before earlier work on the caller's stream
    JAMD_HIP(hipEventRecord(n->ev_start, st));
    JAMD_HIP(hipStreamWaitEvent(n->side, n->ev_start, 0));
  }
  for (int c = 0, t0 = 0; t0 < T; c++, t0 += per) {
    const int Tc = (T - t0 < per) ? T - t0 : per;
    if ((rc = dnn_launch_layers(n, st, dev_frames, t0, Tc, dev_out)) != JAMD_OK) return rc;
    hipStream_t ts = st;
    if (nchunk > 1) {
      JAMD_HIP(hipEventRecord(n->ev_gemm[c], st));
      JAMD_HIP(hipStreamWaitEvent(n->side, n->ev_gemm[c], 0));
      ts = n->side;
    }
    if ((rc = dnn_launch_tail(n, ts, t0, Tc, dev_out)) != JAMD_OK) return rc;
  }
  if (nchunk > 1) {     // join: the caller's stream continues only after the last tail
    JAMD_HIP(hipEventRecord(n->ev_tail, n->side));
    JAMD_HIP(hipStreamWaitEvent(st, n->ev_tail, 0));
  }
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    jamd_set_error("jamd_dnn_outprob_dev: launch failed: %s", hipGetErrorString(le));
    return JAMD_ELAUNCH;
  }
  return JAMD_OK;
}

int jamd_dnn_outprob_host(jamd_dnn *n, const float *host_frames, int T, float *host_out) {
  if (!n || !host_frames || !host_out || T < 0) {
    jamd_set_error("jamd_dnn_outprob_host: bad argument");
    return JAMD_EINVAL;
  }
  if (T == 0) return JAMD_OK;
  const int D = n->dims[0], S = n->dims[n->nlayer];
  return jamd_host_call(&n->stage, n->eng, host_frames, (size_t)T * D, host_out, (size_t)T * S,
                        [&](const float *in, float *o, hipStream_t st) -> long long {
                          const int rc = jamd_dnn_outprob_dev(n, in, T, o, st);
                          return rc != JAMD_OK ? rc : (long long)T * S;
                        }, JAMD_ELAUNCH);
}

}  // extern "C"
