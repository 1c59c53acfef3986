// gmm_ms_host.h -- the host side of multi-stream GMM scoring: the model object, which gmm_ms_api.hip builds and owns
// (validation, packing, the C ABI of jamd_gmm_ms), and the launcher through which it reaches the kernel (gmm_ms.hip,
// K1m).  gmm_ms_api.hip launches nothing itself.  Internal, not installed.
#pragma once
#include "jamd_host.h"

// One mixture pdf / one stream as the kernel reads them (two ints each, one 8-byte scalar load).
struct JamdMsPdf { int rec; int n; };        // first float of the pdf's records in d_rec, mixture entries
struct JamdMsStream { int off; int len; };   // the stream's slice of the input vector

struct JAMD_LOCAL jamd_gmm_ms {
  jamd_engine *eng = nullptr;
  int S = 0, D = 0, nstream = 0, npdf = 0;
  // device model, written once by jamd_gmm_ms_create(); no call writes any of it
  JamdDev<float> d_rec;            // per pdf, its entries back to back: mean[len] | ivar[len] | gconst | ln w, padded to 4
                                   //   floats (len = the pdf's stream's vsize; a NULL density has gconst = NaN)
  JamdDev<JamdMsPdf> d_pdf;        // [npdf]
  JamdDev<JamdMsStream> d_stream;  // [nstream]
  JamdDev<int> d_st_pdf;           // [S][nstream]
  JamdDev<float> d_st_w;           // [S][nstream]
  size_t dyn_lds = 0;              // the kernel's dynamic LDS (the block's frames, transposed), reserved once at create
  JamdStage<float, float> stage;   // outprob_host
  char last_kernel[96] = {0};
};

// floats of one Gaussian record of a stream of `len` dimensions
static inline int jamd_ms_rec(int len) { return ((2 * len + 2) + 3) & ~3; }

// ---- gmm_ms.hip
// Once per model, from jamd_gmm_ms_create(): the LDS the kernel needs for this vector length (refused when a CU does
// not have it), so that the stream-ordered call asks the runtime nothing.
JAMD_LOCAL int jamd_gmm_ms_setup(jamd_gmm_ms *g);
// Every state of T frames: K1m.
JAMD_LOCAL int jamd_gmm_ms_launch(jamd_gmm_ms *g, const float *frames, int T, float *out, hipStream_t st);
