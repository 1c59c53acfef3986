// jamd_internal.h -- shared internals of the gfx950 engine (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "julius_amd.h"

// addlog.c:28-30
#define JAMD_TBLSIZE 500000
#define JAMD_TMAG 33333.3333
// stddefs.h:176 / :111 / :109 (double constants in the reference)
#define JAMD_LOG_ADDMIN (-13.815510558)
#define JAMD_INV_LOG_TEN (.434294482)
#define JAMD_LOG_TEN 2.30258509
// calc_dnn.c:344-347
#define JAMD_LOGISTIC_FACTOR 20000
#define JAMD_LOGISTIC_MAX (16 * JAMD_LOGISTIC_FACTOR)

void jamd_set_error(const char *fmt, ...);

#define JAMD_HIP(call)                                                            \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      jamd_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),       \
                     __FILE__, __LINE__);                                         \
      return (e_ == hipErrorOutOfMemory) ? JAMD_ENOMEM : JAMD_ENODEV;             \
    }                                                                             \
  } while (0)

struct jamd_engine {
  int device = 0;
  hipStream_t stream = nullptr;   // the engine's own stream
  float *d_addlog = nullptr;      // [JAMD_TBLSIZE + 1]; the extra last entry is 0.0f
  float *d_logistic = nullptr;    // [JAMD_LOGISTIC_MAX + 1]
  float addmin_f = 0.f;           // smallest float >= LOG_ADDMIN (exact float form of the double compare)
  int num_cu = 256;
};

// A kernel whose static + dynamic LDS passes the default 64 KB window needs the attribute raised, and the sum
// must fit the 160 KB of a CU (the generic-D kernels keep 2 KB of frame data per vector component in LDS).
static inline int jamd_reserve_dyn_lds(const void *kernel, size_t dyn, const char *what) {
  if (dyn == 0) return JAMD_OK;
  hipFuncAttributes fa;
  JAMD_HIP(hipFuncGetAttributes(&fa, kernel));
  if (fa.sharedSizeBytes + dyn > 160u * 1024u) {
    jamd_set_error("%s: the vector length needs %zu bytes of LDS per workgroup (%zu static + %zu), the CU has 163840",
                   what, fa.sharedSizeBytes + dyn, (size_t)fa.sharedSizeBytes, dyn);
    return JAMD_EINVAL;
  }
  JAMD_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  return JAMD_OK;
}

// The first-pass tables of a binary N-gram file (mkbingram v5), as jamd_lexicon_desc carries them (csrc/readers.hip)
struct JamdNgramTables {
  int mode = 0, nword = 0, nbigram = 0, n = 0, dir = 0;
  std::vector<float> uni_prob, uni_bo, bi_prob;
  std::vector<int> bi_bgn, bi_num, bi_wid;
  std::string names;                     // the vocabulary, every name followed by NUL, in N-gram id order
};
bool jamd_read_bingram_tables(const char *path, JamdNgramTables &out);

static inline hipStream_t jamd_stream(jamd_engine *e, void *s) {
  return s ? (hipStream_t)s : e->stream;
}
