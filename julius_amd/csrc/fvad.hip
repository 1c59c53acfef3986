// fvad.hip -- the kernels of the voice-activity detector (jamd_fvad) and their launchers (fvad_host.h).
//
// The detector is serial in time twice over -- the filter states run from sample to sample, the models from frame to
// frame -- and independent between channels, so a lane takes a channel and walks its frames in order; a workgroup is
// one wave of 64 channels and needs no barrier.  Everything a frame indexes at run time (the bands behind the split
// tree: 40 / 20 / 10 / 5 samples, the 2 x 12 Gaussians, the 6 x 16 entries of the minimum tracker and their ages, the
// per-Gaussian terms of the model update) lives in the lane's column of LDS, word i of lane l at [i * 64 + l]: two
// lanes share a bank's dword, a wave's access touches each bank once, and nothing goes to private memory (scratch).
// LogOfEnergy needs a band's maximum before it sums its squares, which is why a band is held at all; the first split
// needs no input buffer, it takes its samples (at 16 kHz: made from two each) as they come.  Between pushes the core
// lies in global memory, word-major ([word][channel]), so that the wave's loads and stores at either end are whole
// lines.  The arithmetic is fvad_core.h, shared with the host check; the model is read through a uniform pointer
// (scalar loads).  No atomics, no floating point.
#include "fvad_host.h"

struct FvGlobalArr {
  short *p;
  long long stride;
  __host__ __device__ short &operator[](int i) const { return p[i * stride]; }
};

struct FvPushArgs {
  const FvModel *model;
  const FvChanTab *tab;
  const int16_t *in;
  unsigned char *out;
  short *s16, *pend;
  int *s32, *npend;
  int nchan, fs;
};

__global__ __launch_bounds__(kFvLanes) void fv_push_kernel(FvPushArgs a) {
  __shared__ short lds[kFvWords * kFvLanes];
  const int c = blockIdx.x * kFvLanes + threadIdx.x;
  if (c >= a.nchan) return;
  const FvChanTab t = a.tab[c];
  if (t.n <= 0) return;                        // idle: untouched
  const long long C = a.nchan;
  const FvArr<kFvLanes> w{lds + threadIdx.x};
  for (int i = 0; i < kFvKept; i++) w[i] = a.s16[i * C + c];
  int s32[3] = {a.s32[c], a.s32[C + c], a.s32[2 * C + c]};
  const FvModel &m = *a.model;
  const int fs = a.fs, npend = a.npend[c];
  const bool wide = fs == kFvMaxFrame;
  const int16_t *in = a.in + t.src_off;
  const short *pend = a.pend + c;
  const long long total = (long long)npend + t.n;
  long long nf = total / fs;
  if (nf > t.nf) nf = t.nf;                   // (the host's count, which sized the output: the two agree)
  unsigned char *out = a.out + t.out_off;
  for (long long f = 0; f < nf; f++) {
    const long long base = f * fs - npend;     // of the frame's first sample in the chunk; negative: still waiting ones
    const int r = fv_frame(w, s32, m, wide, [&](int j) -> short {
      const long long i = base + j;
      return i < 0 ? pend[(i + npend) * C] : in[i];
    });
    out[f] = (unsigned char)r;
  }
  // what is left waits for its frame
  short *pw = a.pend + c;
  if (nf == 0) {
    for (int j = 0; j < t.n && npend + j < kFvMaxFrame; j++) pw[(npend + j) * C] = in[j];
    a.npend[c] = npend + t.n < kFvMaxFrame ? npend + t.n : kFvMaxFrame;
  } else {
    const long long from = nf * fs - npend;
    const int rest = (int)(t.n - from) < fs ? (int)(t.n - from) : fs;
    for (int j = 0; j < rest; j++) pw[j * C] = in[from + j];
    a.npend[c] = rest;
  }
  for (int i = 0; i < kFvKept; i++) a.s16[i * C + c] = w[i];
  a.s32[c] = s32[0]; a.s32[C + c] = s32[1]; a.s32[2 * C + c] = s32[2];
}

__global__ void fv_reset_kernel(const FvModel *model, const unsigned char *mask, short *s16, int *s32, int *npend, int nchan) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchan || (mask && !mask[c])) return;
  int s[3];
  fv_init(FvGlobalArr{s16 + c, nchan}, s, *model);
  s32[c] = s[0]; s32[nchan + c] = s[1]; s32[2 * (long long)nchan + c] = s[2];
  if (npend) npend[c] = 0;
}

int fv_launch_push(jamd_fvad *f, hipStream_t st, const FvChanTab *d_tab, const int16_t *dev_in, unsigned char *dev_out) {
  FvPushArgs a{f->d_model, d_tab, dev_in, dev_out, f->d_s16, f->d_pend, f->d_s32, f->d_npend, f->nchan, f->fs};
  hipLaunchKernelGGL(fv_push_kernel, dim3((f->nchan + kFvLanes - 1) / kFvLanes), dim3(kFvLanes), 0, st, a);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int fv_launch_reset_at(hipStream_t st, const FvModel *d_model, const unsigned char *d_mask, short *s16, int *s32, int *npend,
                       int nchan) {
  hipLaunchKernelGGL(fv_reset_kernel, dim3((nchan + 255) / 256), dim3(256), 0, st, d_model, d_mask, s16, s32, npend, nchan);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int fv_launch_reset(jamd_fvad *f, hipStream_t st, const unsigned char *d_mask) {
  return fv_launch_reset_at(st, f->d_model, d_mask, f->d_s16, f->d_s32, f->d_npend, f->nchan);
}
