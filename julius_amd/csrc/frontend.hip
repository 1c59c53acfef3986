// frontend.hip -- the audio front end on gfx950: int16 PCM -> MFCC / FBANK / MELSPEC features.
//
// Reproduces the reference's buffered front end bit for bit: Wav2MFCC() (libsent/src/wav2mfcc/
// wav2mfcc-buffer.c:58-100) with WMP_calc() and the tables of mfcc-core.c (MFCC_SINCOS_TABLE), then
// the splicing of libjulius/src/wav2mfcc.c:162-169.  Every expression keeps the reference's types
// (float *= double in Hamming and liftering, double butterflies with float stores, float += double in
// the DCT, ...) and, like the rest of the library, is compiled with -ffp-contract=off.  Every SUM of
// the reference stays serial in its own order on one lane: the zero-mean sum, the energy sum, each
// filter-bank bin, each DCT coefficient, C0 and the per-utterance CMN / MVN sums.  What is
// independent is spread over lanes: samples, pre-emphasis, the window, the butterflies of an FFT
// stage, the bins, the coefficients, the frames.
//
//   fe_frame_kernel   one wave per frame, four frames per workgroup: WMP_calc() -> statics[T][baselen]; its
//                     instantiation <true> carries the spectral subtraction of MakeFBank() behind the FFT
//   fe_noise_frame    one wave per head frame: |X| of all fftN indices in double (new_SS_calculate(), ss.c:110-172)
//   fe_noise_mean     one lane per (utterance, FFT index): the float chain over the head frames, then / framenum
//   fe_emax_kernel    one workgroup per utterance: the max of NormaliseLogE() (order-free)
//   fe_feat_kernel    one lane per (frame, element): normalised energy, Delta(), Accel() -> feat[T][veclen]
//   fe_stats_kernel   one lane per (utterance, dimension): the serial float sums of CMN() / MVN()
//   fe_write_kernel   one lane per output element: normalisation and splicing -> out[T'][veclen * splice]
//
// This unit holds the kernels and, at its end, their launchers (declared in frontend_host.h); the jamd_frontend_* entries
// that call them are in frontend_api.hip, the tables the kernels read are built in frontend_tables.h.
#include "jamd_device.h"
#include "frontend_host.h"
#include <cmath>
#include <cstdint>

namespace {

constexpr int kFeFrames = 4;   // frames (waves) per workgroup of the frame kernel

// One window -> its spectrum in xr / xi: load, ZMeanFrame(), PreEmphasise(), Hamming(), zero padding, FFT().  This
// is the first half of WMP_calc() and the whole per-frame work of new_SS_calculate(); the two energy sums of
// WMP_calc() sit at their places in it (kEnergy; new_SS_calculate() has no energy term).  Returns the log energy
// on lane 0.  (FeParams by value: by reference the register allocation of the whole frame kernel changes.)
template <bool kEnergy>
__device__ __forceinline__ float fe_spectrum(const FeParams p, const int16_t *wave, int lane, float *xr, float *xi, float *tmp, double *misc) {
  const int nv2 = p.fftN >> 1;
  for (int i = lane; i < p.fftN; i += 64) { xr[i] = i < p.framesize ? (float)wave[i] : 0.0f; xi[i] = 0.0f; }
  __syncthreads();
  if (p.zmean) {                              // ZMeanFrame(): float sum in sample order
    if (lane == 0) {
      float mean = 0.0f;
      for (int i = 0; i < p.framesize; i++) mean += xr[i];
      mean /= p.framesize;
      misc[0] = mean;
    }
    __syncthreads();
    const float mean = (float)misc[0];
    for (int i = lane; i < p.framesize; i += 64) xr[i] -= mean;
    __syncthreads();
  }
  float energy = 0.0f;
  if (kEnergy && p.energy && p.raw_e && lane == 0) {     // CalcLogRawE(): double accumulator of float products
    double raw_E = 0.0;
    for (int i = 0; i < p.framesize; i++) raw_E += xr[i] * xr[i];
    energy = (float)log(raw_E);
  }
  // PreEmphasise() (descending in place = every sample minus its ORIGINAL predecessor), via xi
  for (int i = lane; i < p.framesize; i += 64)
    xi[i] = i > 0 ? xr[i] - xr[i - 1] * p.preEmph : (float)(xr[0] * (1.0 - p.preEmph));
  __syncthreads();
  for (int i = lane; i < p.fftN; i += 64) {   // Hamming(): float *= double
    if (i < p.framesize) xr[i] = (float)(xi[i] * p.ham[i]);
    xi[i] = 0.0f;
  }
  __syncthreads();
  if (kEnergy && p.energy && !p.raw_e && lane == 0) {
    double raw_E = 0.0;
    for (int i = 0; i < p.framesize; i++) raw_E += xr[i] * xr[i];
    energy = (float)log(raw_E);
  }
  // FFT(): the serial loop's bit-reversal swaps are the bit-reversal permutation (Im is all zero here)
  for (int i = lane; i < p.fftN; i += 64) tmp[i] = xr[i];
  __syncthreads();
  for (int i = lane; i < p.fftN; i += 64) xr[__brev((unsigned)i) >> (32 - p.logn)] = tmp[i];
  __syncthreads();
  for (int m = 1; m <= p.logn; m++) {
    const int me1 = 1 << (m - 1);
    for (int b = lane; b < nv2; b += 64) {
      const int j = b & (me1 - 1);
      const int i = ((b >> (m - 1)) << m) + j, ip = i + me1;
      const double uRe = p.twRe[me1 - 1 + j], uIm = p.twIm[me1 - 1 + j];
      const float pr = xr[ip], pi = xi[ip], ar = xr[i], ai = xi[i];
      const double tRe = pr * uRe - pi * uIm;
      const double tIm = pr * uIm + pi * uRe;
      xr[ip] = (float)(ar - tRe); xi[ip] = (float)(ai - tIm);
      xr[i] = (float)(ar + tRe);  xi[i] = (float)(ai + tIm);
    }
    __syncthreads();
  }
  return energy;
}

// LDS per wave: Re[fftN] | Im[fftN] | A[nv2 + 1] (double; also the bit-reversal staging) | fb[fbank_num + 1] | misc[2]
// noise / nstride / alpha / floor_ are read by the <true> instantiation only: the spectrum of utterance u is
// noise + u * nstride (-sscalc: nstride fftN; -ssload: one spectrum for all, nstride 0).
template <bool kSS>
__global__ void __launch_bounds__(64 * kFeFrames)
fe_frame_kernel(FeParams p, const int16_t *__restrict__ samples, const long long *__restrict__ soff,
                const int *__restrict__ foff, int Ttot, float *__restrict__ statics, const float *__restrict__ noise,
                int nstride, float alpha, float floor_) {
  extern __shared__ double fe_lds[];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nv2 = p.fftN >> 1;
  const size_t per = (size_t)p.fftN + (nv2 + 1) + (p.fbank_num + 1) + 2;   // doubles per wave
  double *base = fe_lds + per * wv;
  float *xr = (float *)base, *xi = xr + p.fftN;
  double *A = base + p.fftN, *fb = A + nv2 + 1, *misc = fb + p.fbank_num + 1;
  float *tmp = (float *)A;

  const int g = blockIdx.x * (int)(blockDim.x >> 6) + wv;   // kFeFrames waves per workgroup, fewer for fftN 4096
  const bool valid = g < Ttot;
  const int gg = valid ? g : Ttot - 1;       // idle waves recompute the last frame (same barriers), store nothing
  const int u = jamd::find_span(foff, p.nutt, gg);
  const long long s0 = soff[u] + (long long)(gg - foff[u]) * p.frameshift;
  const int16_t *wave = samples + s0;
  const float energy = fe_spectrum<true>(p, wave, lane, xr, xi, tmp, misc);
  if (kSS) {
    // MakeFBank()'s spectral subtraction (mfcc-core.c:473-487) over the indices the filter bank reads; every lane
    // rewrites the k it reads below, so the barrier behind the FFT is all this needs.  P == 0 over a zero noise
    // entry divides 0 by 0: NaN, as there.
    const float *np = noise + (size_t)u * nstride;
    for (int k = p.klo + lane; k <= p.khi; k += 64) {
      const double Re = xr[k - 1], Im = xi[k - 1];
      const double P = sqrt(Re * Re + Im * Im);
      const double NP = np[k - 1];
      const double d = P * P - alpha * NP * NP;
      double H;
      if (d < 0) H = floor_;
      else H = sqrt(d) / P;
      xr[k - 1] = (float)(H * Re);
      xi[k - 1] = (float)(H * Im);
    }
  }
  // MakeFBank(): |X| (or |X|^2) per FFT index, then every bin sums its k in ascending order
  for (int k = p.klo + lane; k <= p.khi; k += 64) {
    const double re = xr[k - 1], im = xi[k - 1];
    A[k] = p.usepower ? re * re + im * im : sqrt(re * re + im * im);
  }
  __syncthreads();
  for (int bin = 1 + lane; bin <= p.fbank_num; bin += 64) {
    double f = 0.0;
    for (int k = p.kfirst[bin]; k <= p.klast[bin]; k++) {
      const double a = A[k];
      const double re = p.loWt[k] * a;
      if (p.loChan[k] == bin) f += re;        // this bin is the k's lower channel
      else f += a - re;                       // loChan == bin - 1
    }
    if (p.log_fbank) {
      if (f < 1.0) f = 1.0;
      f = log(f);
    }
    fb[bin] = f;
  }
  __syncthreads();
  float *out = statics + (size_t)gg * p.baselen;
  if (p.fbank_only) {
    for (int q = lane; q < p.mfcc_dim; q += 64)
      if (valid) out[q] = (float)fb[q + 1];
    return;
  }
  for (int i = lane; i < p.mfcc_dim; i += 64) {   // MakeMFCC() + WeightCepstrum()
    const double *tb = p.dct + (size_t)i * p.fbank_num;
    float c = 0.0f;
    for (int j = 1; j <= p.fbank_num; j++) c += fb[j] * tb[j - 1];
    c *= p.sqrt2var;
    c *= p.wcep[i];
    if (valid) out[i] = c;
  }
  if (lane == 0 && valid) {
    int q = p.mfcc_dim;
    if (p.c0) {                               // CalcC0(): float += double
      float S = 0.0f;
      for (int i = 1; i <= p.fbank_num; i++) S += fb[i];
      out[q++] = S * p.sqrt2var;
    }
    if (p.energy) out[q] = energy;
  }
}

// new_SS_calculate() (ss.c:130-161), the part per frame: |X| of every FFT index of head frame g, in double, to
// mag[g][fftN].  `hoff` holds the head frames of the utterances back to back, as foff holds all their frames; the grid
// decode and the LDS carve are the frame kernel's.
__global__ void __launch_bounds__(64 * kFeFrames)
fe_noise_frame(FeParams p, const int16_t *__restrict__ samples, const long long *__restrict__ soff,
               const int *__restrict__ hoff, int Htot, double *__restrict__ mag) {
  extern __shared__ double fe_lds[];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nv2 = p.fftN >> 1;
  const size_t per = (size_t)p.fftN + (nv2 + 1) + (p.fbank_num + 1) + 2;   // doubles per wave
  double *base = fe_lds + per * wv;
  float *xr = (float *)base, *xi = xr + p.fftN;
  double *A = base + p.fftN, *misc = A + (nv2 + 1) + (p.fbank_num + 1);   // (no bins here: the frame kernel's carve)
  float *tmp = (float *)A;

  const int g = blockIdx.x * (int)(blockDim.x >> 6) + wv;   // kFeFrames waves per workgroup, fewer for fftN 4096
  const bool valid = g < Htot;
  const int gg = valid ? g : Htot - 1;       // idle waves recompute the last frame (same barriers), store nothing
  const int u = jamd::find_span(hoff, p.nutt, gg);
  const long long s0 = soff[u] + (long long)(gg - hoff[u]) * p.frameshift;
  const int16_t *wave = samples + s0;
  (void)fe_spectrum<false>(p, wave, lane, xr, xi, tmp, misc);
  if (!valid) return;
  double *out = mag + (size_t)gg * p.fftN;
  for (int i = lane; i < p.fftN; i += 64) {
    const double x = xr[i], y = xi[i];
    out[i] = sqrt(x * x + y * y);
  }
}

// new_SS_calculate()'s sum (ss.c:158-167): spec[i] += |X| is float += double, a rounding chain per index in frame
// order, so one lane walks the head frames of its (utterance, index); then the float division by the frame count.
// Consecutive lanes take consecutive indices of one row of mag.
__global__ void __launch_bounds__(256)
fe_noise_mean(int fftN, int nutt, const int *__restrict__ hoff, const double *__restrict__ mag, float *__restrict__ noise) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)nutt * fftN) return;
  const int u = (int)(idx / fftN), i = (int)(idx % fftN);
  const int h0 = hoff[u], framenum = hoff[u + 1] - h0;
  const double *col = mag + (size_t)h0 * fftN + i;
  float acc = 0.0f;
  for (int t = 0; t < framenum; t++) acc = (float)((double)acc + col[(size_t)t * fftN]);
  acc /= (float)framenum;
  noise[idx] = acc;
}

// NormaliseLogE()'s max: order-free, so a tree (no NaN reaches it: log of a non-negative double)
__global__ void __launch_bounds__(256)
fe_emax_kernel(FeParams p, const float *__restrict__ statics, const int *__restrict__ foff, float *__restrict__ emax) {
  __shared__ float red[256];
  const int u = blockIdx.x, l = p.baselen - 1;
  float m = -INFINITY;
  for (int t = foff[u] + threadIdx.x; t < foff[u + 1]; t += 256) m = fmaxf(m, statics[(size_t)t * p.baselen + l]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) emax[u] = red[0];
}

__device__ __forceinline__ float fe_base(const FeParams &p, const float *statics, const float *emax, int u, int g, int n) {
  float v = statics[(size_t)g * p.baselen + n];
  if (p.enormal && p.energy && n == p.baselen - 1) {   // NormaliseLogE()
    const float max = emax[u];
    const float min = (float)(max - (p.silFloor * JAMD_LOG_TEN) / 10.0);
    float f = v;
    if (f < min) f = min;
    v = (float)(1.0 - (max - f) * p.escale);
  }
  return v;
}

__device__ __forceinline__ float fe_delta(const FeParams &p, const float *statics, const float *emax, int u, int g0,
                                          int T, int t, int n) {   // Delta(), edge frames replicated
  int B = 0;
  for (int th = 1; th <= p.delWin; th++) B += th * th;
  float sum = 0;
  for (int th = 1; th <= p.delWin; th++) {
    const float A1 = fe_base(p, statics, emax, u, g0 + (t - th < 0 ? 0 : t - th), n);
    const float A2 = fe_base(p, statics, emax, u, g0 + (t + th >= T ? T - 1 : t + th), n);
    sum += th * (A2 - A1);
  }
  sum /= (2.0 * B);
  return sum;
}

// One lane per (frame, element) of the vector after Delta() / Accel(); the deltas are read from the
// statics (never from a half-written vector), so the in-place order of the reference does not matter.
__global__ void __launch_bounds__(256)
fe_feat_kernel(FeParams p, const float *__restrict__ statics, const float *__restrict__ emax, const int *__restrict__ foff,
               int Ttot, float *__restrict__ feat) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Ttot * p.veclen) return;
  const int g = (int)(idx / p.veclen), e = (int)(idx % p.veclen);
  const int u = jamd::find_span(foff, p.nutt, g);
  const int g0 = foff[u], T = foff[u + 1] - g0, t = g - g0;
  const int nb = p.baselen - (p.absesup ? 1 : 0);
  float v;
  if (e < nb) v = fe_base(p, statics, emax, u, g, e);
  else if (e < nb + p.baselen) v = fe_delta(p, statics, emax, u, g0, T, t, e - nb);
  else {                                      // Accel() over the deltas
    const int n = e - nb - p.baselen;
    int B = 0;
    for (int th = 1; th <= p.accWin; th++) B += th * th;
    float sum = 0;
    for (int th = 1; th <= p.accWin; th++) {
      const float A1 = fe_delta(p, statics, emax, u, g0, T, t - th < 0 ? 0 : t - th, n);
      const float A2 = fe_delta(p, statics, emax, u, g0, T, t + th >= T ? T - 1 : t + th, n);
      sum += th * (A2 - A1);
    }
    v = sum / (2 * B);
  }
  feat[idx] = v;
}

// CMN() / MVN() statistics: float sums serial over t, one lane per (utterance, dimension)
__global__ void __launch_bounds__(64)
fe_stats_kernel(FeParams p, const float *__restrict__ feat, const int *__restrict__ foff, float *__restrict__ mean,
                float *__restrict__ sd) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= p.nutt * p.veclen) return;
  const int u = idx / p.veclen, d = idx % p.veclen;
  const int g0 = foff[u], T = foff[u + 1] - g0;
  const float *col = feat + (size_t)g0 * p.veclen + d;
  float s = 0.0f;
  if (!p.cvn) {                               // CMN(): sum / frame_num
    if (d >= p.basedim) return;
    for (int t = 0; t < T; t++) s += col[(size_t)t * p.veclen];
    mean[idx] = s / T;
    return;
  }
  for (int t = 0; t < T; t++) s += col[(size_t)t * p.veclen];   // MVN()
  s /= (float)T;
  mean[idx] = s;
  if (!p.cvar_static) {
    float q = 0.0f;
    for (int t = 0; t < T; t++) {
      const float x = col[(size_t)t * p.veclen] - s;
      q += x * x;
    }
    sd[idx] = (float)sqrt((double)(q / (float)T));
  }
}

// normalisation + splicing: out[t][i * veclen + d] = feat[t + i][d]
__global__ void __launch_bounds__(256)
fe_write_kernel(FeParams p, const float *__restrict__ feat, const int *__restrict__ foff, const int *__restrict__ ooff,
                const float *__restrict__ mean, const float *__restrict__ sd, int Tout, float *__restrict__ out) {
  const int VL = p.veclen * p.splice;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Tout * VL) return;
  const int o = (int)(idx / VL), c = (int)(idx % VL);
  const int u = jamd::find_span(ooff, p.nutt, o);
  const int i = c / p.veclen, d = c % p.veclen;
  const int g = foff[u] + (o - ooff[u]) + i;
  float v = feat[(size_t)g * p.veclen + d];
  const size_t sx = (size_t)u * p.veclen + d;
  if (p.cmn && !p.cvn) {                      // CMN()
    if (d < p.basedim) v -= p.cmean_static ? p.cmean[d] : mean[sx];
  } else if (p.cmn || p.cvn) {                // MVN()
    if (p.cmn && d < p.basedim) v -= p.cmean_static ? p.cmean[d] : mean[sx];
    if (p.cvn) {
      if (p.cvar_static) v = (float)(v / p.cvar_sqrt[d]);
      else v /= sd[sx];
    }
  }
  out[idx] = v;
}

}  // namespace

// ---------------------------------------------------------------------------------- launchers (frontend_host.h)
int fe_reserve_lds(jamd_frontend *f) {
  // four frames per workgroup; two where four would pass the CU's 160 KB (fftN 4096: windows of 2049 .. 4096 samples)
  const FeTables &w = f->tb;
  const size_t per_wave = sizeof(double) * ((size_t)w.fftN + (w.nv2 + 1) + (f->d.fbank_num + 1) + 2);
  f->fpb = per_wave * kFeFrames <= 160u * 1024u ? kFeFrames : per_wave * 2 <= 160u * 1024u ? 2 : 1;
  f->lds = per_wave * f->fpb;
  int rc;
  for (const void *k : {(const void *)fe_frame_kernel<false>, (const void *)fe_frame_kernel<true>, (const void *)fe_noise_frame})
    if ((rc = jamd_reserve_dyn_lds(k, f->lds, "jamd_frontend_create")) != JAMD_OK) return rc;
  return JAMD_OK;
}

int fe_launch_frames(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const long long *d_soff,
                     const int *d_foff, int nutt, int T) {
  FeParams p = f->p;
  p.nutt = nutt;
  const dim3 grid((T + f->fpb - 1) / f->fpb), block(64 * f->fpb);
  if (f->ss_mode == JAMD_SS_OFF) {
    hipLaunchKernelGGL(fe_frame_kernel<false>, grid, block, f->lds, st, p, dev_samples, d_soff, d_foff, T, f->d_stat,
                       (const float *)nullptr, 0, 0.0f, 0.0f);
  } else {
    // -sscalc: the spectrum of every utterance's head; -ssload: one spectrum for every utterance
    const bool calc = f->ss_mode == JAMD_SS_CALC;
    hipLaunchKernelGGL(fe_frame_kernel<true>, grid, block, f->lds, st, p, dev_samples, d_soff, d_foff, T, f->d_stat,
                       (const float *)(calc ? f->d_noise : f->d_ssload), calc ? f->tb.fftN : 0, f->ss_alpha, f->ss_floor);
  }
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int fe_launch_noise(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const long long *d_soff,
                    const int *d_hoff, int nutt, int Htot, float *dev_noise) {
  int rc;
  if ((rc = f->d_mag.grow((size_t)Htot * f->tb.fftN * sizeof(double))) != JAMD_OK) return rc;
  FeParams p = f->p;
  p.nutt = nutt;
  hipLaunchKernelGGL(fe_noise_frame, dim3((Htot + f->fpb - 1) / f->fpb), dim3(64 * f->fpb), f->lds, st, p, dev_samples,
                     d_soff, d_hoff, Htot, f->d_mag);
  JAMD_HIP(hipGetLastError());
  const long long nn = (long long)nutt * f->tb.fftN;
  hipLaunchKernelGGL(fe_noise_mean, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, f->tb.fftN, nutt, d_hoff,
                     f->d_mag, dev_noise);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int fe_launch_feats(jamd_frontend *f, hipStream_t st, const int *d_foff, const int *d_ooff, int nutt, int T,
                    long long Tout, float *dev_out) {
  const jamd_frontend_desc &d = f->d;
  FeParams p = f->p;
  p.nutt = nutt;
  float *d_mean = f->d_ms, *d_sd = d_mean + (size_t)nutt * d.veclen, *d_emax = d_sd + (size_t)nutt * d.veclen;
  if (p.enormal && p.energy) {
    hipLaunchKernelGGL(fe_emax_kernel, dim3(nutt), dim3(256), 0, st, p, f->d_stat, d_foff, d_emax);
    JAMD_HIP(hipGetLastError());
  }
  const long long nfeat = (long long)T * d.veclen;
  hipLaunchKernelGGL(fe_feat_kernel, dim3((unsigned)((nfeat + 255) / 256)), dim3(256), 0, st, p, f->d_stat, d_emax,
                     d_foff, T, f->d_feat);
  JAMD_HIP(hipGetLastError());
  const bool need_stats = (p.cmn && !p.cvn && !p.cmean_static) || (p.cvn && !(p.cmean_static && p.cvar_static));
  if (need_stats) {
    hipLaunchKernelGGL(fe_stats_kernel, dim3((nutt * d.veclen + 63) / 64), dim3(64), 0, st, p, f->d_feat, d_foff,
                       d_mean, d_sd);
    JAMD_HIP(hipGetLastError());
  }
  const long long nout = Tout * d.veclen * d.splice;
  hipLaunchKernelGGL(fe_write_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, p, f->d_feat, d_foff,
                     d_ooff, d_mean, d_sd, (int)Tout, dev_out);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

