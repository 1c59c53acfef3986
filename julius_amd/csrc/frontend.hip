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
#include "jamd_device.h"
#include "frontend_host.h"
#include "ss_file.h"
#include <cmath>
#include <cstdint>

// stddefs.h:97 / :109 (the reference's own constants, not M_PI)
#define FE_PI 3.14159265358979
#define FE_LOG_TEN 2.30258509

namespace {

// The tables WMP_work_new() / InitFBank() build (mfcc-core.c), computed with the same expressions.
struct FeTables {
  int fftN = 0, n = 0, klo = 0, khi = 0, nv2 = 0, maxChan = 0;
  float fres = 0.f, sqrt2var = 0.f;
  std::vector<float> cf, loWt;
  std::vector<short> loChan;
  std::vector<double> ham, fftcos, fftsin, dct, wcep, twRe, twIm;
  std::vector<int> kfirst, klast;      // [fbank_num + 1]: the k whose loChan is bin-1 or bin, ascending
};

float fe_mel(int k, float fres) { return (float)(1127 * log((double)(1 + (k - 1) * fres))); }   // Mel(), mfcc-core.c

// VTLN_recreate_fbank_cf() (mfcc-core.c)
bool fe_vtln(std::vector<float> &cf, const jamd_frontend_desc *p, float mlo, float mhi, int maxChan) {
  float minf = (float)(700.0 * (exp(mlo / 1127.0) - 1.0));
  float maxf = (float)(700.0 * (exp(mhi / 1127.0) - 1.0));
  if (p->vtln_upper > maxf) {
    jamd_set_error("frontend: VTLN upper cut-off greater than upper frequency bound: %.1f > %.1f", p->vtln_upper, maxf);
    return false;
  }
  if (p->vtln_lower < minf) {
    jamd_set_error("frontend: VTLN lower cut-off smaller than lower frequency bound: %.1f < %.1f", p->vtln_lower, minf);
    return false;
  }
  float scale = (float)(1.0 / p->vtln_alpha);
  float cu = p->vtln_upper * 2 / (1 + scale);
  float cl = p->vtln_lower * 2 / (1 + scale);
  float au = (maxf - cu * scale) / (maxf - cu);
  float al = (cl * scale - minf) / (cl - minf);
  for (int chan = 1; chan <= maxChan; chan++) {
    float cf_orig = (float)(700.0 * (exp(cf[chan] / 1127.0) - 1.0));
    float cf_new;
    if (cf_orig > cu) cf_new = au * (cf_orig - cu) + scale * cu;
    else if (cf_orig < cl) cf_new = al * (cf_orig - minf) + minf;
    else cf_new = scale * cf_orig;
    cf[chan] = (float)(1127.0 * log(1.0 + cf_new / 700.0));
  }
  return true;
}

bool fe_build_tables(const jamd_frontend_desc *p, FeTables &w) {
  if (p->framesize < 2 || p->framesize > 4096 || p->frameshift < 1 || p->fbank_num < 1 || p->smp_period <= 0) {
    jamd_set_error("frontend: framesize %d (2..4096), frameshift %d, fbank_num %d, smp_period %d out of range",
                   p->framesize, p->frameshift, p->fbank_num, p->smp_period);
    return false;
  }
  // InitFBank()
  w.fftN = 2; w.n = 1;
  while (p->framesize > w.fftN) { w.fftN *= 2; w.n++; }
  int nv2 = w.nv2 = w.fftN / 2;
  w.fres = (float)(1.0E7 / (p->smp_period * w.fftN * 700.0));
  int maxChan = w.maxChan = p->fbank_num + 1;
  w.klo = 2; w.khi = nv2;
  float mlo = 0, mhi = fe_mel(nv2 + 1, w.fres);
  if (p->lopass >= 0) {
    mlo = (float)(1127 * log(1 + (float)p->lopass / 700.0));
    w.klo = (int)(((float)p->lopass * p->smp_period * 1.0e-7 * w.fftN) + 2.5);
    if (w.klo < 2) w.klo = 2;
  }
  if (p->hipass >= 0) {
    mhi = (float)(1127 * log(1 + (float)p->hipass / 700.0));
    w.khi = (int)(((float)p->hipass * p->smp_period * 1.0e-7 * w.fftN) + 0.5);
    if (w.khi > nv2) w.khi = nv2;
  }
  w.cf.assign(maxChan + 1, 0.f);
  float ms = mhi - mlo;
  for (int chan = 1; chan <= maxChan; chan++) w.cf[chan] = ((float)chan / maxChan) * ms + mlo;
  if (p->vtln_alpha != 1.0f && !fe_vtln(w.cf, p, mlo, mhi, maxChan)) return false;
  w.loChan.assign(nv2 + 1, 0);
  for (int k = 1, chan = 1; k <= nv2; k++) {
    if (k < w.klo || k > w.khi) w.loChan[k] = -1;
    else {
      float melk = fe_mel(k, w.fres);
      while (chan <= maxChan && w.cf[chan] < melk) ++chan;   // (the reference tests cf[chan] first: same result)
      w.loChan[k] = (short)(chan - 1);
    }
  }
  w.loWt.assign(nv2 + 1, 0.f);
  for (int k = 1; k <= nv2; k++) {
    int chan = w.loChan[k];
    if (k < w.klo || k > w.khi) w.loWt[k] = 0.0f;
    else if (chan > 0) w.loWt[k] = (w.cf[chan + 1] - fe_mel(k, w.fres)) / (w.cf[chan + 1] - w.cf[chan]);
    else w.loWt[k] = (w.cf[1] - fe_mel(k, w.fres)) / (w.cf[1] - mlo);
  }
  w.sqrt2var = (float)sqrt(2.0 / p->fbank_num);
  // make_costbl_hamming(), make_fft_table(), make_costbl_makemfcc(), make_sintbl_wcep()
  w.ham.resize(p->framesize);
  float a = (float)(2.0 * FE_PI / (p->framesize - 1));
  for (int i = 1; i <= p->framesize; i++) w.ham[i - 1] = 0.54 - 0.46 * cos((double)(a * (i - 1)));
  w.fftcos.resize(w.n); w.fftsin.resize(w.n);
  for (int m = 1; m <= w.n; m++) {
    int me1 = (1 << m) / 2;
    w.fftcos[m - 1] = cos(FE_PI / me1);
    w.fftsin[m - 1] = -sin(FE_PI / me1);
  }
  if (p->mfcc_dim > 0) {
    w.dct.resize((size_t)p->fbank_num * p->mfcc_dim);
    float B = (float)(FE_PI / p->fbank_num);
    int k = 0;
    for (int i = 1; i <= p->mfcc_dim; i++) {
      float C = i * B;
      for (int j = 1; j <= p->fbank_num; j++) w.dct[k++] = cos(C * (j - 0.5));
    }
    w.wcep.resize(p->mfcc_dim);
    if (p->lifter > 0) {
      float la = (float)(FE_PI / p->lifter), lb = (float)(p->lifter / 2.0);
      for (int i = 0; i < p->mfcc_dim; i++) w.wcep[i] = 1.0 + lb * sin((double)((i + 1) * la));
    } else {
      for (int i = 0; i < p->mfcc_dim; i++) w.wcep[i] = 1.0;
    }
  }
  // The twiddle SEQUENCE of every FFT stage by the serial loop's own recurrence (u <- u * w,
  // mfcc-core.c FFT()): stage m's u_j lands at [me1 - 1 + j], so a butterfly reads the u the loop had.
  w.twRe.assign(w.fftN, 0.0); w.twIm.assign(w.fftN, 0.0);
  for (int m = 1; m <= w.n; m++) {
    int me1 = 1 << (m - 1);
    double uRe = 1.0, uIm = 0.0, wRe = w.fftcos[m - 1], wIm = w.fftsin[m - 1];
    for (int j = 0; j < me1; j++) {
      w.twRe[me1 - 1 + j] = uRe; w.twIm[me1 - 1 + j] = uIm;
      double vRe = uRe * wRe - uIm * wIm, vIm = uRe * wIm + uIm * wRe;
      uRe = vRe; uIm = vIm;
    }
  }
  // per-bin k ranges (loChan is non-decreasing over [klo, khi])
  w.kfirst.assign(p->fbank_num + 1, 1); w.klast.assign(p->fbank_num + 1, 0);
  for (int k = w.klo; k <= w.khi; k++) {
    int bin = w.loChan[k];
    if (bin > p->fbank_num) {   // the reference would write fbank[fbank_num + 1]
      jamd_set_error("frontend: FFT bin %d lies above the last filter-bank channel (lopass/hipass/VTLN)", k);
      return false;
    }
    for (int b = bin; b <= bin + 1; b++) {
      if (b < 1 || b > p->fbank_num) continue;
      if (w.klast[b] < w.kfirst[b]) w.kfirst[b] = k;
      w.klast[b] = k;
    }
  }
  return true;
}

// ---------------------------------------------------------------------------------- kernels
struct FeParams {
  int framesize, frameshift, fftN, logn, klo, khi, fbank_num, mfcc_dim, baselen, veclen, splice, nutt;
  int zmean, energy, raw_e, c0, fbank_only, log_fbank, usepower;
  int enormal, delta, acc, absesup, delWin, accWin, cmn, cvn, cmean_static, cvar_static, basedim;
  float preEmph, sqrt2var, escale, silFloor;
  const double *ham, *twRe, *twIm, *dct, *wcep, *cvar_sqrt;
  const short *loChan;
  const float *loWt, *cmean;
  const int *kfirst, *klast;
};

constexpr int kFeFrames = 4;   // frames (waves) per workgroup of the frame kernel

__device__ __forceinline__ int fe_find(const int *off, int n, int g) {   // u with off[u] <= g < off[u+1]
  int lo = 0, hi = n;
  while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}

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
  const int u = fe_find(foff, p.nutt, gg);
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
  const int u = fe_find(hoff, p.nutt, gg);
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
    const float min = (float)(max - (p.silFloor * FE_LOG_TEN) / 10.0);
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
  const int u = fe_find(foff, p.nutt, g);
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
  const int u = fe_find(ooff, p.nutt, o);
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

struct jamd_frontend {
  jamd_engine *eng = nullptr;
  jamd_frontend_desc d{};
  FeTables tb;
  FeParams p{};
  size_t lds = 0;
  int fpb = kFeFrames;                       // frames (waves) per workgroup of the frame kernel
  std::vector<void *> owned;                 // device tables
  float *d_stat = nullptr; size_t stat_cap = 0;
  float *d_feat = nullptr; size_t feat_cap = 0;
  float *d_ms = nullptr; size_t ms_cap = 0;  // mean[nutt][veclen] | sd[nutt][veclen] | emax[nutt]
  char *d_off = nullptr; size_t off_cap = 0; // soff (int64) | foff | ooff (int32)
  char *h_off = nullptr; size_t h_off_cap = 0; hipEvent_t ev_off = nullptr;
  int16_t *d_in = nullptr; size_t in_cap = 0;   // run_host staging
  float *d_out = nullptr; size_t out_cap = 0;
  // spectral subtraction (jamd_frontend_set_ss)
  int ss_mode = JAMD_SS_OFF;
  long long ss_head = 0;                     // -sscalclen in samples
  float ss_alpha = 0.f, ss_floor = 0.f;
  float *d_ssload = nullptr;                 // -ssload: the one spectrum [fftN]
  float *d_noise = nullptr; size_t noise_cap = 0;   // -sscalc: [nutt][fftN]; noise_host staging
  double *d_mag = nullptr; size_t mag_cap = 0;      // |X| of the head frames [head frames][fftN]
};

template <typename T>
static int fe_reserve(T **ptr, size_t *cap, size_t n) {
  if (n <= *cap) return JAMD_OK;
  if (*ptr) JAMD_HIP(hipFree(*ptr));
  *ptr = nullptr; *cap = 0;
  JAMD_HIP(hipMalloc((void **)ptr, n * sizeof(T)));
  *cap = n;
  return JAMD_OK;
}

extern "C" {

int jamd_frontend_set_kind(jamd_frontend_desc *d, int param_type, int vec_size) {
  if (!d) { jamd_set_error("jamd_frontend_set_kind: d is NULL"); return JAMD_EINVAL; }
  // calc_para_from_header() (para.c:323-372)
  d->paramtype = param_type; d->vecsize = vec_size;
  d->basetype = param_type & 0x003f;
  d->delta = (param_type & JAMD_F_D) ? 1 : 0;
  d->acc = (param_type & JAMD_F_A) ? 1 : 0;
  d->energy = (param_type & JAMD_F_E) ? 1 : 0;
  d->c0 = (param_type & JAMD_F_0) ? 1 : 0;
  d->absesup = (param_type & JAMD_F_N) ? 1 : 0;
  d->cmn = (param_type & JAMD_F_Z) ? 1 : 0;
  int dim = vec_size;
  if (d->absesup) dim++;
  dim /= 1 + (d->delta ? 1 : 0) + (d->acc ? 1 : 0);
  if (d->energy) dim--;
  if (d->c0) dim--;
  d->mfcc_dim = dim;
  d->baselen = d->mfcc_dim + (d->c0 ? 1 : 0) + (d->energy ? 1 : 0);
  d->vecbuflen = d->baselen * (1 + (d->delta ? 1 : 0) + (d->acc ? 1 : 0));
  d->veclen = d->vecbuflen - (d->absesup ? 1 : 0);
  if (d->basetype == JAMD_F_FBANK || d->basetype == JAMD_F_MELSPEC) d->fbank_num = dim;
  return JAMD_OK;
}

int jamd_frontend_default_desc(int param_type, int vec_size, jamd_frontend_desc *d) {
  if (!d) { jamd_set_error("jamd_frontend_default_desc: d is NULL"); return JAMD_EINVAL; }
  memset(d, 0, sizeof(*d));
  // make_default_para() (para.c:86-107; DEF_* of mfcc.h:56-66)
  d->smp_period = 625; d->smp_freq = 16000;
  d->framesize = 400; d->frameshift = 160;
  d->preEmph = 0.97f;
  d->fbank_num = 24; d->lifter = 22; d->delWin = 2; d->accWin = 2;
  d->raw_e = 0; d->enormal = 0; d->escale = 1.0f; d->silFloor = 50.0f;
  d->cvn = 0; d->hipass = -1; d->lopass = -1;
  d->vtln_alpha = 1.0f; d->vtln_upper = 0.0f; d->vtln_lower = 0.0f;
  d->zmeanframe = 0; d->usepower = 0;
  d->splice = 1;
  return jamd_frontend_set_kind(d, param_type, vec_size);
}

int jamd_frontend_htkconf(const char *path, jamd_frontend_desc *para) {
  if (!path || !para) { jamd_set_error("jamd_frontend_htkconf: NULL argument"); return JAMD_EINVAL; }
  FILE *fp = fopen(path, "r");
  if (!fp) { jamd_set_error("jamd_frontend_htkconf: failed to open HTK Config file: %s", path); return JAMD_EINVAL; }
  // htk_config_file_parse() (para.c:196-321): the same tokenising, the same conversions
  jamd_frontend_desc p = *para;
  char buf[512];
  float srate = 0.0f;
  auto istok = [](char c) { return c == ' ' || c == '\t' || c == '\n'; };
  while (fgets(buf, sizeof buf, fp)) {
    int nl = (int)strlen(buf) - 1;           // getl_fp(): chop \n and \r, skip blank lines
    if (nl >= 0 && buf[nl] == '\n') { buf[nl] = '\0'; nl--; }
    if (nl >= 0 && buf[nl] == '\r') buf[nl] = '\0';
    if (buf[0] == '\0') continue;
    char *s = buf;
    if (*s == '#') continue;
    while (*s != '\0' && istok(*s)) s++;
    if (*s == '\0') continue;
    char *k = s;
    while (*s != '\0' && !istok(*s) && *s != '=') s++;
    if (*s == '\0') continue;
    *s = '\0'; s++;
    while (*s != '\0' && (istok(*s) || *s == '=')) s++;
    if (*s == '\0') continue;
    char *a = s;
    while (*s != '\0' && !istok(*s)) s++;
    *s = '\0';
    if (!strcmp(k, "SOURCERATE")) srate = (float)atof(a);
    else if (!strcmp(k, "TARGETRATE")) p.frameshift = (int)atof(a);
    else if (!strcmp(k, "WINDOWSIZE")) p.framesize = (int)atof(a);
    else if (!strcmp(k, "ZMEANSOURCE")) p.zmeanframe = a[0] == 'T';
    else if (!strcmp(k, "USEPOWER")) p.usepower = a[0] == 'T';
    else if (!strcmp(k, "PREEMCOEF")) p.preEmph = (float)atof(a);
    else if (!strcmp(k, "USEHAMMING")) {
      if (a[0] != 'T') {
        fclose(fp);
        jamd_set_error("jamd_frontend_htkconf: %s: USEHAMMING should be T", path);
        return JAMD_EINVAL;
      }
    } else if (!strcmp(k, "NUMCHANS")) p.fbank_num = atoi(a);
    else if (!strcmp(k, "CEPLIFTER")) p.lifter = atoi(a);
    else if (!strcmp(k, "DELTAWINDOW")) p.delWin = atoi(a);
    else if (!strcmp(k, "ACCWINDOW")) p.accWin = atoi(a);
    else if (!strcmp(k, "LOFREQ")) p.lopass = (int)atof(a);
    else if (!strcmp(k, "HIFREQ")) p.hipass = (int)atof(a);
    else if (!strcmp(k, "RAWENERGY")) p.raw_e = a[0] == 'T';
    else if (!strcmp(k, "ENORMALISE")) p.enormal = a[0] == 'T';
    else if (!strcmp(k, "ESCALE")) p.escale = (float)atof(a);
    else if (!strcmp(k, "SILFLOOR")) p.silFloor = (float)atof(a);
    else if (!strcmp(k, "WARPFREQ")) p.vtln_alpha = (float)atof(a);
    else if (!strcmp(k, "WARPLCUTOFF")) p.vtln_lower = (float)atof(a);
    else if (!strcmp(k, "WARPUCUTOFF")) p.vtln_upper = (float)atof(a);
    else if (!strcmp(k, "TARGETKIND") || !strcmp(k, "NUMCEPS")) { /* determined by the AM header */ }
    else {
      fclose(fp);
      jamd_set_error("jamd_frontend_htkconf: %s: key \"%s\" is not one the reference takes", path, k);
      return JAMD_EINVAL;
    }
  }
  fclose(fp);
  if (srate == 0.0f) srate = 625;
  p.smp_period = (int)srate;
  p.smp_freq = (int)(10000000.0 / (float)p.smp_period);   // period2freq(), speech.h:106
  p.frameshift = (int)(p.frameshift / srate);
  p.framesize = (int)(p.framesize / srate);
  *para = p;
  return JAMD_OK;
}

int jamd_frontend_table(const jamd_frontend_desc *d, const char *name, void *out, int cap) {
  if (!d || !name) { jamd_set_error("jamd_frontend_table: NULL argument"); return JAMD_EINVAL; }
  FeTables w;
  if (!fe_build_tables(d, w)) return JAMD_EINVAL;
  auto put = [&](const auto &v) {
    size_t n = v.size() < (size_t)(cap > 0 ? cap : 0) ? v.size() : (size_t)(cap > 0 ? cap : 0);
    if (out && n) memcpy(out, v.data(), n * sizeof(v[0]));
    return (int)v.size();
  };
  const std::string s(name);
  if (s == "hamming") return put(w.ham);
  if (s == "fft_cos") return put(w.fftcos);
  if (s == "fft_sin") return put(w.fftsin);
  if (s == "dct") return put(w.dct);
  if (s == "wcep") return put(w.wcep);
  if (s == "twiddle_re") return put(std::vector<double>(w.twRe.begin(), w.twRe.begin() + w.fftN - 1));
  if (s == "twiddle_im") return put(std::vector<double>(w.twIm.begin(), w.twIm.begin() + w.fftN - 1));
  if (s == "cf") return put(w.cf);
  if (s == "lowt") return put(w.loWt);
  if (s == "lochan") return put(w.loChan);
  if (s == "info") return put(std::vector<int>{w.fftN, w.n, w.klo, w.khi});
  if (s == "scalars") return put(std::vector<float>{w.fres, w.sqrt2var});
  jamd_set_error("jamd_frontend_table: unknown table \"%s\"", name);
  return JAMD_EINVAL;
}

void jamd_frontend_destroy(jamd_frontend *f) {
  if (!f) return;
  for (void *q : f->owned) (void)hipFree(q);
  if (f->d_stat) (void)hipFree(f->d_stat);
  if (f->d_feat) (void)hipFree(f->d_feat);
  if (f->d_ms) (void)hipFree(f->d_ms);
  if (f->d_off) (void)hipFree(f->d_off);
  if (f->d_in) (void)hipFree(f->d_in);
  if (f->d_out) (void)hipFree(f->d_out);
  if (f->d_ssload) (void)hipFree(f->d_ssload);
  if (f->d_noise) (void)hipFree(f->d_noise);
  if (f->d_mag) (void)hipFree(f->d_mag);
  if (f->ev_off) { (void)hipEventSynchronize(f->ev_off); (void)hipEventDestroy(f->ev_off); }
  if (f->h_off) (void)hipHostFree(f->h_off);
  delete f;
}

static int fe_upload(jamd_frontend *f, const void *src, size_t bytes, void **dst) {
  *dst = nullptr;
  if (!bytes) return JAMD_OK;
  JAMD_HIP(hipMalloc(dst, bytes));
  f->owned.push_back(*dst);
  JAMD_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return JAMD_OK;
}

int jamd_frontend_create(jamd_engine *e, const jamd_frontend_desc *d, jamd_frontend **out) {
  if (!e || !d || !out) { jamd_set_error("jamd_frontend_create: NULL argument"); return JAMD_EINVAL; }
  *out = nullptr;
  if (d->ss) {
    jamd_set_error("jamd_frontend_create: ss != 0 in the descriptor, which carries none of the parameters of spectral "
                   "subtraction: leave it 0 and call jamd_frontend_set_ss() on the created object");
    return JAMD_EINVAL;
  }
  if (d->realtime) { jamd_set_error("jamd_frontend_create: realtime input / MAP-CMN is not served (buffered front end only)"); return JAMD_EINVAL; }
  if (d->basetype != JAMD_F_MFCC && d->basetype != JAMD_F_FBANK && d->basetype != JAMD_F_MELSPEC) {
    jamd_set_error("jamd_frontend_create: parameter kind %d is not MFCC, FBANK or MELSPEC", d->basetype);
    return JAMD_EINVAL;
  }
  if (d->basetype != JAMD_F_MFCC && (d->energy || d->c0)) {
    jamd_set_error("jamd_frontend_create: _E / _0 with a filter-bank kind (the reference leaves those slots unset)");
    return JAMD_EINVAL;
  }
  if ((d->absesup && !(d->energy && d->delta)) || (d->acc && !d->delta)) {
    jamd_set_error("jamd_frontend_create: _N needs _E and _D, _A needs _D");
    return JAMD_EINVAL;
  }
  if (d->mfcc_dim < 1 || d->veclen < 1 || d->splice < 1 || d->delWin < 1 || (d->acc && d->accWin < 1)) {
    jamd_set_error("jamd_frontend_create: kind 0x%x with vector size %d gives %d cepstra (splice %d, windows %d/%d)",
                   d->paramtype, d->vecsize, d->mfcc_dim, d->splice, d->delWin, d->accWin);
    return JAMD_EINVAL;
  }
  if (d->cvn && d->cmean_init && !d->cvar_init) {
    jamd_set_error("jamd_frontend_create: static CVN needs cvar_init");
    return JAMD_EINVAL;
  }
  jamd_frontend *f = new jamd_frontend();
  f->eng = e;
  f->d = *d;
  f->d.cmean_init = nullptr; f->d.cvar_init = nullptr;
  if (!fe_build_tables(d, f->tb)) { delete f; return JAMD_EINVAL; }
  JAMD_HIP(hipSetDevice(e->device));
  FeParams &p = f->p;
  const FeTables &w = f->tb;
  p.framesize = d->framesize; p.frameshift = d->frameshift; p.fftN = w.fftN; p.logn = w.n;
  p.klo = w.klo; p.khi = w.khi; p.fbank_num = d->fbank_num; p.mfcc_dim = d->mfcc_dim; p.baselen = d->baselen;
  p.veclen = d->veclen; p.splice = d->splice;
  p.zmean = d->zmeanframe != 0; p.energy = d->energy != 0; p.raw_e = d->raw_e != 0; p.c0 = d->c0 != 0;
  p.fbank_only = d->basetype != JAMD_F_MFCC; p.log_fbank = d->basetype != JAMD_F_MELSPEC; p.usepower = d->usepower != 0;
  p.enormal = d->enormal != 0; p.delta = d->delta; p.acc = d->acc; p.absesup = d->absesup;
  p.delWin = d->delWin; p.accWin = d->accWin; p.cmn = d->cmn != 0; p.cvn = d->cvn != 0;
  p.basedim = d->mfcc_dim + (d->c0 ? 1 : 0);
  p.preEmph = d->preEmph; p.sqrt2var = w.sqrt2var; p.escale = d->escale; p.silFloor = d->silFloor;
  // CMN() takes cmean_init whenever it is set; MVN() does unless static_cvn_only, which keeps only the variance
  p.cmean_static = d->cmean_init && (!p.cvn || !d->static_cvn_only);
  p.cvar_static = p.cvn && d->cmean_init != nullptr;
  int rc;
  void *q;
#define FE_UP(field, vec, T)                                                           \
  if ((rc = fe_upload(f, (vec).data(), (vec).size() * sizeof(T), &q)) != JAMD_OK) { \
    jamd_frontend_destroy(f); return rc;                                              \
  }                                                                                   \
  p.field = (const T *)q;
  FE_UP(ham, w.ham, double)
  FE_UP(twRe, w.twRe, double)
  FE_UP(twIm, w.twIm, double)
  FE_UP(dct, w.dct, double)
  FE_UP(wcep, w.wcep, double)
  FE_UP(loChan, w.loChan, short)
  FE_UP(loWt, w.loWt, float)
  FE_UP(kfirst, w.kfirst, int)
  FE_UP(klast, w.klast, int)
  if (p.cmean_static) {
    std::vector<float> cm(d->cmean_init, d->cmean_init + p.basedim);
    FE_UP(cmean, cm, float)
  }
  if (p.cvar_static) {
    std::vector<double> cs(d->veclen);
    for (int i = 0; i < d->veclen; i++) cs[i] = sqrt(d->cvar_init[i]);   // sqrt(c->cvar_init[i]) in double
    FE_UP(cvar_sqrt, cs, double)
  }
#undef FE_UP
  // four frames per workgroup; two where four would pass the CU's 160 KB (fftN 4096: windows of 2049 .. 4096 samples)
  const size_t per_wave = sizeof(double) * ((size_t)w.fftN + (w.nv2 + 1) + (d->fbank_num + 1) + 2);
  f->fpb = per_wave * kFeFrames <= 160u * 1024u ? kFeFrames : per_wave * 2 <= 160u * 1024u ? 2 : 1;
  f->lds = per_wave * f->fpb;
  for (const void *k : {(const void *)fe_frame_kernel<false>, (const void *)fe_frame_kernel<true>, (const void *)fe_noise_frame})
    if ((rc = jamd_reserve_dyn_lds(k, f->lds, "jamd_frontend_create")) != JAMD_OK) {
      jamd_frontend_destroy(f);
      return rc;
    }
  *out = f;
  return JAMD_OK;
}

int jamd_frontend_veclen(const jamd_frontend *f) { return f ? f->d.veclen * f->d.splice : JAMD_EINVAL; }

static long long fe_frames_raw(const jamd_frontend_desc &d, int64_t n) {
  if (n < d.framesize) return 0;
  return (n - d.framesize) / d.frameshift + 1;
}

int jamd_frontend_frames(const jamd_frontend_desc *d, int64_t nsamples) {
  if (!d || d->framesize < 1 || d->frameshift < 1 || d->splice < 1) {
    jamd_set_error("jamd_frontend_frames: NULL descriptor, or framesize / frameshift / splice < 1");
    return JAMD_EINVAL;
  }
  long long T = fe_frames_raw(*d, nsamples) - (d->splice - 1);
  return T > 0x7fffffff ? 0x7fffffff : (int)T;
}

int jamd_frontend_fftn(const jamd_frontend *f) { return f ? f->tb.fftN : JAMD_EINVAL; }

int jamd_frontend_ss_default(jamd_frontend_ss *ss) {
  if (!ss) { jamd_set_error("jamd_frontend_ss_default: ss is NULL"); return JAMD_EINVAL; }
  // default.c:158-162 with DEF_SSALPHA / DEF_SSFLOOR of mfcc.h:68-69
  ss->mode = JAMD_SS_OFF; ss->calc_len_ms = 300;
  ss->alpha = 2.0f; ss->floor = 0.5f;
  ss->noise = nullptr; ss->noise_len = 0;
  return JAMD_OK;
}

int jamd_frontend_set_ss(jamd_frontend *f, const jamd_frontend_ss *ss) {
  if (!f || !ss) { jamd_set_error("jamd_frontend_set_ss: NULL argument"); return JAMD_EINVAL; }
  long long head = 0;
  if (ss->mode == JAMD_SS_CALC) {
    // m_fusion.c:1409: the head must hold a frame (the reference's product is an int; one past int is refused here)
    head = (long long)ss->calc_len_ms * f->d.smp_freq / 1000;
    if (head < f->d.framesize || (long long)ss->calc_len_ms * f->d.smp_freq > 0x7fffffffLL) {
      jamd_set_error("jamd_frontend_set_ss: head length for SS (%d msec = %lld samples) is shorter than a frame (%d "
                     "samples), or out of range", ss->calc_len_ms, head, f->d.framesize);
      return JAMD_EINVAL;
    }
  } else if (ss->mode == JAMD_SS_LOAD) {
    if (!ss->noise || ss->noise_len != f->tb.fftN) {   // Wav2MFCC() refuses ssbuflen != fftN (wav2mfcc-buffer.c:64-69)
      jamd_set_error("jamd_frontend_set_ss: JAMD_SS_LOAD needs a noise spectrum of fftN = %d values (got %s, length %d)",
                     f->tb.fftN, ss->noise ? "one" : "NULL", ss->noise_len);
      return JAMD_EINVAL;
    }
    JAMD_HIP(hipSetDevice(f->eng->device));
    // a buffer of its own per upload: a run queued earlier keeps reading the spectrum it was launched with
    float *q = nullptr;
    JAMD_HIP(hipMalloc((void **)&q, sizeof(float) * f->tb.fftN));
    hipError_t e = hipMemcpy(q, ss->noise, sizeof(float) * f->tb.fftN, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(q);
      jamd_set_error("jamd_frontend_set_ss: hipMemcpy failed: %s", hipGetErrorString(e));
      return JAMD_ENODEV;
    }
    if (f->d_ssload) (void)hipFree(f->d_ssload);   // (hipFree waits for the device)
    f->d_ssload = q;
  } else if (ss->mode != JAMD_SS_OFF) {
    jamd_set_error("jamd_frontend_set_ss: unknown mode %d (JAMD_SS_OFF, JAMD_SS_CALC, JAMD_SS_LOAD)", ss->mode);
    return JAMD_EINVAL;
  }
  f->ss_mode = ss->mode; f->ss_head = head;
  f->ss_alpha = ss->alpha; f->ss_floor = ss->floor;
  return JAMD_OK;
}

int jamd_frontend_ss_read(const char *path, float *out, int cap) {
  if (!path || (cap > 0 && !out)) { jamd_set_error("jamd_frontend_ss_read: NULL argument"); return JAMD_EINVAL; }
  std::string err;
  const int n = ssf_read(path, out, cap > 0 ? cap : 0, err);
  if (n < 0) { jamd_set_error("jamd_frontend_ss_read: %s", err.c_str()); return JAMD_EINVAL; }
  return n;
}

int jamd_frontend_ss_write(const char *path, const float *noise, int n) {
  if (!path || !noise || n < 0) { jamd_set_error("jamd_frontend_ss_write: NULL argument or n < 0"); return JAMD_EINVAL; }
  std::string err;
  if (ssf_write(path, noise, n, err) != 0) { jamd_set_error("jamd_frontend_ss_write: %s", err.c_str()); return JAMD_EINVAL; }
  return JAMD_OK;
}

// The offsets go up through a pinned buffer that is rewritten only once the copy that read it is done.
// blob = soff (int64 [nutt + 1]) followed by ntab int32 tables [nutt + 1].
static int fe_put_offsets(jamd_frontend *f, hipStream_t st, const int64_t *sample_off, int nutt,
                          const std::vector<const std::vector<int> *> &tabs) {
  const size_t offb = sizeof(long long) * (nutt + 1) + tabs.size() * sizeof(int) * (nutt + 1);
  int rc;
  if ((rc = fe_reserve(&f->d_off, &f->off_cap, offb)) != JAMD_OK) return rc;
  if (f->ev_off) JAMD_HIP(hipEventSynchronize(f->ev_off));
  else JAMD_HIP(hipEventCreateWithFlags(&f->ev_off, hipEventDisableTiming));
  if (f->h_off_cap < offb) {
    if (f->h_off) JAMD_HIP(hipHostFree(f->h_off));
    f->h_off = nullptr; f->h_off_cap = 0;
    JAMD_HIP(hipHostMalloc((void **)&f->h_off, offb, hipHostMallocDefault));
    f->h_off_cap = offb;
  }
  memcpy(f->h_off, sample_off, sizeof(long long) * (nutt + 1));
  char *q = f->h_off + sizeof(long long) * (nutt + 1);
  for (const std::vector<int> *t : tabs) { memcpy(q, t->data(), sizeof(int) * (nutt + 1)); q += sizeof(int) * (nutt + 1); }
  JAMD_HIP(hipMemcpyAsync(f->d_off, f->h_off, offb, hipMemcpyHostToDevice, st));
  JAMD_HIP(hipEventRecord(f->ev_off, st));
  return JAMD_OK;
}

// Head frames of every utterance (head_samples <= 0: the whole utterance) -> hoff [nutt + 1]; false with the error
// set when sample_off is not in order or a head holds no full frame.
static bool fe_head_frames(const jamd_frontend *f, const char *who, const int64_t *sample_off, int nutt,
                           long long head_samples, std::vector<int> &hoff) {
  hoff.assign(nutt + 1, 0);
  long long Hall = 0;
  for (int u = 0; u < nutt; u++) {
    if (sample_off[u] < 0 || sample_off[u + 1] < sample_off[u]) {
      jamd_set_error("%s: sample_off is not non-decreasing from 0 at utterance %d", who, u);
      return false;
    }
    long long n = sample_off[u + 1] - sample_off[u];
    if (head_samples > 0 && head_samples < n) n = head_samples;
    const long long H = fe_frames_raw(f->d, n);
    if (H < 1) {
      jamd_set_error("%s: the head of utterance %d (%lld samples) holds no full frame", who, u, n);
      return false;
    }
    hoff[u] = (int)Hall;
    Hall += H;
    if (Hall > 0x7fffffffLL) { jamd_set_error("%s: batch too large (%lld head frames)", who, Hall); return false; }
  }
  hoff[nutt] = (int)Hall;
  return true;
}

// fe_noise_frame + fe_noise_mean over the head frames d_hoff describes -> dev_noise [nutt][fftN]
static int fe_noise_launch(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const long long *d_soff,
                           const int *d_hoff, int nutt, int Htot, float *dev_noise) {
  int rc;
  if ((rc = fe_reserve(&f->d_mag, &f->mag_cap, (size_t)Htot * f->tb.fftN)) != JAMD_OK) return rc;
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

int jamd_frontend_noise_dev(jamd_frontend *f, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                            int64_t head_samples, float *dev_noise, void *stream) {
  if (!f || !dev_samples || !sample_off || !dev_noise || nutt < 1) {
    jamd_set_error("jamd_frontend_noise_dev: NULL argument or nutt < 1");
    return JAMD_EINVAL;
  }
  if ((long long)nutt * f->tb.fftN > 0x7fffffffLL) { jamd_set_error("jamd_frontend_noise_dev: batch too large"); return JAMD_EINVAL; }
  std::vector<int> hoff;
  if (!fe_head_frames(f, "jamd_frontend_noise_dev", sample_off, nutt, head_samples, hoff)) return JAMD_EINVAL;
  JAMD_HIP(hipSetDevice(f->eng->device));
  hipStream_t st = jamd_stream(f->eng, stream);
  int rc;
  if ((rc = fe_put_offsets(f, st, sample_off, nutt, {&hoff})) != JAMD_OK) return rc;
  const long long *d_soff = (const long long *)f->d_off;
  return fe_noise_launch(f, st, dev_samples, d_soff, (const int *)(d_soff + nutt + 1), nutt, hoff[nutt], dev_noise);
}

int jamd_frontend_noise_host(jamd_frontend *f, const int16_t *samples, const int64_t *sample_off, int nutt,
                             int64_t head_samples, float *noise) {
  if (!f || !samples || !sample_off || !noise || nutt < 1) {
    jamd_set_error("jamd_frontend_noise_host: NULL argument or nutt < 1");
    return JAMD_EINVAL;
  }
  if ((long long)nutt * f->tb.fftN > 0x7fffffffLL) { jamd_set_error("jamd_frontend_noise_host: batch too large"); return JAMD_EINVAL; }
  std::vector<int> hoff;
  if (!fe_head_frames(f, "jamd_frontend_noise_host", sample_off, nutt, head_samples, hoff)) return JAMD_EINVAL;
  JAMD_HIP(hipSetDevice(f->eng->device));
  int rc;
  const size_t ns = (size_t)sample_off[nutt], nn = (size_t)nutt * f->tb.fftN;
  if ((rc = fe_reserve(&f->d_in, &f->in_cap, ns > 0 ? ns : 1)) != JAMD_OK) return rc;
  if ((rc = fe_reserve(&f->d_noise, &f->noise_cap, nn)) != JAMD_OK) return rc;
  hipStream_t st = f->eng->stream;
  JAMD_HIP(hipMemcpyAsync(f->d_in, samples, ns * sizeof(int16_t), hipMemcpyHostToDevice, st));
  if ((rc = jamd_frontend_noise_dev(f, f->d_in, sample_off, nutt, head_samples, f->d_noise, st)) != JAMD_OK) return rc;
  JAMD_HIP(hipMemcpyAsync(noise, f->d_noise, nn * sizeof(float), hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  return JAMD_OK;
}

int jamd_frontend_run_dev(jamd_frontend *f, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                          float *dev_out, int *frame_off, void *stream) {
  if (!f || !dev_samples || !sample_off || !dev_out || nutt < 1) {
    jamd_set_error("jamd_frontend_run_dev: NULL argument or nutt < 1");
    return JAMD_EINVAL;
  }
  const jamd_frontend_desc &d = f->d;
  std::vector<int> foff(nutt + 1), ooff(nutt + 1);
  long long Tall = 0, Tout = 0;
  for (int u = 0; u < nutt; u++) {
    if (sample_off[u] < 0 || sample_off[u + 1] < sample_off[u]) {
      jamd_set_error("jamd_frontend_run_dev: sample_off is not non-decreasing from 0 at utterance %d", u);
      return JAMD_EINVAL;
    }
    long long T = fe_frames_raw(d, sample_off[u + 1] - sample_off[u]);
    if (T - (d.splice - 1) < 1) {
      jamd_set_error("jamd_frontend_run_dev: utterance %d too short (%lld samples)", u,
                     (long long)(sample_off[u + 1] - sample_off[u]));
      return JAMD_EINVAL;
    }
    foff[u] = (int)Tall; ooff[u] = (int)Tout;
    Tall += T; Tout += T - (d.splice - 1);
    if ((Tall + 1) * (long long)d.vecbuflen * d.splice > 0x7fffffffLL) {
      jamd_set_error("jamd_frontend_run_dev: batch too large (%lld frames)", Tall);
      return JAMD_EINVAL;
    }
  }
  foff[nutt] = (int)Tall; ooff[nutt] = (int)Tout;
  std::vector<int> hoff;                     // -sscalc: the head frames (every utterance holds a frame, so its head does)
  if (f->ss_mode == JAMD_SS_CALC) {
    if ((long long)nutt * f->tb.fftN > 0x7fffffffLL) { jamd_set_error("jamd_frontend_run_dev: batch too large"); return JAMD_EINVAL; }
    if (!fe_head_frames(f, "jamd_frontend_run_dev", sample_off, nutt, f->ss_head, hoff)) return JAMD_EINVAL;
  }
  JAMD_HIP(hipSetDevice(f->eng->device));
  hipStream_t st = jamd_stream(f->eng, stream);
  int rc;
  if ((rc = fe_reserve(&f->d_stat, &f->stat_cap, (size_t)Tall * d.baselen)) != JAMD_OK) return rc;
  if ((rc = fe_reserve(&f->d_feat, &f->feat_cap, (size_t)Tall * d.veclen)) != JAMD_OK) return rc;
  if ((rc = fe_reserve(&f->d_ms, &f->ms_cap, (size_t)nutt * (2 * d.veclen + 1))) != JAMD_OK) return rc;
  if (f->ss_mode == JAMD_SS_CALC) rc = fe_put_offsets(f, st, sample_off, nutt, {&foff, &ooff, &hoff});
  else rc = fe_put_offsets(f, st, sample_off, nutt, {&foff, &ooff});
  if (rc != JAMD_OK) return rc;
  const long long *d_soff = (const long long *)f->d_off;
  const int *d_foff = (const int *)(d_soff + nutt + 1), *d_ooff = d_foff + nutt + 1;
  float *d_mean = f->d_ms, *d_sd = d_mean + (size_t)nutt * d.veclen, *d_emax = d_sd + (size_t)nutt * d.veclen;

  FeParams p = f->p;
  p.nutt = nutt;
  const int T = (int)Tall, w_fftN = f->tb.fftN;
  if (f->ss_mode == JAMD_SS_OFF) {
    hipLaunchKernelGGL(fe_frame_kernel<false>, dim3((T + f->fpb - 1) / f->fpb), dim3(64 * f->fpb), f->lds, st, p,
                       dev_samples, d_soff, d_foff, T, f->d_stat, (const float *)nullptr, 0, 0.0f, 0.0f);
  } else {
    const float *d_noise = f->d_ssload;      // -ssload: one spectrum for every utterance
    if (f->ss_mode == JAMD_SS_CALC) {        // -sscalc: the spectrum of every utterance's head first, on this stream
      if ((rc = fe_reserve(&f->d_noise, &f->noise_cap, (size_t)nutt * w_fftN)) != JAMD_OK) return rc;
      if ((rc = fe_noise_launch(f, st, dev_samples, d_soff, d_ooff + nutt + 1, nutt, hoff[nutt], f->d_noise)) != JAMD_OK)
        return rc;
      d_noise = f->d_noise;
    }
    hipLaunchKernelGGL(fe_frame_kernel<true>, dim3((T + f->fpb - 1) / f->fpb), dim3(64 * f->fpb), f->lds, st, p,
                       dev_samples, d_soff, d_foff, T, f->d_stat, d_noise, f->ss_mode == JAMD_SS_CALC ? w_fftN : 0,
                       f->ss_alpha, f->ss_floor);
  }
  JAMD_HIP(hipGetLastError());
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
  if (frame_off) memcpy(frame_off, ooff.data(), sizeof(int) * (nutt + 1));
  return JAMD_OK;
}

int jamd_frontend_run_host(jamd_frontend *f, const int16_t *samples, const int64_t *sample_off, int nutt, float *out,
                           int *frame_off) {
  if (!f || !samples || !sample_off || !out || nutt < 1) {
    jamd_set_error("jamd_frontend_run_host: NULL argument or nutt < 1");
    return JAMD_EINVAL;
  }
  long long Tout = 0;
  for (int u = 0; u < nutt; u++) {
    if (sample_off[u] < 0 || sample_off[u + 1] < sample_off[u]) {
      jamd_set_error("jamd_frontend_run_host: sample_off is not non-decreasing from 0 at utterance %d", u);
      return JAMD_EINVAL;
    }
    const int T = jamd_frontend_frames(&f->d, sample_off[u + 1] - sample_off[u]);
    if (T < 1) {
      jamd_set_error("jamd_frontend_run_host: utterance %d too short (%lld samples)", u,
                     (long long)(sample_off[u + 1] - sample_off[u]));
      return JAMD_EINVAL;
    }
    Tout += T;
  }
  JAMD_HIP(hipSetDevice(f->eng->device));
  int rc;
  const size_t ns = (size_t)sample_off[nutt], no = (size_t)Tout * f->d.veclen * f->d.splice;
  if ((rc = fe_reserve(&f->d_in, &f->in_cap, ns > 0 ? ns : 1)) != JAMD_OK) return rc;
  if ((rc = fe_reserve(&f->d_out, &f->out_cap, no)) != JAMD_OK) return rc;
  hipStream_t st = f->eng->stream;
  JAMD_HIP(hipMemcpyAsync(f->d_in, samples, ns * sizeof(int16_t), hipMemcpyHostToDevice, st));
  if ((rc = jamd_frontend_run_dev(f, f->d_in, sample_off, nutt, f->d_out, frame_off, st)) != JAMD_OK) return rc;
  JAMD_HIP(hipMemcpyAsync(out, f->d_out, no * sizeof(float), hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  return JAMD_OK;
}

}  // extern "C"

// ---- what csrc/frontend_live.hip takes from this unit (frontend_host.h)
void fe_info(const jamd_frontend *f, FeInfo *out) {
  out->eng = f->eng; out->d = f->d; out->ss_mode = f->ss_mode; out->fftN = f->tb.fftN;
}

int fe_base_frames(jamd_frontend *f, hipStream_t st, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                   const std::vector<const std::vector<int> *> &tabs, const float **d_stat, const int **d_tabs) {
  const int T = (*tabs[0])[nutt];
  int rc;
  if ((rc = fe_reserve(&f->d_stat, &f->stat_cap, (size_t)(T > 0 ? T : 1) * f->d.baselen)) != JAMD_OK) return rc;
  if ((rc = fe_put_offsets(f, st, sample_off, nutt, tabs)) != JAMD_OK) return rc;
  const long long *d_soff = (const long long *)f->d_off;
  const int *d_foff = (const int *)(d_soff + nutt + 1);
  *d_stat = f->d_stat; *d_tabs = d_foff;
  if (T < 1) return JAMD_OK;
  FeParams p = f->p;
  p.nutt = nutt;
  if (f->ss_mode == JAMD_SS_OFF)
    hipLaunchKernelGGL(fe_frame_kernel<false>, dim3((T + f->fpb - 1) / f->fpb), dim3(64 * f->fpb), f->lds, st, p,
                       dev_samples, d_soff, d_foff, T, f->d_stat, (const float *)nullptr, 0, 0.0f, 0.0f);
  else
    hipLaunchKernelGGL(fe_frame_kernel<true>, dim3((T + f->fpb - 1) / f->fpb), dim3(64 * f->fpb), f->lds, st, p,
                       dev_samples, d_soff, d_foff, T, f->d_stat, (const float *)f->d_ssload, 0, f->ss_alpha, f->ss_floor);
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}
