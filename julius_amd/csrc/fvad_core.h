// fvad_core.h -- the arithmetic of the voice-activity detector behind -fvad (libfvad / WebRTC VAD, 10 ms frames at
// 8 or 16 kHz), restated for one channel: the two-branch all-pass that halves 16 kHz, the tree of five all-pass split
// filters and the high-pass that make six bands, a log energy in Q4 per band with the "total power", the two-Gaussian
// noise and speech models per band with their likelihood-ratio test, the update of whichever model the decision names,
// the long-term correction by the median of the smallest values of the last 100 frames, the separation of models that
// come too close, the drift limits and the hangover.  16-bit and 32-bit integers only.  It is bit-reproducible because
// every narrowing to 16 bits, every arithmetic right shift of a negative value and every wrap-around of the reference
// (vad_core.c:115-118 names one; saturated input makes more) is kept: sums and products that can pass 2^31 are done
// unsigned, which is the two's-complement result the reference's builds give.
// Every array constant comes from the caller's jamd_fvad_model (FvModel); scalar constants of the arithmetic are here.
// One function body serves the kernel (fvad.hip: arrays in LDS, one lane per channel, element i of a lane at
// p[i * STRIDE]) and the host check (tests/fvad_core_check.cpp: STRIDE 1), so what the CPU check proves against the
// reference is the code the device runs.  No HIP header.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FV_HD __host__ __device__ __forceinline__
#else
#define FV_HD inline
#endif

constexpr int kFvBands = 6, kFvTab = 12;     // bands; Gaussians over all bands (band + 6 * k)
constexpr int kFvMinEnergy = 10;             // total power a frame needs for the models to be looked at
constexpr int kFvMaxSpeechFrames = 6;        // cap of num_of_speech
constexpr int kFvMinStd = 384;               // floor of every deviation, Q7

// The model as the code reads it: the caller's tables narrowed to 16 bits, and of the per-mode tables the entries of
// the object's mode (10 ms frames).
struct FvModel {
  short allpass_q15[2], allpass_q13[2], hp_zero[3], hp_pole[3];
  short offset[6], spectrum_weight[6], min_diff[6], max_speech[6], max_noise[6], min_mean[2];
  short noise_weight[12], speech_weight[12], noise_mean[12], speech_mean[12], noise_std[12], speech_std[12];
  short over_hang_1, over_hang_2, local_thres, global_thres;
};

// What a channel keeps between frames, as 16-bit words in this order (the two 32-bit states of the 16 -> 8 kHz stage
// and the frame counter are kept beside them), and behind it what a frame needs while it is worked on.
enum {
  kFvNoiseMean = 0, kFvSpeechMean = 12, kFvNoiseStd = 24, kFvSpeechStd = 36, kFvOverHang = 48, kFvNumSpeech = 49,
  kFvAge = 50, kFvLow = 146, kFvMeanValue = 242, kFvUpper = 248, kFvLower = 253, kFvHp = 258, kFvKept = 262,
  kFvDeltaN = kFvKept, kFvDeltaS = kFvDeltaN + 12, kFvRespN = kFvDeltaS + 12, kFvRespS = kFvRespN + 12,
  kFvFeat = kFvRespS + 12, kFvB = kFvFeat + 6, kFvC = kFvB + 40, kFvD = kFvC + 40, kFvE = kFvD + 20, kFvWords = kFvE + 20
};

template <int STRIDE>
struct FvArr {
  short *p;
  FV_HD short &operator[](int i) const { return p[i * STRIDE]; }
  FV_HD FvArr at(int off) const { return FvArr{p + off * STRIDE}; }
};

FV_HD int fv_clz(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return x ? __clz((int)x) : 32;
#else
  return x ? __builtin_clz(x) : 32;
#endif
}
FV_HD int fv_norm_w32(int a) { return a == 0 ? 0 : fv_clz((uint32_t)(a < 0 ? ~a : a)) - 1; }
FV_HD int fv_div(int num, short den) { return den != 0 ? num / den : 0x7FFFFFFF; }
FV_HD int fv_mul_wrap(int a, int b) { return (int)((uint32_t)a * (uint32_t)b); }
FV_HD int fv_add_wrap(int a, int b) { return (int)((uint32_t)a + (uint32_t)b); }
FV_HD int fv_sub_wrap(int a, int b) { return (int)((uint32_t)a - (uint32_t)b); }

// A fresh core in the mode of `m`: as fvad_new() + fvad_set_mode() leave it
template <typename Arr>
FV_HD void fv_init(Arr w, int *s32, const FvModel &m) {
  s32[0] = s32[1] = s32[2] = 0;
  for (int i = 0; i < kFvTab; i++) {
    w[kFvNoiseMean + i] = m.noise_mean[i]; w[kFvSpeechMean + i] = m.speech_mean[i];
    w[kFvNoiseStd + i] = m.noise_std[i]; w[kFvSpeechStd + i] = m.speech_std[i];
  }
  w[kFvOverHang] = 0; w[kFvNumSpeech] = 0;
  for (int i = 0; i < 16 * kFvBands; i++) { w[kFvAge + i] = 0; w[kFvLow + i] = 10000; }
  for (int i = 0; i < kFvBands; i++) w[kFvMeanValue + i] = 1600;
  for (int i = kFvUpper; i < kFvKept; i++) w[i] = 0;
}

// One all-pass branch of a split: state in Q(-1) between frames, Q15 inside
struct FvAllPass {
  int st, coef;
  FV_HD short step(short x) {
    const int t32 = fv_add_wrap(st, coef * x);
    const short y = (short)(t32 >> 16);
    st = fv_sub_wrap(x * 16384, coef * y);
    st = fv_mul_wrap(st, 2);
    return y;
  }
};

// 2 * n samples of `in` -> n of the upper and n of the lower half band (in may not be an output)
template <int STRIDE>
FV_HD void fv_split(FvArr<STRIDE> in, int n, short c0, short c1, short &up_state, short &lo_state, FvArr<STRIDE> hp,
                    FvArr<STRIDE> lp) {
  FvAllPass u{(int)up_state * 65536, c0}, l{(int)lo_state * 65536, c1};
  for (int i = 0; i < n; i++) {
    const short a = u.step(in[2 * i]), b = l.step(in[2 * i + 1]);
    hp[i] = (short)(a - b);
    lp[i] = (short)(b + a);
  }
  up_state = (short)(u.st >> 16);
  lo_state = (short)(l.st >> 16);
}

// 10 * log10(energy of the n samples) in Q4 plus `offset`; adds to `total` while that is <= kFvMinEnergy
template <int STRIDE>
FV_HD short fv_log_energy(FvArr<STRIDE> x, int n, short offset, short &total) {
  const int nbits = 32 - fv_clz((uint32_t)n);
  short smax = -1;
  for (int i = 0; i < n; i++) {
    const short v = x[i], sabs = (short)(v > 0 ? v : -v);    // (-32768 stays negative and never is the maximum)
    smax = sabs > smax ? sabs : smax;
  }
  int scaling = 0;
  if (smax != 0) {
    const int t = fv_norm_w32(smax * smax);
    scaling = t > nbits ? 0 : nbits - t;
  }
  uint32_t energy = 0;
  for (int i = 0; i < n; i++) {
    const int v = x[i];
    energy += (uint32_t)((v * v) >> scaling);
  }
  if (energy == 0) return offset;
  int rshifts = scaling;
  const int norm = 17 - fv_clz(energy);        // to 15 bits
  rshifts += norm;
  if (norm < 0) energy <<= -norm; else energy >>= norm;
  const short log2e = (short)(14336 + (short)((energy & 0x3FFF) >> 4));    // Q10
  short le = (short)(((24660 * log2e) >> 19) + ((rshifts * 24660) >> 9));  // 160 * log10(2) in Q9
  if (le < 0) le = 0;
  le = (short)(le + offset);
  if (total <= kFvMinEnergy) {
    if (rshifts >= 0) total = (short)(total + kFvMinEnergy + 1);
    else total = (short)(total + (short)(energy >> -rshifts));
  }
  return le;
}

// Probability of `input` (Q4) under N(mean, std) (Q7) in Q20; *delta = (x - m) / s^2 in Q11
FV_HD int fv_gauss(short input, short mean, short std, short *delta) {
  const short inv_std = (short)fv_div(131072 + (std >> 1), std);           // Q10
  short t16 = (short)(inv_std >> 2);
  const short inv_std2 = (short)((t16 * t16) >> 2);                         // Q14
  t16 = (short)(input << 3);
  t16 = (short)(t16 - mean);
  *delta = (short)((inv_std2 * t16) >> 10);
  const int e = (*delta * t16) >> 9;                                        // (x - m)^2 / (2 s^2), Q10
  short exp_value = 0;
  if (e < 22005) {
    t16 = (short)((5909 * e) >> 12);                                        // log2(exp(1)) in Q12
    t16 = (short)-t16;
    exp_value = (short)(0x0400 | (t16 & 0x03FF));
    t16 = (short)(t16 ^ 0xFFFF);
    t16 = (short)(t16 >> 10);
    t16 = (short)(t16 + 1);
    exp_value = (short)(exp_value >> t16);
  }
  return inv_std * exp_value;
}

// Adds `offset` to both means of a band and returns their weighted sum
template <int STRIDE>
FV_HD int fv_weighted(FvArr<STRIDE> data, short offset, const short *weights) {
  int s = 0;
  for (int k = 0; k < 2; k++) {
    data[k * kFvBands] = (short)(data[k * kFvBands] + offset);
    s += data[k * kFvBands] * weights[k * kFvBands];
  }
  return s;
}

// `value` enters the 16 smallest of the band's last 100 frames; returns the smoothed median of the smallest
template <int STRIDE>
FV_HD short fv_find_minimum(FvArr<STRIDE> w, int frame_counter, short value, int band) {
  FvArr<STRIDE> age = w.at(kFvAge + 16 * band), low = w.at(kFvLow + 16 * band);
  for (int i = 0; i < 16; i++) {
    if (age[i] != 100) {
      age[i] = (short)(age[i] + 1);
    } else {                                   // too old: the larger ones move down
      for (int j = i; j < 15; j++) { low[j] = low[j + 1]; age[j] = age[j + 1]; }
      age[15] = 101; low[15] = 10000;
    }
  }
  int pos = -1;                                // (the reference's search tree: the first entry that `value` is below)
  if (value < low[7]) {
    if (value < low[3]) {
      if (value < low[1]) pos = value < low[0] ? 0 : 1;
      else pos = value < low[2] ? 2 : 3;
    } else if (value < low[5]) pos = value < low[4] ? 4 : 5;
    else pos = value < low[6] ? 6 : 7;
  } else if (value < low[15]) {
    if (value < low[11]) {
      if (value < low[9]) pos = value < low[8] ? 8 : 9;
      else pos = value < low[10] ? 10 : 11;
    } else if (value < low[13]) pos = value < low[12] ? 12 : 13;
    else pos = value < low[14] ? 14 : 15;
  }
  if (pos > -1) {
    for (int i = 15; i > pos; i--) { low[i] = low[i - 1]; age[i] = age[i - 1]; }
    low[pos] = value; age[pos] = 1;
  }
  short median = 1600, alpha = 0;
  if (frame_counter > 2) median = low[2];
  else if (frame_counter > 0) median = low[0];
  const short mv = w[kFvMeanValue + band];
  if (frame_counter > 0) alpha = median < mv ? 6553 : 32439;               // 0.2, 0.99 in Q15
  int t = (alpha + 1) * mv;
  t += (32767 - alpha) * median;
  t += 16384;
  w[kFvMeanValue + band] = (short)(t >> 15);
  return w[kFvMeanValue + band];
}

// The decision for the frame whose features are at w[kFvFeat ..]: 0, 1, or 2 + the hangover left
template <int STRIDE>
FV_HD int fv_decide(FvArr<STRIDE> w, int &frame_counter, short total_power, const FvModel &m) {
  FvArr<STRIDE> nm = w.at(kFvNoiseMean), sm = w.at(kFvSpeechMean), ns = w.at(kFvNoiseStd), ss = w.at(kFvSpeechStd);
  FvArr<STRIDE> dN = w.at(kFvDeltaN), dS = w.at(kFvDeltaS), resp_n = w.at(kFvRespN), resp_s = w.at(kFvRespS), feat = w.at(kFvFeat);
  short is_speech = 0;
  if (total_power > kFvMinEnergy) {
    int ratio_sum = 0;
    for (int i = 0; i < kFvTab; i++) { resp_n[i] = 0; resp_s[i] = 0; }
    for (int ch = 0; ch < kFvBands; ch++) {
      int like_noise = 0, like_speech = 0, np0 = 0, sp0 = 0;
      for (int k = 0; k < 2; k++) {
        const int g = ch + k * kFvBands;
        short d;
        const int pn = m.noise_weight[g] * fv_gauss(feat[ch], nm[g], ns[g], &d);
        dN[g] = d;
        like_noise += pn;
        const int ps = m.speech_weight[g] * fv_gauss(feat[ch], sm[g], ss[g], &d);
        dS[g] = d;
        like_speech += ps;
        if (k == 0) { np0 = pn; sp0 = ps; }
      }
      const short norm_noise = (short)(like_noise == 0 ? 31 : fv_norm_w32(like_noise));
      const short norm_speech = (short)(like_speech == 0 ? 31 : fv_norm_w32(like_speech));
      const short ratio = (short)(norm_noise - norm_speech);
      ratio_sum += ratio * m.spectrum_weight[ch];
      if (ratio * 4 > m.local_thres) is_speech = 1;
      const short like_noise_q15 = (short)(like_noise >> 12);
      if (like_noise_q15 > 0) {
        const int t = (int)(((uint32_t)np0 & 0xFFFFF000u) << 2);
        resp_n[ch] = (short)fv_div(t, like_noise_q15);
        resp_n[ch + kFvBands] = (short)(16384 - resp_n[ch]);
      } else {
        resp_n[ch] = 16384;
      }
      const short like_speech_q15 = (short)(like_speech >> 12);
      if (like_speech_q15 > 0) {
        const int t = (int)(((uint32_t)sp0 & 0xFFFFF000u) << 2);
        resp_s[ch] = (short)fv_div(t, like_speech_q15);
        resp_s[ch + kFvBands] = (short)(16384 - resp_s[ch]);
      }
    }
    is_speech = (short)(is_speech | (ratio_sum >= m.global_thres));

    short speech_cap = 12800;
    for (int ch = 0; ch < kFvBands; ch++) {
      const short floor_q4 = fv_find_minimum(w, frame_counter, feat[ch], ch);
      int noise_global = fv_weighted(nm.at(ch), 0, m.noise_weight + ch);
      short t1 = (short)(noise_global >> 6);
      for (int k = 0; k < 2; k++) {
        const int g = ch + k * kFvBands;
        const short noise_mu = nm[g], speech_mu = sm[g];
        short noise_sd = ns[g], speech_sd = ss[g];
        short noise_mu_adapted = noise_mu;
        if (!is_speech) {
          const short step = (short)((resp_n[g] * dN[g]) >> 11);
          noise_mu_adapted = (short)(noise_mu + (short)((step * 655) >> 22));                // noise update constant, Q15
        }
        const short pull = (short)((floor_q4 << 4) - t1);
        short noise_mu_new = (short)(noise_mu_adapted + (short)((pull * 154) >> 9));           // long-term correction, Q8
        short lim = (short)((k + 5) << 7);
        if (noise_mu_new < lim) noise_mu_new = lim;
        lim = (short)((72 + k - ch) << 7);
        if (noise_mu_new > lim) noise_mu_new = lim;
        nm[g] = noise_mu_new;
        if (is_speech) {
          const short step = (short)((resp_s[g] * dS[g]) >> 11);
          short t = (short)((step * 6554) >> 21);                           // speech update constant, Q15
          short speech_mu_new = (short)(speech_mu + ((t + 1) >> 1));
          const short mu_cap = (short)(speech_cap + 640);
          if (speech_mu_new < m.min_mean[k]) speech_mu_new = m.min_mean[k];
          if (speech_mu_new > mu_cap) speech_mu_new = mu_cap;
          sm[g] = speech_mu_new;
          t = (short)((speech_mu + 4) >> 3);
          t = (short)(feat[ch] - t);
          int a = (dS[g] * t) >> 3;
          int b = a - 4096;
          t = (short)(resp_s[g] >> 2);
          a = fv_mul_wrap(t, b);
          b = a >> 4;
          if (b > 0) {
            t = (short)fv_div(b, (short)(speech_sd * 10));
          } else {
            t = (short)fv_div(-b, (short)(speech_sd * 10));
            t = (short)-t;
          }
          t = (short)(t + 128);
          speech_sd = (short)(speech_sd + (t >> 8));
          if (speech_sd < kFvMinStd) speech_sd = kFvMinStd;
          ss[g] = speech_sd;
        } else {
          short t = (short)(feat[ch] - (noise_mu >> 3));
          int a = (dN[g] * t) >> 3;
          a -= 4096;
          t = (short)((resp_n[g] + 2) >> 2);
          const int b = fv_mul_wrap(t, a);     // (the product the reference lets overflow)
          a = b >> 14;
          if (a > 0) {
            t = (short)fv_div(a, noise_sd);
          } else {
            t = (short)fv_div(-a, noise_sd);
            t = (short)-t;
          }
          t = (short)(t + 32);
          noise_sd = (short)(noise_sd + (t >> 6));
          if (noise_sd < kFvMinStd) noise_sd = kFvMinStd;
          ns[g] = noise_sd;
        }
      }
      // models that have come too close are moved apart
      noise_global = fv_weighted(nm.at(ch), 0, m.noise_weight + ch);
      int speech_global = fv_weighted(sm.at(ch), 0, m.speech_weight + ch);
      const short diff = (short)((short)(speech_global >> 9) - (short)(noise_global >> 9));
      if (diff < m.min_diff[ch]) {
        const short t = (short)(m.min_diff[ch] - diff);
        t1 = (short)((13 * t) >> 2);
        const short t2 = (short)((3 * t) >> 2);
        speech_global = fv_weighted(sm.at(ch), t1, m.speech_weight + ch);
        noise_global = fv_weighted(nm.at(ch), (short)-t2, m.noise_weight + ch);
      }
      // drift limits
      speech_cap = m.max_speech[ch];
      short t2 = (short)(speech_global >> 7);
      if (t2 > speech_cap) {
        t2 = (short)(t2 - speech_cap);
        for (int k = 0; k < 2; k++) sm[ch + k * kFvBands] = (short)(sm[ch + k * kFvBands] - t2);
      }
      t2 = (short)(noise_global >> 7);
      if (t2 > m.max_noise[ch]) {
        t2 = (short)(t2 - m.max_noise[ch]);
        for (int k = 0; k < 2; k++) nm[ch + k * kFvBands] = (short)(nm[ch + k * kFvBands] - t2);
      }
    }
    frame_counter++;
  }
  // hangover
  if (!is_speech) {
    if (w[kFvOverHang] > 0) {
      is_speech = (short)(2 + w[kFvOverHang]);
      w[kFvOverHang] = (short)(w[kFvOverHang] - 1);
    }
    w[kFvNumSpeech] = 0;
  } else {
    w[kFvNumSpeech] = (short)(w[kFvNumSpeech] + 1);
    if (w[kFvNumSpeech] > kFvMaxSpeechFrames) {
      w[kFvNumSpeech] = kFvMaxSpeechFrames;
      w[kFvOverHang] = m.over_hang_2;
    } else {
      w[kFvOverHang] = m.over_hang_1;
    }
  }
  return is_speech;
}

// One 10 ms frame: src(j) is its sample j (160 at 16 kHz with wide != 0, else 80).  s32: the two states of the
// 16 -> 8 kHz stage and the frame counter.  Returns the core's raw value.
template <int STRIDE, typename Src>
FV_HD int fv_frame(FvArr<STRIDE> w, int *s32, const FvModel &m, bool wide, Src src) {
  FvArr<STRIDE> B = w.at(kFvB), Cb = w.at(kFvC), D = w.at(kFvD), E = w.at(kFvE), feat = w.at(kFvFeat);
  FvArr<STRIDE> up = w.at(kFvUpper), lo = w.at(kFvLower), hp = w.at(kFvHp);
  // 0 - 4000 Hz -> B: 2000 - 4000, Cb: 0 - 2000 (40 each); at 16 kHz each input of the split is made from two samples
  {
    FvAllPass u{(int)up[0] * 65536, m.allpass_q15[0]}, l{(int)lo[0] * 65536, m.allpass_q15[1]};
    int d0 = s32[0], d1 = s32[1];
    const int c0 = m.allpass_q13[0], c1 = m.allpass_q13[1];
    for (int i = 0; i < 40; i++) {
      short x[2];
      for (int h = 0; h < 2; h++) {
        if (wide) {
          const short a = src(4 * i + 2 * h), b = src(4 * i + 2 * h + 1);
          const short y0 = (short)((d0 >> 1) + ((c0 * a) >> 14));
          d0 = a - ((c0 * y0) >> 12);
          const short y1 = (short)((d1 >> 1) + ((c1 * b) >> 14));
          d1 = b - ((c1 * y1) >> 12);
          x[h] = (short)(y0 + y1);
        } else {
          x[h] = src(2 * i + h);
        }
      }
      const short a = u.step(x[0]), b = l.step(x[1]);
      B[i] = (short)(a - b);
      Cb[i] = (short)(b + a);
    }
    up[0] = (short)(u.st >> 16); lo[0] = (short)(l.st >> 16);
    s32[0] = d0; s32[1] = d1;
  }
  short total = 0;
  const short c0 = m.allpass_q15[0], c1 = m.allpass_q15[1];
  fv_split(B, 20, c0, c1, up[1], lo[1], D, E);               // D: 3000 - 4000, E: 2000 - 3000
  feat[5] = fv_log_energy(D, 20, m.offset[5], total);
  feat[4] = fv_log_energy(E, 20, m.offset[4], total);
  fv_split(Cb, 20, c0, c1, up[2], lo[2], D, E);              // D: 1000 - 2000, E: 0 - 1000
  feat[3] = fv_log_energy(D, 20, m.offset[3], total);
  fv_split(E, 10, c0, c1, up[3], lo[3], B, Cb);              // B: 500 - 1000, Cb: 0 - 500
  feat[2] = fv_log_energy(B, 10, m.offset[2], total);
  fv_split(Cb, 5, c0, c1, up[4], lo[4], D, E);               // D: 250 - 500, E: 0 - 250
  feat[1] = fv_log_energy(D, 5, m.offset[1], total);
  for (int i = 0; i < 5; i++) {                              // E without 0 - 80 Hz -> B
    const short x = E[i];
    int t = m.hp_zero[0] * x;
    t = fv_add_wrap(t, m.hp_zero[1] * hp[0]);
    t = fv_add_wrap(t, m.hp_zero[2] * hp[1]);
    hp[1] = hp[0]; hp[0] = x;
    t = fv_sub_wrap(t, m.hp_pole[1] * hp[2]);
    t = fv_sub_wrap(t, m.hp_pole[2] * hp[3]);
    hp[3] = hp[2]; hp[2] = (short)(t >> 14);
    B[i] = hp[2];
  }
  feat[0] = fv_log_energy(B, 5, m.offset[0], total);
  return fv_decide(w, s32[2], total, m);
}
