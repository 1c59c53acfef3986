// adin_host.h -- the host side of the audio conditioning stage (jamd_adin): the object, which adin_api.hip builds and
// owns (validation, the tables of a push, scratch, the C ABI), and the launchers through which it reaches the kernels
// in adin.hip.  The API unit launches nothing itself; a launcher checks nothing.  What needs no device is in
// adin_plan.h.  Internal, not installed.
#pragma once
#include "jamd_host.h"
#include "adin_plan.h"

// One channel of one FIR stage in a push (AdPush), with where its new inputs lie and where its outputs go
struct AdStageTab { long long in_off, out_off; int n_in, pend, t_b, n_raw, drop, adv; };
// One channel behind the cascade: n samples at src_off of the source, the level-scaled, stripped ones to pre_off of
// the scratch
struct AdChanTab { long long src_off, pre_off; int n, pad; };

constexpr int kAdFirTile = 1024;             // outputs of a FIR stage per workgroup
constexpr int kAdPostTile = 1024;            // samples per step of the strip / zmean workgroup, and per workgroup of the last kernel
constexpr int kAdHistMax = 512 + kAdBlock - 1;   // a stage's history and its pending inputs at the most

struct JAMD_LOCAL jamd_adin {
  jamd_engine *eng = nullptr;
  jamd_adin_desc d{};                        // as created, the table pointers NULL
  int nchan = 0;
  AdCascade cas{};
  JamdDev<double> d_fir[2];                  // 3to4, 2to1 [kAdMaxTaps]
  JamdDev<double> d_hist[3];                 // per stage [nchan][hist + 255]: consumed history | pending
  JamdDev<int> d_zlen;                       // [nchan]
  JamdDev<float> d_zmean;                    // [nchan]
  std::vector<long long> arrived[3];         // per stage and channel, since the last JAMD_ADIN_DS reset
  // scratch of a push
  JamdDev<double> d_mid[2];                  // 64 kHz, 32 kHz
  JamdDev<int16_t> d_ds;                     // 16 kHz out of the cascade
  JamdDev<int16_t> d_pre;                    // scaled and stripped, before the mean is taken off
  JamdDev<int> d_cnt;                        // [nchan] samples left after stripping
  JamdDev<long long> d_ooff;                 // [nchan + 1]
  JamdDev<unsigned char> d_mask;             // [nchan]
  JamdPinned tab;                            // AdStageTab [3][nchan] | AdChanTab [nchan]
  JamdHostBuf h_ooff;                        // [nchan + 1] int64
  JamdStage<int16_t, int16_t> stage;         // push_host
};

// ---- adin.hip
// Stage s of the cascade for the channels d_tab [nchan] describes; max_raw is the largest n_raw among them (> 0).
// Stage 0 reads int16 at `in`, the others double; stage 2 writes int16 (C's short = double), the others double.
JAMD_LOCAL int ad_launch_fir(jamd_adin *a, hipStream_t st, int s, const AdStageTab *d_tab, const void *in, void *out,
                                int max_raw);
// After the three stages: every stage's history moves on by what the push consumed.  d_tab [3][nchan].
JAMD_LOCAL int ad_launch_hist(jamd_adin *a, hipStream_t st, const AdStageTab *d_tab, const int16_t *in0);
// Level, strip_zero() and the sub_zmean() chain of every channel: src -> a->d_pre, a->d_cnt, a->d_zlen / d_zmean; then
// the offsets (a->d_ooff) and the samples, the mean taken off, back to back -> dev_out.  max_n: the longest chunk (> 0).
JAMD_LOCAL int ad_launch_post(jamd_adin *a, hipStream_t st, const AdChanTab *d_tab, const int16_t *src, int16_t *dev_out,
                                 int max_n);
// The channels d_mask names (NULL: all) back to the start
JAMD_LOCAL int ad_launch_reset(jamd_adin *a, hipStream_t st, const unsigned char *d_mask, int what);
