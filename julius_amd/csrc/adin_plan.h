// adin_plan.h -- what the audio conditioning stage (jamd_adin, adin_api.hip) works out without a device: the three FIR
// stages of ds48to16() (libsent/src/adin/ds48to16.c) as closed-form counts over each stage's cumulative input stream,
// what one push does to a stage, the descriptor checks, and the coefficient file of the reference's load_filter().
// Plain C++, no HIP header: tests/adin_plan_check.cpp compiles it alone, under the host sanitizers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "julius_amd.h"

constexpr int kAdBlock = 256;                // DS_BUFSIZE: a stage consumes whole blocks only
constexpr int kAdMaxTaps = 513;              // DS_RBSIZE + 1 entries of hdn[]
constexpr int kAdZmeanSamples = 48000;       // ZMEANSAMPLES
constexpr int kAdStripWin = 16;              // strip.c WINDOWLEN

// One FIR stage: decrate input ticks per output, intrate ticks per input (init_filter()).  Output m of the stream sits
// at tick dec * m: input k = tick / intr, phase i = tick % intr, value sum_j x[k - j] * h[i + intr * j].  `hist` inputs
// behind the newest are ever read (rounded up to even for the two-way split of stages 1 and 2).
struct AdStage {
  int hdn_len, dec, intr, delay, hist;
};

static inline AdStage ad_stage(int ntaps, int dec, int intr) {
  AdStage s;
  s.hdn_len = ntaps - 1; s.dec = dec; s.intr = intr;
  s.delay = s.hdn_len / (2 * dec);
  s.hist = s.hdn_len / intr;
  s.hist += s.hist & 1;
  return s;
}

// Inputs a stage has consumed of A arrived
static inline long long ad_consumed(long long A) { return A / kAdBlock * kAdBlock; }
// Outputs computed, the dropped first `delay` included, once P inputs are consumed: ticks dec * m < intr * P
static inline long long ad_raw(const AdStage &s, long long P) { return (s.intr * P + s.dec - 1) / s.dec; }
// Outputs a stage has handed on of A arrived
static inline long long ad_emitted(const AdStage &s, long long A) {
  const long long m = ad_raw(s, ad_consumed(A)) - s.delay;
  return m > 0 ? m : 0;
}

// What a push of n_in inputs does to a stage that had A arrived.  The kernel sees Z = [hist consumed inputs | pend
// pending | the n_in new], with Z[hist] the first unconsumed input; output r of the push (0 <= r < n_raw) sits at tick
// t_b + dec * r counted from there.  The first `drop` are not handed on, `adv` inputs are consumed.
struct AdPush {
  int n_in, pend, t_b, n_raw, drop, adv, n_out;
};

static inline AdPush ad_push(const AdStage &s, long long A, long long n_in) {
  AdPush p;
  const long long Pb = ad_consumed(A), Pa = ad_consumed(A + n_in);
  const long long mb = ad_raw(s, Pb), ma = ad_raw(s, Pa);
  long long drop = s.delay - mb;
  if (drop < 0) drop = 0;
  if (drop > ma - mb) drop = ma - mb;
  p.n_in = (int)n_in; p.pend = (int)(A - Pb);
  p.t_b = (int)(s.dec * mb - s.intr * Pb);
  p.n_raw = (int)(ma - mb); p.drop = (int)drop; p.adv = (int)(Pa - Pb);
  p.n_out = p.n_raw - p.drop;
  return p;
}

struct AdCascade {
  AdStage st[3];
};

// 48 -> 64 -> 32 -> 16 kHz (ds48to16_new())
static inline AdCascade ad_cascade(int n_3to4, int n_2to1) {
  AdCascade c;
  c.st[0] = ad_stage(n_3to4, 3, 4);
  c.st[1] = ad_stage(n_2to1, 2, 1);
  c.st[2] = ad_stage(n_2to1, 2, 1);
  return c;
}

// 16 kHz samples out of the cascade once `a48` 48 kHz samples have arrived
static inline long long ad_cascade_emitted(const AdCascade &c, long long a48) {
  long long a = a48;
  for (int s = 0; s < 3; s++) a = ad_emitted(c.st[s], a);
  return a;
}

// The descriptor as _create and the host-only counts need it.  Returns false with the reason in `err`.
static inline bool ad_check_desc(const jamd_adin_desc *d, bool need_tables, std::string &err) {
  if (!d) { err = "the descriptor is NULL"; return false; }
  if (d->down48) {
    if (d->n_3to4 < 1 || d->n_3to4 > kAdMaxTaps || d->n_2to1 < 1 || d->n_2to1 > kAdMaxTaps) {
      err = "down48 needs two coefficient tables of 1 ... 513 entries (got " + std::to_string(d->n_3to4) + " and " +
            std::to_string(d->n_2to1) + ")";
      return false;
    }
    if (need_tables && (!d->fir_3to4 || !d->fir_2to1)) { err = "down48 without coefficient tables"; return false; }
  }
  // (SP16)((float)s * coef) goes through a 32-bit integer: |s * coef| must stay below 2^31
  const double c = d->level_coef < 0 ? -(double)d->level_coef : (double)d->level_coef;
  if (!(32768.0 * c < 2147483648.0)) { err = "level_coef out of range: 32768 * |coef| must stay below 2^31"; return false; }
  return true;
}

// load_filter(): one atof() per fgets() line of at most 511 characters, DS_RBSIZE + 1 entries at the most.  Returns the
// number of entries (copies them to out[0 .. cap)), or -1 with the reason in `err`: unreadable, empty, or cap too small.
static inline int ad_fir_read(const char *path, double *out, int cap, std::string &err) {
  FILE *fp = fopen(path, "r");
  if (!fp) { err = "cannot open the file"; return -1; }
  char buf[512];
  int n = 0;
  while (n < kAdMaxTaps && fgets(buf, sizeof buf, fp)) {
    if (n >= cap) { fclose(fp); err = "more entries than the caller has room for"; return -1; }
    out[n++] = atof(buf);
  }
  fclose(fp);
  if (n == 0) { err = "no coefficient in the file"; return -1; }
  return n;
}
