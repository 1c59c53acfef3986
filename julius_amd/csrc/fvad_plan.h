// fvad_plan.h -- what the voice-activity detector (jamd_fvad, fvad_api.hip) works out without a device: the checks
// of the descriptor and of the caller's model, the model as the kernels read it, the model file, and the closed-form
// frame counts -- of the detector alone, and of fvad_proceed() (libjulius/src/adin-cut.c:264-311) as a function of the
// stream -- with the smallest speech count that opens its gate.  Plain C++, no HIP header: tests/fvad_core_check.cpp
// compiles it alone, under the host sanitizers.
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "julius_amd.h"
#include "fvad_core.h"

constexpr int kFvMaxFrame = 160;             // samples of 10 ms at 16 kHz

// Samples of one frame, or 0 for a rate that is not served
static inline int fv_frame_size(int sfreq) { return sfreq == 8000 ? 80 : sfreq == 16000 ? 160 : 0; }

// Every entry is an int16_t in the reference.  Returns false with the reason in `err`.
static inline bool fv_check_model(const jamd_fvad_model *m, std::string &err) {
  if (!m) { err = "the model is NULL"; return false; }
  const int *v = (const int *)m;
  for (int i = 0; i < JAMD_FVAD_MODEL_INTS; i++)
    if (v[i] < -32768 || v[i] > 32767) {
      err = "model entry " + std::to_string(i) + " (" + std::to_string(v[i]) + ") is no 16-bit value";
      return false;
    }
  return true;
}

static inline bool fv_check_desc(const jamd_fvad_desc *d, std::string &err) {
  if (!d) { err = "the descriptor is NULL"; return false; }
  if (d->sfreq == 32000 || d->sfreq == 48000) {
    err = "sfreq " + std::to_string(d->sfreq) + ": valid for the detector but not served (8000 and 16000 are)";
    return false;
  }
  if (!fv_frame_size(d->sfreq)) {
    err = "sfreq " + std::to_string(d->sfreq) + ": the detector takes 8000 or 16000 (the reference goes on after "
          "fvad_set_sample_rate() has failed; that is not reproduced)";
    return false;
  }
  if (d->mode < 0 || d->mode > 3) { err = "mode " + std::to_string(d->mode) + " is not in 0 ... 3"; return false; }
  return fv_check_model(d->model, err);
}

// The checked model in the object's mode
static inline FvModel fv_model(const jamd_fvad_model *s, int mode) {
  FvModel m;
#define FV_COPY(f) for (size_t i = 0; i < sizeof m.f / sizeof m.f[0]; i++) m.f[i] = (short)s->f[i]
  FV_COPY(allpass_q15); FV_COPY(allpass_q13); FV_COPY(hp_zero); FV_COPY(hp_pole);
  FV_COPY(offset); FV_COPY(spectrum_weight); FV_COPY(min_diff); FV_COPY(max_speech); FV_COPY(max_noise); FV_COPY(min_mean);
  FV_COPY(noise_weight); FV_COPY(speech_weight); FV_COPY(noise_mean); FV_COPY(speech_mean); FV_COPY(noise_std);
  FV_COPY(speech_std);
#undef FV_COPY
  m.over_hang_1 = (short)s->over_hang_1[mode]; m.over_hang_2 = (short)s->over_hang_2[mode];
  m.local_thres = (short)s->local_thres[mode]; m.global_thres = (short)s->global_thres[mode];
  return m;
}

// The model file: JAMD_FVAD_MODEL_INTS decimal integers in the order of jamd_fvad_model's members, one per line; a line
// that begins with '#' and an empty line are skipped.  Returns false with the reason in `err`.
static inline bool fv_model_read(const char *path, jamd_fvad_model *out, std::string &err) {
  FILE *fp = fopen(path, "r");
  if (!fp) { err = "cannot open the file"; return false; }
  char buf[512];
  int *v = (int *)out, n = 0, line = 0;
  while (fgets(buf, sizeof buf, fp)) {
    line++;
    char *p = buf;
    while (*p == ' ' || *p == '\t') p++;
    if (*p == '#' || *p == '\n' || *p == '\r' || *p == '\0') continue;
    char *end;
    errno = 0;
    const long x = strtol(p, &end, 10);
    while (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n') end++;
    if (end == p || *end != '\0' || errno != 0) { err = "line " + std::to_string(line) + " is no integer"; fclose(fp); return false; }
    if (x < -32768 || x > 32767) { err = "line " + std::to_string(line) + " is no 16-bit value"; fclose(fp); return false; }
    if (n >= JAMD_FVAD_MODEL_INTS) { err = "more than " + std::to_string(JAMD_FVAD_MODEL_INTS) + " entries"; fclose(fp); return false; }
    v[n++] = (int)x;
  }
  fclose(fp);
  if (n < JAMD_FVAD_MODEL_INTS) {
    err = std::to_string(n) + " entries, the model has " + std::to_string(JAMD_FVAD_MODEL_INTS);
    return false;
  }
  return true;
}

// Frames the detector alone has completed after e samples: every whole frame
FV_HD long long fv_frames_done(long long e, int fs) { return e / fs; }

// Frames fvad_proceed() has processed once its blocks end at sample e of the stream: `while (i + fs < len)` takes a
// frame only once one more sample is there, so max(0, ceil(e / fs) - 1), whatever the blocks were
FV_HD long long fv_gate_frames(long long e, int fs) {
  const long long n = (e + fs - 1) / fs - 1;
  return n > 0 ? n : 0;
}

// The smallest count c of speech frames among the last N with (float)c / (float)N >= thres in float, N + 1 if none
static inline int fv_gate_cmin(int N, float thres) {
  for (int c = 0; c <= N; c++)
    if ((float)c / (float)N >= thres) return c;
  return N + 1;
}
