/*
 * jamd_fvad_export -- write the model file of the device's voice-activity detector (-fvad) from a Julius tree.
 *
 *   jamd_fvad_export OUT.txt
 *
 * The detector's array constants (filter coefficients, per-band offsets, weights and limits, the initial Gaussians,
 * the per-mode hangover and threshold tables) are `static const` tables inside libfvad's sources, so this file takes
 * those sources in at compile time and prints the tables: JAMD_FVAD_MODEL_INTS integers, one per line, in the order
 * of jamd_fvad_model's members (include/julius_amd.h), which jamd_fvad_model_read() takes back.  Of the per-mode tables
 * the entries for 10 ms frames are written, the only frame length adin_cut() uses.  Compiled against JULIUS_SRC by
 * julius_amd/shim/Makefile (target fvad_export) together with the rest of libfvad, like the other shim programs.
 */
#include <stdio.h>
#include <stdlib.h>

#include "vad/vad_core.c"
#include "vad/vad_filterbank.c"
#include "vad/vad_sp.c"

#include "julius_amd.h"

static int put(FILE *fp, const char *name, const int16_t *v, int n)
{
  int i;
  fprintf(fp, "# %s\n", name);
  for (i = 0; i < n; i++) fprintf(fp, "%d\n", (int)v[i]);
  return n;
}

int main(int argc, char **argv)
{
  const int16_t oh1[4] = { kOverHangMax1Q[0], kOverHangMax1LBR[0], kOverHangMax1AGG[0], kOverHangMax1VAG[0] };
  const int16_t oh2[4] = { kOverHangMax2Q[0], kOverHangMax2LBR[0], kOverHangMax2AGG[0], kOverHangMax2VAG[0] };
  const int16_t loc[4] = { kLocalThresholdQ[0], kLocalThresholdLBR[0], kLocalThresholdAGG[0], kLocalThresholdVAG[0] };
  const int16_t glo[4] = { kGlobalThresholdQ[0], kGlobalThresholdLBR[0], kGlobalThresholdAGG[0], kGlobalThresholdVAG[0] };
  FILE *fp;
  int n = 0;

  if (argc != 2) {
    fprintf(stderr, "usage: jamd_fvad_export OUT.txt\n");
    return 2;
  }
  if ((fp = fopen(argv[1], "w")) == NULL) {
    perror(argv[1]);
    return 1;
  }
  fprintf(fp, "# jamd_fvad_model: %d integers, one per line, in the order of the members in julius_amd.h\n", JAMD_FVAD_MODEL_INTS);
  n += put(fp, "allpass_q15", kAllPassCoefsQ15, 2);
  n += put(fp, "allpass_q13", kAllPassCoefsQ13, 2);
  n += put(fp, "hp_zero", kHpZeroCoefs, 3);
  n += put(fp, "hp_pole", kHpPoleCoefs, 3);
  n += put(fp, "offset", kOffsetVector, 6);
  n += put(fp, "spectrum_weight", kSpectrumWeight, 6);
  n += put(fp, "min_diff", kMinimumDifference, 6);
  n += put(fp, "max_speech", kMaximumSpeech, 6);
  n += put(fp, "max_noise", kMaximumNoise, 6);
  n += put(fp, "min_mean", kMinimumMean, 2);
  n += put(fp, "noise_weight", kNoiseDataWeights, 12);
  n += put(fp, "speech_weight", kSpeechDataWeights, 12);
  n += put(fp, "noise_mean", kNoiseDataMeans, 12);
  n += put(fp, "speech_mean", kSpeechDataMeans, 12);
  n += put(fp, "noise_std", kNoiseDataStds, 12);
  n += put(fp, "speech_std", kSpeechDataStds, 12);
  n += put(fp, "over_hang_1 (mode 0 ... 3)", oh1, 4);
  n += put(fp, "over_hang_2", oh2, 4);
  n += put(fp, "local_thres", loc, 4);
  n += put(fp, "global_thres", glo, 4);
  if (fclose(fp) != 0 || n != JAMD_FVAD_MODEL_INTS) {
    fprintf(stderr, "jamd_fvad_export: wrote %d of %d entries\n", n, JAMD_FVAD_MODEL_INTS);
    return 1;
  }
  return 0;
}
