// fvad_core_check.cpp -- the device's voice-activity detector on the host: julius_amd/csrc/fvad_core.h is the code
// the kernel runs (there with its arrays in LDS, here in a plain array), fvad_plan.h what its host layer works out
// without a device.  tests/test_fvad_host.py compiles this file alone (under the host sanitizers) and compares what it
// prints with the reference and the committed fixtures.
//   run MODEL SFREQ MODE PCM    the raw value of every whole 10 ms frame of the int16 file PCM (one line), then the
//                               core's state in the order of jamd_fvad_state_get() without its last entry (one line)
//   read MODEL                  "ok" and the entries, or "refused: <reason>" (exit status 1)
//   gate FS E...                fvad_proceed()'s frame count at each E
//   frames FS E...              the detector's own
//   cmin N THRES                the smallest speech count that opens the gate
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fvad_plan.h"

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::string err;
  const std::string cmd = argv[1];
  if (cmd == "read") {
    jamd_fvad_model m;
    if (!fv_model_read(argv[2], &m, err)) { printf("refused: %s\n", err.c_str()); return 1; }
    printf("ok");
    for (int i = 0; i < JAMD_FVAD_MODEL_INTS; i++) printf(" %d", ((const int *)&m)[i]);
    printf("\n");
    return 0;
  }
  if (cmd == "gate" || cmd == "frames") {
    const int fs = atoi(argv[2]);
    for (int i = 3; i < argc; i++)
      printf("%lld\n", cmd == "gate" ? fv_gate_frames(atoll(argv[i]), fs) : fv_frames_done(atoll(argv[i]), fs));
    return 0;
  }
  if (cmd == "cmin" && argc == 4) {
    printf("%d\n", fv_gate_cmin(atoi(argv[2]), (float)atof(argv[3])));
    return 0;
  }
  if (cmd == "run" && argc == 6) {
    jamd_fvad_model src;
    if (!fv_model_read(argv[2], &src, err)) { printf("refused: %s\n", err.c_str()); return 1; }
    jamd_fvad_desc d{atoi(argv[3]), atoi(argv[4]), &src};
    if (!fv_check_desc(&d, err)) { printf("refused: %s\n", err.c_str()); return 1; }
    const FvModel m = fv_model(&src, d.mode);
    const int fs = fv_frame_size(d.sfreq);
    FILE *fp = fopen(argv[5], "rb");
    if (!fp) return 2;
    std::vector<short> pcm;
    short buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(short), 4096, fp)) > 0) pcm.insert(pcm.end(), buf, buf + n);
    fclose(fp);
    std::vector<short> work(kFvWords, 0);
    int s32[3];
    FvArr<1> w{work.data()};
    fv_init(w, s32, m);
    const long long nf = fv_frames_done((long long)pcm.size(), fs);
    for (long long f = 0; f < nf; f++) {
      const short *x = pcm.data() + f * fs;
      printf(f ? " %d" : "%d", fv_frame(w, s32, m, fs == 160, [x](int j) { return x[j]; }));
    }
    printf("\n%d %d", s32[0], s32[1]);
    for (int i = 0; i < kFvKept; i++) {
      if (i == kFvOverHang) printf(" %d", s32[2]);
      printf(" %d", work[i]);
    }
    printf("\n");
    return 0;
  }
  return 2;
}
