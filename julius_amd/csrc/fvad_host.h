// fvad_host.h -- the host side of the voice-activity detector (jamd_fvad): the object, which fvad_api.hip builds and
// owns (validation, the table of a push, the C ABI), and the launchers through which it reaches the kernels in
// fvad.hip.  The API unit launches nothing itself; a launcher checks nothing.  What needs no device is in fvad_plan.h,
// the arithmetic in fvad_core.h.  Internal, not installed.
#pragma once
#include <vector>

#include "jamd_host.h"
#include "fvad_plan.h"

// One channel in a push: n samples at src_off of the input, its nf frames' bytes to out_off of the output
struct FvChanTab { long long src_off, out_off; int n, nf; };

constexpr int kFvLanes = 64;                 // channels per workgroup: one wave, a lane per channel

struct JAMD_LOCAL jamd_fvad {
  jamd_engine *eng = nullptr;
  int nchan = 0, sfreq = 0, mode = 0, fs = 0;
  JamdDev<FvModel> d_model;                  // [1]
  JamdDev<short> d_s16;                      // [kFvKept][nchan] the core's 16-bit words (fvad_core.h)
  JamdDev<int> d_s32;                        // [3][nchan] the 16 -> 8 kHz stage's two states, frame_counter
  JamdDev<short> d_pend;                     // [kFvMaxFrame][nchan] samples of an incomplete frame
  JamdDev<int> d_npend;                      // [nchan]
  JamdDev<unsigned char> d_mask;             // [nchan]
  std::vector<long long> arrived;            // per channel, since its last reset
  JamdPinned tab;                            // FvChanTab [nchan]
  JamdStage<int16_t, unsigned char> stage;   // push_host
};

// The detector inside the silence cutting stage (jamd_adin_cut_create_fvad(), adin_cut_fvad.hip): a core per channel
// in two copies -- a push works from d_*16 / d_*32 into the n(ext) ones, and only the push's last kernel makes them
// the channel's -- and V[k], the speech frames among frames 0 ... k - 1 of the stream: those of a push in scratch, the
// last `vhist` of earlier pushes in a ring by k.
struct JAMD_LOCAL FvGate {
  int fs = 0, N = 0, cmin = 0, vhist = 0;
  JamdDev<FvModel> d_model;                  // [1]
  JamdDev<short> d_s16, d_s16n;              // [kFvKept][nchan]
  JamdDev<int> d_s32, d_s32n;                // [3][nchan]
  JamdDev<unsigned> d_vh;                    // [nchan][vhist] V[k] in slot k % vhist
  JamdDev<unsigned> d_vnew;                  // scratch of a push: V[F0 + 1 ...] of every channel at its v_off
  JamdPinned vtab;                           // long long v_off [nchan]
};

// A core as jamd_fvad_state_get() hands it out (the order is in julius_amd.h)
static inline void fv_state_ints(const short *s16, const int *s32, int npend, int *state) {
  int n = 0;
  state[n++] = s32[0]; state[n++] = s32[1];
  for (int i = 0; i < kFvKept; i++) {
    if (i == kFvOverHang) state[n++] = s32[2];               // frame_counter sits in front of over_hang
    state[n++] = s16[i];
  }
  state[n++] = npend;
  static_assert(2 + kFvKept + 1 + 1 == JAMD_FVAD_STATE_INTS, "the order in julius_amd.h");
}

// ---- fvad.hip
// The frames every channel's chunk completes -> dev_out; the cores and the waiting samples move on
JAMD_LOCAL int fv_launch_push(jamd_fvad *f, hipStream_t st, const FvChanTab *d_tab, const int16_t *dev_in,
                                 unsigned char *dev_out);
// The channels d_mask names (NULL: all) get a fresh core
JAMD_LOCAL int fv_launch_reset(jamd_fvad *f, hipStream_t st, const unsigned char *d_mask);
// The same on bare tables ([kFvKept][nchan], [3][nchan]; npend may be NULL)
JAMD_LOCAL int fv_launch_reset_at(hipStream_t st, const FvModel *d_model, const unsigned char *d_mask, short *s16, int *s32,
                                     int *npend, int nchan);
