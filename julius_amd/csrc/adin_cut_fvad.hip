// adin_cut_fvad.hip -- the detector inside the silence cutting stage (-fvad; jamd_adin_cut_create_fvad()): the two
// kernels that an object with the gate launches around those of adin_cut.hip, and their launchers (adin_cut_host.h).
//
// fvad_proceed() (libjulius/src/adin-cut.c:264-311) has processed max(0, ceil(e / fs) - 1) frames once its blocks end at
// sample e, on a frame grid fixed at the stream's start, so which frames a push owes is closed-form in the channel's
// state and chunk (ac_gate_span()): those below the end of the last block the push walks, and not one more -- samples
// that still wait for their block stay out of the detector, or a reset would leave frames in the core that the
// reference never saw.  A lane takes a channel and walks its frames in order, as fv_push_kernel does (fvad.hip; the
// arithmetic is fvad_core.h, the arrays in the lane's column of LDS); a frame's samples come out of the history ring of
// the cutting stage where they arrived with earlier pushes.  The decisions leave as V[k], the speech frames among
// frames 0 ... k - 1: the blocks kernel needs V[n] - V[n - N] only.  The core is read from the channel's copy and
// written to a second one, which acg_advance_kernel makes the channel's when the push is certain to go through.
#include "adin_cut_host.h"

struct AcgArgs {
  const FvModel *model;
  const AcChanTab *tab;
  const AcState *state;
  const long long *voff;
  const int16_t *in, *hs;
  short *s16, *s16n;
  int *s32, *s32n;
  unsigned *vh, *vnew;
  int nchan, chunk, hist, fs, vhist;
};

__global__ __launch_bounds__(kFvLanes) void acg_frames_kernel(AcgArgs a) {
  __shared__ short lds[kFvWords * kFvLanes];
  const int c = blockIdx.x * kFvLanes + threadIdx.x;
  if (c >= a.nchan) return;
  const AcChanTab t = a.tab[c];
  if (t.n == 0 && !t.eos) return;              // idle
  const AcState s = a.state[c];
  const AcGateSpan g = ac_gate_span(s, t, a.chunk, a.fs);
  const long long C = a.nchan, B = s.pos;
  const FvArr<kFvLanes> w{lds + threadIdx.x};
  for (int i = 0; i < kFvKept; i++) w[i] = a.s16[i * C + c];
  int s32[3] = {a.s32[c], a.s32[C + c], a.s32[2 * C + c]};
  const FvModel &m = *a.model;
  const int fs = a.fs, hist = a.hist;
  const bool wide = fs == kFvMaxFrame;
  const int16_t *in = a.in + t.src_off, *ring = a.hs + (size_t)c * hist;
  unsigned vc = g.F0 <= 0 ? 0u : a.vh[(size_t)c * a.vhist + g.F0 % a.vhist];
  unsigned *vnew = a.vnew + a.voff[c];
  for (long long f = g.F0; f < g.F1; f++) {
    const long long q0 = f * fs;
    const int r = fv_frame(w, s32, m, wide, [&](int j) -> short {
      const long long q = q0 + j;
      return q < B ? ring[q % hist] : in[q - B];
    });
    vc += r > 0;
    vnew[f - g.F0] = vc;
  }
  for (int i = 0; i < kFvKept; i++) a.s16n[i * C + c] = w[i];
  a.s32n[c] = s32[0]; a.s32n[C + c] = s32[1]; a.s32n[2 * C + c] = s32[2];
}

// Before ac_advance_kernel, which overwrites the state the span is worked out from
__global__ __launch_bounds__(kFvLanes) void acg_advance_kernel(AcgArgs a) {
  const int c = blockIdx.x * kFvLanes + threadIdx.x;
  if (c >= a.nchan) return;
  const AcChanTab t = a.tab[c];
  if (t.n == 0 && !t.eos) return;
  const AcGateSpan g = ac_gate_span(a.state[c], t, a.chunk, a.fs);
  const long long C = a.nchan, cnt = g.F1 - g.F0;
  for (int i = 0; i < kFvKept; i++) a.s16[i * C + c] = a.s16n[i * C + c];
  for (int i = 0; i < 3; i++) a.s32[i * C + c] = a.s32n[i * C + c];
  const unsigned *vnew = a.vnew + a.voff[c];
  for (long long i = cnt > a.vhist ? cnt - a.vhist : 0; i < cnt; i++)
    a.vh[(size_t)c * a.vhist + (g.F0 + 1 + i) % a.vhist] = vnew[i];
}

static AcgArgs acg_args(jamd_adin_cut *k, const AcChanTab *d_tab, const long long *d_voff, const int16_t *dev_in) {
  FvGate &q = *k->gate;
  return AcgArgs{q.d_model, d_tab, k->d_state, d_voff, dev_in, k->d_hs, q.d_s16, q.d_s16n, q.d_s32, q.d_s32n, q.d_vh, q.d_vnew,
                 k->nchan, k->g.chunk, k->g.hist, q.fs, q.vhist};
}

int acg_launch_frames(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const long long *d_voff, const int16_t *dev_in) {
  hipLaunchKernelGGL(acg_frames_kernel, dim3((k->nchan + kFvLanes - 1) / kFvLanes), dim3(kFvLanes), 0, st,
                     acg_args(k, d_tab, d_voff, dev_in));
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}

int acg_launch_advance(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const long long *d_voff) {
  hipLaunchKernelGGL(acg_advance_kernel, dim3((k->nchan + kFvLanes - 1) / kFvLanes), dim3(kFvLanes), 0, st,
                     acg_args(k, d_tab, d_voff, nullptr));
  JAMD_HIP(hipGetLastError());
  return JAMD_OK;
}
