// adin_cut_host.h -- the host side of the silence cutting stage (jamd_adin_cut): the object, which adin_cut_api.hip
// builds and owns (validation, the table of a push, scratch, the C ABI), and the launchers through which it reaches the
// kernels in adin_cut.hip.  The API unit launches nothing itself; a launcher checks nothing.  What needs no device is in
// adin_cut_plan.h.  Internal, not installed.
#pragma once
#include "jamd_host.h"
#include "adin_cut_plan.h"
#include "fvad_host.h"

// One channel between pushes.  `pos` counts the samples given since the last reset; the last `carried` of them wait for
// their block to fill.  count_zc_e() runs ahead of the blocks: `trig` (is_trig * 2 + (sign == ZC_NEGATIVE)) and `cum`
// (crossings so far, modulo 2^32) stand behind sample pos - 1, `zc` is the count the last block returned.
struct AcState { long long pos; unsigned cum; int trig, is_valid, nc, rest_tail, sblen, zc, carried; };
// One channel in a push: n samples at src_off of the input, their running counts at cnt_off of the scratch
struct AcChanTab { long long src_off, cnt_off; int n, eos; };
// The numbers the kernels take
struct AcDev { int trigger, chunk, c_length, noise_zc, nc_max, sbsize, hist, nchan; };

// What the blocks kernel reads of the gate (-fvad): V[k] of this push at vnew[voff[c] + k - F0 - 1], older in the ring
struct AcGateDev { const unsigned *vnew, *vh; const long long *voff; int fs, N, cmin, vhist; };
// Frames fvad_proceed() has processed by the ends of the last block before a push and of the last block the push walks
struct AcGateSpan { long long F0, F1; };
#if defined(__HIPCC__)
__device__ __forceinline__ AcGateSpan ac_gate_span(const AcState &s, const AcChanTab &t, int chunk, int fs) {
  const long long e0 = s.pos - s.carried, avail = s.carried + (long long)t.n;
  const long long e1 = t.eos ? e0 + avail : e0 + avail / chunk * chunk;   // (end of stream: the short last block too)
  AcGateSpan g{fv_gate_frames(e0, fs), fv_gate_frames(e1, fs)};
  const long long cap = ac_gate_frames_cap(t.n, chunk, fs);               // (what the host made room for)
  if (g.F1 - g.F0 > cap) g.F1 = g.F0 + cap;
  return g;
}
#endif

constexpr int kAcTile = 1024;                // samples per step of the scan workgroup
constexpr int kAcCopyTile = 2048;            // samples per workgroup of the gather

// What a push leaves on the device for the host, one allocation, one copy: the part count, then for `cap` parts
// part_off [cap][nchan + 1], part_start [cap][nchan] (int64 each), part_final [cap][nchan] (bytes).
struct AcTabs {
  long long *nparts, *off, *start;
  unsigned char *fin;
};
static inline size_t ac_tabs_bytes(int nchan, int cap) {
  return sizeof(long long) * (1 + (size_t)cap * (nchan + 1) + (size_t)cap * nchan) + (size_t)cap * nchan;
}
static inline AcTabs ac_tabs_at(void *base, int nchan, int cap) {
  AcTabs t;
  t.nparts = (long long *)base;
  t.off = t.nparts + 1;
  t.start = t.off + (size_t)cap * (nchan + 1);
  t.fin = (unsigned char *)(t.start + (size_t)cap * nchan);
  return t;
}

struct JAMD_LOCAL jamd_adin_cut {
  jamd_engine *eng = nullptr;
  jamd_adin_cut_desc d{};
  AcParams p{};
  AcDev g{};
  int nchan = 0;
  JamdDev<AcState> d_state, d_next;          // [nchan]: between pushes; what the push in flight will leave
  JamdDev<int16_t> d_hs;                     // [nchan][hist] stream sample q in slot q % hist
  JamdDev<unsigned> d_hc;                    // [nchan][hist] crossings among samples 0 ... q, likewise
  JamdDev<int> d_strig;                      // [nchan] count_zc_e()'s state behind the push's last sample
  JamdDev<unsigned> d_scum;                  // [nchan]
  JamdDev<unsigned char> d_mask;             // [nchan]
  // scratch of a push
  JamdDev<unsigned> d_cnt;                   // the running count behind every new sample
  JamdDev<long long> d_pa;                   // [cap][nchan] where in the stream a part's range begins
  JamdDev<int> d_pl;                         // [cap][nchan] its length
  JamdDev<int> d_used;                       // [nchan] parts the channel needs
  JamdDev<char> d_tabs;                      // AcTabs
  JamdHostBuf h_tabs;                        // the same, brought down
  JamdPinned tab;                            // AcChanTab [nchan]
  JamdStage<int16_t, int16_t> stage;         // push_host
  std::unique_ptr<FvGate> gate;              // -fvad: only where jamd_adin_cut_create_fvad() made the object
};

// ---- adin_cut.hip
// count_zc_e() over every channel's new samples -> k->d_cnt, k->d_strig / d_scum; the blocks of every channel ->
// k->d_next, the parts' ranges (k->d_pa / d_pl / d_used) and flags; the part-major offsets and the part count -> `t`
// (on the device, `cap` parts of room).  Moves no state.
JAMD_LOCAL int ac_launch_plan(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const int16_t *dev_in, AcTabs t,
                                 int cap);
// The ranges of nparts parts, none longer than max_len (> 0), -> dev_out
JAMD_LOCAL int ac_launch_gather(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const int16_t *dev_in, AcTabs t,
                                   int cap, int nparts, int max_len, int16_t *dev_out);
// After everything has read the old history: the new samples and counts enter it, k->d_next becomes k->d_state
JAMD_LOCAL int ac_launch_advance(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const int16_t *dev_in);
// The channels d_mask names (NULL: all) back to the start
JAMD_LOCAL int ac_launch_reset(jamd_adin_cut *k, hipStream_t st, const unsigned char *d_mask);

// ---- adin_cut_fvad.hip (objects with k->gate only)
// Ahead of ac_launch_plan(): the detector over the frames that fvad_proceed() has seen by the end of the last block
// this push walks, from k->gate->d_s16 / d_s32 into the next copies, their running speech count -> k->gate->d_vnew at
// d_voff[c].  Moves no state.
JAMD_LOCAL int acg_launch_frames(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const long long *d_voff,
                                    const int16_t *dev_in);
// Ahead of ac_launch_advance(), which ends the push: the next cores become the channels', the newest counts enter the ring
JAMD_LOCAL int acg_launch_advance(jamd_adin_cut *k, hipStream_t st, const AcChanTab *d_tab, const long long *d_voff);
