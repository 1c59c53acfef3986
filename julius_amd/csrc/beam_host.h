// beam_host.h -- the host side of the first pass, laid out as every object's host layer: the lexicon
// (beam_lexicon_image.h: check and arena image, no device; beam_lexicon_api.hip: the C ABI; beam_lexicon.hip: the kernel that
// builds the cross-word LM table), the work area and the C ABI over it (beam_api.hip, no kernel), and the interfaces through
// which beam_api.hip reaches the kernels: beam.hip (the canonical-tie kernel K6, fbeam_*), beam_strict.hip (the strict-order
// cross-check, sbeam_*) and beam_exact.hip / beam_exact_layout.hip (the exact-order kernels and their LDS layout, xbeam_*
// in beam_exact.h).  Both objects own their device memory through jamd_host.h.  Internal, not installed.
#pragma once
#include <vector>

#include "beam_exact.h"
#include "beam_lexicon_image.h"

namespace jamdb {

// ---- beam_lexicon.hip: the cross-word LM table (LexDev::iwtab), nctx x niso floats at `tab`, built on `st` and waited for
JAMD_LOCAL hipError_t iwtab_build(const LexDev &lx, float *tab, int nctx, int niso, hipStream_t st);

// ---- beam.hip: the frame-parallel canonical-tie kernel (JAMD_ORDER_FAST)
// Fills the LDS image of `w` (survivor image, Viterbi cells, histogram) for beam width w->beam.
JAMD_LOCAL void fbeam_layout(Work *w);
JAMD_LOCAL hipError_t fbeam_prepare();
// smode 0: whole utterances; 1 / 2: a streaming push / the final one.  The score row joins the LDS image when it fits.
JAMD_LOCAL void fbeam_launch(const LexDev &lx, const Work &w, const float *scores, int nstate, const int *d_utt_off, int nutt,
                             int smode, bool timed, hipStream_t st);

// ---- beam_strict.hip: the sequential strict-order kernel (JAMD_ORDER_STRICT), one lane per utterance
struct STok;
struct StrictWork {            // what the kernel receives
  STok *tl[2];     // [utt][cap]   tlist[2]
  int *ti[2];      // [utt][cap]   tindex[2]
  int *token;      // [utt][nnode] node -> token id of the current list (-1 none)
  int cap;
};
struct JAMD_LOCAL StrictMem {  // ... and the memory behind it, made on first use (sized in beam_strict.hip alone)
  JamdDev<STok> tl[2];
  JamdDev<int> ti[2], token;
  StrictWork view{};
};
// Allocates the strict work area of `max_utts` utterances on first use.
JAMD_LOCAL int sbeam_prepare(StrictMem *sm, const Work &w, bool multipath, int max_utts);
JAMD_LOCAL void sbeam_launch(const LexDev &lx, const Work &w, const StrictWork &sw, bool multipath, const float *scores, int nstate,
                             const int *d_utt_off, int nutt, hipStream_t st);

}  // namespace jamdb

struct JAMD_LOCAL jamd_lexicon : jamdb::LexHost {
  int device = 0;                  // (the engine is not kept: it may go first)
  jamdb::LexDev d{};
  JamdDev<unsigned char> arena;    // d.base
  JamdDev<float> iwtab;            // d.iwtab, where there was room for it
};

struct JAMD_LOCAL jamd_beam {
  jamd_engine *eng = nullptr;
  int device = 0;                  // eng->device, for the destroy: the engine may have gone first
  jamd_lexicon *lex = nullptr;
  jamdb::Work w{};                 // its pointers are those of the owners below
  JamdDev<unsigned char> slices;
  JamdDev<jamd_pass1_result> res;
  JamdDev<jamdb::StreamState> stream;   // made by the first jamd_beam_stream_begin()
  int max_utts = 0;
  JamdDev<int> d_utt_off;          // [nutt + 1] row offsets, then [nutt] the launch order (see upload_utt_off())
  std::vector<int> h_utt_off;      // host image of the same (the copy is asynchronous)
  int order = JAMD_ORDER_FAST;     // the current JAMD_ORDER_* value: which kernel a launch goes to (XWork::prune_mode follows from it)
  int exact_status = -3;           // 0 = the exact-order kernel can serve this work area (xbeam_layout())
  jamdb::XWork xw{};
  jamdb::XWork xw_half{};          // the same work area for the half shape (two workgroups per CU), when it fits
  int half_status = -2;            // 0 = xw_half is usable
  int shape_mode = JAMD_SHAPE_AUTO;
  bool stream_half = false;        // the shape of the open streaming session (the parked state is the layout's)
  hipEvent_t ev_started = nullptr; // recorded right before the latest first-pass launch (jamd_beam_wait_started())
  JamdDev<unsigned> d_resident;    // signal memory: first-pass workgroups started so far (Work::resident), empty = the device cannot wait on memory
  unsigned resident_target = 0;    // its value once the workgroups of the latest launch that fit the device at once have started
  unsigned launched_wg = 0;        // workgroups of all launches so far
  // jamd_beam_prune_order() scratch for pcap tokens; d_parr: jamd_beam_prune_arrange()'s whole array, made on its first call
  JamdDev<unsigned> d_pkeys; JamdDev<int> d_pout, d_parr; size_t pcap = 0;
  bool timed = false;               // JAMD_BEAM_TIMING=1: launch the instrumented instantiation
  int streaming = 0;               // utterances of the open streaming session, 0 = none
  int stream_pushes = 0;
  std::vector<int> stream_frames;  // frames pushed so far per utterance of the session (limit 32767 each)
  jamdb::StrictMem sm;
  ~jamd_beam() { if (ev_started) (void)hipEventDestroy(ev_started); }
};
