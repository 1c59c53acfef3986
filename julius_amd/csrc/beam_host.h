// beam_host.h -- the host side of the first pass: the lexicon (beam_lexicon.hip), the work area and the C ABI over it
// (beam_api.hip), and the interfaces through which beam_api.hip reaches the kernels: beam.hip (the canonical-tie kernel
// K6, fbeam_*), beam_strict.hip (the strict-order cross-check, sbeam_*) and beam_exact.hip / beam_exact_layout.hip (the exact-order
// kernels and their LDS layout, xbeam_* in beam_exact.h).  Internal, not installed.
#pragma once
#include <vector>

#include "beam_exact.h"

namespace jamdb {

// ---- beam.hip: the frame-parallel canonical-tie kernel (JAMD_ORDER_FAST)
// Fills the LDS image of `w` (survivor image, Viterbi cells, histogram) for beam width w->beam.
void fbeam_layout(Work *w);
hipError_t fbeam_prepare();
// smode 0: whole utterances; 1 / 2: a streaming push / the final one.  The score row joins the LDS image when it fits.
void fbeam_launch(const LexDev &lx, const Work &w, const float *scores, int nstate, const int *d_utt_off, int nutt,
                  int smode, bool timed, hipStream_t st);

// ---- beam_strict.hip: the sequential strict-order kernel (JAMD_ORDER_STRICT), one lane per utterance
struct STok;
struct StrictWork {
  STok *tl[2];     // [utt][cap]   tlist[2]
  int *ti[2];      // [utt][cap]   tindex[2]
  int *token;      // [utt][nnode] node -> token id of the current list (-1 none)
  int cap;
};
// Allocates the strict work area of `max_utts` utterances on first use; the device memory is appended to `owned`.
int sbeam_prepare(StrictWork *sw, const Work &w, bool multipath, int max_utts, std::vector<void *> &owned);
void sbeam_launch(const LexDev &lx, const Work &w, const StrictWork &sw, bool multipath, const float *scores, int nstate,
                  const int *d_utt_off, int nutt, hipStream_t st);

}  // namespace jamdb

struct jamd_lexicon {
  jamd_engine *eng = nullptr;
  jamdb::LexDev d{};
  int maxfan = 2, nscword = 0;
  bool multipath = false;          // JAMD_LM_MULTIPATH lexicon: its own frame (beam_exact_mp.h; strict order: beam_strict_kernel<true>)
  bool mp_parallel = false;        // ... and no root reaches a word-end node along its own arcs: the frame-parallel kernel can decode it
  // multipath: where a token entering a word goes (the root has no output: beam.c:2467-2510) -- one int4 {target node,
  // transition bits, root number * maxfan + transition number, root number / fscore bits} per transition a root really has,
  // in visiting order; byte offsets into the lexicon arena + entry counts (XWork carries them to the kernel)
  unsigned o_mp_iso = 0, o_mp_shared = 0, o_mp_start = 0;
  int n_mp_iso = 0, n_mp_shared = 0, n_mp_start = 0;
  // ... and the nodes those transitions lead to, numbered densely: int [nnode], -1 = never entered from a root.  Only such a
  // node can meet a token of the frame's second half, so the per-utterance "which token sits on this node" table of the
  // multipath frame (XWork::o_nodetok) has n_mp_tgt entries instead of nnode (a few KB that stay in L2 instead of a
  // megabyte per utterance written four bytes at a time).
  unsigned o_mp_tgt = 0;
  int n_mp_tgt = 0;
  std::vector<void *> owned;
};

struct jamd_beam {
  jamd_engine *eng = nullptr;
  jamd_lexicon *lex = nullptr;
  jamdb::Work w{};
  int max_utts = 0;
  int *d_utt_off = nullptr;        // [nutt + 1] row offsets, then [nutt] the launch order (see upload_utt_off())
  std::vector<int> h_utt_off;      // host image of the same (the copy is asynchronous)
  int order = JAMD_ORDER_FAST;     // the current JAMD_ORDER_* value: which kernel a launch goes to (XWork::prune_mode follows from it)
  int exact_status = -3;           // 0 = the exact-order kernel can serve this work area (xbeam_layout())
  jamdb::XWork xw{};
  jamdb::XWork xw_half{};          // the same work area for the half shape (two workgroups per CU), when it fits
  int half_status = -2;            // 0 = xw_half is usable
  int shape_mode = JAMD_SHAPE_AUTO;
  bool stream_half = false;        // the shape of the open streaming session (the parked state is the layout's)
  hipEvent_t ev_started = nullptr; // recorded right before the latest first-pass launch (jamd_beam_wait_started())
  int *d_parr = nullptr;           // jamd_beam_prune_arrange(): the whole array
  unsigned *d_resident = nullptr;  // signal memory: first-pass workgroups started so far (Work::resident), nullptr = the device cannot wait on memory
  unsigned resident_target = 0;    // its value once the workgroups of the latest launch that fit the device at once have started
  unsigned launched_wg = 0;        // workgroups of all launches so far
  unsigned *d_pkeys = nullptr; int *d_pout = nullptr; size_t pcap = 0;   // jamd_beam_prune_order() scratch
  bool timed = false;               // JAMD_BEAM_TIMING=1: launch the instrumented instantiation
  int streaming = 0;               // utterances of the open streaming session, 0 = none
  int stream_pushes = 0;
  std::vector<int> stream_frames;  // frames pushed so far per utterance of the session (limit 32767 each)
  jamdb::StrictWork sw{};
  std::vector<void *> owned;
};
