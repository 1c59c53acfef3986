// adin_cut_plan.h -- what the silence cutting stage (jamd_adin_cut, adin_cut_api.hip) works out without a device: the
// parameters of adin_setup_param() (libjulius/src/adin-cut.c:171-185) in the reference's own arithmetic, the descriptor
// checks, the history a channel keeps and the closed-form bounds of what one push can deliver.
// Plain C++, no HIP header.
#pragma once
#include <cstdint>
#include <string>

#include "julius_amd.h"

constexpr int kAcMaxLen = 1 << 24;           // c_length, sbsize and chunk_size at the most (17 minutes at 16 kHz)

struct AcParams {
  int c_length, noise_zerocross, nc_max, sbsize;
  int hist;                                  // samples of the stream a channel keeps behind its newest
};

// Returns false with the reason in `err`.
static inline bool ac_params(const jamd_adin_cut_desc *d, AcParams &p, std::string &err) {
  if (!d) { err = "the descriptor is NULL"; return false; }
  if (d->sfreq <= 0) { err = "sfreq <= 0"; return false; }
  if (d->chunk_size < 1) { err = "chunk_size < 1"; return false; }
  if (d->head_margin_msec < 0 || d->tail_margin_msec < 0 || d->zero_cross_num < 0) {
    err = "a negative margin or zero-cross count";
    return false;
  }
  const float sim = (float)d->sfreq / (float)1000.0;         // samples_in_msec
  const float cl = (float)d->head_margin_msec * sim;
  const float tail = d->tail_margin_msec * sim;
  if (!(cl < (float)kAcMaxLen) || !(tail < (float)kAcMaxLen) || d->chunk_size > kAcMaxLen || d->zero_cross_num > kAcMaxLen) {
    err = "a margin, chunk_size or zero_cross_num beyond 2^24";
    return false;
  }
  p.c_length = (int)cl;
  if (d->chunk_size > p.c_length) {
    err = "chunk size (" + std::to_string(d->chunk_size) + ") > header margin (" + std::to_string(p.c_length) + ")";
    return false;
  }
  const long long zl = (long long)d->zero_cross_num * p.c_length;   // the reference multiplies in int
  if (zl > 0x7fffffffLL) { err = "zero_cross_num * c_length does not fit an int"; return false; }
  p.noise_zerocross = (int)(zl / d->sfreq);
  p.nc_max = (int)((float)(tail / (float)d->chunk_size)) + 2;
  const float sb = tail + (float)(int)(zl / 200);
  if (!(sb < (float)kAcMaxLen)) { err = "sbsize beyond 2^24"; return false; }
  p.sbsize = (int)sb;
  // Blocks of a tail are delivered while rest_tail (sbsize - c_length at first) lasts, the others, up to the nc_max-th,
  // go to the swap buffer: the reference writes past it where they do not fit ("swap buffer for re-triggering
  // overflow").  Refused here.
  const long long rest = (long long)p.sbsize - p.c_length, cs = d->chunk_size;
  const long long delivered = rest >= 0 ? (rest + cs - 1) / cs : -((-rest) / cs);   // ceil(rest / chunk_size)
  if (((long long)p.nc_max - delivered) * cs > p.sbsize) {
    err = "the tail would overflow the reference's swap buffer: (nc_max " + std::to_string(p.nc_max) + " - " +
          std::to_string(delivered) + " delivered blocks) * chunk_size " + std::to_string(d->chunk_size) + " > sbsize " +
          std::to_string(p.sbsize);
    return false;
  }
  p.hist = (p.c_length > p.sbsize ? p.c_length : p.sbsize) + d->chunk_size;
  return true;
}

// Frames of fs samples that fvad_proceed() can process in a push of n samples: the blocks the push walks cover less
// than n + chunk_size samples, and ceil(e / fs) - 1 grows by ceil(that / fs) at the most
constexpr long long ac_gate_frames_cap(long long n, int chunk_size, int fs) { return (n + chunk_size) / fs + 2; }

// Blocks a push of `chunk` samples can complete: the carry is below chunk_size, and end of stream adds one short block
static inline long long ac_blocks_cap(const jamd_adin_cut_desc *d, long long chunk) {
  return (chunk + d->chunk_size - 1) / d->chunk_size + 1;
}
// A segment that ends by silence spans its trigger block and nc_max blocks below the threshold, so triggers lie
// nc_max + 1 blocks apart, and so do ends; the first of either can fall into the push's first block.
static inline long long ac_events_cap(const jamd_adin_cut_desc *d, const AcParams &p, long long chunk) {
  return 1 + (ac_blocks_cap(d, chunk) - 1) / ((long long)p.nc_max + 1);
}
// Parts: one per end, and the part left open behind the last one
static inline long long ac_parts_cap(const jamd_adin_cut_desc *d, const AcParams &p, long long chunk) {
  return ac_events_cap(d, p, chunk) + 1;
}
// Samples: every sample the push's blocks cover goes out once at the most as a block or out of the swap buffer
// (chunk + chunk_size - 1 with a full carry), the swap buffer may hold sbsize from before the push, and every trigger
// delivers a head margin below c_length -- the second and later ones of a push deliver again what the tail of the
// segment before has delivered.
static inline long long ac_push_cap(const jamd_adin_cut_desc *d, const AcParams &p, long long chunk) {
  return chunk + (d->chunk_size - 1) + p.sbsize + ac_events_cap(d, p, chunk) * p.c_length;
}
