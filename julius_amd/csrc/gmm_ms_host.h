// gmm_ms_host.h -- the host side of multi-stream GMM scoring: the model object, which gmm_ms_api.hip builds and owns
// (validation, packing, the C ABI of jamd_gmm_ms), and the launchers through which it reaches the kernels (gmm_ms.hip,
// K1m; gmm_ms_tied.hip, K1mt).  gmm_ms_api.hip launches nothing itself.  Internal, not installed.
#pragma once
#include "jamd_host.h"

// One mixture pdf / one stream as the kernel reads them (two ints each, one 8-byte scalar load).
struct JamdMsPdf { int rec; int n; };        // first float of the pdf's records in d_rec, mixture entries
struct JamdMsStream { int off; int len; };   // the stream's slice of the input vector

// K1mt.  A CACHED pdf is scored from the per-(frame, book) cache: a tied-mixture pdf from its codebook's column, and
// under gprune safe a plain pdf from a column of its own (a "book" nobody shares, whose list never has a history).
struct JamdMsBook { int rec; int n; int off; int len; };     // records in d_rec, members, the slice of its stream
struct JamdMsTpdf { int book; int ent; int nmax; int pad; }; // cache column (-1: not cached), first entry in d_ent_logw,
                                                             //   min(cap, members): the slots a frame can hold
// The runs of frames one launch of the order pass walks, chunk-local: frames first .. end - 1, each of which has a
// predecessor in the same utterance (cache row `frame`: row 0 is the last frame of the chunk before).
constexpr int kJamdMsSegs = 64;
struct JamdMsSegs { int first[kJamdMsSegs]; int end[kJamdMsSegs]; };

struct JAMD_LOCAL jamd_gmm_ms {
  jamd_engine *eng = nullptr;
  int S = 0, D = 0, nstream = 0, npdf = 0;
  // device model, written once by jamd_gmm_ms_create(); no call writes any of it
  JamdDev<float> d_rec;            // per pdf, its entries back to back: mean[len] | ivar[len] | gconst | ln w, padded to 4
                                   //   floats (len = the pdf's stream's vsize; a NULL density has gconst = NaN); K1mt: the
                                   //   books' members after them, in the same form
  JamdDev<JamdMsPdf> d_pdf;        // [npdf]
  JamdDev<JamdMsStream> d_stream;  // [nstream]
  JamdDev<int> d_st_pdf;           // [S][nstream]
  JamdDev<float> d_st_w;           // [S][nstream]
  size_t dyn_lds = 0;              // the kernel's dynamic LDS (the block's frames, transposed), reserved once at create
  JamdStage<float, float> stage;   // outprob_host
  char last_kernel[96] = {0};

  // ---- K1mt (jamd_gmm_ms_create_opt() with a tied-mixture pdf, or gprune safe); cached == false: none of it is used
  bool cached = false;
  int gprune = 0, cap = 0, chunk = 0;   // JAMD_GPRUNE_NONE | _SAFE; cache slots per (frame, book); frames per chunk
  int nbook = 0, nbook_all = 0;         // codebooks of the model; with the plain pdfs' own columns after them (safe)
  int maxbook = 0, maxlen = 0;          // members of the largest book that has a history; longest slice of any book
  bool has_plain = false;               // some pdf is scored by K1m's loop (gprune none): the state kernel holds the frames
  JamdDev<JamdMsBook> d_book;           // [nbook_all]
  JamdDev<JamdMsTpdf> d_tpdf;           // [npdf]
  JamdDev<float> d_ent_logw;            // [nentry] bweight / ln w of the cached pdfs' entries
  // device scratch a call writes, chunk + 1 rows innermost: row 0 carries the last frame of the chunk before
  JamdDev<float> d_c_score;             // [nbook_all][cap][chunk + 1]
  JamdDev<int> d_c_id;                  // [nbook_all][cap][chunk + 1]
  JamdDev<int> d_c_num, d_c_flag;       // [nbook_all][chunk + 1]
  size_t dyn_book = 0, dyn_order = 0, dyn_state = 0;
};

// floats of one Gaussian record of a stream of `len` dimensions
static inline int jamd_ms_rec(int len) { return ((2 * len + 2) + 3) & ~3; }

// ---- gmm_ms.hip
// Once per model, from jamd_gmm_ms_create(): the LDS the kernel needs for this vector length (refused when a CU does
// not have it), so that the stream-ordered call asks the runtime nothing.
JAMD_LOCAL int jamd_gmm_ms_setup(jamd_gmm_ms *g);
// Every state of T frames: K1m.
JAMD_LOCAL int jamd_gmm_ms_launch(jamd_gmm_ms *g, const float *frames, int T, float *out, hipStream_t st);

// ---- gmm_ms_tied.hip
// Once per model with cached pdfs: the LDS of its three kernels, as jamd_gmm_ms_setup().
JAMD_LOCAL int jamd_gmm_ms_tied_setup(jamd_gmm_ms *g);
// K1mt over the frames of nutt utterances (utt_off: host, checked by the caller), chunk by chunk on `st`: the cache,
// under gprune safe its marked frames again in the reference's order, then every state into out.  out == nullptr: the
// cache of the model's codebooks goes to o_score / o_id [T][nbook][cap] and o_num [T][nbook] instead.
JAMD_LOCAL int jamd_gmm_ms_tied_launch(jamd_gmm_ms *g, const float *frames, const int *utt_off, int nutt, float *out,
                                       float *o_score, int *o_id, int *o_num, hipStream_t st);
