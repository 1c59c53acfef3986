/*
 * julius_amd.h -- C ABI of the MI355X (gfx950) engine for Julius' frame-
 * synchronous first pass: acoustic scoring (GMM / tied-mixture / DNN) and
 * first-pass token passing.  Plain pointers and sizes only; no torch, no
 * reference types.  The reference-side binding (a C shim compiled inside the
 * Julius tree that flattens HTK_HMM_INFO / DNNData / WCHMM_INFO and exports the
 * reference's own symbols) is julius_amd/shim/ and is described in
 * INTEGRATION.md.  All paths cited below are relative to the reference root.
 *
 * Conventions
 *   - every entry point returns 0 on success and a negative JAMD_E* code on
 *     failure; jamd_last_error() returns a message for the calling thread.
 *     (The reference's boolean/LOG_ZERO error returns are produced by the shim
 *     from these codes.)
 *   - "host" pointers are ordinary process memory, "dev" pointers are HIP device
 *     memory on the engine's device; `stream` is a hipStream_t passed as void*
 *     (NULL = the engine's own stream).
 *   - scores are fp32 log10 likelihoods exactly as LOGPROB in
 *     libsent/include/sent/stddefs.h:194; LOG_ZERO = -1000000 (:171).
 *   - an engine object is not re-entrant (neither is HMMWork,
 *     libsent/include/sent/hmm_calc.h:90-111); use one per thread/stream.
 */
#ifndef JULIUS_AMD_H
#define JULIUS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JAMD_ABI_VERSION 4

#define JAMD_OK        0
#define JAMD_EINVAL   -1   /* bad argument / unsupported model feature        */
#define JAMD_ENODEV   -2   /* no usable gfx950 device / HIP runtime failure   */
#define JAMD_ENOMEM   -3
#define JAMD_ELAUNCH  -4   /* kernel launch or execution failed               */
#define JAMD_ESTATE   -5   /* call sequence violation                         */

#define JAMD_LOG_ZERO (-1000000.0f)

/* Gaussian pruning selector (GPRUNE_SEL_*, libsent/include/sent/hmm_calc.h:38-45).  All four are served for
 * every model.  heu and beam prune with thresholds taken from the N best Gaussians of the PREVIOUS frame's
 * codebook cache (last_id), which exists only for tied-mixture codebooks (calc_tied_mix.c:203-215).  For plain
 * mixture states calc_mix() passes last_id == NULL (calc_mix.c:63), where both functions ARE safe pruning
 * (gprune_heu.c:337-350, gprune_beam.c:337-350).  For tied-mixture codebooks the previous frame's cache depends, in
 * the reference, on which frames its lazy search happened to score; the device scores every state of every frame,
 * so its results are the reference's under eager scoring (outprob_set_batch_computation(), outprob.c:230-242) --
 * bit for bit, cache contents included -- and an utterance's first frame takes the no-history branch. */
#define JAMD_GPRUNE_NONE 0  /* gprune_none()  libsent/src/phmm/gprune_none.c:133 */
#define JAMD_GPRUNE_SAFE 1  /* gprune_safe()  libsent/src/phmm/gprune_safe.c:160 */
#define JAMD_GPRUNE_HEU  2  /* gprune_heu()   gprune_heu.c:295  (tied-mixture codebooks: parity under eager scoring) */
#define JAMD_GPRUNE_BEAM 3  /* gprune_beam()  gprune_beam.c:291 (ditto) */

/* pseudo-phone set reduction (hmminfo->cdset_method, htk_hmm.h:388) */
#define JAMD_IWCD_MAX   0   /* outprob_cd_max   libsent/src/phmm/outprob.c:332 */
#define JAMD_IWCD_AVG   1   /* outprob_cd_avg   outprob.c:356 */
#define JAMD_IWCD_NBEST 2   /* outprob_cd_nbest outprob.c:287 */

typedef struct jamd_engine jamd_engine;
typedef struct jamd_gmm    jamd_gmm;
typedef struct jamd_cdset  jamd_cdset;
typedef struct jamd_dnn    jamd_dnn;

/* ------------------------------------------------------------------ engine */
int         jamd_abi_version(void);
const char *jamd_last_error(void);
int         jamd_device_count(void);

/* Create an engine on HIP device `device`.  Builds the addlog table of
 * make_log_tbl() (libsent/src/phmm/addlog.c:42) and the logistic table of
 * logistic_table_build() (libsent/src/phmm/calc_dnn.c:349) on the host with the
 * same libm expressions and uploads them.  Replaces the table part of
 * outprob_init() (libsent/src/phmm/outprob_init.c:161). */
int  jamd_engine_create(int device, jamd_engine **out);
void jamd_engine_destroy(jamd_engine *e);
int  jamd_engine_device(const jamd_engine *e);
int  jamd_engine_sync(jamd_engine *e);
/* Device allocation helpers for callers without their own HIP runtime. */
int  jamd_malloc(jamd_engine *e, size_t bytes, void **dev);
int  jamd_free(jamd_engine *e, void *dev);
/* Page-locked host memory: copies to and from it run at the PCIe rate instead of the pageable-memory rate
 * (about 3x); the bindings keep the score rows they hand to Julius' outprob cache in such buffers. */
int  jamd_host_alloc(jamd_engine *e, size_t bytes, void **host);
int  jamd_host_free(jamd_engine *e, void *host);
int  jamd_memcpy_h2d(jamd_engine *e, void *dev, const void *host, size_t bytes);
int  jamd_memcpy_d2h(jamd_engine *e, void *host, const void *dev, size_t bytes);
/* Streams for callers without their own HIP runtime (the `stream` arguments below take any hipStream_t): a batch
 * driver scores input k+1 on one stream while the first pass of input k runs on another -- the first pass keeps
 * one workgroup per utterance busy, the scoring kernels fill whatever CUs that leaves (host/jamd_batch.c).
 * jamd_stream_wait(): everything submitted to `waiter` after the call starts only when everything submitted to
 * `signaler` before the call is done (an event record + wait; NULL = the engine's own stream).
 * Two things such a driver has to know: (1) the first pass must be ON the device before the next input's scoring is
 * queued (jamd_beam_wait_started() below), or the scoring workgroups take the LDS it is waiting for; (2) the ROCm
 * runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) in creation order, and two streams
 * on one queue run one after the other -- a process that creates many streams raises that limit before its first HIP
 * call (jamd_batch and bench.py set 16). */
int  jamd_stream_create(jamd_engine *e, void **stream);
int  jamd_stream_destroy(jamd_engine *e, void *stream);
int  jamd_stream_wait(jamd_engine *e, void *waiter, void *signaler);
int  jamd_stream_sync(jamd_engine *e, void *stream);
int  jamd_memcpy_h2d_async(jamd_engine *e, void *dev, const void *host, size_t bytes, void *stream);

/* --------------------------------------------------------------- GMM model */
/* Flattened HTK_HMM_INFO (libsent/include/sent/htk_hmm.h:330-420) after
 * outprob_init() has inverted the variances (outprob_init.c:74-79):
 *   densities   mean[ndens][veclen], ivar[ndens][veclen], gconst[ndens]
 *               (HTK_HMM_Dens, htk_hmm.h:120-131; gconst as computed by
 *               libsent/src/hmminfo/rdhmmdef_dens.c:39-48)
 *   states      st_off[nstate+1] into the entry arrays, in HTK_HMM_State.id order
 *   entries     ent_dens[nentry] (density index, -1 for a NULL density),
 *               ent_logw[nentry] (bweight = ln w, rdhmmdef_mpdf.c:189)
 *   st_book     [nstate] codebook id of a tied-mixture state (its entries list
 *               the GCODEBOOK's densities in codebook order, htk_hmm.h:196-201),
 *               -1 for a plain state; may be NULL when nbook == 0.
 * Single-stream models only (nstream must be 1; multi-stream -> JAMD_EINVAL). */
typedef struct {
  int nstate, veclen, ndens, nentry, nbook, nstream;
  const float *mean, *ivar, *gconst;
  const int   *st_off;
  const int   *ent_dens;
  const float *ent_logw;
  const int   *st_book;
} jamd_gmm_desc;

/* Replaces outprob_init()'s selection of compute_gaussset/calc_outprob
 * (outprob_init.c:99-147): gprune = JAMD_GPRUNE_*, gprune_num = -tmix /
 * OP_gprune_num (ignored for NONE).  Uploads the model in the engine's device
 * layout (DESIGN.md "HBM layout"). */
int  jamd_gmm_create(jamd_engine *e, const jamd_gmm_desc *d, int gprune, int gprune_num,
                     jamd_gmm **out);
/* The same from a "JAMDGMM1" file: the flattened model as jamd_gmm_save()
 * (julius_amd/shim/jamd_flatten.c) wrote it from the HTK_HMM_INFO that Julius' own
 * hmmdefs / binhmm reader (libsent/src/hmminfo/rdhmmdef.c, read_binhmm.c) built.
 * For workers that never link Julius. */
int  jamd_gmm_load(jamd_engine *e, const char *path, int gprune, int gprune_num, jamd_gmm **out);
void jamd_gmm_destroy(jamd_gmm *g);
int  jamd_gmm_nstate(const jamd_gmm *g);
int  jamd_gmm_veclen(const jamd_gmm *g);

/* Score every state for frames 0..T-1: out[t][s] = log10 b_s(o_t), the values
 * outprob_state() (libsent/src/phmm/outprob.c:184) would cache in
 * outprob_cache[t][s] via calc_mix() (calc_mix.c:41) / calc_tied_mix()
 * (calc_tied_mix.c:162) with the batch loop outprob.c:230-242.
 * frames is [T][veclen] row-major, out is [T][nstate] row-major (the
 * outprob_cache layout, outprob.c:127-129).
 * The model's device scratch (the per-Gaussian scores of a call of at most 256 frames, the codebook cache of a
 * tied-mixture model, the staged utterance boundaries, the eight ticket heads from which the waves of a long call's
 * scoring kernel draw their tiles, zeroed on `stream` ahead of it) is reused by every call: calls on one jamd_gmm must not be in
 * flight on two streams at once -- queue them on one stream (they are then ordered), or use one object per stream.
 * The first call of at most 256 frames allocates its scratch (256 x the model's mixture entries, floats); a growing
 * codebook cache allocates as well: such a call is not free of device allocation. */
int  jamd_gmm_outprob_dev(jamd_gmm *g, const float *dev_frames, int T, float *dev_out,
                          void *stream);
/* The same for a BATCH of utterances laid back to back: utterance u owns frames utt_off[u]..utt_off[u+1]) (utt_off is
 * a HOST array of nutt+1 ints, utt_off[0] = 0).  The boundaries matter to one configuration only: gprune heu / beam
 * over tied-mixture codebooks, whose thresholds at frame t come from the codebook's winners at frame t-1 of the SAME
 * input (calc_tied_mix.c:203-215; outprob_prepare() clears the cache per input, outprob.c:138-166);
 * jamd_gmm_outprob_dev() treats its T frames as one utterance. */
int  jamd_gmm_outprob_utts_dev(jamd_gmm *g, const float *dev_frames, const int *utt_off, int nutt, float *dev_out,
                               void *stream);
/* Same with host buffers (packs HTK_Param rows, uploads, scores, downloads). */
int  jamd_gmm_outprob_host(jamd_gmm *g, const float *host_frames, int T, float *host_out);
/* Tied-mixture codebook cache of calc_tied_mix.c:189-227 for inspection: top-N
 * (score,id) per (frame, codebook), descending, as MIXCACHE (hmm_calc.h:57-60).
 * dev_score/dev_id are [T][nbook][jamd_gmm_tmix_cap()]; dev_num [T][nbook]. */
int  jamd_gmm_tmix_cache_dev(jamd_gmm *g, const float *dev_frames, int T,
                             float *dev_score, int *dev_id, int *dev_num, void *stream);
/* Slots per (frame, codebook) of that cache (gprune_num for safe, the largest
 * codebook for none; 0 when the model has no tied-mixture state) and the
 * codebook count. */
int  jamd_gmm_tmix_cap(const jamd_gmm *g);
int  jamd_gmm_nbook(const jamd_gmm *g);
/* Name of the kernel variant the last outprob call used ("tile<39,2>", ...). */
const char *jamd_gmm_last_kernel(const jamd_gmm *g);
/* Per-Gaussian scores for Julius' official plugin slot (compute_gaussset: calcmix(),
 * plugin/calcmix.c:86-323): out[t][e] = (gconst_e + sum_d (o_td - mean_ed)^2 * ivar_ed) * -0.5
 * for every mixture entry e (state order, e = st_off[s] + i for component i of state s), LOG_ZERO
 * for a NULL density -- what the sample plugin's calcmix() stores in OP_calced_score[i]; calc_mix()
 * then adds the weights and takes the log-sum itself.  out is [T][jamd_gmm_nentry()] row-major.
 * Single-stream models whose states are all plain or all tied-mixture. */
int  jamd_gmm_nentry(const jamd_gmm *g);
/* For a model whose states are all tied-mixture the columns are the codebook Gaussians instead
 * (what calc_tied_mix() sends through the slot: book->d, libsent/src/phmm/calc_tied_mix.c:189-227):
 * column jamd_gmm_book_offsets()[b] + k is Gaussian k of codebook b; off receives nbook + 1 ints. */
int  jamd_gmm_book_offsets(const jamd_gmm *g, int *off, int cap);
int  jamd_gmm_dens_dev(jamd_gmm *g, const float *dev_frames, int T, float *dev_out, void *stream);
int  jamd_gmm_dens_host(jamd_gmm *g, const float *host_frames, int T, float *host_out);

/* ---------------------------------------------------- multi-stream GMM model */
/* HTK_HMM_INFO of a model with opt.stream_info.num > 1 (`~o <StreamInfo> n v1 .. vn`), after outprob_init() has
 * inverted the variances: what calc_mix() (libsent/src/phmm/calc_mix.c:41-81) walks for one state -- OP_nstream
 * mixture pdfs, each over its own slice of the input vector (outprob.c:199-203), the streams' log-sums joined as
 * sum_s weight[s] * logprob_s.  jamd_gmm_create() and its kin keep refusing nstream != 1; such a model has this
 * object of its own.  A single-stream model (nstream = 1) is accepted too and scores as jamd_gmm does.
 *   nstate, veclen   states (HTK_HMM_State.id order, htk_hmm.h:171-178) and opt.vec_size (htk_hmm.h:104)
 *   nstream          opt.stream_info.num, 1 .. 50 (MAXSTREAMNUM, htk_defs.h:112; HTK_HMM_StreamInfo, htk_hmm.h:96-99)
 *   vsize            [nstream] opt.stream_info.vsize[]; sums to veclen.  Stream s sees o[off_s .. off_s + vsize[s]),
 *                    off_s = vsize[0] + .. + vsize[s - 1]
 *   mixture pdfs     the pool of HTK_HMM_PDF (htk_hmm.h:157-165); a `~p` macro shared by several states is ONE pdf.
 *                    pdf_stream[npdf]   stream_id (:160)
 *                    pdf_off[npdf + 1]  the pdf's mixture entries in ent_dens / ent_logw (mix_num = the difference)
 *                    pdf_book[npdf]     codebook id of a tied-mixture pdf (tmix, :159), -1 for a plain one; NULL = all
 *                                       plain.  The ids are dense, 0 .. nbook - 1 (GCODEBOOK.id).  The entries of a
 *                                       tied-mixture pdf name its codebook's densities d[0 .. num) in order (-1 for a
 *                                       member the file leaves undefined) and carry its bweight: every pdf of a book
 *                                       lists the same ent_dens and has the same pdf_stream.  jamd_gmm_ms_create()
 *                                       refuses a tied-mixture pdf; jamd_gmm_ms_create_opt() serves it
 *   entries          ent_dens[nentry]   density index (b[i], :162), -1 for a NULL density
 *                    ent_logw[nentry]   bweight[i] = ln w (:163, rdhmmdef_mpdf.c:189)
 *   states           st_pdf[nstate][nstream]     pdf index of stream s (HTK_HMM_State.pdf[s], :175)
 *                    st_weight[nstate][nstream]  stream weights (HTK_HMM_State.w->weight[s], :174, :142-147); 1.0 for
 *                                                a state without <SWeights> (calc_mix.c:54-55); NULL = all 1.0
 *   densities        HTK_HMM_Dens (:128-139) of DIFFERENT lengths: density g is as long as the stream that uses it
 *                    dens_off[ndens + 1]  into mean / ivar (floats; length = the difference)
 *                    mean, ivar           [dens_off[ndens]] values back to back; gconst[ndens]
 * Arithmetic, bit for bit the reference's x86-64 object code: per Gaussian gconst, then for the slice's dimensions
 * ascending four separately rounded fp32 operations, * -0.5 (LOG_ZERO for a NULL density), + ln w; addlog_array() from
 * the pdf's last entry to its first; a stream at or below LOG_ZERO is skipped, any other adds logprob * weight (a
 * rounded multiply, then a rounded add, from 0.0f); 0 or <= LOG_ZERO gives LOG_ZERO, anything else * INV_LOG_TEN.
 * jamd_gmm_ms_create() is `-gprune none` over plain mixtures; tied-mixture codebooks and `-gprune safe` are
 * jamd_gmm_ms_create_opt()'s (below).
 * NOT SERVED (JAMD_EINVAL): gprune heu | beam for multi-stream objects; multi-stream models at the shim / plugin
 * boundaries (jamd_flatten_hmminfo() refuses them, julius_amd/shim/jamd_flatten.c:109); MSD. */
typedef struct jamd_gmm_ms jamd_gmm_ms;
typedef struct {
  int nstate, veclen, nstream;
  int npdf, nentry, ndens;
  const int   *vsize;
  const int   *pdf_stream;
  const int   *pdf_off;
  const int   *pdf_book;
  const int   *ent_dens;
  const float *ent_logw;
  const int   *st_pdf;
  const float *st_weight;
  const int   *dens_off;
  const float *mean, *ivar, *gconst;
} jamd_gmm_ms_desc;

/* Checks the whole description before the first device call (a refusal names the field and costs no upload), then
 * packs every pdf's Gaussians in the order the kernel reads them and uploads once. */
int  jamd_gmm_ms_create(jamd_engine *e, const jamd_gmm_ms_desc *d, jamd_gmm_ms **out);
/* The same from the binary HMM definition mkbinhmm writes for such a model (read_binhmm.c: stream_info :261, the
 * stream weights :445, stream_id per `~p` macro :588, nstream pdf ids and a weight id per state :633-690). */
int  jamd_gmm_ms_load_binhmm(jamd_engine *e, const char *binhmm_path, jamd_gmm_ms **out);
void jamd_gmm_ms_destroy(jamd_gmm_ms *g);
int  jamd_gmm_ms_nstate(const jamd_gmm_ms *g);
int  jamd_gmm_ms_veclen(const jamd_gmm_ms *g);
int  jamd_gmm_ms_nstream(const jamd_gmm_ms *g);
/* out[t][s] = log10 b_s(o_t) for frames [T][veclen] -> [T][nstate], both row-major: the matrix jamd_cdset_*,
 * jamd_beam_pass1_dev() and jamd_beam_stream_push_dev() take.  An object made by jamd_gmm_ms_create() keeps no device scratch that a
 * call writes: calls on it may be in flight on several streams at once (for jamd_gmm_ms_create_opt()'s see there).  (_host stages through buffers the object
 * owns and runs on the engine's own stream: one _host call at a time.) */
int  jamd_gmm_ms_outprob_dev(jamd_gmm_ms *g, const float *dev_frames, int T, float *dev_out, void *stream);
int  jamd_gmm_ms_outprob_host(jamd_gmm_ms *g, const float *host_frames, int T, float *host_out);
/* Name and launch shape of the kernel the last outprob call used. */
const char *jamd_gmm_ms_last_kernel(const jamd_gmm_ms *g);

/* The same object for a model with tied-mixture codebooks (calc_tied_mix() / calc_compound_mix()'s stream loops over
 * the per-(frame, codebook) cache, libsent/src/phmm/calc_tied_mix.c:177-236, :274-345), and for any multi-stream model
 * under `-gprune safe`.
 *   gprune        JAMD_GPRUNE_NONE or JAMD_GPRUNE_SAFE; HEU and BEAM are refused by name
 *   gprune_num    OP_gprune_num (-tmix); ignored for NONE, 1 .. 64 for SAFE as jamd_gmm_create()
 *   chunk_frames  0, or the frames the object's device scratch covers at a time.  0 = 2048, or as many fewer (in steps
 *                 of 128, at least 128) as keep the scratch within 256 MiB.  Results do not depend on it.
 * The scratch -- the cache [books][cap][chunk_frames + 1] of (score, id) and [books][chunk_frames + 1] of (num, mark);
 * under SAFE every plain pdf has a column of its own beside the codebooks' -- is allocated ONCE, here; an outprob call
 * walks its frames chunk by chunk on the caller's stream and neither allocates nor waits for the device.  So an object
 * with a tied-mixture pdf, or under SAFE, serves ONE call at a time (queue calls on one stream, or use one object per
 * stream); a model of plain pdfs under NONE is exactly what jamd_gmm_ms_create() makes, several streams at once
 * included.  Arithmetic as above, with calc_tied_mix()'s `score + bweight[id]` (one rounded add) over the cached
 * slots, log-summed from the last slot down. */
typedef struct { int gprune; int gprune_num; int chunk_frames; } jamd_gmm_ms_opt;
int  jamd_gmm_ms_create_opt(jamd_engine *e, const jamd_gmm_ms_desc *d, const jamd_gmm_ms_opt *opt, jamd_gmm_ms **out);
/* ... from the binary HMM definition: rd_tmix()'s codebook section and the tmix form of a pdf (read_binhmm.c:489-567). */
int  jamd_gmm_ms_load_binhmm_opt(jamd_engine *e, const char *binhmm_path, const jamd_gmm_ms_opt *opt, jamd_gmm_ms **out);
/* A BATCH of utterances laid back to back, utt_off a HOST array of nutt + 1 ints with utt_off[0] = 0 (as
 * jamd_gmm_outprob_utts_dev()).  The boundaries matter only under SAFE with tied-mixture pdfs: an utterance's first
 * frame has no history (calc_tied_mix.c:203-215; outprob_prepare() clears the cache).  jamd_gmm_ms_outprob_dev() /
 * _host() treat their T frames as one utterance. */
int  jamd_gmm_ms_outprob_utts_dev(jamd_gmm_ms *g, const float *dev_frames, const int *utt_off, int nutt, float *dev_out,
                                  void *stream);
int  jamd_gmm_ms_outprob_utts_host(jamd_gmm_ms *g, const float *host_frames, const int *utt_off, int nutt, float *host_out);
/* Cache slots per (frame, codebook) -- the largest codebook for NONE, min(gprune_num, the largest mixture or
 * codebook) for SAFE; 0 without a tied-mixture pdf -- and the codebook count. */
int  jamd_gmm_ms_tmix_cap(const jamd_gmm_ms *g);
int  jamd_gmm_ms_nbook(const jamd_gmm_ms *g);
/* The codebook cache for inspection, as jamd_gmm_tmix_cache_dev(): dev_score / dev_id [T][nbook][cap], dev_num
 * [T][nbook]; T frames of one utterance. */
int  jamd_gmm_ms_tmix_cache_dev(jamd_gmm_ms *g, const float *dev_frames, int T, float *dev_score, int *dev_id, int *dev_num,
                                void *stream);

/* ---- Gaussian mixture selection (-gshmm FILE -gsnum N) --------------------------------------
 * Replaces gms_state() (libsent/src/phmm/gms.c:394-412, with compute_gs_scores()/do_gms(),
 * gms.c:189-264, and compute_g_max(), gms_gprune.c:80-150).  gs is the flattened selection model
 * (plain single-stream GMM states, one per GS HMM state in gms.c:106-117's order), state2gs[s] the
 * selection state of state s of the real model (state2gs in gms.c:119-145; -1 = state not mapped,
 * left alone), nbest the -gsnum value.  jamd_gms_apply_dev() turns a [T][nstate] matrix of real
 * scores into what outprob_state() returns under GMS: where the selection state of s is not among
 * the frame's nbest, scores[t][s] becomes the selection state's own score.  utt_off[nutt+1] (host)
 * gives the first frame of every utterance in the T concatenated frames (the reference resets the
 * last-best Gaussian at every utterance, gms_gprune.c:190-207); NULL = one utterance. */
typedef struct jamd_gms jamd_gms;
int  jamd_gms_create(jamd_engine *e, const jamd_gmm_desc *gs, const int *state2gs, int nstate, int nbest,
                     jamd_gms **out);
/* A selection model file written by jamd_export (-gshmm given): jamd_gms_save(),
 * julius_amd/shim/jamd_flatten.c. */
int  jamd_gms_load(jamd_engine *e, const char *path, jamd_gms **out);
/* on != 0: select with the reference's heap (sort_gsindex_upward(), gms.c:189-230) on one lane, so
 * that an exact tie between two selection states on the nbest boundary falls as in the reference;
 * default is the wave-parallel ranking, where the lower state id wins such a tie. */
int  jamd_gms_set_strict_order(jamd_gms *m, int on);
int  jamd_gms_nstate(const jamd_gms *m);     /* states of the REAL model (columns of the score matrix) */
void jamd_gms_destroy(jamd_gms *m);
int  jamd_gms_apply_dev(jamd_gms *m, const float *dev_frames, int T, const int *utt_off, int nutt,
                        float *dev_scores, void *stream);
/* The same over host buffers (frames in, scores in and out), on the engine's own stream. */
int  jamd_gms_apply_host(jamd_gms *m, const float *host_frames, int T, const int *utt_off, int nutt,
                         float *host_scores);

/* ---- GMM-based input verification / rejection (-gmm FILE -gmmnum N -gmmreject NAMES) ---------
 * Replaces the scoring inside gmm_proceed() (libjulius/src/gmm.c:574-600; gmm_calc_mix() :335-370,
 * gmm_gprune_safe() :296-313 with gmm_compute_g_base() :177-194 / gmm_compute_g_safe() :218-240):
 * per frame, the log10 likelihood of each verification GMM's single output state under gmm.c's own
 * top-N pruning -- which is not libsent's arithmetic (gconst is added last for the first N
 * Gaussians), so this is a separate kernel, not jamd_gmm_outprob_*().  gmm is the flattened GMM
 * definition file (jamd_flatten_hmminfo(recog->gmm)), model_state[k] the state id of model k's
 * output state (d->s[1]->id in recog->gmm->start order, the order of gc->gmm_score[]),
 * gprune_num the -gmmnum value (jconf->reject.gmm_gprune_num, default 10).
 *   frame scores  [T][nmodel]     what one gmm_proceed() adds to gc->gmm_score[k]
 *   utt scores    [nutt][nmodel]  gc->gmm_score[] at gmm_end(): float sums in frame order
 * gmm_end()'s winner / confidence / gmm_valid_input() stay with the caller (a few flops). */
typedef struct jamd_rejgmm jamd_rejgmm;
int  jamd_rejgmm_create(jamd_engine *e, const jamd_gmm_desc *gmm, const int *model_state, int nmodel,
                        int gprune_num, jamd_rejgmm **out);
void jamd_rejgmm_destroy(jamd_rejgmm *m);
/* A file written by jamd_export (-gmm given: jamd_rejgmm_save(), julius_amd/shim/jamd_flatten.c):
 * the GMMs, -gmmnum, the model names and which of them -gmmreject names. */
int  jamd_rejgmm_load(jamd_engine *e, const char *path, jamd_rejgmm **out);
/* Names and gc->is_voice[] (gmm_init(), gmm.c:466-480: 0 for models named by -gmmreject) for a handle
 * made with jamd_rejgmm_create(); jamd_rejgmm_load() sets them from the file. */
int  jamd_rejgmm_set_models(jamd_rejgmm *m, const char *const *names, const unsigned char *is_voice);
const char *jamd_rejgmm_model_name(const jamd_rejgmm *m, int k);
/* gmm_end() (gmm.c:614-660) + gmm_valid_input() (:672-679) on one row of utterance sums (host
 * arithmetic, a few flops): the winning model, its confidence 1 / sum_i 10^(0.05 (score_i - max)), and
 * whether the input is accepted (the winner is not a rejected model). */
int  jamd_rejgmm_verdict(const jamd_rejgmm *m, const float *utt_scores, int *winner, float *cm, int *accepted);
int  jamd_rejgmm_nmodel(const jamd_rejgmm *m);
int  jamd_rejgmm_veclen(const jamd_rejgmm *m);
int  jamd_rejgmm_frame_scores_dev(jamd_rejgmm *m, const float *dev_frames, int T, float *dev_out, void *stream);
int  jamd_rejgmm_utt_scores_dev(jamd_rejgmm *m, const float *dev_frame_scores, int T, const int *utt_off, int nutt,
                                float *dev_out, void *stream);
/* Host buffers in and out; either output may be NULL (utt_off/nutt only needed for utt scores). */
int  jamd_rejgmm_scores_host(jamd_rejgmm *m, const float *host_frames, int T, const int *utt_off, int nutt,
                             float *host_frame_scores, float *host_utt_scores);

/* ------------------------------------------------- pseudo-phone state sets */
/* CD_State_Set table (htk_hmm.h:249-253): set i = states[set_off[i]..set_off[i+1]).
 * Replaces outprob_cd() (outprob.c:383): cd[t][i] from one [T][nstate] score
 * matrix. nbest = hmminfo->cdmax_num. */
int  jamd_cdset_create(jamd_engine *e, int nset, const int *set_off, const int *states,
                       int method, int nbest, jamd_cdset **out);
void jamd_cdset_destroy(jamd_cdset *c);
int  jamd_cdset_nset(const jamd_cdset *c);
int  jamd_cdset_outprob_dev(jamd_cdset *c, const float *dev_scores, int T, int nstate,
                            float *dev_cd, void *stream);

/* --------------------------------------------------------------------- DNN */
/* Flattened DNNData (libsent/include/sent/dnn.h:41-74): nlayer = hnum + 1
 * affine layers, dims[0..nlayer] = inputnodenum, hidden..., outputnodenum;
 * w[l] is [dims[l+1]][dims[l]] row-major exactly as dnn_layer_load() reads the
 * .npy (calc_dnn.c:225-335), b[l] is [dims[l+1]]; state_prior[dims[nlayer]] as
 * stored after dnn_setup() (log10 already applied when state_prior_log10nize,
 * calc_dnn.c:699-703). */
typedef struct {
  int nlayer;
  const int *dims;
  const float *const *w;
  const float *const *b;
  const float *state_prior;
} jamd_dnn_desc;

int  jamd_dnn_create(jamd_engine *e, const jamd_dnn_desc *d, jamd_dnn **out);
/* The same from Julius' own on-disk DNN definition: the -dnnconf text file, the NumPy
 * .npy weight / bias files and the state prior list it names, read as the reference does
 * (dnn_config_file_parse(), libjulius/src/m_jconf.c:577-735; load_npy() / dnn_layer_load()
 * / prior file, libsent/src/phmm/calc_dnn.c:225-335, :390-434, :678-707).  Relative
 * paths are relative to the dnnconf file. */
int  jamd_dnn_load(jamd_engine *e, const char *dnnconf_path, jamd_dnn **out);
void jamd_dnn_destroy(jamd_dnn *n);
int  jamd_dnn_nstate(const jamd_dnn *n);   /* dims[nlayer] */
int  jamd_dnn_veclen(const jamd_dnn *n);   /* dims[0]      */
/* Replaces dnn_calc_outprob() (calc_dnn.c:774) for a batch of frames:
 * out[t][i] = INV_LOG_TEN*(x_i - addlog_array(x)) - state_prior[i]
 * (calc_dnn.c:858-866).  frames [T][dims[0]] already spliced
 * (libjulius/src/wav2mfcc.c:163-169 does the splicing upstream). */
int  jamd_dnn_outprob_dev(jamd_dnn *n, const float *dev_frames, int T, float *dev_out,
                          void *stream);
int  jamd_dnn_outprob_host(jamd_dnn *n, const float *host_frames, int T, float *host_out);


/* ------------------------------------------------- first-pass beam (pass 1) */
/* Flattened read side of the first pass: the tree lexicon WCHMM_INFO
 * (libjulius/include/julius/wchmm.h:211-278), the cross-word context tables
 * that outprob_style() (libjulius/src/outprob_style.c:354) resolves by name
 * lookups, the LM factoring tables (libjulius/src/factoring_sub.c:345-468) and
 * the forward 2-gram the beam reads through ngram->bigram_prob
 * (libsent/src/ngram/ngram_access.c:288-403).  N-gram LM with 1-gram factoring (the
 * reference's default "fast" setup), DFA grammar with per-category trees, or isolated word list; multipath models
 * through jamd_flatten_lexicon_multipath() (JAMD_LM_MULTIPATH below).  All indices are
 * 32-bit; WORD_INVALID is -1 here.  Built by jamd_flatten_lexicon()
 * (julius_amd/shim/jamd_flatten_lex.c) from an unmodified RecogProcess.
 * NOT SERVED -- the flattener returns JAMD_EINVAL, the shim's get_back_trellis_init() logs the reason and returns FALSE
 * (there is no CPU first pass behind this library):
 *   - a grammar without per-category trees (not a runtime choice of the reference: multigram_build() sets
 *     wchmm->category_tree = TRUE for every grammar, multi-gram.c:101), and user-defined LM functions (LM_NGRAM_USER);
 *   - N-gram lexicons built without 1-gram factoring (a non-default ./configure of the reference). */
#define JAMD_AS_STATE 0   /* AS_STATE  wchmm.h:105: out_id = state id                   */
#define JAMD_AS_LSET  1   /* AS_LSET   wchmm.h:106: out_id = state-set id                */
#define JAMD_AS_RSET  2   /* AS_RSET   wchmm.h:107: out_id = row of lc_tab               */
#define JAMD_AS_LRSET 3   /* AS_LRSET  wchmm.h:108: out_id = row of lc_tab               */
#define JAMD_AS_NONE  4   /* multipath only: non-emitting node (state[n].out.state == NULL) */

#define JAMD_LM_NGRAM 0   /* LM_PROB  */
#define JAMD_LM_DFA   1   /* LM_DFA, LM_DFA_GRAMMAR with the default per-category tree */
#define JAMD_LM_WORD  2   /* LM_DFA, LM_DFA_WORD: isolated word recognition (-w): every word of the list starts
                           * with a token (beam.c:1762-1788), no cross-word transition (:2810, :2875), the
                           * result is the best word on the last frame (find_1pass_result_word(), :561).
                           * Uses ninit / init_node / init_lscore (all 0.0); cat_pair is not read. */

/* OR-ed into lm_type by jamd_flatten_lexicon_multipath(): a multipath lexicon (hmminfo->multipath:
 * non-emitting word-begin / word-end nodes, word_head[] = wchmm->wordbegin[], wordend_a unused,
 * the frame loop of beam.c:2747-2836: word-internal transitions, the beam over the NEW tokens, cross-word transitions
 * from the word ends among them with the root expanded along its own arcs inside the frame, output probabilities on
 * emitting nodes, the final cut).  Decoded by the exact-order kernel's multipath frame (csrc/beam_exact_mp.h: one
 * workgroup per utterance, either workgroup shape, streaming included) in the reference's own tie order, or by the strict-order
 * kernel (JAMD_ORDER_STRICT); JAMD_ORDER_FAST does not take them.  One kind of lexicon is strict-order only: a root
 * that reaches a word-end node along its own arcs (a word made of tee models only) -- jamd_beam_order_mode() then
 * reports JAMD_ORDER_FAST for the new work area and jamd_beam_set_order_mode(b, JAMD_ORDER_EXACT) says why.  The reference
 * never builds such a lexicon (wchmm_add_word() rejects the word: "WORD SKIPPING TRANSITION NOT ALLOWED", wchmm.c:1345-1362;
 * tests/test_beam_oracle.py shows it for a grammar and for an N-gram), so jamd_export / the shim cannot produce one: the
 * restriction concerns hand-written descriptors only. */
#define JAMD_LM_MULTIPATH 0x100

#define JAMD_NG_NORMAL         0  /* bi_prob_normal()            ngram_access.c:288 */
#define JAMD_NG_ADDITIONAL_OLD 1  /* bi_prob_additional_oldbin() ngram_access.c:320 */
#define JAMD_NG_ADDITIONAL     2  /* bi_prob_additional()        ngram_access.c:351 */
#define JAMD_NG_COMPUTE        3  /* bi_prob_compute()           ngram_access.c:383 */

typedef struct {
  /* tree lexicon */
  int nnode, nword, startnum, isolatenum;
  const float *self_a, *next_a;        /* [nnode] wchmm->self_a / next_a (next goes to node+1)   */
  const int   *ac_off;                 /* [nnode+1] extra arcs (A_CELL2 chains, wchmm.h:162) in   */
  const int   *ac_to;                  /*           the order beam_intra_word() walks them        */
  const float *ac_a;                   /*           (libjulius/src/beam.c:2173-2177)              */
  const int   *stend;                  /* [nnode] word ending here or -1 (wchmm->stend)           */
  const int   *scid;                   /* [nnode] wchmm->state[n].scid                            */
  const unsigned char *out_kind;       /* [nnode] JAMD_AS_*  (wchmm->outstyle)                    */
  const int   *out_id;                 /* [nnode] see JAMD_AS_*                                   */
  /* cross-word left context: column = base phone of the previous word's last
   * phone (center_name(), libsent/src/hmminfo/cdhmm.c:144); column nlc = no
   * previous word.  Entry >= 0: state id; < 0: ~(state-set id). */
  int nlc, nlcrow;
  const int   *lc_tab;                 /* [nlcrow][nlc+1]                                         */
  const int   *word_lc;                /* [nword] column a word selects as LEFT context           */
  /* pseudo-phone state sets (CD_State_Set) used by AS_LSET nodes and lc_tab */
  int nset;
  const int   *set_off, *set_states;   /* CSR                                                     */
  int cdset_method, cdmax_num;         /* JAMD_IWCD_*, hmminfo->cdmax_num                         */
  /* tree roots */
  const int   *startnode;              /* [startnum] wchmm->startnode                             */
  const int   *start2isolate;          /* [startnum] wchmm->start2isolate (-1 = shared root)      */
  /* words */
  const float *wordend_a;              /* [nword] wchmm->wordend_a                                */
  const int   *wton;                   /* [nword] winfo->wton (N-gram entry id)                   */
  const float *cprob;                  /* [nword] winfo->cprob                                    */
  const unsigned char *is_transparent; /* [nword]                                                 */
  const int   *word_head;              /* [nword] wchmm->offset[w][0]                             */
  int head_silwid, tail_silwid;
  /* LM factoring */
  int nfscore, nscword;
  const float *fscore;                 /* [nfscore] wchmm->fscore (index -scid)                   */
  const int   *scword;                 /* [nscword] wchmm->scword (index scid)                    */
  /* forward 2-gram as ngram->bigram_prob reads it */
  int ng_mode;                         /* JAMD_NG_*                                               */
  int ng_nword, ng_nbigram, ng_unk_id;
  float ng_unk_num_log;
  const float *ng_uni_prob;            /* d[0].prob                                               */
  const float *ng_uni_bo;              /* d[0].bo_wt, or bo_wt_1 for the ADDITIONAL modes         */
  const int   *ng_bi_bgn;              /* d[1].bgn  (-1 = NNID_INVALID)                           */
  const int   *ng_bi_num;              /* d[1].num                                                */
  const int   *ng_bi_wid;              /* d[1].nnid2wid                                           */
  const float *ng_bi_prob;             /* d[1].prob, or p_2 for the ADDITIONAL modes              */
  /* FSBeam local copies (libjulius/include/julius/recog.h:147-150) */
  float lm_weight, lm_penalty, lm_penalty_trans;
  /* ---- grammar (DFA) mode, lm_type == JAMD_LM_DFA: per-category tree lexicon
   * (wchmm->category_tree), category-pair constraint at the word boundaries
   * (beam_inter_word(), libjulius/src/beam.c:2404-2412; dfa_cp(), libsent/src/dfa/cpair.c),
   * no LM factoring inside words.  For N-gram mode these are 0 / NULL.  In grammar mode
   * `wton` holds the category of each word. */
  int lm_type;                         /* JAMD_LM_NGRAM / JAMD_LM_DFA / JAMD_LM_WORD               */
  int ncat;                            /* dfa->term_num                                            */
  const unsigned char *cat_pair;       /* [ncat][ncat] dfa_cp(dfa, c1, c2): c2 may follow c1       */
  const int   *start2wid;              /* [startnum] wchmm->start2wid (a word of the root's tree)  */
  int ninit;                           /* initial tokens of init_nodescore() (beam.c:1669-1757):   */
  const int   *init_node;              /* [ninit] distinct word-head nodes in creation order       */
  const float *init_lscore;            /* [ninit] penalty1 + cprob of the first word reaching it   */
  float penalty1;                      /* r->config->lmp.penalty1                                  */
  /* ---- a FORWARD DFA beside the reversed one (the `.dfa.forward` file recent mkdfa.pl writes next to `.dfa`,
   * libjulius/src/multi-gram.c:868-880).  Tokens then carry a state of it (TOKEN2.to_state): an initial token of
   * category t takes the arc labelled t out of the grammar's first state (libjulius/src/beam.c:1739-1747), a cross-word
   * transition to a root of category c takes the arc labelled c out of the token's state and is dropped when there is
   * none (:2412-2422), word-internal transitions inherit it (:2120).  nfwd = 0: no forward DFA (all pointers may be NULL).
   * Served by the exact-order kernels (JAMD_ORDER_EXACT, the default; multipath lexicons included) and the strict-order
   * kernels; the canonical-tie kernel (JAMD_ORDER_FAST) carries no such state and is refused for these lexicons. */
  int nfwd;                            /* states of wchmm->dfa_forward                              */
  const int   *fwd_off;                /* [nfwd+1] arcs of a state, in the order of its arc list     */
  const int   *fwd_label;              /*          arc label = word category                         */
  const int   *fwd_to;                 /*          next state                                        */
  const int   *init_to_state;          /* [ninit] to_state of initial token e (-1: no such arc)      */
} jamd_lexicon_desc;

/* One emitted word-trellis record (TRELLIS_ATOM, libjulius/include/julius/
 * trellis.h:28-41) as save_trellis() fills it (beam.c:2209-2247).  last_tre is
 * the index of the predecessor atom in the same output array, -1 for the
 * sentence-start sentinel (FSBeam.bos). */
typedef struct {
  int   wid;
  int   last_tre;
  float backscore;
  float lscore;
  short begintime;
  short endtime;
} jamd_trellis_atom;


typedef struct jamd_lexicon jamd_lexicon;
typedef struct jamd_beam    jamd_beam;

/* Upload the first-pass tables.  Replaces, for the device, what
 * get_back_trellis_init() reads from r->wchmm (libjulius/src/beam.c:1825).
 * JAMD_EINVAL for inconsistent tables (a root without factoring value / successor word). */
int  jamd_lexicon_create(jamd_engine *e, const jamd_lexicon_desc *d, jamd_lexicon **out);
/* Julius' BINARY model files read directly, without a Julius process (julius_amd/csrc/readers.hip):
 *   jamd_gmm_load_binhmm()   the binary HMM definition of mkbinhmm (libsent/src/hmminfo/read_binhmm.c:756): the
 *                            same device model as jamd_export's PREFIX.am made from that file;
 *   jamd_binhmm_to_blob()    the same conversion to a "JAMDGMM1" file (byte for byte jamd_export's; no device);
 * The tree lexicon is the output of libjulius/src/wchmm.c over dictionary + HMMList + LM (its factoring values and
 * the words kept out of the tree are functions of the LM), not a file format: PREFIX.lex -- tree and N-gram tables
 * together -- comes from jamd_export, which links Julius' own loaders. */
int  jamd_gmm_load_binhmm(jamd_engine *e, const char *binhmm_path, int gprune, int gprune_num, jamd_gmm **out);
int  jamd_binhmm_to_blob(const char *binhmm_path, const char *blob_path);

/* The same from a "JAMDLEX1" file written by jamd_lexicon_save()
 * (julius_amd/shim/jamd_flatten_lex.c) in a process that loaded the dictionary and LM
 * with Julius' own readers. */
int  jamd_lexicon_load(jamd_engine *e, const char *path, jamd_lexicon **out);
/* The same with the N-gram half read DIRECTLY from a binary N-gram file (mkbingram v5 -- what `-d` names;
 * libsent/src/ngram/ngram_read_bin.c:240-365,603): the 1-gram / 2-gram tables of the first pass and the choice of the
 * 2-gram (forward, or the additional forward 2-gram of a backward N-gram, ngram_access.c:449-466) come from the file,
 * the cross-word LM table is built from them; the tree half -- nodes, factoring values, word -> N-gram ids, class
 * probabilities -- stays PREFIX.lex's, which is the output of libjulius/src/wchmm.c over the dictionary and not a file
 * format.  The two must share their vocabulary (names in N-gram id order: PREFIX.lex records it; refused otherwise).
 * With the N-gram the tree was built from the result equals jamd_lexicon_load()'s.  A RETRAINED N-gram over the same
 * vocabulary: the tree depends on the 1-gram in two places -- which words wchmm.c keeps out of the tree (the -sepnum most
 * frequent ones, libjulius/src/wchmm.c:1470, :1882) and the 1-gram factoring value of every shared node
 * (libjulius/src/factoring_sub.c:429-463).  The loader recomputes the factoring values from the file's 1-gram (the best
 * uni_prob + class probability over the words below the node) when the same words stay out of the tree -- the result is
 * then the lexicon a fresh jamd_export with that N-gram writes -- and refuses (JAMD_EINVAL, "export the lexicon again")
 * when the tree itself would differ or PREFIX.lex does not record -sepnum (written before this check existed). */
int  jamd_lexicon_load_ngram(jamd_engine *e, const char *path, const char *bingram_path, jamd_lexicon **out);
/* Host only: do PREFIX.lex and a binary N-gram share their vocabulary (JAMD_OK, else JAMD_EINVAL with the reason), and
 * -- *same_tables, may be NULL -- are the file's first-pass tables byte for byte the ones PREFIX.lex holds? */
int  jamd_bingram_check(const char *lex_path, const char *bingram_path, int *same_tables);
/* Host only: the 1-gram factoring values jamd_lexicon_load_ngram() would use -- fscore[0..*nfscore) (at most `cap` are
 * written; index 0 is unused, as in WCHMM_INFO.fscore) -- with the same acceptance rules and errors. */
int  jamd_bingram_fscore(const char *lex_path, const char *bingram_path, float *fscore, int cap, int *nfscore);
/* Diagnostic: 1 = the cross-word LM table exists, 0 = the first-pass kernels compute its entries as they need them (a
 * grammar or word list, a table past 2 GB, an allocation that failed, JAMD_NO_IWTAB), -1 = NULL. */
int  jamd_lexicon_lm_table(const jamd_lexicon *l);
void jamd_lexicon_destroy(jamd_lexicon *l);

/* First-pass status of one utterance */
#define JAMD_PASS1_OK        0  /* J_RESULT_STATUS_SUCCESS                                   */
#define JAMD_PASS1_FAIL      1  /* no sentence-end word survived (find_1pass_result(),        */
                                /* beam.c:424-429 -> J_RESULT_STATUS_FAIL)                     */
#define JAMD_PASS1_DIED      2  /* "no nodes left in beam" at frame died_at: _proceed()       */
                                /* returned FALSE (beam.c:3012-3015); the caller segments     */
#define JAMD_PASS1_OVERFLOW  3  /* more trellis atoms than atoms_per_utt                      */

typedef struct {
  int   status;          /* JAMD_PASS1_*                                              */
  int   natom;           /* trellis atoms emitted                                     */
  int   wnum;            /* r->pass1_wnum                                             */
  float score;           /* r->pass1_score (best->backscore, beam.c:505)              */
  int   died_at;         /* frame index for JAMD_PASS1_DIED, else -1                  */
  int   ties;            /* exact score ties met by a max/selection:  */
                         /* 0 => the result does not depend on visiting order         */
  int   frames;          /* T                                                         */
  int   max_tokens;      /* high-water mark of tokens alive in one frame              */
  int   ties_node, ties_wordend, ties_cut;   /* ties by kind: Viterbi max at a node, best    */
                         /* word end, rank cut                                        */
  int   phase_us[8];     /* device time spent in: A intra-word+atoms, B cross-word,   */
                         /* C finalize+outprob, D rank pruning (microseconds); [4..6] */
                         /* thread 0's share of C: key fetch, payload, outprob        */
  int   wseq[150];       /* r->pass1_wseq, MAXSEQNUM = 150 (libsent speech.h:50)      */
} jamd_pass1_result;

/* Work area for up to max_utts utterances decoded at once (FSBeam,
 * libjulius/include/julius/recog.h:115-174, one per utterance).
 * beam_width = r->trellis_beam_width (<= 65536), score_pruning_width =
 * r->config->pass1.score_pruning_width (< 0 disables, beam.c:2954-2960),
 * atoms_per_utt bounds the word trellis of one utterance. */
int  jamd_beam_create(jamd_engine *e, jamd_lexicon *l, int beam_width, float score_pruning_width,
                      int max_utts, int atoms_per_utt, jamd_beam **out);
void jamd_beam_destroy(jamd_beam *b);

/* The whole first pass for nutt utterances at once: for each utterance
 * get_back_trellis_init() (beam.c:1825), get_back_trellis_proceed() for
 * t = 1..T-1 (beam.c:2663), get_back_trellis_end() (beam.c:3052) and
 * find_1pass_result() (beam.c:372).  dev_scores holds the state score rows of
 * all utterances back to back: utterance u owns rows utt_off[u]..utt_off[u+1])
 * of [.][nstate] (what outprob_state() would return for every state: the output
 * of jamd_gmm_outprob_dev / jamd_dnn_outprob_dev).  utt_off is a HOST array of
 * nutt+1 ints.  Asynchronous on `stream`; results are read with
 * jamd_beam_results() / jamd_beam_trellis(), which synchronise.
 * ONE launch per work area at a time: the utterance table, the slices and the result records of a jamd_beam belong to
 * its latest launch, so the next jamd_beam_pass1_dev() / jamd_beam_stream_push_dev() on the same work area goes on the
 * SAME stream (it then queues behind the first) or after the first has completed; work areas are independent of each
 * other.  The same holds for the scoring calls of one jamd_gmm with history pruning (utterance boundaries are staged per
 * model). */
int  jamd_beam_pass1_dev(jamd_beam *b, const float *dev_scores, int nstate, const int *utt_off,
                         int nutt, void *stream);
/* Streaming form of jamd_beam_pass1_dev() for input that arrives in pieces (Julius calls
 * get_back_trellis_proceed() once per frame, libjulius/src/pass1.c:242; live audio never has
 * the whole utterance).  jamd_beam_stream_begin() opens a session for utterance slots
 * 0..nutt-1; each jamd_beam_stream_push_dev() advances every utterance by the rows
 * chunk_off[u]..chunk_off[u+1]) of dev_scores (any number of frames, zero included) and keeps
 * the search state on the device; `final` != 0 additionally runs get_back_trellis_end() and the
 * traceback, after which jamd_beam_results()/jamd_beam_trellis() return exactly what one
 * jamd_beam_pass1_dev() call over the concatenated rows would.  jamd_beam_results() may also
 * be called between pushes (natom / frames so far).  In strict-order mode a session must
 * consist of one final push. */
int  jamd_beam_stream_begin(jamd_beam *b, int nutt);
int  jamd_beam_stream_push_dev(jamd_beam *b, const float *dev_scores, int nstate, const int *chunk_off,
                               int nutt, int final, void *stream);

/* Verification mode.  on != 0: later jamd_beam_pass1_dev() calls run the reference's
 * SEQUENTIAL algorithm (same token creation order, same partial heap sort
 * beam.c:1342-1516, first-writer-wins propagation) with one lane per utterance, so that
 * the word trellis equals the reference's bit for bit even where exact score ties are
 * broken by visiting order.  Two to three orders of magnitude slower per utterance;
 * parallel only across the utterances of a batch.  on == 0 returns to the work area's
 * default (jamd_beam_create()), from JAMD_ORDER_EXACT_SERIAL too: JAMD_ORDER_EXACT where the
 * exact-order kernel serves the work area, else JAMD_ORDER_FAST.  A grammar with a forward
 * DFA is the exception: the canonical-tie kernel cannot carry its state, so such a work area
 * that the exact-order kernel cannot serve starts in strict order, and on == 0 is refused
 * (JAMD_ESTATE; the mode stays strict).  Either direction returns JAMD_ESTATE while a
 * streaming session is open. */
int  jamd_beam_set_strict_order(jamd_beam *b, int on);
/* How exact score ties are resolved (they are the only freedom a parallel schedule has; every
 * float is the reference's float in all modes):
 *   JAMD_ORDER_EXACT   (default; multipath lexicons included; beams up to about 12 000: up to ~950 the survivors live
 *       in LDS; wider beams keep them in the utterance's slice of HBM and the pruning step overlays the whole LDS
 *       image; the closed-form extraction serves beams up to about 5 000, beyond that the heap's extraction loop itself
 *       runs pipelined on one wave):
 *       frame-parallel kernel with the reference's own semantics -- candidates keyed by their position
 *       in the reference's visiting order (first writer wins, propagate_token() beam.c:1945-1980,
 *       wordend_best :2308), token creation order, and the partial heap sort of
 *       sort_token_no_order() (beam.c:1342-1516) reproduced exactly.  The word trellis equals the
 *       reference's bit for bit, ties included.
 *   JAMD_ORDER_EXACT_SERIAL  the same kernel with the heap's extraction loop run sequentially on one
 *       lane instead of in closed form / pipelined (cross-check and timing).
 *   JAMD_ORDER_FAST    frame-parallel kernel with canonical tie breaks (larger source id, smaller node
 *       on the rank cut): identical to the reference whenever jamd_pass1_result.ties == 0.
 *   JAMD_ORDER_STRICT  = jamd_beam_set_strict_order(b, 1): the sequential algorithm, one lane per utterance.
 * jamd_beam_set_strict_order(b, 0) returns to the default of the work area. */
#define JAMD_ORDER_FAST 0
#define JAMD_ORDER_STRICT 1
#define JAMD_ORDER_EXACT 2
#define JAMD_ORDER_EXACT_SERIAL 3
int  jamd_beam_set_order_mode(jamd_beam *b, int mode);
int  jamd_beam_order_mode(const jamd_beam *b);
/* Workgroup shape of the exact-order kernel (a scheduling choice: the results are the same bit for bit).
 *   JAMD_SHAPE_FULL  one utterance per CU: 1024 threads and the CU's whole LDS -- the lowest latency per utterance.
 *   JAMD_SHAPE_HALF  512 threads and half the LDS, so two utterances share a CU and the barriers and wave-serial
 *       sections of one overlap the work of the other: more frames per second once a launch carries more
 *       utterances than the device can hold in the full shape.  Available while half a CU's LDS still holds a
 *       typical frame (beams up to about 1 000, a little more with few word-initial nodes); JAMD_ESTATE otherwise.
 *   JAMD_SHAPE_AUTO  (default) HALF for launches (and streaming sessions) of more than 1.5 x the CU count
 *       utterances when available, else FULL.
 * jamd_beam_workgroup_shape() tells which one a launch of nutt utterances would use in the exact order modes (the
 * canonical-tie and strict-order kernels have one shape each and ignore the setting).  A streaming session keeps the
 * shape it was opened with. */
#define JAMD_SHAPE_AUTO 0
#define JAMD_SHAPE_FULL 1
#define JAMD_SHAPE_HALF 2
int  jamd_beam_set_workgroup_shape(jamd_beam *b, int shape);
int  jamd_beam_workgroup_shape(const jamd_beam *b, int nutt);
/* Which LDS image the exact-order kernel uses for this work area in its full shape: 0 = it cannot serve the work area,
 * 1 = narrow (survivors in LDS: beams up to ~950), 2 = wide (survivors in the utterance's slice; the sweep replay and the
 * closed form of the downward sort live in this one).  Same results either way; for tests and diagnostics. */
int  jamd_beam_exact_layout(const jamd_beam *b);
/* Blocks the host until everything queued ahead of the latest first-pass launch of this work area has completed, i.e.
 * until that kernel is next to run (returns at once when nothing was launched).  For hosts that pipeline batches: a
 * first pass that fills the device (one or two workgroups per CU, all of a CU's LDS) must get its workgroups placed
 * before the scoring kernels of the NEXT batch are queued on another stream -- queued earlier they take the LDS the
 * first pass wants, and the first pass of 512 utterances takes twice as long; queued once it runs they only fill the
 * CUs its shorter utterances leave (julius_amd/host/jamd_batch.c, bench.py: -5 % per step). */
int  jamd_beam_wait_started(jamd_beam *b);
/* The same ordering WITHOUT the host: work queued on `stream` after this call starts only when the workgroups of the
 * latest first-pass launch of this work area that fit the device at once (one per CU; two in the exact-order kernel's
 * half shape) have started -- they bump a counter in signal memory as their first instruction and `stream`'s command
 * processor waits on it (hipStreamWaitValue32).  A pipelining host calls it between the first-pass launch of batch k
 * and the scoring launches of batch k+1 (jamd_batch.c, bench.py): no event wait, no sleep, nothing to time.  Devices
 * without wait-on-memory fall back to jamd_beam_wait_started() plus a millisecond's pause inside this call. */
int  jamd_beam_stream_wait_resident(jamd_beam *b, void *stream);
/* Test entry: sets the resident counter (the device word the first-pass workgroups bump, and the host's bookkeeping of
 * it) to `count`, as if that many workgroups had been launched since the work area was created.  The counter is 32 bits
 * wide and drained back to zero before it could wrap (csrc/beam_api.hip mark_started()); a test starts it just below that
 * point instead of launching 2^31 workgroups.  The device is synchronised first. */
int  jamd_beam_debug_preset_resident(jamd_beam *b, unsigned count);
/* Test entry: workgroups accounted since the last drain (*launched) and the value the next
 * jamd_beam_stream_wait_resident() waits for (*target). */
int  jamd_beam_debug_resident(const jamd_beam *b, unsigned *launched, unsigned *target);
/* The rank-pruning step alone (sort_token_no_order(), beam.c:1492): given the scores of the n tokens of
 * a frame in creation order (host array), writes the token indices the next frame visits, in visiting
 * order (tindex[n_start..n_end]), for the work area's beam width; *nkeep = how many.  Runs the
 * exact-order kernel's pruning code on the device; diagnostic / test entry. */
int  jamd_beam_prune_order(jamd_beam *b, const float *scores, int n, int *order, int *nkeep);
/* The same step with the WHOLE array out: tindex[0..n) = the token ids at array positions 0..n-1 after
 * sort_token_no_order() (residual heap and extracted part: what the multipath frame's final cut starts from,
 * csrc/beam_exact_mp.h) beside order[].  Test entry like jamd_beam_prune_order(); full workgroup shape. */
int  jamd_beam_prune_arrange(jamd_beam *b, const float *scores, int n, int *order, int *nkeep, int *tindex);
/* How the latest jamd_beam_prune_order() call resolved the events of the extraction loop (tail positions that hold a
 * top element, beam.c:1369-1383): *sweep_rounds = rounds of the all-at-once sweep replay (csrc/beam_sweep.h) when it
 * ran and converged, -1 = it ran and handed the frame to the extraction loop, 0 = not needed (few candidates, or no
 * tied element among them); *sweep_us (may be NULL) = its duration on the device, *sweep_events (may be NULL) = events
 * it held at the end.  Diagnostic / test entry. */
int  jamd_beam_prune_info(jamd_beam *b, int *sweep_rounds, int *sweep_us, int *sweep_events);
/* How the rank pruning steps (sort_token_no_order(), beam.c:1492) of utterance `utt` were resolved by the exact-order
 * kernel since the work area was created or the counters were last reset -- frames counted by path:
 *   [0] frames pruned (more tokens than the beam)          [1] upward, closed form, no tied element on a tail position
 *   [2] upward, wave-serial event replay                   [3] upward, sweep replay converged
 *   [4] upward, sweep gave the frame to the extraction loop [5] downward, closed form (sweep + residual-heap replay)
 *   [6] extraction loop itself (pipelined / serial)        [7] sweep rounds, total
 * and the work of the frames (sums over the frames): [8] tokens created, [9] survivors visited, [10] word ends among them,
 * [11] frames; [12] multipath frame: frames whose new tokens exceeded the beam (the mid-frame sort really sorted);
 * the lane split of the state-set reductions (outprob_cd() inside the frame, csrc/beam_exact.hip step C):
 *   [13] frames that ran two lanes per set                 [14] frames that ran one lane per set
 *   [15] state-set reductions, summed over the frames
 * (four-lane frames = [11] - [13] - [14]; the N-gram's initial token is scored before the frame loop and is in none of
 * [8..15]).  The multipath frame reduces a set on one lane per token and has no split:
 * it leaves [13..15] at 0.  reset != 0 clears them.  Diagnostic. */
int  jamd_beam_prune_stats(jamd_beam *b, int utt, int stats[16], int reset);
int  jamd_beam_results(jamd_beam *b, jamd_pass1_result *out, int nutt);
/* Word trellis of utterance u in emission order (last_tre indexes the same
 * array).  bt_relocate_rw()/bt_sort_rw() order (libjulius/src/backtrellis.c:
 * 218-267,468-477) is (endtime, wid). */
int  jamd_beam_trellis(jamd_beam *b, int utt, jamd_trellis_atom *atoms, int cap, int *natom);

/* ---- audio front end: PCM samples -> MFCC / FBANK / MELSPEC features ------------------------
 * The reference's buffered (non-realtime) front end, the one `julius -input rawfile` runs:
 * Wav2MFCC() (libsent/src/wav2mfcc/wav2mfcc-buffer.c) with WMP_calc() and the tables of
 * mfcc-core.c (MFCC_SINCOS_TABLE on), then the splicing of libjulius/src/wav2mfcc.c:162-169.
 * Bit-identical to it.  The descriptor carries the fields of Value (libsent/include/sent/mfcc.h:
 * 76-115), the static CMN/CVN vectors of CMNWork (-cmnload FILE -cmnstatic) and the splice count.
 * paramtype is an HTK parameter kind code: base JAMD_F_MFCC / _FBANK / _MELSPEC ORed with the
 * qualifier bits below (htk_defs.h:57-66); vecsize the vector size the acoustic model declares.
 *
 * Spectral subtraction (-sscalc [-sscalclen], -ssload, -ssalpha, -ssfloor) is served through
 * jamd_frontend_set_ss() on the created object, bit-identical as well (MakeFBank(), mfcc-core.c:473-487;
 * new_SS_calculate(), ss.c:110-172).
 *
 * NOT SERVED -- jamd_frontend_create() returns JAMD_EINVAL and says why (there is no host front end
 * behind this library):
 *   - ss != 0 in the descriptor: the descriptor carries none of the parameters of spectral subtraction,
 *     which is switched on with jamd_frontend_set_ss();
 *   - realtime != 0: the descriptor of the buffered front end stays the buffered one.  The pipelined front end of
 *     wav2mfcc-pipe.c (microphone, socket, -realtime: MAP-CMN, energy by the previous maximum, cyclic deltas) is an
 *     object of its own made from a created jamd_frontend: jamd_frontend_live_create() below;
 *   - kinds other than MFCC, FBANK and MELSPEC, FBANK / MELSPEC with _E or _0 (WMP_calc() leaves
 *     those slots unwritten), _N without _E and _D, _A without _D. */
#define JAMD_F_MFCC     6
#define JAMD_F_FBANK    7
#define JAMD_F_MELSPEC  8
#define JAMD_F_E        0x0040
#define JAMD_F_N        0x0080
#define JAMD_F_D        0x0100
#define JAMD_F_A        0x0200
#define JAMD_F_Z        0x0800
#define JAMD_F_0        0x2000

typedef struct {
  int paramtype, vecsize;             /* kind and model vector size the derived fields come from         */
  int smp_period, smp_freq;           /* 100 ns units / Hz                                                */
  int framesize, frameshift;          /* samples                                                          */
  float preEmph;
  int lifter, fbank_num, delWin, accWin;
  float silFloor, escale;
  int hipass, lopass;                 /* Hz, -1 = off                                                     */
  int enormal, raw_e, zmeanframe, usepower, cvn;
  float vtln_alpha, vtln_upper, vtln_lower;
  /* derived by calc_para_from_header() (para.c:323-372) */
  int basetype, delta, acc, energy, c0, absesup, cmn, mfcc_dim, baselen, vecbuflen, veclen;
  /* -cmnload: static mean [veclen] (the first mfcc_dim + c0 entries are read) and variance [veclen];
   * NULL = computed over each utterance.  static_cvn_only = CMNWork.static_cvn_only. */
  const float *cmean_init;
  const float *cvar_init;
  int static_cvn_only;
  int splice;                         /* -splice N (1 = none)                                             */
  int ss, realtime;                   /* refused: see NOT SERVED (SS: jamd_frontend_set_ss()) / realtime  */
} jamd_frontend_desc;

typedef struct jamd_frontend jamd_frontend;
/* make_default_para() (para.c:86-107) then calc_para_from_header(paramtype, vecsize); splice 1. */
int  jamd_frontend_default_desc(int paramtype, int vecsize, jamd_frontend_desc *d);
/* calc_para_from_header() alone (the kind fields, and fbank_num for FBANK / MELSPEC). */
int  jamd_frontend_set_kind(jamd_frontend_desc *d, int paramtype, int vecsize);
/* htk_config_file_parse() (para.c:196-321) over d in place.  Keys the reference does not take are
 * refused (JAMD_EINVAL naming the key); TARGETKIND and NUMCEPS are skipped as there. */
int  jamd_frontend_htkconf(const char *path, jamd_frontend_desc *d);
/* Host only: a table the front end is built from, as WMP_work_new() makes it.  name: "hamming",
 * "fft_cos", "fft_sin", "dct", "wcep", "twiddle_re", "twiddle_im" (double), "cf", "lowt" (float,
 * [maxChan + 1] / [fftN/2 + 1]), "lochan" (short, [fftN/2 + 1]), "info" (int: fftN, n, klo, khi),
 * "scalars" (float: fres, sqrt2var).  Returns the element count (copies min(count, cap)). */
int  jamd_frontend_table(const jamd_frontend_desc *d, const char *name, void *out, int cap);
int  jamd_frontend_create(jamd_engine *e, const jamd_frontend_desc *d, jamd_frontend **out);
void jamd_frontend_destroy(jamd_frontend *f);
int  jamd_frontend_veclen(const jamd_frontend *f);             /* veclen * splice: floats per output frame */
/* Output frames of one utterance of nsamples samples: (n - framesize)/frameshift + 1 - (splice - 1),
 * <= 0 when the input is too short (also when n < framesize). */
int  jamd_frontend_frames(const jamd_frontend_desc *d, int64_t nsamples);
/* nutt utterances back to back in dev_samples (int16), utterance u = samples [sample_off[u],
 * sample_off[u+1]) (host array).  Writes the features of all utterances back to back into dev_out
 * ([sum frames][veclen * splice], the layout jamd_gmm_outprob_utts_dev / jamd_dnn_outprob_dev /
 * jamd_beam_pass1_dev take) and, if frame_off is not NULL, the host frame offsets [nutt + 1].
 * An utterance too short for one output frame: JAMD_EINVAL, nothing written.
 * The object's device scratch (per-frame statics, the vectors before normalisation, the CMN / MVN statistics, the
 * offsets) is reused by every call: calls on one object must not be in flight on two streams at once -- queue them on
 * one stream (they are then ordered), or use one object per stream.  Windows of up to 4096 samples are served (fftN
 * up to 4096; the frame kernel takes two frames per workgroup instead of four at fftN 4096). */
int  jamd_frontend_run_dev(jamd_frontend *f, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                           float *dev_out, int *frame_off, void *stream);
int  jamd_frontend_run_host(jamd_frontend *f, const int16_t *samples, const int64_t *sample_off, int nutt,
                            float *out, int *frame_off);

/* Spectral subtraction.  jamd_frontend_set_ss() switches it on a created object; it may be called between runs
 * (the rule of one stream per object covers it), and every later jamd_frontend_run_*() applies it:
 *   JAMD_SS_CALC  the noise spectrum of every utterance is new_SS_calculate() over its first
 *                 min(calc_len_ms * smp_freq / 1000, length) samples, computed on the same stream before the
 *                 frames, into the object's scratch (8 * fftN bytes per head frame).  calc_len_ms * smp_freq / 1000
 *                 < framesize is refused (the reference's start-up rule, m_fusion.c:1403-1412);
 *   JAMD_SS_LOAD  one spectrum (host array of fftN floats, uploaded once by the call) for every utterance;
 *                 noise == NULL or noise_len != fftN is refused;
 *   JAMD_SS_OFF   the front end without spectral subtraction.
 * A refused call (also an unknown mode) leaves the object as it was.  Where the reference divides 0 by 0 (|X| == 0
 * over a noise entry of 0, or alpha 0) the features are NaN here too. */
#define JAMD_SS_OFF  0
#define JAMD_SS_CALC 1            /* -sscalc [-sscalclen]: noise spectrum from the head of every utterance */
#define JAMD_SS_LOAD 2            /* -ssload: one spectrum for every utterance */
typedef struct {
  int mode, calc_len_ms;          /* -sscalclen */
  float alpha, floor;             /* -ssalpha, -ssfloor */
  const float *noise; int noise_len;   /* JAMD_SS_LOAD: host array, must be fftN long */
} jamd_frontend_ss;
int  jamd_frontend_ss_default(jamd_frontend_ss *ss);                 /* OFF, 300, DEF_SSALPHA, DEF_SSFLOOR, NULL, 0 */
int  jamd_frontend_set_ss(jamd_frontend *f, const jamd_frontend_ss *ss);
int  jamd_frontend_fftn(const jamd_frontend *f);
/* new_SS_calculate() per utterance over its first min(head_samples, length) samples (head_samples <= 0: the whole
 * utterance, which is what mkss computes): out [nutt][fftN] float.  An utterance whose head holds no full frame:
 * JAMD_EINVAL, nothing written.  Uses the object's scratch like jamd_frontend_run_dev(). */
int  jamd_frontend_noise_dev (jamd_frontend *f, const int16_t *dev_samples, const int64_t *sample_off, int nutt,
                              int64_t head_samples, float *dev_noise, void *stream);
int  jamd_frontend_noise_host(jamd_frontend *f, const int16_t *samples, const int64_t *sample_off, int nutt,
                              int64_t head_samples, float *noise);
/* host only: the mkss / -ssload file format (big-endian int32 count, then that many big-endian float32).  read
 * returns the count in the file (copies min(count, cap)); a file shorter than its count is refused. */
int  jamd_frontend_ss_read (const char *path, float *out, int cap);
int  jamd_frontend_ss_write(const char *path, const float *noise, int n);

/* ---- live-input front end: whole segments of many independent channels per call ----------------
 * What the reference computes for a microphone, a socket or -realtime, bit-identical: the vectors RealTimeMFCC()
 * (libjulius/src/realtime-1stpass.c:496-602) and the flush loop of RealTimeParam() (:1215-1304, splicing included)
 * store into mfcc->param, from the state reset_mfcc() / CMN_realtime_prepare() leave.  They differ from the buffered
 * features in every normalised element: the cepstral mean is MAP over the frames seen so far, seeded from earlier
 * segments (CMN_realtime(), wav2mfcc-pipe.c:342-399); the energy is normalised by the previous segment's maximum
 * (energy_max_normalize()); the deltas go through the cyclic buffers in float (WMP_deltabuf_calc()); the window is
 * framesize + 1 samples.  The object is made from a created jamd_frontend, whose tables, frame kernel, spectral
 * subtraction (JAMD_SS_LOAD / JAMD_SS_OFF) and device scratch it shares: the one-stream rule of
 * jamd_frontend_run_dev() covers the parent and every live object made from it together.  The state the reference
 * carries from one utterance to the next (ENERGYWork.max, CMNWork) is kept per channel on the device.
 * Which julius option is which call: INTEGRATION.md.
 *
 * A segment goes in whole (jamd_frontend_live_run_*) or in chunks cut anywhere (jamd_frontend_live_push_*): the
 * reference is frame-synchronous, so both deliver the same rows and leave the same state.
 *
 * NOT SERVED: _N together with _A (refused by _create: the reference's two loops disagree on it,
 * realtime-1stpass.c:1233-1241 against :583-587); JAMD_SS_CALC on the parent (refused by _run / _push: a live segment
 * has no head known in advance); frameshift beyond the window; gzipped -cmnload files.  -48, -lvscale, -zmean and
 * zero-sample stripping: jamd_adin_*; silence cutting (-cutsilence, -lv, -zc): jamd_adin_cut_*, whose rows are this
 * object's pushes; both in front of this object. */
typedef struct {
  int   map_cmn;                 /* 1 = MAP-CMN, 0 = -cmnstatic (CMNWork.do_map)                          */
  float map_weight;              /* -cmnmapweight                                                         */
  const float *cmean_init;       /* -cmnload, for every channel: [veclen] or NULL (cmean_init_set FALSE)  */
  const float *cvar_init;        /* [veclen] or NULL; read only when the kind has cvn, then needed        */
} jamd_frontend_live_desc;
typedef struct jamd_frontend_live jamd_frontend_live;
#define JAMD_LIVE_CMEAN_SET 1    /* flags of _state_get: CMNWork.cmean_init_set                           */
#define JAMD_LIVE_LOADED    2    /*                      CMNWork.loaded_from_file                         */

int  jamd_frontend_live_default(jamd_frontend_live_desc *d);          /* 1, 100.0 (default.c:153-156), NULL, NULL */
/* nchan channels, each with the state of a fresh start (energy maximum 5.0, no history).  `f` must outlive it. */
int  jamd_frontend_live_create(jamd_frontend *f, const jamd_frontend_live_desc *d, int nchan, jamd_frontend_live **out);
void jamd_frontend_live_destroy(jamd_frontend_live *l);
/* Host only.  Rows one segment of nsamples samples yields.  Not jamd_frontend_frames(): the live window is
 * framesize + 1 samples (realtime-1stpass.c:290), so Tb = (n - framesize - 1) / frameshift + 1 base frames for
 * n >= framesize + 1; the flush loop ends at the first WMP_deltabuf_flush() that finds its slot empty, so with _D a
 * segment of Tb < delWin emits nothing, and with _A neither does one of fewer than accWin delta vectors; splice takes
 * splice - 1 more.  Never negative.  (Where the delta vectors of the flush loop meet an acceleration buffer still in
 * its delay, Tb < delWin + accWin, the reference advances its frame counter without storing a vector; the rows
 * counted and returned here are the vectors it does store.) */
int  jamd_frontend_live_frames(const jamd_frontend_desc *d, int64_t nsamples);
/* One segment per channel: channel c gets samples [sample_off[c], sample_off[c+1]) of dev_samples (host offsets
 * [nchan + 1]).  Output as jamd_frontend_run_dev(): rows back to back in dev_out, host row offsets [nchan + 1] in
 * frame_off (may be NULL).  A channel without samples is idle: no rows, its state untouched.  A channel whose segment
 * yields no row is no error: it reports none, the maximum of its base frames' energies still becomes the next
 * segment's, and a commit leaves it alone (CMN_realtime_update() returns when now.framenum is 0).  Every run starts
 * from CMN_realtime_prepare(): two runs without a commit between them both start from the same initial mean. */
int  jamd_frontend_live_run_dev (jamd_frontend_live *l, const int16_t *dev_samples, const int64_t *sample_off,
                                 float *dev_out, int *frame_off, void *stream);
int  jamd_frontend_live_run_host(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off, float *out,
                                 int *frame_off);
/* A segment in chunks.  Channel c appends samples [sample_off[c], sample_off[c+1]) (host offsets [nchan + 1]) to its
 * open segment; its first push after creation or after a segment ended opens one (reset_mfcc() +
 * CMN_realtime_prepare() + energy_max_prepare()).  A non-zero byte of `final` ([nchan], host; NULL = none) ends the
 * channel's segment behind this chunk: the flush loop of RealTimeParam() runs, the segment's energy maximum becomes the
 * next one's, and now.mfcc_sum / mfcc_var / framenum are where jamd_frontend_live_commit() reads them.  The rows the
 * call completes go back to back into dev_out, their host offsets into frame_off (may be NULL); how many a push
 * yields: jamd_frontend_live_push_frames().  However a segment is cut, its pushes deliver, concatenated, the rows one
 * jamd_frontend_live_run_*() over the concatenated samples delivers, and leave the same state.  A channel with no
 * samples and a zero byte is untouched; with no samples and a non-zero byte its open segment ends (without one:
 * nothing happens).  dev_samples may be NULL when no channel has samples, dev_out when no row is due.
 * Per channel the device keeps the samples behind the last whole window, the last 2 * (delWin + accWin) base vectors,
 * the running energy maximum, the CMN chains and the last splice - 1 vectors.  The call is queued on `stream` and
 * allocates only when a buffer has to grow; like _run_dev it waits for the previous call's offset upload alone.
 * While a channel's segment is open, _run_* (any channel open), _commit with a non-zero byte for it and _state_set on
 * it return JAMD_ESTATE.  Whole segments and chunked ones may alternate on one object. */
int  jamd_frontend_live_push_dev (jamd_frontend_live *l, const int16_t *dev_samples, const int64_t *sample_off,
                                  const unsigned char *final, float *dev_out, int *frame_off, void *stream);
int  jamd_frontend_live_push_host(jamd_frontend_live *l, const int16_t *samples, const int64_t *sample_off,
                                  const unsigned char *final, float *out, int *frame_off);
/* Host only.  Rows a push of `chunk` samples yields on a segment that has taken samples_before.  With
 * L = (delta ? delWin : 0) + (acc ? accWin : 0) and Tb(n) the base frames of n samples, max(0, Tb - L) vectors have
 * left the main loop before the end, and from the splice-th on each completes a row:
 * max(0, max(0, Tb - L) - (splice - 1)) rows so far.  final != 0: what is left of jamd_frontend_live_frames() of
 * all the samples. */
int  jamd_frontend_live_push_frames(const jamd_frontend_desc *d, int64_t samples_before, int64_t chunk, int final);
/* With cvn and splice 1 the reference re-estimates now.mfcc_var at the end of a segment from every stored row
 * (wav2mfcc-pipe.c:418-434), so the object keeps the rows of each open segment: at most max_rows per channel
 * (default 3000, half a minute at 10 ms; the buffer grows on demand up to it).  A push that would pass it returns
 * JAMD_EINVAL before anything is launched, the state unchanged.  Other kinds keep no rows.  JAMD_ESTATE while a
 * segment is open. */
int  jamd_frontend_live_stream_cap(jamd_frontend_live *l, int max_rows);
/* CMN_realtime_update(wrk, param) (wav2mfcc-pipe.c:407-479) for the channels whose byte of `update` ([nchan], host) is
 * non-zero; NULL = every channel.  -cmnnoupdate: never call it; an input that was rejected
 * (realtime-1stpass.c:1416-1442): a zero byte.  Queued on `stream` behind the run it belongs to.  It is that call
 * and nothing more: it works on the channel's last segment, so give a channel that was idle in the run a zero byte
 * (a non-zero one enters its last segment into the history again, as a second CMN_realtime_update() would).  The energy maximum
 * is not its business: it moves at the next run, where energy_max_prepare() sits. */
int  jamd_frontend_live_commit(jamd_frontend_live *l, const unsigned char *update, void *stream);
/* The state of one channel after everything queued so far (both wait for the device): cmean_init / cvar_init [veclen]
 * (cvar only meaningful with cvn), ENERGYWork.max, JAMD_LIVE_* flags; any pointer may be NULL.  _state_set is -cmnload
 * on that channel (cvar needed when the kind has cvn): as CMN_load_from_file() it also stops the variance updates. */
int  jamd_frontend_live_state_get(jamd_frontend_live *l, int chan, float *cmean, float *cvar, float *emax, int *flags);
int  jamd_frontend_live_state_set(jamd_frontend_live *l, int chan, const float *cmean, const float *cvar);
/* host only: the -cmnload / -cmnsave file.  read takes both forms of CMN_load_from_file() (:514-652): the ASCII
 * <CEPSNORM> form, whose <MEAN> has veclen or mfcc_dim (cepstra + c0) entries and whose <VARIANCE> is optional, and
 * the old big-endian binary form (whose variance is read when want_var != 0).  Returns 1 when a variance was read, 0
 * for a mean alone, JAMD_EINVAL where the reference refuses the file.  write is CMN_save_to_file(), byte for byte;
 * cvar == NULL writes no variance. */
int  jamd_frontend_cmn_read (const char *path, int veclen, int mfcc_dim, int want_var, float *cmean, float *cvar);
int  jamd_frontend_cmn_write(const char *path, int veclen, const float *cmean, const float *cvar);

/* ---- audio conditioning in front of the two front ends: -48, -lvscale, zero stripping, -zmean -------------
 * What adin_cut() does to the samples of one ad_read() before anything looks at them (libjulius/src/adin-cut.c:470-545),
 * bit-identical and in its order: ds48to16() (three double FIR stages 48 -> 64 -> 32 -> 16 kHz), the level scaling
 * (SP16)((float)s * coef), strip_zero() (runs of 16 or more samples that are 0 or -32767 are dropped) and sub_zmean()
 * (the mean of the first 48000 samples, estimated chunk by chunk).  strip_zero() and sub_zmean() act per read, so their
 * result depends on how the input was cut: one push is one ad_read() per channel.  For file input the reference's first
 * read asks for 320000 samples (960000 under -48): a file shorter than 20 s is one chunk.  The output is what
 * jamd_frontend_run_dev() / jamd_frontend_live_push_dev() take as dev_samples, the offsets their sample_off: samples
 * never visit the host.  The down-sampling state (filter history, pending samples, the spent delay) and the DC state
 * (zlen, zmean) are kept per channel on the device.  The reference resets the second at every stream start
 * (zmean_reset(), adin-cut.c:1416,1444) and the first never (the DS_BUFFER is made once, m_adin.c:216): the program
 * carries filter state from one file into the next, hence the two bits of jamd_adin_reset().  ds48to16_new() leaves the
 * filter history uninitialised; here the samples before the stream start are 0.0.
 * Silence cutting (-cutsilence, -lv, zero-cross counting) is the next stage: jamd_adin_cut_*, below. */
typedef struct {
  int   down48;                  /* -48: the input is 48 kHz                                              */
  const double *fir_3to4;        /* the caller's lpfcoef_3to4[] (n_3to4 entries) and lpfcoef_2to1[]: from */
  int   n_3to4;                  /* libsent, or a file through jamd_adin_fir_read(); 1 ... 513 entries    */
  const double *fir_2to1;        /* each, needed with down48, copied by _create                           */
  int   n_2to1;
  float level_coef;              /* -lvscale; applied when != 1.0; 32768 * |coef| < 2^31                  */
  int   strip_zero;              /* default 1 (default.c:92); -nostrip: 0                                 */
  int   zmean;                   /* -zmean                                                                */
} jamd_adin_desc;
typedef struct jamd_adin jamd_adin;
#define JAMD_ADIN_DS    1        /* jamd_adin_reset(): the down-sampling state, as ds48to16_new() leaves it */
#define JAMD_ADIN_ZMEAN 2        /*                    zmean_reset()                                        */

int  jamd_adin_default(jamd_adin_desc *d);                   /* 0, NULL / 0, NULL / 0, 1.0, 1, 0 */
/* host only: the text format of the reference's load_filter(): one atof() per line, 513 entries at the most.  Returns
 * the number of entries; JAMD_EINVAL for a file that cannot be read, holds none, or holds more than `cap`. */
int  jamd_adin_fir_read(const char *path, double *out, int cap);
/* nchan channels, each as ds48to16_new() + zmean_reset() leave it */
int  jamd_adin_create(jamd_engine *e, const jamd_adin_desc *d, int nchan, jamd_adin **out);
void jamd_adin_destroy(jamd_adin *a);
/* The channels with a non-zero byte of mask ([nchan], host; NULL = all) go back to the start: `what` is
 * JAMD_ADIN_DS | JAMD_ADIN_ZMEAN or one of them.  Queued on `stream`. */
int  jamd_adin_reset(jamd_adin *a, const unsigned char *mask, int what, void *stream);
/* host only: 16 kHz samples that a push of `chunk` 48 kHz samples completes on a channel that has taken
 * samples_before since its last JAMD_ADIN_DS reset.  Each stage consumes whole blocks of 256 of its input and drops its
 * first hdn_len / (2 * decrate) outputs, so the first 767 samples of a stream yield nothing.  Needs n_3to4 / n_2to1 of
 * the descriptor only.  Without down48: chunk. */
int64_t jamd_adin_ds_count(const jamd_adin_desc *d, int64_t samples_before, int64_t chunk);
/* host only: an upper bound of what such a push writes (zero stripping can only shorten it), for sizing dev_out */
int64_t jamd_adin_push_cap(const jamd_adin_desc *d, int64_t samples_before, int64_t chunk);
/* One chunk per channel: channel c's is [in_off[c], in_off[c+1]) of dev_in (host offsets [nchan + 1]).  The conditioned
 * samples go back to back into dev_out (room: the sum of jamd_adin_push_cap()), their host offsets [nchan + 1] into
 * out_off.  A channel with an empty chunk is idle: its state is untouched and sub_zmean() is not called; a chunk that
 * stripping empties still is one (with zlen 0 the reference's mean becomes 0 / 0 and every later sample 0; so here).
 * With strip_zero the counts are data: the call returns after they have arrived, which costs one wait on `stream`.
 * Without it they are closed-form and the call only enqueues.  One stream per object, as for jamd_frontend_run_dev(). */
int  jamd_adin_push_dev (jamd_adin *a, const int16_t *dev_in, const int64_t *in_off, int16_t *dev_out, int64_t *out_off,
                         void *stream);
/* The same from and to host memory, on the engine's stream; `out` has room for the sum of jamd_adin_push_cap(). */
int  jamd_adin_push_host(jamd_adin *a, const int16_t *samples, const int64_t *in_off, int16_t *out, int64_t *out_off);
/* One channel after everything queued so far (waits for the device): sub_zmean()'s zlen and zmean, and per FIR stage the
 * inputs arrived and the outputs handed on since the last JAMD_ADIN_DS reset ([3] each).  Any pointer may be NULL. */
int  jamd_adin_state_get(jamd_adin *a, int chan, int *zlen, float *zmean, int64_t *arrived, int64_t *emitted);

/* ---- silence cutting between jamd_adin and the live front end: -cutsilence, -lv, -zc, -headmargin, -tailmargin ----
 * The rest of adin_cut() (libjulius/src/adin-cut.c:600-984) around count_zc_e() (libsent/src/adin/zc-e.c): the
 * conditioned stream of a channel is walked in blocks of chunk_size samples however the pushes cut it; a block whose
 * zero-cross count over the last c_length samples passes the threshold triggers; the head margin comes out of the cycle
 * buffer, the tail margin is delivered, blocks behind it wait in the swap buffer for a re-trigger, and nc_max blocks
 * below the threshold end the segment.  What the reference would have passed to ad_process() after the samples given so
 * far is delivered, in its order, bit for bit.  Every delivery is a contiguous range of the stream, so the device keeps
 * per channel the last max(c_length, sbsize) + chunk_size samples (with their running crossing count) and copies
 * ranges; cbuf / swapbuf have no copies.  Per channel it also keeps is_valid_data, nc, rest_tail, sblen, the trigger
 * state of count_zc_e() and the samples of an incomplete block.
 * -fvad / -fvad_param (the libfvad detector gating the trigger) is jamd_adin_cut_create_fvad(), further below.
 * NOT SERVED: -rejectshort / -powerthres; segmentation asked for by the recogniser (ad_process() returning 1) or
 * by MAXSPEECHLEN; last_trigger_len beyond part_start; audio files in jamd_batch.  Descriptors with which the reference
 * overruns its swap buffer are refused (jamd_adin_cut_params()). */
typedef struct {
  int sfreq;                     /* of the samples given: 16000 behind jamd_adin                          */
  int level_thres;               /* -lv        (default.c:75-80: 2000)                                    */
  int zero_cross_num;            /* -zc        (60 per second)                                            */
  int head_margin_msec;          /* -headmargin (300)                                                     */
  int tail_margin_msec;          /* -tailmargin (400)                                                     */
  int chunk_size;                /* -chunksize (1000)                                                     */
} jamd_adin_cut_desc;
typedef struct jamd_adin_cut jamd_adin_cut;

int  jamd_adin_cut_default(jamd_adin_cut_desc *d);           /* 16000, 2000, 60, 300, 400, 1000 */
/* host only: adin_setup_param()'s c_length, noise_zerocross, nc_max and sbsize in its arithmetic (any pointer may be
 * NULL).  JAMD_EINVAL for sfreq <= 0, chunk_size < 1, chunk_size > c_length (as the reference), negative margins or
 * counts, sizes beyond 2^24, and where (nc_max - ceil((sbsize - c_length) / chunk_size)) * chunk_size > sbsize: there
 * the reference logs "swap buffer for re-triggering overflow" and writes past swapbuf (-headmargin 30 -tailmargin 40
 * -chunksize 480 is one). */
int  jamd_adin_cut_params(const jamd_adin_cut_desc *d, int *c_length, int *noise_zerocross, int *nc_max, int *sbsize);
/* nchan channels, each as need_init leaves it.  JAMD_EINVAL where jamd_adin_cut_params() refuses. */
int  jamd_adin_cut_create(jamd_engine *e, const jamd_adin_cut_desc *d, int nchan, jamd_adin_cut **out);
void jamd_adin_cut_destroy(jamd_adin_cut *k);
/* The channels with a non-zero byte of mask ([nchan], host; NULL = all) go back to the start.  Queued on `stream`. */
int  jamd_adin_cut_reset(jamd_adin_cut *k, const unsigned char *mask, void *stream);
/* host only: upper bounds of the samples one channel can be handed in a push of `chunk` samples, and of its parts.
 * With B = (chunk + chunk_size - 1) / chunk_size + 1 blocks at the most (a full carry, a short last block) and triggers,
 * like ends, nc_max + 1 blocks apart, E = 1 + (B - 1) / (nc_max + 1) of either fit into a push:
 *   samples  chunk + (chunk_size - 1) + sbsize + E * c_length   (a second trigger's head margin delivers again what
 *            the tail before it has delivered; for E = 1 this is chunk + (chunk_size - 1) + c_length + sbsize)
 *   parts    E + 1
 * Negative (JAMD_EINVAL) for a refused descriptor or chunk < 0. */
int64_t jamd_adin_cut_push_cap (const jamd_adin_cut_desc *d, int64_t chunk);
int64_t jamd_adin_cut_parts_cap(const jamd_adin_cut_desc *d, int64_t chunk);
/* Channel c appends [in_off[c], in_off[c+1]) of dev_in (host offsets [nchan + 1]): what jamd_adin_push_dev() returns, or
 * raw samples.  A non-zero byte of eos ([nchan], host; NULL = none) ends the channel's stream behind this chunk: the
 * remainder is processed as one short block, an open segment closes and the channel is as created.  A channel with an
 * empty chunk and a zero byte is untouched.
 * A channel's deliveries are cut into parts at each segment end: an ended segment closes its part (which may be empty:
 * the block that ends a segment is never delivered), so a segment can only open at a part's beginning.  dev_out (room:
 * the sum of jamd_adin_cut_push_cap()) holds part 0 of channels 0 ... nchan-1 back to back, then part 1, and so on; per
 * part p, host tables with max_parts rows of room:
 *   part_off  [p * (nchan + 1) + c]  int64: where channel c's samples of the part begin; entry nchan: where the part ends
 *   part_final[p * nchan + c]        1: the channel's segment ends behind this part (by silence, or by eos)
 *   part_start[p * nchan + c]        the stream index (samples given to the channel since its last reset) of the first
 *                                    sample of a segment that opens in this part, else -1
 * Row p of part_off and part_final are the sample_off and final of one jamd_frontend_live_push_dev() over dev_out.
 * *nparts is the number of parts in use (0 where nothing was delivered and nothing ended).  The part count is data: the
 * call waits once on `stream` for the tables.  If more than max_parts are needed it returns JAMD_EINVAL with *nparts set
 * and nothing changed: no state has moved, the push can be repeated with more room.  One stream per object. */
int  jamd_adin_cut_push_dev (jamd_adin_cut *k, const int16_t *dev_in, const int64_t *in_off, const unsigned char *eos,
                             int16_t *dev_out, int max_parts, int *nparts, int64_t *part_off, unsigned char *part_final,
                             int64_t *part_start, void *stream);
/* The same from and to host memory, on the engine's stream; `out` has room for the sum of jamd_adin_cut_push_cap(). */
int  jamd_adin_cut_push_host(jamd_adin_cut *k, const int16_t *samples, const int64_t *in_off, const unsigned char *eos,
                             int16_t *out, int max_parts, int *nparts, int64_t *part_off, unsigned char *part_final,
                             int64_t *part_start);
/* One channel after everything queued so far (waits for the device): is_valid_data, nc, rest_tail, sblen, the
 * zero-cross count of the last block, the samples waiting for their block to fill, and the samples given since the last
 * reset.  Any pointer may be NULL. */
int  jamd_adin_cut_state_get(jamd_adin_cut *k, int chan, int *is_valid, int *nc, int *rest_tail, int *sblen,
                             int *zero_cross, int *carried, int64_t *stream_pos);

/* ---- the voice-activity detector behind -fvad: libfvad (WebRTC VAD) on 10 ms frames, many channels per call ----
 * What fvad_process() (libjulius/libfvad) returns for each 10 ms frame of a channel's stream, before it is clamped to
 * 0 / 1: the core's raw value, 0 for noise, 1 for speech, 2 + the hangover left for a noise frame inside the hangover.
 * 16-bit and 32-bit integer arithmetic throughout, bit for bit the reference's, its wrap-arounds on saturated input
 * included.  At 16 kHz a two-branch all-pass halves the rate; five all-pass split filters and a high-pass make six
 * bands; each band gives a log energy; two Gaussians per band for noise and for speech decide, and the decision says
 * which of the two models adapts.  The filter states, the adapted models, the minimum tracker and the hangover are kept
 * per channel on the device, with the samples of an incomplete frame.
 * Every array constant of the reference comes from the caller (as the FIR tables of -48 do): jamd_fvad_model, filled
 * from a file that julius_amd/shim/jamd_fvad_export writes out of the user's Julius tree.
 * NOT SERVED: 32000 and 48000 Hz input (valid in libfvad); frames of 20 and 30 ms (Julius uses 10 ms). */
typedef struct {
  int allpass_q15[2];            /* vad_filterbank.c kAllPassCoefsQ15: the split filters' two branches      */
  int allpass_q13[2];            /* vad_sp.c         kAllPassCoefsQ13: the 16 -> 8 kHz stage                */
  int hp_zero[3];                /* vad_filterbank.c kHpZeroCoefs                                           */
  int hp_pole[3];                /*                  kHpPoleCoefs                                           */
  int offset[6];                 /*                  kOffsetVector, per band                                */
  int spectrum_weight[6];        /* vad_core.c       kSpectrumWeight                                        */
  int min_diff[6];               /*                  kMinimumDifference                                     */
  int max_speech[6];             /*                  kMaximumSpeech                                         */
  int max_noise[6];              /*                  kMaximumNoise                                          */
  int min_mean[2];               /*                  kMinimumMean, per Gaussian                             */
  int noise_weight[12];          /*                  kNoiseDataWeights  [band + 6 * gaussian]               */
  int speech_weight[12];         /*                  kSpeechDataWeights                                     */
  int noise_mean[12];            /*                  kNoiseDataMeans                                        */
  int speech_mean[12];           /*                  kSpeechDataMeans                                       */
  int noise_std[12];             /*                  kNoiseDataStds                                         */
  int speech_std[12];            /*                  kSpeechDataStds                                        */
  int over_hang_1[4];            /* per mode 0 ... 3, the entries for 10 ms frames: kOverHangMax1*[0]       */
  int over_hang_2[4];            /*                                                  kOverHangMax2*[0]       */
  int local_thres[4];            /*                                                  kLocalThreshold*[0]     */
  int global_thres[4];           /*                                                  kGlobalThreshold*[0]    */
} jamd_fvad_model;
#define JAMD_FVAD_MODEL_INTS 130 /* entries of jamd_fvad_model, each a 16-bit value                          */
typedef struct {
  int sfreq;                     /* 8000 or 16000                                                            */
  int mode;                      /* -fvad: 0 ... 3                                                           */
  const jamd_fvad_model *model;  /* copied by _create                                                        */
} jamd_fvad_desc;
typedef struct jamd_fvad jamd_fvad;
/* jamd_fvad_state_get(): the core of one channel as integers, named as in the reference's VadInstT:
 *   [0..1] downsampling_filter_states[0..1]   [2..13] noise_means   [14..25] speech_means   [26..37] noise_stds
 *   [38..49] speech_stds   [50] frame_counter   [51] over_hang   [52] num_of_speech   [53..148] index_vector
 *   [149..244] low_value_vector   [245..250] mean_value   [251..255] upper_state   [256..260] lower_state
 *   [261..264] hp_filter_state   [265] samples of an incomplete frame that wait on the device */
#define JAMD_FVAD_STATE_INTS 266

/* host only: the model file, JAMD_FVAD_MODEL_INTS decimal integers in the order of the members above, one per line;
 * empty lines and lines that begin with '#' are skipped.  JAMD_EINVAL for a file that cannot be read, holds a line that
 * is no integer or no 16-bit value, or holds fewer or more entries. */
int  jamd_fvad_model_read(const char *path, jamd_fvad_model *m);
/* nchan channels, each as fvad_new() + fvad_set_mode() leave it.  JAMD_EINVAL for a rate other than 8000 / 16000 (the
 * reference ignores fvad_set_sample_rate()'s failure and goes on at 8000; not reproduced), a mode outside 0 ... 3, a
 * NULL model or a model entry that is no 16-bit value. */
int  jamd_fvad_create(jamd_engine *e, const jamd_fvad_desc *d, int nchan, jamd_fvad **out);
void jamd_fvad_destroy(jamd_fvad *f);
/* The channels with a non-zero byte of mask ([nchan], host; NULL = all) get a fresh core and lose their waiting samples.
 * Queued on `stream`. */
int  jamd_fvad_reset(jamd_fvad *f, const unsigned char *mask, void *stream);
/* host only: frames that a push of `chunk` samples completes on a channel that has taken samples_before since its last
 * reset: floor((samples_before + chunk) / fs) - floor(samples_before / fs) with fs = sfreq / 100.  Needs sfreq only. */
int64_t jamd_fvad_frames(const jamd_fvad_desc *d, int64_t samples_before, int64_t chunk);
/* Channel c appends [in_off[c], in_off[c+1]) of dev_in (host offsets [nchan + 1], as for jamd_adin_push_dev()).  Every
 * frame that completes is processed; the rest waits on the device.  Per frame one byte, the core's raw value, goes to
 * dev_out, channel after channel; their host offsets [nchan + 1] into out_off.  The counts are closed-form
 * (jamd_fvad_frames()), so the call only enqueues.  A channel with an empty chunk is untouched.  One stream per object. */
int  jamd_fvad_push_dev (jamd_fvad *f, const int16_t *dev_in, const int64_t *in_off, unsigned char *dev_out,
                         int64_t *out_off, void *stream);
/* The same from and to host memory, on the engine's stream; `out` has room for the sum of jamd_fvad_frames(). */
int  jamd_fvad_push_host(jamd_fvad *f, const int16_t *samples, const int64_t *in_off, unsigned char *out, int64_t *out_off);
/* One channel after everything queued so far (waits for the device): state [JAMD_FVAD_STATE_INTS], in the order above. */
int  jamd_fvad_state_get(jamd_fvad *f, int chan, int *state);

/* ---- -fvad / -fvad_param inside the silence cutting: the detector gates the zero-cross trigger ----------------
 * adin_cut() calls fvad_proceed() for every block before it tests the zero-cross count, and the block triggers only if
 * both hold (adin-cut.c:264-311, :662-668).  fvad_proceed() runs the detector on the 10 ms frames of the stream -- a
 * frame only once one more sample is there, so max(0, ceil(e / fs) - 1) frames by the end e of a block, on a grid fixed
 * at the stream's start whatever the blocks are -- and answers whether, of the last `smoothnum` results (zeros before
 * the first), the mean in float reaches `thres`.  need_init (end of stream, jamd_adin_cut_reset()) clears the results
 * and the grid but not the detector: fvad_new() is called once and fvad_reset() never, so filter states, adapted models
 * and hangover run on into the next stream, as the -48 filter state does.  A last whole frame that still waited for
 * its one more sample at the end of a stream never reaches the detector.
 * A push runs the detector over exactly the frames the reference has processed by the end of the last block the push
 * walks, reading samples of earlier pushes out of the channel's history, and commits the detector with the rest of
 * the state: a push refused for max_parts leaves it where it was. */
typedef struct {
  jamd_fvad_desc det;            /* sfreq must be the cutting descriptor's                                  */
  int   smoothnum;               /* -fvad_param, first argument:  1 ... JAMD_FVAD_SMOOTH_MAX (default.c: 5) */
  float thres;                   /*              second argument: 0 ... 1 (0.5); 0 never closes the gate    */
} jamd_adin_cut_fvad;
#define JAMD_FVAD_SMOOTH_MAX 1000
/* As jamd_adin_cut_create(), with the gate.  JAMD_EINVAL where that or jamd_fvad_create() refuses, for smoothnum or
 * thres out of range (the reference clamps with a warning, m_chkparam.c:349-371), for det.sfreq != d->sfreq, and for
 * chunk_size + sfreq / 100 > 320000 (MAXSPEECHLEN), where fvad_proceed() drops samples. */
int  jamd_adin_cut_create_fvad(jamd_engine *e, const jamd_adin_cut_desc *d, const jamd_adin_cut_fvad *fv, int nchan,
                               jamd_adin_cut **out);
/* The channels with a non-zero byte of mask ([nchan], host; NULL = all) get a fresh detector, as fvad_new() +
 * fvad_set_mode() leave it; nothing else of them changes.  JAMD_EINVAL for an object without the gate.  Queued on
 * `stream`. */
int  jamd_adin_cut_fvad_reset(jamd_adin_cut *k, const unsigned char *mask, void *stream);
/* The detector of one channel after everything queued so far, as jamd_fvad_state_get() (the last entry is 0: nothing
 * waits here, the frames are read out of the history). */
int  jamd_adin_cut_fvad_state_get(jamd_adin_cut *k, int chan, int *state);

#ifdef __cplusplus
}
#endif
#endif /* JULIUS_AMD_H */
