// gmm_ms_tied.hip -- K1mt: state likelihoods of a MULTI-STREAM GMM acoustic model with tied-mixture codebooks, and of
// any multi-stream model under gprune safe, for gfx950 (CDNA4).
//
// Replaces, for a chunk of frames at once, the stream loops of calc_tied_mix() and calc_compound_mix()
// (libsent/src/phmm/calc_tied_mix.c:177-236, :274-345) over the per-(frame, codebook) cache (:189-227), under
// gprune_none() (gprune_none.c:133-147) or gprune_safe() (gprune_safe.c:160-202), and calc_mix()'s (calc_mix.c:52-80)
// under gprune_safe().
//
// Three kernels, K1m's plan in each (one lane = one frame, a packed pair per lane; Gaussian records wave-uniform through
// scalar loads; the wave's frames in LDS transposed [d][128]; gauss_slice's arithmetic; nothing fused):
//   ms_book_kernel   per (frame block, book) over the slice of the book's stream: the cache row of every frame.
//                    none: every member's score in index order.  safe: a register-resident top-N in index order
//                    (topn_push_safe), and a mark on the frames where the visiting order can show (topn_order_shows).
//                    A book is a codebook of the model, or -- under safe -- a plain pdf's own Gaussians: gprune_safe()
//                    called without history (calc_compound_mix :330, calc_mix) keeps the same list in the same order,
//                    and `score + ln w` summed from the last slot down is what calc_tied_mix does with `bweight`.
//   ms_order_kernel  safe, codebooks only: one wave per (codebook, run of frames that have a predecessor in their
//                    utterance) walks the marked frames in order, starting from frame t - 1's winners, as
//                    tmix_book_safe_order_kernel (gmm_pruned.hip) does over the whole vector.  Cache row 0 holds the
//                    last frame of the chunk before, so a chunk's first frame finds its history like any other.
//   ms_state_kernel  16 states x 128 frames per wave tile as K1m.  Stream loop per state: a cached pdf takes
//                    `score + bweight[id]` (one rounded add) of its book's cached slots, log-summed from the last slot
//                    down to the first; a plain pdf under none is K1m's loop; then `if (logprob <= LOG_ZERO) continue;
//                    logprobsum += logprob * weight`, and finish_state().
// See DESIGN.md "K1mt".
#include "gmm_ms_dev.h"
#include "gmm_ms_host.h"

namespace {
using namespace jamd;

constexpr int kWaves = 4;    // waves per workgroup
constexpr int kNS = 16;      // states per block = the width of the output tile (as K1m)
constexpr int kFPW = kMsFPW;

__device__ __forceinline__ int ms_rec(int len) { return ((2 * len + 2) + 3) & ~3; }

// ---- the cache: per (frame, book) the scores the states of that frame share -----------------------------------
// frames -> the chunk's first frame, n its frames.  The cache is [book][slot][rows] (score, id) and [book][rows] (num,
// mark), frames innermost: a wave's lanes are consecutive frames, so its stores here and its loads in the state kernel
// are whole lines.  Row t + 1 is frame t's (row 0: the chunk before).  NMAX == 0: gprune none.
template <int NMAX>
__global__ void __launch_bounds__(64 * kWaves)
ms_book_kernel(const float *__restrict__ rec, const JamdMsBook *__restrict__ book, const float *__restrict__ frames,
               float *__restrict__ c_score, int *__restrict__ c_id, int *__restrict__ c_num, int *__restrict__ c_flag,
               int n, int D, int rows, int cap) {
  extern __shared__ __align__(16) float dyn[];  // [kWaves][len][kFPW]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = (blockIdx.y * kWaves + wave) * kFPW;   // (books on x: a model may have more than 65535)
  if (t0 >= n) return;
  const int b = blockIdx.x;
  const JamdMsBook bk = book[b];
  const int len = bk.len;
  float *vs = dyn + (size_t)wave * len * kFPW;  // the slice of the book's stream, nothing else of the vector
  {
    int ta = t0 + lane, tb = ta + 64;
    if (ta > n - 1) ta = n - 1;
    if (tb > n - 1) tb = n - 1;
    const float *fa = frames + (size_t)ta * D + bk.off, *fb = frames + (size_t)tb * D + bk.off;
    for (int d = 0; d < len; d++) { vs[d * kFPW + lane] = fa[d]; vs[d * kFPW + 64 + lane] = fb[d]; }
    wave_sync();
  }
  const int REC = ms_rec(len);
  const float *__restrict__ r0 = rec + (size_t)bk.rec;
  const int ta = t0 + lane, tb = ta + 64;
  const size_t ra = (size_t)b * rows + ta + 1, rb = ra + 64;              // (num, mark) of the lane's two frames
  const size_t oa = (size_t)b * cap * rows + ta + 1, ob = oa + 64;          // slot 0 of them; slot i is i * rows on
  if constexpr (NMAX == 0) {
    for (int k = 0; k < bk.n; k++) {
      const f2 g = gauss_slice(vs, lane, len, r0 + (size_t)k * REC);
      if (ta < n) { c_score[oa + (size_t)k * rows] = g.x; c_id[oa + (size_t)k * rows] = k; }
      if (tb < n) { c_score[ob + (size_t)k * rows] = g.y; c_id[ob + (size_t)k * rows] = k; }
    }
    if (ta < n) c_num[ra] = bk.n;
    if (tb < n) c_num[rb] = bk.n;
  } else {
    float sc0[NMAX], sc1[NMAX];
    int id0[NMAX], id1[NMAX];
    int len0 = 0, len1 = 0;
#pragma unroll
    for (int i = 0; i < NMAX; i++) { sc0[i] = sc1[i] = JAMD_LOG_ZERO; id0[i] = id1[i] = 0; }
    bool ord0 = false, ord1 = false;
    for (int k = 0; k < bk.n; k++) {
      const f2 g = gauss_slice(vs, lane, len, r0 + (size_t)k * REC);
      ord0 |= topn_order_shows<NMAX>(sc0, len0, g.x);
      ord1 |= topn_order_shows<NMAX>(sc1, len1, g.y);
      topn_push_safe<NMAX>(sc0, id0, len0, cap, g.x, k);
      topn_push_safe<NMAX>(sc1, id1, len1, cap, g.y, k);
    }
    if (ta < n) c_flag[ra] = ord0;
    if (tb < n) c_flag[rb] = ord1;
#pragma unroll
    for (int i = 0; i < NMAX; i++) {
      if (i < cap) {
        if (ta < n) { c_score[oa + (size_t)i * rows] = sc0[i]; c_id[oa + (size_t)i * rows] = id0[i]; }
        if (tb < n) { c_score[ob + (size_t)i * rows] = sc1[i]; c_id[ob + (size_t)i * rows] = id1[i]; }
      }
    }
    if (ta < n) c_num[ra] = len0;
    if (tb < n) c_num[rb] = len1;
  }
}

// ---- gprune safe: the frames where the visiting order shows, again in the reference's order -------------------
// gprune_safe() called with last_id = the codebook's winners of frame t - 1 (gprune_safe.c:166-183): those are scored by
// compute_g_base() and pushed first, then every other Gaussian in index order by compute_g_safe() against the list's
// last score, dropped unless above it.  One wave per (codebook, run): a marked frame's predecessor may be one the wave
// has just rewritten, so the run is walked in order.  The runs leave out every utterance's first frame: no history
// there (calc_tied_mix.c:203-215), index order is its order.
__global__ void __launch_bounds__(64)
ms_order_kernel(const float *__restrict__ rec, const JamdMsBook *__restrict__ book, const float *__restrict__ frames,
                const int *__restrict__ c_flag, float *__restrict__ c_score, int *__restrict__ c_id,
                int *__restrict__ c_num, const JamdMsSegs segs, int D, int rows, int cap) {
  extern __shared__ __align__(16) float dyn[];
  const int lane = threadIdx.x, b = blockIdx.x;
  const JamdMsBook bk = book[b];
  const int len = bk.len, K = bk.n, REC = ms_rec(len);
  float *x = dyn;                                      // [len]  the frame's slice
  int *calced = reinterpret_cast<int *>(x + len);      // [K]    mixcalced
  const float *__restrict__ r0 = rec + (size_t)bk.rec;
  for (int i = lane; i < K; i += 64) calced[i] = 0;
  TopList L; L.sc = JAMD_LOG_ZERO; L.id = 0; L.len = 0; L.cap = cap;
  int kept_t = -2;                                     // the frame whose list the registers hold (-1 is row 0's)
  wave_sync();
  const int first = segs.first[blockIdx.y], end = segs.end[blockIdx.y];
  for (int c0 = first; c0 < end; c0 += 64) {
    const int tc = c0 + lane;
    unsigned long long marked = __ballot(tc < end && c_flag[(size_t)b * rows + tc + 1] != 0);
    while (marked) {
      const int t = c0 + __ffsll((long long)marked) - 1;
      marked &= marked - 1ull;
      const size_t rp = (size_t)b * rows + t;          // frame t - 1's row (row 0: the chunk before)
      const size_t op = (size_t)b * cap * rows + t;    // ... and its slot 0
      int last_id, lnum;
      if (kept_t == t - 1) { last_id = L.id; lnum = L.len; }
      else {
        lnum = c_num[rp];
        last_id = lane < lnum ? c_id[op + (size_t)lane * rows] : 0;
      }
      if (lnum == 0) continue;                         // nothing cached for frame t - 1: no history
      for (int d = lane; d < len; d += 64) x[d] = frames[(size_t)t * D + bk.off + d];
      wave_sync();
      auto g_base = [&](int i) {                       // compute_g_base(), the operation order of gauss_slice()
        const float *__restrict__ r = r0 + (size_t)i * REC;
        const float gc = r[2 * len];
        float acc = gc;
        for (int d = 0; d < len; d++) { float v = x[d] - r[d]; v = v * v; v = v * r[len + d]; acc = acc + v; }
        return (gc != gc) ? JAMD_LOG_ZERO : acc * -0.5f;
      };
      float psc = JAMD_LOG_ZERO;
      if (lane < lnum) { psc = g_base(last_id); calced[last_id] = 1; }
      wave_sync();
      L.len = 0;
      for (int j = 0; j < lnum; j++) L.push(__shfl(psc, j, 64), __shfl(last_id, j, 64), lane);
      float thres = __shfl(L.sc, L.len - 1, 64);
      for (int i0 = 0; i0 < K; i0 += 64) {
        const int i = i0 + lane;
        float sc = JAMD_LOG_ZERO;
        bool cand = false;
        if (i < K) {
          if (calced[i]) calced[i] = 0;
          else { sc = g_base(i); cand = true; }
        }
        unsigned long long m = __ballot(cand);
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1ull;
          float s_l = __shfl(sc, l, 64);
          if (s_l < thres) s_l = JAMD_LOG_ZERO;        // compute_g_safe(): the partial sum passed -2 x thres
          if (s_l <= thres) continue;
          L.push(s_l, i0 + l, lane);
          thres = __shfl(L.sc, L.len - 1, 64);
        }
      }
      if (lane < L.len) { c_score[op + 1 + (size_t)lane * rows] = L.sc; c_id[op + 1 + (size_t)lane * rows] = L.id; }   // frame t's row
      if (lane == 0) c_num[rp + 1] = L.len;
      kept_t = t;
      wave_sync();
    }
  }
}

// ---- the states ------------------------------------------------------------------------------------------------
// PLAIN: some pdf is scored by K1m's loop (gprune none beside tied-mixture pdfs), so the wave's frames are in LDS;
// without one the kernel reads the cache alone.
template <bool PLAIN>
__global__ void __launch_bounds__(64 * kWaves)
ms_state_kernel(const float *__restrict__ rec, const JamdMsPdf *__restrict__ pdf, const JamdMsTpdf *__restrict__ tpdf,
                const JamdMsStream *__restrict__ strm, const int *__restrict__ st_pdf, const float *__restrict__ st_w,
                const float *__restrict__ ent_logw, const float *__restrict__ frames,
                const float *__restrict__ c_score, const int *__restrict__ c_id, const int *__restrict__ c_num,
                const float *__restrict__ tbl, float *__restrict__ out, int n, int S, int D, int nstream, int rows,
                int cap, int nfb, int nstb, float addmin_f) {
  __shared__ float tile[kWaves][kFPW][kNS + 1];
  extern __shared__ __align__(16) float dyn[];  // PLAIN: [kWaves][D][kFPW]

  int fb, sb;
  if (!decode_block(nfb, nstb, fb, sb)) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int t0 = (fb * kWaves + wave) * kFPW;
  if (t0 >= n) return;
  float *vt = dyn + (size_t)wave * D * kFPW;
  if constexpr (PLAIN) load_frames<0>(nullptr, vt, frames, t0, n, D, lane);
  int ta = t0 + lane, tb = ta + 64;              // the lane's two frames (past the end: the last one, not stored)
  if (ta > n - 1) ta = n - 1;
  if (tb > n - 1) tb = n - 1;
  const size_t ra = (size_t)ta + 1, rb = (size_t)tb + 1;   // their cache rows

  const int s_begin = sb * kNS;
  const int ns = min(kNS, S - s_begin);
  for (int si = 0; si < ns; si++) {
    const int *__restrict__ sp = st_pdf + (size_t)(s_begin + si) * nstream;
    const float *__restrict__ sw = st_w + (size_t)(s_begin + si) * nstream;
    float sum0 = 0.0f, sum1 = 0.0f;          // logprobsum of the lane's two frames
    for (int k = 0; k < nstream; k++) {
      const int p = sp[k];
      const JamdMsTpdf tp = tpdf[p];
      const float w = sw[k];
      float y0 = JAMD_LOG_ZERO, y1 = JAMD_LOG_ZERO;
      if (tp.book >= 0) {
        // calc_tied_mix.c:192-198, :229: the cached slots re-weighted, summed from the last one down
        const size_t bn = (size_t)tp.book * rows, bo = bn * cap;
        const int n0 = c_num[bn + ra], n1 = c_num[bn + rb];
        const float *__restrict__ bw = ent_logw + tp.ent;
        for (int i = tp.nmax - 1; i >= 0; i--) {
          const size_t o = bo + (size_t)i * rows;
          if (i < n0) y0 = addlog_step(y0, c_score[o + ra] + bw[c_id[o + ra]], tbl, addmin_f);
          if (i < n1) y1 = addlog_step(y1, c_score[o + rb] + bw[c_id[o + rb]], tbl, addmin_f);
        }
      } else if constexpr (PLAIN) {
        const JamdMsStream sd = strm[k];
        const JamdMsPdf pd = pdf[p];
        const float *vs = vt + sd.off * kFPW;  // the stream's slice of the transposed frames
        const int len = sd.len;
        const int REC = ms_rec(len);
        for (int e = pd.n - 1; e >= 0; e--) {
          const float *__restrict__ r = rec + (size_t)pd.rec + (size_t)e * REC;
          const float lw = r[2 * len + 1];
          const f2 g = gauss_slice(vs, lane, len, r);
          y0 = addlog_step(y0, g.x + lw, tbl, addmin_f);
          y1 = addlog_step(y1, g.y + lw, tbl, addmin_f);
        }
      }
      // :231, :340: a stream whose outprob is zero is skipped
      if (!(y0 <= JAMD_LOG_ZERO)) { const float q = y0 * w; sum0 = sum0 + q; }
      if (!(y1 <= JAMD_LOG_ZERO)) { const float q = y1 * w; sum1 = sum1 + q; }
    }
    tile[wave][lane][si] = finish_state(sum0);
    tile[wave][64 + lane][si] = finish_state(sum1);
  }
  store_tile<kNS, kFPW>(tile[wave], out, t0, n, S, s_begin, ns, lane);
}

// ---- the cache of the model's codebooks, for inspection ------------------------------------------------------
__global__ void __launch_bounds__(256)
ms_cache_out_kernel(const float *__restrict__ c_score, const int *__restrict__ c_id, const int *__restrict__ c_num,
                    float *__restrict__ o_score, int *__restrict__ o_id, int *__restrict__ o_num, int n, int rows,
                    int nbook, int cap) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n * nbook * cap) return;
  const int k = (int)(i % cap), b = (int)(i / cap % nbook), t = (int)(i / cap / nbook);
  const int num = c_num[(size_t)b * rows + t + 1];
  const size_t src = ((size_t)b * cap + k) * rows + t + 1;
  if (k < num) { o_score[i] = c_score[src]; o_id[i] = c_id[src]; }
  if (k == 0) o_num[(size_t)t * nbook + b] = num;
}

// The lists of a chunk's last frame (row n) become row 0 of the next chunk: what the order pass reads of them.
__global__ void __launch_bounds__(256)
ms_carry_kernel(int *__restrict__ c_id, int *__restrict__ c_num, int n, int rows, int nbook, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nbook * cap) c_id[(size_t)i * rows] = c_id[(size_t)i * rows + n];
  if (i < nbook) c_num[(size_t)i * rows] = c_num[(size_t)i * rows + n];
}

constexpr size_t kCuLds = 160u * 1024u;

// As jamd_gmm_ms_setup(): the attribute belongs to the kernel, so it is raised to all a CU has beside the static part.
int raise_dyn(const void *kernel, size_t dyn, const char *what) {
  hipFuncAttributes fa;
  JAMD_HIP(hipFuncGetAttributes(&fa, kernel));
  if (fa.sharedSizeBytes + dyn > kCuLds)
    return jamd_refuse("jamd_gmm_ms_create_opt: %s needs %zu bytes of LDS per workgroup (%zu static + %zu), the CU has %zu",
                       what, fa.sharedSizeBytes + dyn, (size_t)fa.sharedSizeBytes, dyn, kCuLds);
  if (dyn) JAMD_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kCuLds - fa.sharedSizeBytes)));
  return JAMD_OK;
}

template <typename F>
int with_book_kernel(const jamd_gmm_ms *g, F &&f) {
  if (g->gprune == JAMD_GPRUNE_NONE) return f(std::integral_constant<int, 0>{});
  return dispatch_topn<2>(g->cap, f);
}

}  // namespace

int jamd_gmm_ms_tied_setup(jamd_gmm_ms *g) {
  g->dyn_book = sizeof(float) * kWaves * (size_t)g->maxlen * kFPW;
  g->dyn_order = sizeof(float) * (size_t)g->maxlen + sizeof(int) * (size_t)g->maxbook;
  g->dyn_state = g->has_plain ? sizeof(float) * kWaves * (size_t)g->D * kFPW : 0;
  int rc = with_book_kernel(g, [&](auto nm) {
    return raise_dyn((const void *)ms_book_kernel<decltype(nm)::value>, g->dyn_book, "the codebook kernel (the longest stream slice)");
  });
  if (rc != JAMD_OK) return rc;
  if (g->gprune == JAMD_GPRUNE_SAFE && g->nbook > 0 &&
      (rc = raise_dyn((const void *)ms_order_kernel, g->dyn_order, "the order pass (the largest codebook)")) != JAMD_OK) return rc;
  if (g->has_plain) return raise_dyn((const void *)ms_state_kernel<true>, g->dyn_state, "the state kernel (veclen)");
  return JAMD_OK;
}

int jamd_gmm_ms_tied_launch(jamd_gmm_ms *g, const float *frames, const int *utt_off, int nutt, float *out,
                            float *o_score, int *o_id, int *o_num, hipStream_t st) {
  constexpr int FPB = kWaves * kFPW;
  const int T = utt_off[nutt], nbk = g->nbook_all, cap = g->cap, rows = g->chunk + 1;
  const bool order = g->gprune == JAMD_GPRUNE_SAFE && g->nbook > 0;
  const int nstb = (g->S + kNS - 1) / kNS;
  int u = 0;                                   // the first utterance that does not end before the chunk
  int grid = 0;
  for (int c0 = 0; c0 < T; c0 += g->chunk) {
    const int n = T - c0 < g->chunk ? T - c0 : g->chunk, c1 = c0 + n;
    const int nfb = (n + FPB - 1) / FPB;
    const float *fr = frames + (size_t)c0 * g->D;
    with_book_kernel(g, [&](auto nm) {
      hipLaunchKernelGGL((ms_book_kernel<decltype(nm)::value>), dim3(nbk, nfb), dim3(64 * kWaves), g->dyn_book, st,
                         g->d_rec, g->d_book, fr, g->d_c_score, g->d_c_id, g->d_c_num, g->d_c_flag, n, g->D, rows, cap);
      return JAMD_OK;
    });
    if (order) {
      // the runs of this chunk: of every utterance that reaches into it, the frames after its first
      JamdMsSegs segs;
      int nseg = 0;
      auto flush = [&] {
        if (nseg)
          hipLaunchKernelGGL(ms_order_kernel, dim3(g->nbook, nseg), dim3(64), g->dyn_order, st, g->d_rec, g->d_book, fr,
                             g->d_c_flag, g->d_c_score, g->d_c_id, g->d_c_num, segs, g->D, rows, cap);
        nseg = 0;
      };
      while (u < nutt && utt_off[u] < c1) {
        const int a = utt_off[u], b = utt_off[u + 1];
        if (b > c0) {
          const int first = (a + 1 > c0 ? a + 1 : c0) - c0, end = (b < c1 ? b : c1) - c0;
          if (first < end) {
            segs.first[nseg] = first; segs.end[nseg] = end;
            if (++nseg == kJamdMsSegs) flush();
          }
        }
        if (b > c1) break;                     // the utterance goes on in the next chunk
        u++;
      }
      flush();
      if (c1 < T)                              // the last frame's lists: row 0 of the next chunk
        hipLaunchKernelGGL(ms_carry_kernel, dim3((g->nbook * cap + 255) / 256), dim3(256), 0, st, g->d_c_id, g->d_c_num, n, rows,
                           g->nbook, cap);
    }
    if (out) {
      grid = xcd_grid(nstb, nfb);
      float *o = out + (size_t)c0 * g->S;
      if (g->has_plain)
        hipLaunchKernelGGL(ms_state_kernel<true>, dim3(grid), dim3(64 * kWaves), g->dyn_state, st, g->d_rec, g->d_pdf, g->d_tpdf,
                           g->d_stream, g->d_st_pdf, g->d_st_w, g->d_ent_logw, fr, g->d_c_score, g->d_c_id, g->d_c_num,
                           g->eng->d_addlog, o, n, g->S, g->D, g->nstream, rows, cap, nfb, nstb, g->eng->addmin_f);
      else
        hipLaunchKernelGGL(ms_state_kernel<false>, dim3(grid), dim3(64 * kWaves), 0, st, g->d_rec, g->d_pdf, g->d_tpdf,
                           g->d_stream, g->d_st_pdf, g->d_st_w, g->d_ent_logw, fr, g->d_c_score, g->d_c_id, g->d_c_num,
                           g->eng->d_addlog, o, n, g->S, g->D, g->nstream, rows, cap, nfb, nstb, g->eng->addmin_f);
    } else if (g->nbook > 0) {
      const size_t tot = (size_t)n * g->nbook * cap, at = (size_t)c0 * g->nbook;
      hipLaunchKernelGGL(ms_cache_out_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, g->d_c_score, g->d_c_id,
                         g->d_c_num, o_score + at * cap, o_id + at * cap, o_num + at, n, rows, g->nbook, cap);
    }
  }
  snprintf(g->last_kernel, sizeof(g->last_kernel), "gmm_ms_tied<%s> books=%d+%d cap=%d chunk=%d grid=%d",
           g->gprune == JAMD_GPRUNE_SAFE ? "safe" : "none", g->nbook, nbk - g->nbook, cap, g->chunk, grid);
  return JAMD_OK;
}
