// beam_api.hip -- the first pass's work area (jamd_beam) and every jamd_beam_* entry of the C ABI: creation, the order
// and shape switches, whole-utterance and streaming launches, the resident counter, results, the prune-order test
// entries.  No kernel lives here: launches go through the three interfaces of beam_host.h -- fbeam_* (canonical-tie
// kernel), sbeam_* (strict-order kernel), xbeam_* (exact-order kernels).
#include "jamd_device.h"
#include <algorithm>

#include "beam_host.h"

using namespace jamdb;

// The exact-order kernel's workgroup shape for a launch of nutt utterances.  The full shape (1024 threads, a CU's whole
// LDS) is the faster one per utterance; the half shape lets two utterances share a CU, which pays once the batch has
// clearly more utterances than the device has CUs (one's barriers and wave-serial sections hide behind the other's work).
static bool use_half_shape(const jamd_beam *b, int nutt) {
  if (b->half_status != 0 || b->shape_mode == JAMD_SHAPE_FULL) return false;
  if (b->shape_mode == JAMD_SHAPE_HALF) return true;
  return nutt > b->eng->num_cu + b->eng->num_cu / 2;
}

static bool order_is_exact(const jamd_beam *b) { return b->order == JAMD_ORDER_EXACT || b->order == JAMD_ORDER_EXACT_SERIAL; }

// The order a work area starts in and jamd_beam_set_strict_order(b, 0) returns to: the exact-order kernel where it can
// serve the work area.  Else the frame-parallel canonical-tie kernel -- but that one carries no forward-DFA state, the
// strict-order kernel does, so a grammar with a forward DFA falls back to strict order.
static int default_order(const jamd_beam *b) {
  return b->exact_status == 0 ? JAMD_ORDER_EXACT : b->lex->d.nfwd > 0 ? JAMD_ORDER_STRICT : JAMD_ORDER_FAST;
}

// The exact-order kernel's arguments for a launch in the current state: shape, streaming state, extraction mode.
static XWork xwork_now(const jamd_beam *b, bool half) {
  XWork xw = half ? b->xw_half : b->xw;
  xw.w.stream = b->w.stream;
  xw.prune_mode = b->order == JAMD_ORDER_EXACT_SERIAL ? 1 : 0;
  return xw;
}

// Row offsets of the launch, followed by the ORDER in which the workgroups take the utterances: longest first.  With
// more utterances than CUs the dispatcher hands the next workgroup to the first CU that frees up, so longest-first is
// the classic greedy balance (a 512-utterance batch of 1 200-1 600-frame utterances: the slowest CU carries two average
// utterances instead of the two longest; 274 -> 245 ms).  The exact-order kernel reads it; the others ignore it.
static int upload_utt_off(jamd_beam *b, const int *utt_off, int nutt, hipStream_t st) {
  std::vector<int> &h = b->h_utt_off;
  h.assign((size_t)2 * nutt + 1, 0);
  for (int u = 0; u <= nutt; u++) h[(size_t)u] = utt_off[u];
  int *order = h.data() + nutt + 1;
  for (int u = 0; u < nutt; u++) order[u] = u;
  if (nutt > b->eng->num_cu)       // (one round: every workgroup starts at once, the order is irrelevant)
    std::stable_sort(order, order + nutt, [&](int a, int c) { return utt_off[a + 1] - utt_off[a] > utt_off[c + 1] - utt_off[c]; });
  JAMD_HIP(hipMemcpyAsync(b->d_utt_off, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st));
  return JAMD_OK;
}

// An event behind everything the launch stream holds before the first-pass kernel: it completes when that kernel is
// next to run (jamd_beam_wait_started()).  The workgroups of the launch are NOT accounted here: account_launch() does
// that once the launch is known to have been accepted, so a refused or failed call leaves the resident counter's
// bookkeeping where the device's counter will really be (a phantom workgroup would make every later
// jamd_beam_stream_wait_resident() wait for a value the counter never reaches).
static int mark_started(jamd_beam *b, hipStream_t st) {
  if (!b->ev_started) JAMD_HIP(hipEventCreateWithFlags(&b->ev_started, hipEventDisableTiming));
  // The counter and its targets are 32-bit and compared with >=: long before they could wrap (2^31 workgroups), drain
  // the device once and start again from zero.  (A reset enqueued on the launch stream would not do: a wait that another
  // stream has queued but not yet evaluated would then see 0 against its old target.)
  if (b->d_resident && b->launched_wg > 0x7fffffffu) {
    JAMD_HIP(hipDeviceSynchronize());
    JAMD_HIP(hipMemset(b->d_resident, 0, sizeof(unsigned)));
    b->launched_wg = 0; b->resident_target = 0;
  }
  JAMD_HIP(hipEventRecord(b->ev_started, st));
  return JAMD_OK;
}

// After a launch that hipGetLastError() accepted.  The workgroups of the frame-parallel kernels bump Work::resident
// when they start; the strict-order kernel's do not.
static void account_launch(jamd_beam *b, int nutt) {
  if (b->order != JAMD_ORDER_STRICT) {
    // what fits the device at once: one workgroup per CU, two in the exact-order kernel's half shape
    const int cap = b->eng->num_cu * ((order_is_exact(b) && use_half_shape(b, nutt)) ? 2 : 1);
    // ... less a sixteenth: a launch that fills the device has nearly all of its workgroups placed within microseconds,
    // but the last handful may start only when others end (measured on 512 utterances: any threshold up to 98 % releases
    // the waiting stream at once, 100 % holds it for 170 ms; JAMD_RESIDENT_SHARE=<percent> for experiments)
    int share = nutt < cap ? nutt : cap;
    int pct = 94;
    { const char *pc = getenv("JAMD_RESIDENT_SHARE"); if (pc && atoi(pc) > 0 && atoi(pc) <= 100) pct = atoi(pc); }
    share = (int)((long long)share * pct / 100);
    b->resident_target = b->launched_wg + (unsigned)(share > 0 ? share : 1);
    b->launched_wg += (unsigned)nutt;
  } else b->resident_target = b->launched_wg;
}

// One first-pass launch: every utterance advances by the rows utt_off[u]..utt_off[u+1]) of `dev_scores`.  smode 0: whole
// utterances; 1 / 2: a push of the open streaming session / its final one.  `who`: the public entry, for the messages.
static int launch_pass1(jamd_beam *b, const float *dev_scores, int nstate, const int *utt_off, int nutt, int smode,
                        void *stream, const char *who) {
  if (b->lex->multipath && b->order == JAMD_ORDER_FAST) {   // (state checks come before anything is enqueued or accounted)
    jamd_set_error("%s: this multipath lexicon is decoded by the strict-order kernel only: jamd_beam_set_strict_order(b, 1)", who);
    return JAMD_ESTATE;
  }
  JAMD_HIP(hipSetDevice(b->eng->device));
  hipStream_t st = jamd_stream(b->eng, stream);
  { const int rc = upload_utt_off(b, utt_off, nutt, st); if (rc != JAMD_OK) return rc; }
  { const int rc = mark_started(b, st); if (rc != JAMD_OK) return rc; }
  if (b->order == JAMD_ORDER_STRICT)                        // (keeps no state between launches: whole utterances only)
    sbeam_launch(b->lex->d, b->w, b->sm.view, b->lex->multipath, dev_scores, nstate, b->d_utt_off, nutt, st);
  else if (order_is_exact(b))                               // one shape for a whole session: the parked state is the layout's
    xbeam_launch(b->lex->d, xwork_now(b, smode ? b->stream_half : use_half_shape(b, nutt)), dev_scores, nstate, b->d_utt_off,
                 nutt, smode, b->timed, st);
  else
    fbeam_launch(b->lex->d, b->w, dev_scores, nstate, b->d_utt_off, nutt, smode, b->timed, st);
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("%s: launch failed: %s", who, hipGetErrorString(le)); return JAMD_ELAUNCH; }
  account_launch(b, nutt);
  return JAMD_OK;
}

// Selects order `mode` where the work area can be served in it; `who`: the public entry, for the messages.
static int set_order(jamd_beam *b, int mode, const char *who) {
  switch (mode) {
    case JAMD_ORDER_FAST:
      if (b->lex->d.nfwd > 0) { jamd_set_error("%s: the canonical-tie kernel does not carry a forward DFA's state", who); return JAMD_ESTATE; }
      break;
    case JAMD_ORDER_STRICT: {
      JAMD_HIP(hipSetDevice(b->eng->device));
      const int rc = sbeam_prepare(&b->sm, b->w, b->lex->multipath, b->max_utts);
      if (rc != JAMD_OK) return rc;
      break;
    }
    case JAMD_ORDER_EXACT:
    case JAMD_ORDER_EXACT_SERIAL:
      if (b->exact_status != 0) {
        jamd_set_error("%s: the exact-order kernel cannot serve this work area (%s)", who,
                       b->exact_status == -1 ? "visiting index exceeds 32 bits"
                       : b->exact_status == -2 ? "beam too wide for the LDS image" : b->exact_status == -3 ? "more than 2^21 tokens per frame"
                       : b->exact_status == -4 ? "multipath lexicon in which a root reaches a word end along its own arcs" : "no LDS");
        return JAMD_ESTATE;
      }
      break;
    default: return jamd_refuse("%s: mode=%d", who, mode);
  }
  b->order = mode;
  return JAMD_OK;
}

extern "C" {

int jamd_beam_create(jamd_engine *e, jamd_lexicon *l, int beam_width, float score_pruning_width,
                     int max_utts, int atoms_per_utt, jamd_beam **out) {
  if (!e || !l || !out) return jamd_refuse("jamd_beam_create: NULL argument");
  *out = nullptr;
  if (beam_width < 1 || beam_width > 65536) return jamd_refuse("jamd_beam_create: beam_width=%d outside [1,65536]", beam_width);
  if (max_utts < 1 || atoms_per_utt < 1) return jamd_refuse("jamd_beam_create: bad capacity");
  JAMD_HIP(hipSetDevice(e->device));
  std::unique_ptr<jamd_beam> owner(new jamd_beam());
  jamd_beam *b = owner.get();
  b->eng = e; b->device = e->device; b->lex = l; b->max_utts = max_utts;
  { const char *tm = getenv("JAMD_BEAM_TIMING"); b->timed = tm != nullptr && atoi(tm) != 0; }
  Work &w = b->w;
  w.beam = beam_width; w.width = score_pruning_width; w.nnode = l->d.nnode; w.nword = l->d.nword;
  w.atom_cap = atoms_per_utt;
  // every survivor reaches at most maxfan nodes, cross-word candidates only reach roots (multipath: what the roots reach)
  w.tok_cap = beam_width * l->maxfan + l->d.startnum * (l->multipath ? l->maxfan : 1) + l->d.ninit + 1;
  const size_t U = (size_t)max_utts;
  int rc;
  fbeam_layout(&w);                                  // the canonical-tie kernel's LDS image
  // one slice per utterance: every array at a 256-byte aligned 32-bit offset
  w.nscword = l->nscword > 0 ? l->nscword : 1;
  size_t at = 0;
  auto place = [&](unsigned *off, size_t bytes) { *off = (unsigned)at; at = (at + bytes + 255) & ~(size_t)255; };
  place(&w.o_nodekey, (size_t)w.nnode * sizeof(unsigned long long));
  place(&w.o_cur, (size_t)w.tok_cap * (sizeof(Tok) + 16));   // + the exact-order kernel's 16-byte records of a frame's tokens (REC())
  place(&w.o_cur_key, (size_t)w.tok_cap * sizeof(unsigned));
  place(&w.o_touched, (size_t)w.tok_cap * sizeof(int2));
  place(&w.o_arcq, (size_t)w.tok_cap * sizeof(int2));
  place(&w.o_atoms, (size_t)w.atom_cap * sizeof(jamd_trellis_atom));
  place(&w.o_lmcache, (size_t)w.nscword * sizeof(unsigned long long));
  // exact-order kernel (beam_exact.hip): its extra per-utterance arrays and the multipath lists go into `xs`, ONCE; the
  // XWork of either shape is a copy of `xs` with that shape's LDS layout on top (lay()), so the two cannot drift apart
  XWork xs{};
  const bool mp = l->multipath;
  const int mp_roots = (l->d.lm_type == JAMD_LM_NGRAM) ? l->d.isolatenum : l->d.startnum;   // roots a word end is followed by
  auto lay = [&](XWork *x, bool half) {
    *x = xs;
    return xbeam_layout(x, w, l->maxfan, mp ? mp_roots : l->d.startnum, l->d.ninit, l->d.nshared, half, mp);
  };
  b->exact_status = (mp && !l->mp_parallel) ? -4 : lay(&b->xw, false);     // (here for the verdict and the size of the survivor image)
  b->half_status = b->exact_status != 0 ? -2 : lay(&b->xw_half, true);
  if (mp && getenv("JAMD_MP_HALF_OFF") != nullptr) b->half_status = -2;    // (development: the multipath frame in the full shape only, as in round 4)
  size_t sv_max = (size_t)w.sv_bytes;
  if (b->exact_status == 0 && (size_t)b->xw.w.sv_bytes > sv_max) sv_max = (size_t)b->xw.w.sv_bytes;
  if (b->half_status == 0 && (size_t)b->xw_half.w.sv_bytes > sv_max) sv_max = (size_t)b->xw_half.w.sv_bytes;
  place(&w.o_sv, sv_max);
  if (b->exact_status == 0) {
    // the bitmap holds one bit per visiting index: maxfan per survivor plus startnum per word end
    size_t bits = (size_t)(beam_width + 2) * (size_t)(l->maxfan + l->d.startnum) + (size_t)l->d.nshared + (size_t)l->d.ninit + 64;
    if (mp) bits = (size_t)(beam_width + 2) * (size_t)l->maxfan * (size_t)(mp_roots > 1 ? mp_roots : 1) + (size_t)l->d.nshared * l->maxfan + 64;
    place(&xs.o_nodefirst, (size_t)w.nnode * sizeof(unsigned));
    place(&xs.o_bitmap, (bits + 31) / 32 * 4);
    place(&xs.o_heap, ((size_t)w.tok_cap + 2) * sizeof(unsigned long long));
    place(&xs.o_collect, ((size_t)beam_width + 256) * 16);
    place(&xs.o_sweep, xbeam_sweep_bytes(beam_width));
    place(&xs.o_pstat, 16 * sizeof(int));
    xs.o_mp_iso = l->o_mp_iso; xs.o_mp_shared = l->o_mp_shared; xs.o_mp_start = l->o_mp_start;
    xs.n_mp_iso = l->n_mp_iso; xs.n_mp_shared = l->n_mp_shared; xs.n_mp_start = l->n_mp_start;
    xs.o_mp_tgt = l->o_mp_tgt; xs.n_mp_tgt = l->n_mp_tgt;
    if (mp) {
      place(&xs.o_nodetok, (size_t)(l->n_mp_tgt > 0 ? l->n_mp_tgt : 1) * sizeof(unsigned));
      place(&xs.o_arr, (size_t)w.tok_cap * sizeof(int));
      place(&xs.o_key2, (size_t)w.tok_cap * sizeof(unsigned));
    }
  }
  if (at >= ((size_t)1 << 32)) return jamd_refuse("jamd_beam_create: per-utterance work area exceeds 4 GB");
  w.utt_stride = at;
  if ((rc = b->slices.alloc(U * (size_t)w.utt_stride, true)) != JAMD_OK) return rc;    // zero: empty Viterbi cells
  if ((rc = b->res.alloc(U, true)) != JAMD_OK) return rc;
  w.slices = b->slices; w.res = b->res;
  w.resident = nullptr;
  {
    // a counter the first-pass workgroups bump when they start, in signal memory so that another stream's command
    // processor can wait on it (jamd_beam_stream_wait_resident()); JAMD_NO_WAIT_VALUE=1 keeps the host-side wait
    int can = 0;
    (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, e->device);
    const char *off = getenv("JAMD_NO_WAIT_VALUE");
    if (can && !(off && off[0] == '1')) {
      void *p = nullptr;
      if (hipExtMallocWithFlags(&p, 8, hipMallocSignalMemory) == hipSuccess && p) {
        b->d_resident.adopt((unsigned *)p, 8);
        if (hipMemset(p, 0, 8) == hipSuccess) w.resident = b->d_resident;
        else b->d_resident.adopt(nullptr, 0);
      }
      (void)hipGetLastError();
    }
  }
  const hipError_t ae = fbeam_prepare();
  if (ae != hipSuccess) {
    jamd_set_error("jamd_beam_create: cannot reserve %d bytes of LDS: %s", w.sv_bytes, hipGetErrorString(ae));
    return JAMD_ENODEV;
  }
  if ((rc = b->d_utt_off.alloc(2 * U + 1, true)) != JAMD_OK) return rc;
  if (b->exact_status == 0) {
    // once more, over the finished Work and slice offsets: same slices in both shapes, only the LDS image differs
    lay(&b->xw, false);
    if (b->half_status == 0) lay(&b->xw_half, true);
    if (xbeam_prepare() != hipSuccess) b->exact_status = -5;
  }
  {
    // The work area starts in its default order.  For a grammar with a forward DFA that the exact-order kernel cannot
    // serve (beam too wide for the LDS image, a root that reaches a word end, no LDS) that is strict order instead of a
    // refusal: the caller has no beam to call jamd_beam_set_strict_order() on when create fails.
    rc = set_order(b, default_order(b), "jamd_beam_create");
    if (rc != JAMD_OK) {
      jamd_set_error("jamd_beam_create: a grammar with a forward DFA needs the exact-order or the strict-order kernel; "
                     "neither can serve beam %d on this lexicon", w.beam);
      return rc;
    }
  }
  *out = owner.release();
  return JAMD_OK;
}

void jamd_beam_destroy(jamd_beam *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;                                  // (the engine is not looked at: it may have gone first)
}

int jamd_beam_pass1_dev(jamd_beam *b, const float *dev_scores, int nstate, const int *utt_off, int nutt,
                        void *stream) {
  if (!b || !dev_scores || !utt_off || nstate <= 0) return jamd_refuse("jamd_beam_pass1_dev: bad argument");
  if (nutt < 0 || nutt > b->max_utts) return jamd_refuse("jamd_beam_pass1_dev: nutt=%d exceeds the work area (%d)", nutt, b->max_utts);
  for (int u = 0; u < nutt; u++) {
    const int T = utt_off[u + 1] - utt_off[u];
    if (T < 0 || T > 32767)     // TRELLIS_ATOM times are short (trellis.h:32-33)
      return jamd_refuse("jamd_beam_pass1_dev: utterance %d has %d frames (limit 32767)", u, T);
  }
  if (nutt == 0) return JAMD_OK;
  return launch_pass1(b, dev_scores, nstate, utt_off, nutt, 0, stream, "jamd_beam_pass1_dev");
}

int jamd_beam_stream_begin(jamd_beam *b, int nutt) {
  if (!b || nutt < 1 || nutt > b->max_utts) return jamd_refuse("jamd_beam_stream_begin: bad argument");
  JAMD_HIP(hipSetDevice(b->eng->device));
  if (b->w.stream == nullptr) {
    const int rc = b->stream.alloc((size_t)b->max_utts);
    if (rc != JAMD_OK) return rc;
    b->w.stream = b->stream;
  }
  JAMD_HIP(hipMemsetAsync(b->w.stream, 0, sizeof(StreamState) * (size_t)nutt, b->eng->stream));
  JAMD_HIP(hipStreamSynchronize(b->eng->stream));
  b->streaming = nutt; b->stream_pushes = 0;
  b->stream_half = use_half_shape(b, nutt);           // one shape for the whole session: the parked state is the layout's
  b->stream_frames.assign((size_t)nutt, 0);
  return JAMD_OK;
}

int jamd_beam_stream_push_dev(jamd_beam *b, const float *dev_scores, int nstate, const int *chunk_off, int nutt,
                              int final, void *stream) {
  if (!b || !chunk_off || nstate <= 0 || (!dev_scores && chunk_off[nutt > 0 ? nutt : 0] > 0)) return jamd_refuse("jamd_beam_stream_push_dev: bad argument");
  if (b->streaming <= 0 || nutt != b->streaming) {
    jamd_set_error("jamd_beam_stream_push_dev: call jamd_beam_stream_begin(b, %d) first", nutt); return JAMD_ESTATE;
  }
  for (int u = 0; u < nutt; u++) {
    if (chunk_off[u + 1] < chunk_off[u]) return jamd_refuse("jamd_beam_stream_push_dev: chunk_off must be non-decreasing");
    if ((long)b->stream_frames[u] + (chunk_off[u + 1] - chunk_off[u]) > 32767)     // TRELLIS_ATOM times are short
      return jamd_refuse("jamd_beam_stream_push_dev: utterance %d would exceed 32767 frames", u);
  }
  if (b->order == JAMD_ORDER_STRICT) {
    if (!final || b->stream_pushes != 0) {
      // the strict-order kernel keeps no state between launches: one push carrying everything
      jamd_set_error("jamd_beam_stream_push_dev: strict-order mode needs the whole utterance in one final push");
      return JAMD_ESTATE;
    }
    b->streaming = 0;
    return jamd_beam_pass1_dev(b, dev_scores, nstate, chunk_off, nutt, stream);
  }
  { const int rc = launch_pass1(b, dev_scores, nstate, chunk_off, nutt, final ? 2 : 1, stream, "jamd_beam_stream_push_dev"); if (rc != JAMD_OK) return rc; }
  for (int u = 0; u < nutt; u++) b->stream_frames[u] += chunk_off[u + 1] - chunk_off[u];   // only an accepted push counts
  b->stream_pushes++;
  if (final) b->streaming = 0;
  return JAMD_OK;
}

int jamd_beam_set_strict_order(jamd_beam *b, int on) {
  if (!b) return jamd_refuse("jamd_beam_set_strict_order: NULL");
  // (the parked state of an open session is the layout of the kernel that wrote it)
  if (b->streaming > 0) { jamd_set_error("jamd_beam_set_strict_order: a streaming session is open"); return JAMD_ESTATE; }
  if (!on && default_order(b) == JAMD_ORDER_STRICT) {
    // the canonical-tie kernel would drop the forward DFA's state
    jamd_set_error("jamd_beam_set_strict_order: a grammar with a forward DFA stays in strict order where the exact-order "
                   "kernel cannot serve the work area (beam %d)", b->w.beam);
    return JAMD_ESTATE;
  }
  return set_order(b, on ? JAMD_ORDER_STRICT : default_order(b), "jamd_beam_set_strict_order");
}

int jamd_beam_set_order_mode(jamd_beam *b, int mode) {
  if (!b) return jamd_refuse("jamd_beam_set_order_mode: NULL");
  if (b->streaming > 0) { jamd_set_error("jamd_beam_set_order_mode: a streaming session is open"); return JAMD_ESTATE; }
  return set_order(b, mode, "jamd_beam_set_order_mode");
}

int jamd_beam_set_workgroup_shape(jamd_beam *b, int shape) {
  if (!b) return jamd_refuse("jamd_beam_set_workgroup_shape: NULL");
  if (b->streaming > 0) { jamd_set_error("jamd_beam_set_workgroup_shape: a streaming session is open"); return JAMD_ESTATE; }
  if (shape != JAMD_SHAPE_AUTO && shape != JAMD_SHAPE_FULL && shape != JAMD_SHAPE_HALF) return jamd_refuse("jamd_beam_set_workgroup_shape: shape=%d", shape);
  if (shape == JAMD_SHAPE_HALF && b->half_status != 0) {
    jamd_set_error("jamd_beam_set_workgroup_shape: beam %d does not fit the half shape (%s)", b->w.beam,
                   b->exact_status != 0 ? "the exact-order kernel cannot serve this work area" : "half a CU's LDS holds no typical frame");
    return JAMD_ESTATE;
  }
  b->shape_mode = shape;
  return JAMD_OK;
}

int jamd_beam_wait_started(jamd_beam *b) {
  if (!b) return jamd_refuse("jamd_beam_wait_started: NULL");
  if (!b->ev_started) return JAMD_OK;                  // nothing launched yet
  JAMD_HIP(hipSetDevice(b->eng->device));
  JAMD_HIP(hipEventSynchronize(b->ev_started));
  return JAMD_OK;
}

int jamd_beam_stream_wait_resident(jamd_beam *b, void *stream) {
  if (!b) return jamd_refuse("jamd_beam_stream_wait_resident: NULL");
  if (!b->ev_started) return JAMD_OK;                  // nothing launched yet
  JAMD_HIP(hipSetDevice(b->eng->device));
  if (b->d_resident) {
    // the command processor of `stream` waits until the counter the first-pass workgroups bump when they start has
    // reached the latest launch's share; the host is not involved
    JAMD_HIP(hipStreamWaitValue32(jamd_stream(b->eng, stream), b->d_resident, b->resident_target, hipStreamWaitValueGte, 0xffffffffu));
    return JAMD_OK;
  }
  JAMD_HIP(hipEventSynchronize(b->ev_started));       // no wait-on-memory on this device: the host waits, and gives the dispatcher a moment
  struct timespec ms = {0, 1000000};
  nanosleep(&ms, nullptr);
  return JAMD_OK;
}

int jamd_beam_debug_preset_resident(jamd_beam *b, unsigned count) {
  if (!b) return jamd_refuse("jamd_beam_debug_preset_resident: NULL");
  JAMD_HIP(hipSetDevice(b->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  if (b->d_resident) JAMD_HIP(hipMemcpy(b->d_resident, &count, sizeof(unsigned), hipMemcpyHostToDevice));
  b->launched_wg = count; b->resident_target = count;
  return JAMD_OK;
}

int jamd_beam_debug_resident(const jamd_beam *b, unsigned *launched, unsigned *target) {
  if (!b) return jamd_refuse("jamd_beam_debug_resident: NULL");
  if (launched) *launched = b->launched_wg;
  if (target) *target = b->resident_target;
  return JAMD_OK;
}

int jamd_beam_workgroup_shape(const jamd_beam *b, int nutt) {
  if (!b) return -1;
  return use_half_shape(b, nutt) ? JAMD_SHAPE_HALF : JAMD_SHAPE_FULL;
}

int jamd_beam_exact_layout(const jamd_beam *b) {
  if (!b) return -1;
  return b->exact_status != 0 ? 0 : (b->xw.wide ? 2 : 1);
}

int jamd_beam_order_mode(const jamd_beam *b) {
  if (!b) return -1;
  return b->order;
}

static int prune_order_impl(jamd_beam *b, const float *scores, int n, int *order, int *nkeep, int *arr) {
  if (!b || !scores || !order || !nkeep || n < 1) return jamd_refuse("jamd_beam_prune_order: bad argument");
  if (b->exact_status != 0) { jamd_set_error("jamd_beam_prune_order: the exact-order kernel cannot serve this work area"); return JAMD_ESTATE; }
  if (n > (1 << 20)) return jamd_refuse("jamd_beam_prune_order: n=%d too large", n);
  JAMD_HIP(hipSetDevice(b->eng->device));
  int rc;
  if ((size_t)n > b->pcap) {
    // The old buffers go when the new ones come: nothing is in flight, every call has synchronised its stream before it
    // returned.  pcap is 0 until both are there.
    const size_t cap = ((size_t)n + 1024 + 3) & ~(size_t)3;     // multiple of 4: the heap and the top-list scratch stay aligned
    b->pcap = 0;
    if ((rc = b->d_pkeys.grow(cap * 4)) != JAMD_OK) return rc;
    // out[cap] + nout (+ pad) | heap u64[cap + 2] | top-list scratch u32x4[beam + 256] (wide layout) | sweep replay scratch
    if ((rc = b->d_pout.grow(4 * (cap + 16) + 8 * (cap + 2) + 16 * ((size_t)b->w.beam + 256) + xbeam_sweep_bytes(b->w.beam))) != JAMD_OK) return rc;
    b->pcap = cap;
  }
  if (arr && (rc = b->d_parr.grow(4 * b->pcap)) != JAMD_OK) return rc;
  std::vector<unsigned> keys((size_t)n);
  for (int i = 0; i < n; i++) {
    float f = scores[i] + 0.0f; unsigned u; memcpy(&u, &f, 4);
    keys[i] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  hipStream_t st = b->eng->stream;
  JAMD_HIP(hipMemcpyAsync(b->d_pkeys, keys.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
  int *d_nout = b->d_pout + b->pcap;
  unsigned long long *d_heap = reinterpret_cast<unsigned long long *>(b->d_pout + b->pcap + 16);
  u32x4 *d_collect = reinterpret_cast<u32x4 *>(d_heap + b->pcap + 2);
  unsigned char *d_sweep = reinterpret_cast<unsigned char *>(d_collect + (size_t)b->w.beam + 256);
  xbeam_prune_order_launch(xwork_now(b, !arr && use_half_shape(b, 1)), b->d_pkeys, n, b->w.beam, b->d_pout, d_nout, d_heap, d_collect, d_sweep, arr ? b->d_parr.p : nullptr, st);
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) { jamd_set_error("jamd_beam_prune_order: launch failed: %s", hipGetErrorString(le)); return JAMD_ELAUNCH; }
  JAMD_HIP(hipMemcpyAsync(nkeep, d_nout, 4, hipMemcpyDeviceToHost, st));
  JAMD_HIP(hipStreamSynchronize(st));
  if (*nkeep < 0 || *nkeep > n) { jamd_set_error("jamd_beam_prune_order: the kernel reported %d of %d tokens kept", *nkeep, n); return JAMD_ELAUNCH; }
  JAMD_HIP(hipMemcpy(order, b->d_pout, 4 * (size_t)*nkeep, hipMemcpyDeviceToHost));
  if (arr) JAMD_HIP(hipMemcpy(arr, b->d_parr, 4 * (size_t)n, hipMemcpyDeviceToHost));
  return JAMD_OK;
}

int jamd_beam_prune_order(jamd_beam *b, const float *scores, int n, int *order, int *nkeep) {
  return prune_order_impl(b, scores, n, order, nkeep, nullptr);
}

int jamd_beam_prune_arrange(jamd_beam *b, const float *scores, int n, int *order, int *nkeep, int *tindex) {
  if (!tindex) return jamd_refuse("jamd_beam_prune_arrange: bad argument");
  return prune_order_impl(b, scores, n, order, nkeep, tindex);
}

int jamd_beam_prune_stats(jamd_beam *b, int utt, int stats[16], int reset) {
  if (!b || !stats || utt < 0 || utt >= b->max_utts) return jamd_refuse("jamd_beam_prune_stats: bad argument");
  if (b->exact_status != 0) { jamd_set_error("jamd_beam_prune_stats: the exact-order kernel does not serve this work area"); return JAMD_ESTATE; }
  JAMD_HIP(hipSetDevice(b->eng->device));
  unsigned char *p = b->w.slices + (size_t)utt * b->w.utt_stride + b->xw.o_pstat;
  JAMD_HIP(hipMemcpy(stats, p, 16 * sizeof(int), hipMemcpyDeviceToHost));
  if (reset) JAMD_HIP(hipMemset(p, 0, 16 * sizeof(int)));
  return JAMD_OK;
}

int jamd_beam_prune_info(jamd_beam *b, int *sweep_rounds, int *sweep_us, int *sweep_events) {
  if (!b || !sweep_rounds || !b->d_pout) return jamd_refuse("jamd_beam_prune_info: bad argument (or no jamd_beam_prune_order() call yet)");
  JAMD_HIP(hipSetDevice(b->eng->device));
  int v[15];
  JAMD_HIP(hipMemcpy(v, b->d_pout + b->pcap + 1, sizeof(v), hipMemcpyDeviceToHost));
  if (getenv("JAMD_SWEEP_PROF")) fprintf(stderr, "sweep phases (us): setup %d  tables %d  level0 %d  levels %d  chains %d  rebuild %d | level phase 1 %d  phase 2 %d\n",
                                         v[3] / 100, v[4] / 100, v[5] / 100, v[6] / 100, v[7] / 100, v[8] / 100, v[9] / 100, v[10] / 100);
  if (getenv("JAMD_SWEEP_PROF") && (v[11] | v[12] | v[13] | v[14])) fprintf(stderr, "sift replay (us): load %d  first window's dependencies %d  sifts %d  output %d\n", v[11] / 100, v[12] / 100, v[13] / 100, v[14] / 100);
  *sweep_rounds = v[0];
  if (sweep_us) *sweep_us = v[1] / 100;            // wall_clock64(): 100 MHz
  if (sweep_events) *sweep_events = v[2];
  return JAMD_OK;
}

int jamd_beam_results(jamd_beam *b, jamd_pass1_result *out, int nutt) {
  if (!b || !out || nutt < 0 || nutt > b->max_utts) return jamd_refuse("jamd_beam_results: bad argument");
  JAMD_HIP(hipSetDevice(b->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  if (nutt) JAMD_HIP(hipMemcpy(out, b->w.res, sizeof(jamd_pass1_result) * nutt, hipMemcpyDeviceToHost));
  return JAMD_OK;
}

int jamd_beam_trellis(jamd_beam *b, int utt, jamd_trellis_atom *atoms, int cap, int *natom) {
  if (!b || !natom || utt < 0 || utt >= b->max_utts) return jamd_refuse("jamd_beam_trellis: bad argument");
  JAMD_HIP(hipSetDevice(b->eng->device));
  JAMD_HIP(hipDeviceSynchronize());
  jamd_pass1_result r;
  JAMD_HIP(hipMemcpy(&r, b->w.res + utt, sizeof(r), hipMemcpyDeviceToHost));
  *natom = r.natom;
  if (atoms) {
    const int n = r.natom < cap ? r.natom : cap;
    if (n > 0) JAMD_HIP(hipMemcpy(atoms, b->w.slices + (size_t)utt * b->w.utt_stride + b->w.o_atoms, sizeof(jamd_trellis_atom) * n,
                                  hipMemcpyDeviceToHost));
  }
  return JAMD_OK;
}

}  // extern "C"
