// jamd_host.h -- what the host layer of every object needs and no object owns: the refusal, memory that frees itself,
// the table that goes up through pinned memory, the _host form of an entry around its _dev form, the span check of an
// offset table.  An object's members own their memory, so its *_destroy is "select the device, wait for what still
// runs, delete", and a *_create keeps the object in a std::unique_ptr until it hands it over: any return before that
// releases everything.  Internal, not installed.
#pragma once
#include <memory>
#include <utility>

#include "jamd_internal.h"

#define JAMD_LOCAL __attribute__((visibility("hidden")))   // a launcher, a type of the host layer: stays inside the library

// A refused argument: `if (bad) return jamd_refuse("...", ...);` sets the error text and returns JAMD_EINVAL.
__attribute__((format(printf, 1, 2))) static inline int jamd_refuse(const char *fmt, ...) {
  char b[512];                               // (what jamd_last_error() keeps)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  jamd_set_error("%s", b);
  return JAMD_EINVAL;
}

// Device memory with one owner.  Reads as the pointer it holds; `cap` is its size in bytes.
template <typename T>
struct JAMD_LOCAL JamdDev {
  T *p = nullptr;
  size_t cap = 0;
  JamdDev() = default;
  JamdDev(const JamdDev &) = delete;
  JamdDev &operator=(const JamdDev &) = delete;
  ~JamdDev() { if (p) (void)hipFree(p); }
  operator T *() const { return p; }
  void swap(JamdDev &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  // Room for at least `bytes`; what the buffer held is not kept.
  int grow(size_t bytes) {
    if (cap >= bytes) return JAMD_OK;
    if (p) JAMD_HIP(hipFree(p));
    p = nullptr; cap = 0;
    JAMD_HIP(hipMalloc((void **)&p, bytes));
    cap = bytes;
    return JAMD_OK;
  }
  // Takes over `bytes` at `q` that came from another allocator whose memory hipFree() releases (signal memory).
  void adopt(T *q, size_t bytes) {
    if (p) (void)hipFree(p);
    p = q; cap = bytes;
  }
  // n elements, zeroed if asked.  No table is NULL: an empty one still gets 16 bytes.
  int alloc(size_t n, bool zero = false) {
    int rc;
    if ((rc = grow(n ? n * sizeof(T) : 16)) != JAMD_OK) return rc;
    if (zero && n) JAMD_HIP(hipMemset(p, 0, n * sizeof(T)));
    return JAMD_OK;
  }
  int upload(const T *src, size_t n) {
    int rc;
    if ((rc = alloc(n)) != JAMD_OK) return rc;
    if (n) JAMD_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return JAMD_OK;
  }
};

// Pinned host memory with one owner, for a table that comes down.
struct JAMD_LOCAL JamdHostBuf {
  char *p = nullptr;
  size_t cap = 0;
  JamdHostBuf() = default;
  JamdHostBuf(const JamdHostBuf &) = delete;
  JamdHostBuf &operator=(const JamdHostBuf &) = delete;
  ~JamdHostBuf() { if (p) (void)hipHostFree(p); }
  int grow(size_t bytes) {
    if (cap >= bytes) return JAMD_OK;
    if (p) JAMD_HIP(hipHostFree(p));
    p = nullptr; cap = 0;
    JAMD_HIP(hipHostMalloc((void **)&p, bytes, hipHostMallocDefault));
    cap = bytes;
    return JAMD_OK;
  }
};

// A table that goes up through pinned memory: `h` is rewritten only once the upload that read it is done, and is
// freed only then.
struct JAMD_LOCAL JamdPinned {
  JamdDev<char> d;
  JamdHostBuf h;
  hipEvent_t ev = nullptr;
  ~JamdPinned() { if (ev) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); } }
  // Waits for the last upload and makes room: `h.p` may then be filled with `bytes`.
  int begin(size_t bytes) {
    int rc;
    if ((rc = d.grow(bytes)) != JAMD_OK) return rc;
    if (ev) JAMD_HIP(hipEventSynchronize(ev));
    else JAMD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return h.grow(bytes);
  }
  int send(size_t bytes, hipStream_t st) {
    JAMD_HIP(hipMemcpyAsync(d.p, h.p, bytes, hipMemcpyHostToDevice, st));
    JAMD_HIP(hipEventRecord(ev, st));
    return JAMD_OK;
  }
};

// The _host form of an entry around its _dev form: nin values up to `in`, dev(in, out, stream) on the engine's stream
// with room for out_cap values at `out`, as many values down to dst as dev returned (a JAMD_* error instead ends the
// call), and the stream waited for: a failure there returns sync_rc (the scorers have always said JAMD_ELAUNCH).  The
// staging stays with the object between calls.
template <typename In, typename Out>
struct JAMD_LOCAL JamdStage { JamdDev<In> in; JamdDev<Out> out; };
template <typename In, typename Out, typename Dev>
static int jamd_host_call(JamdStage<In, Out> *g, jamd_engine *eng, const In *src, size_t nin, Out *dst, size_t out_cap, Dev dev,
                          int sync_rc = JAMD_ENODEV) {
  JAMD_HIP(hipSetDevice(eng->device));
  int rc;
  if ((rc = g->in.grow((nin > 0 ? nin : 1) * sizeof(In))) != JAMD_OK) return rc;
  if ((rc = g->out.grow((out_cap > 0 ? out_cap : 1) * sizeof(Out))) != JAMD_OK) return rc;
  hipStream_t st = eng->stream;
  if (nin) JAMD_HIP(hipMemcpyAsync(g->in.p, src, nin * sizeof(In), hipMemcpyHostToDevice, st));
  const long long nout = dev(g->in.p, g->out.p, st);
  if (nout < 0) return (int)nout;
  if (nout) JAMD_HIP(hipMemcpyAsync(dst, g->out.p, (size_t)nout * sizeof(Out), hipMemcpyDeviceToHost, st));
  const hipError_t se = hipStreamSynchronize(st);
  if (se != hipSuccess) {
    jamd_set_error("hipStreamSynchronize failed: %s", hipGetErrorString(se));
    return sync_rc;
  }
  return JAMD_OK;
}

// Samples of channel c in an offset table of a push -> *n; refused when the range is out of order or too long.
constexpr long long kJamdMaxChunk = 0x3fffffffLL;            // samples of one channel in one push
static inline int jamd_span(const char *who, const int64_t *off, int c, long long *n) {
  *n = off[c + 1] - off[c];
  if (off[c] < 0 || *n < 0 || *n > kJamdMaxChunk)
    return jamd_refuse("%s: channel %d: offsets [%lld, %lld) are negative, descending or more than %lld samples", who, c,
                       (long long)off[c], (long long)off[c + 1], kJamdMaxChunk);
  return JAMD_OK;
}
