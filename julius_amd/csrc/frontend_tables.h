// frontend_tables.h -- the part of the audio front end that needs no device: the descriptor (make_default_para(),
// calc_para_from_header(), the -htkconf parser), the tables of WMP_work_new() / InitFBank() (mfcc-core.c), computed
// with the same expressions, and the integer bookkeeping of both front ends: frames per utterance, the sample_off
// check, and the frame / row counts of a live segment, whole or pushed in chunks.  Plain C++ without a HIP header:
// csrc/frontend_api.hip and csrc/frontend_live_api.hip wrap it in the C ABI, and tests/frontend_tables_check.cpp
// compiles it alone under the host sanitizers.  A function that can refuse returns false (or a negative value) with
// the whole message, the caller's name included, in `err`.
#ifndef JAMD_FRONTEND_TABLES_H
#define JAMD_FRONTEND_TABLES_H
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "julius_amd.h"

// stddefs.h:97 (the reference's own constant, not M_PI)
#define FE_PI 3.14159265358979

// The message of a refusal -> err (512 bytes: what jamd_last_error() keeps); false, for `return fe_errf(...)`.
__attribute__((format(printf, 2, 3))) static inline bool fe_errf(std::string &err, const char *fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  err = b;
  return false;
}

// ---------------------------------------------------------------------------------- descriptor
// calc_para_from_header() (para.c:323-372)
static inline void fe_set_kind(jamd_frontend_desc *d, int param_type, int vec_size) {
  d->paramtype = param_type; d->vecsize = vec_size;
  d->basetype = param_type & 0x003f;
  d->delta = (param_type & JAMD_F_D) ? 1 : 0;
  d->acc = (param_type & JAMD_F_A) ? 1 : 0;
  d->energy = (param_type & JAMD_F_E) ? 1 : 0;
  d->c0 = (param_type & JAMD_F_0) ? 1 : 0;
  d->absesup = (param_type & JAMD_F_N) ? 1 : 0;
  d->cmn = (param_type & JAMD_F_Z) ? 1 : 0;
  int dim = vec_size;
  if (d->absesup) dim++;
  dim /= 1 + (d->delta ? 1 : 0) + (d->acc ? 1 : 0);
  if (d->energy) dim--;
  if (d->c0) dim--;
  d->mfcc_dim = dim;
  d->baselen = d->mfcc_dim + (d->c0 ? 1 : 0) + (d->energy ? 1 : 0);
  d->vecbuflen = d->baselen * (1 + (d->delta ? 1 : 0) + (d->acc ? 1 : 0));
  d->veclen = d->vecbuflen - (d->absesup ? 1 : 0);
  if (d->basetype == JAMD_F_FBANK || d->basetype == JAMD_F_MELSPEC) d->fbank_num = dim;
}

// make_default_para() (para.c:86-107; DEF_* of mfcc.h:56-66)
static inline void fe_default_desc(int param_type, int vec_size, jamd_frontend_desc *d) {
  memset(d, 0, sizeof(*d));
  d->smp_period = 625; d->smp_freq = 16000;
  d->framesize = 400; d->frameshift = 160;
  d->preEmph = 0.97f;
  d->fbank_num = 24; d->lifter = 22; d->delWin = 2; d->accWin = 2;
  d->raw_e = 0; d->enormal = 0; d->escale = 1.0f; d->silFloor = 50.0f;
  d->cvn = 0; d->hipass = -1; d->lopass = -1;
  d->vtln_alpha = 1.0f; d->vtln_upper = 0.0f; d->vtln_lower = 0.0f;
  d->zmeanframe = 0; d->usepower = 0;
  d->splice = 1;
  fe_set_kind(d, param_type, vec_size);
}

// htk_config_file_parse() (para.c:196-321): the same tokenising, the same conversions.  *para changes only when the
// whole file was taken.
static inline bool fe_htkconf(const char *path, jamd_frontend_desc *para, std::string &err) {
  FILE *fp = fopen(path, "r");
  if (!fp) return fe_errf(err, "jamd_frontend_htkconf: failed to open HTK Config file: %s", path);
  jamd_frontend_desc p = *para;
  char buf[512];
  float srate = 0.0f;
  auto istok = [](char c) { return c == ' ' || c == '\t' || c == '\n'; };
  while (fgets(buf, sizeof buf, fp)) {
    int nl = (int)strlen(buf) - 1;           // getl_fp(): chop \n and \r, skip blank lines
    if (nl >= 0 && buf[nl] == '\n') { buf[nl] = '\0'; nl--; }
    if (nl >= 0 && buf[nl] == '\r') buf[nl] = '\0';
    if (buf[0] == '\0') continue;
    char *s = buf;
    if (*s == '#') continue;
    while (*s != '\0' && istok(*s)) s++;
    if (*s == '\0') continue;
    char *k = s;
    while (*s != '\0' && !istok(*s) && *s != '=') s++;
    if (*s == '\0') continue;
    *s = '\0'; s++;
    while (*s != '\0' && (istok(*s) || *s == '=')) s++;
    if (*s == '\0') continue;
    char *a = s;
    while (*s != '\0' && !istok(*s)) s++;
    *s = '\0';
    if (!strcmp(k, "SOURCERATE")) srate = (float)atof(a);
    else if (!strcmp(k, "TARGETRATE")) p.frameshift = (int)atof(a);
    else if (!strcmp(k, "WINDOWSIZE")) p.framesize = (int)atof(a);
    else if (!strcmp(k, "ZMEANSOURCE")) p.zmeanframe = a[0] == 'T';
    else if (!strcmp(k, "USEPOWER")) p.usepower = a[0] == 'T';
    else if (!strcmp(k, "PREEMCOEF")) p.preEmph = (float)atof(a);
    else if (!strcmp(k, "USEHAMMING")) {
      if (a[0] != 'T') {
        fclose(fp);
        return fe_errf(err, "jamd_frontend_htkconf: %s: USEHAMMING should be T", path);
      }
    } else if (!strcmp(k, "NUMCHANS")) p.fbank_num = atoi(a);
    else if (!strcmp(k, "CEPLIFTER")) p.lifter = atoi(a);
    else if (!strcmp(k, "DELTAWINDOW")) p.delWin = atoi(a);
    else if (!strcmp(k, "ACCWINDOW")) p.accWin = atoi(a);
    else if (!strcmp(k, "LOFREQ")) p.lopass = (int)atof(a);
    else if (!strcmp(k, "HIFREQ")) p.hipass = (int)atof(a);
    else if (!strcmp(k, "RAWENERGY")) p.raw_e = a[0] == 'T';
    else if (!strcmp(k, "ENORMALISE")) p.enormal = a[0] == 'T';
    else if (!strcmp(k, "ESCALE")) p.escale = (float)atof(a);
    else if (!strcmp(k, "SILFLOOR")) p.silFloor = (float)atof(a);
    else if (!strcmp(k, "WARPFREQ")) p.vtln_alpha = (float)atof(a);
    else if (!strcmp(k, "WARPLCUTOFF")) p.vtln_lower = (float)atof(a);
    else if (!strcmp(k, "WARPUCUTOFF")) p.vtln_upper = (float)atof(a);
    else if (!strcmp(k, "TARGETKIND") || !strcmp(k, "NUMCEPS")) { /* determined by the AM header */ }
    else {
      fclose(fp);
      return fe_errf(err, "jamd_frontend_htkconf: %s: key \"%s\" is not one the reference takes", path, k);
    }
  }
  fclose(fp);
  if (srate == 0.0f) srate = 625;
  p.smp_period = (int)srate;
  p.smp_freq = (int)(10000000.0 / (float)p.smp_period);   // period2freq(), speech.h:106
  p.frameshift = (int)(p.frameshift / srate);
  p.framesize = (int)(p.framesize / srate);
  *para = p;
  return true;
}

// ---------------------------------------------------------------------------------- tables
struct __attribute__((visibility("hidden"))) FeTables {   // (its implicit members are no export of a library)
  int fftN = 0, n = 0, klo = 0, khi = 0, nv2 = 0, maxChan = 0;
  float fres = 0.f, sqrt2var = 0.f;
  std::vector<float> cf, loWt;
  std::vector<short> loChan;
  std::vector<double> ham, fftcos, fftsin, dct, wcep, twRe, twIm;
  std::vector<int> kfirst, klast;      // [fbank_num + 1]: the k whose loChan is bin-1 or bin, ascending
};

static inline float fe_mel(int k, float fres) { return (float)(1127 * log((double)(1 + (k - 1) * fres))); }   // Mel(), mfcc-core.c

// VTLN_recreate_fbank_cf() (mfcc-core.c)
static inline bool fe_vtln(std::vector<float> &cf, const jamd_frontend_desc *p, float mlo, float mhi, int maxChan,
                           std::string &err) {
  float minf = (float)(700.0 * (exp(mlo / 1127.0) - 1.0));
  float maxf = (float)(700.0 * (exp(mhi / 1127.0) - 1.0));
  if (p->vtln_upper > maxf)
    return fe_errf(err, "frontend: VTLN upper cut-off greater than upper frequency bound: %.1f > %.1f", p->vtln_upper, maxf);
  if (p->vtln_lower < minf)
    return fe_errf(err, "frontend: VTLN lower cut-off smaller than lower frequency bound: %.1f < %.1f", p->vtln_lower, minf);
  float scale = (float)(1.0 / p->vtln_alpha);
  float cu = p->vtln_upper * 2 / (1 + scale);
  float cl = p->vtln_lower * 2 / (1 + scale);
  float au = (maxf - cu * scale) / (maxf - cu);
  float al = (cl * scale - minf) / (cl - minf);
  for (int chan = 1; chan <= maxChan; chan++) {
    float cf_orig = (float)(700.0 * (exp(cf[chan] / 1127.0) - 1.0));
    float cf_new;
    if (cf_orig > cu) cf_new = au * (cf_orig - cu) + scale * cu;
    else if (cf_orig < cl) cf_new = al * (cf_orig - minf) + minf;
    else cf_new = scale * cf_orig;
    cf[chan] = (float)(1127.0 * log(1.0 + cf_new / 700.0));
  }
  return true;
}

static inline bool fe_build_tables(const jamd_frontend_desc *p, FeTables &w, std::string &err) {
  if (p->framesize < 2 || p->framesize > 4096 || p->frameshift < 1 || p->fbank_num < 1 || p->smp_period <= 0)
    return fe_errf(err, "frontend: framesize %d (2..4096), frameshift %d, fbank_num %d, smp_period %d out of range",
                   p->framesize, p->frameshift, p->fbank_num, p->smp_period);
  // InitFBank()
  w.fftN = 2; w.n = 1;
  while (p->framesize > w.fftN) { w.fftN *= 2; w.n++; }
  int nv2 = w.nv2 = w.fftN / 2;
  w.fres = (float)(1.0E7 / (p->smp_period * w.fftN * 700.0));
  int maxChan = w.maxChan = p->fbank_num + 1;
  w.klo = 2; w.khi = nv2;
  float mlo = 0, mhi = fe_mel(nv2 + 1, w.fres);
  if (p->lopass >= 0) {
    mlo = (float)(1127 * log(1 + (float)p->lopass / 700.0));
    w.klo = (int)(((float)p->lopass * p->smp_period * 1.0e-7 * w.fftN) + 2.5);
    if (w.klo < 2) w.klo = 2;
  }
  if (p->hipass >= 0) {
    mhi = (float)(1127 * log(1 + (float)p->hipass / 700.0));
    w.khi = (int)(((float)p->hipass * p->smp_period * 1.0e-7 * w.fftN) + 0.5);
    if (w.khi > nv2) w.khi = nv2;
  }
  w.cf.assign(maxChan + 1, 0.f);
  float ms = mhi - mlo;
  for (int chan = 1; chan <= maxChan; chan++) w.cf[chan] = ((float)chan / maxChan) * ms + mlo;
  if (p->vtln_alpha != 1.0f && !fe_vtln(w.cf, p, mlo, mhi, maxChan, err)) return false;
  w.loChan.assign(nv2 + 1, 0);
  for (int k = 1, chan = 1; k <= nv2; k++) {
    if (k < w.klo || k > w.khi) w.loChan[k] = -1;
    else {
      float melk = fe_mel(k, w.fres);
      while (chan <= maxChan && w.cf[chan] < melk) ++chan;   // (the reference tests cf[chan] first: same result)
      if (chan - 1 > p->fbank_num)   // the reference would read cf[maxChan + 1] and write fbank[fbank_num + 1]
        return fe_errf(err, "frontend: FFT bin %d lies above the last filter-bank channel (lopass/hipass/VTLN)", k);
      w.loChan[k] = (short)(chan - 1);
    }
  }
  w.loWt.assign(nv2 + 1, 0.f);
  for (int k = 1; k <= nv2; k++) {
    int chan = w.loChan[k];
    if (k < w.klo || k > w.khi) w.loWt[k] = 0.0f;
    else if (chan > 0) w.loWt[k] = (w.cf[chan + 1] - fe_mel(k, w.fres)) / (w.cf[chan + 1] - w.cf[chan]);
    else w.loWt[k] = (w.cf[1] - fe_mel(k, w.fres)) / (w.cf[1] - mlo);
  }
  w.sqrt2var = (float)sqrt(2.0 / p->fbank_num);
  // make_costbl_hamming(), make_fft_table(), make_costbl_makemfcc(), make_sintbl_wcep()
  w.ham.resize(p->framesize);
  float a = (float)(2.0 * FE_PI / (p->framesize - 1));
  for (int i = 1; i <= p->framesize; i++) w.ham[i - 1] = 0.54 - 0.46 * cos((double)(a * (i - 1)));
  w.fftcos.resize(w.n); w.fftsin.resize(w.n);
  for (int m = 1; m <= w.n; m++) {
    int me1 = (1 << m) / 2;
    w.fftcos[m - 1] = cos(FE_PI / me1);
    w.fftsin[m - 1] = -sin(FE_PI / me1);
  }
  if (p->mfcc_dim > 0) {
    w.dct.resize((size_t)p->fbank_num * p->mfcc_dim);
    float B = (float)(FE_PI / p->fbank_num);
    int k = 0;
    for (int i = 1; i <= p->mfcc_dim; i++) {
      float C = i * B;
      for (int j = 1; j <= p->fbank_num; j++) w.dct[k++] = cos(C * (j - 0.5));
    }
    w.wcep.resize(p->mfcc_dim);
    if (p->lifter > 0) {
      float la = (float)(FE_PI / p->lifter), lb = (float)(p->lifter / 2.0);
      for (int i = 0; i < p->mfcc_dim; i++) w.wcep[i] = 1.0 + lb * sin((double)((i + 1) * la));
    } else {
      for (int i = 0; i < p->mfcc_dim; i++) w.wcep[i] = 1.0;
    }
  }
  // The twiddle SEQUENCE of every FFT stage by the serial loop's own recurrence (u <- u * w,
  // mfcc-core.c FFT()): stage m's u_j lands at [me1 - 1 + j], so a butterfly reads the u the loop had.
  w.twRe.assign(w.fftN, 0.0); w.twIm.assign(w.fftN, 0.0);
  for (int m = 1; m <= w.n; m++) {
    int me1 = 1 << (m - 1);
    double uRe = 1.0, uIm = 0.0, wRe = w.fftcos[m - 1], wIm = w.fftsin[m - 1];
    for (int j = 0; j < me1; j++) {
      w.twRe[me1 - 1 + j] = uRe; w.twIm[me1 - 1 + j] = uIm;
      double vRe = uRe * wRe - uIm * wIm, vIm = uRe * wIm + uIm * wRe;
      uRe = vRe; uIm = vIm;
    }
  }
  // per-bin k ranges (loChan is non-decreasing over [klo, khi], and none lies above fbank_num)
  w.kfirst.assign(p->fbank_num + 1, 1); w.klast.assign(p->fbank_num + 1, 0);
  for (int k = w.klo; k <= w.khi; k++) {
    int bin = w.loChan[k];
    for (int b = bin; b <= bin + 1; b++) {
      if (b < 1 || b > p->fbank_num) continue;
      if (w.klast[b] < w.kfirst[b]) w.kfirst[b] = k;
      w.klast[b] = k;
    }
  }
  return true;
}

// jamd_frontend_table(): the size of the named table, of which min(size, cap) entries go to `out`; -1 with `err` set
static inline int fe_table(const jamd_frontend_desc *d, const char *name, void *out, int cap, std::string &err) {
  FeTables w;
  if (!fe_build_tables(d, w, err)) return -1;
  auto put = [&](const auto &v) {
    size_t n = v.size() < (size_t)(cap > 0 ? cap : 0) ? v.size() : (size_t)(cap > 0 ? cap : 0);
    if (out && n) memcpy(out, v.data(), n * sizeof(v[0]));
    return (int)v.size();
  };
  const std::string s(name);
  if (s == "hamming") return put(w.ham);
  if (s == "fft_cos") return put(w.fftcos);
  if (s == "fft_sin") return put(w.fftsin);
  if (s == "dct") return put(w.dct);
  if (s == "wcep") return put(w.wcep);
  if (s == "twiddle_re") return put(std::vector<double>(w.twRe.begin(), w.twRe.begin() + w.fftN - 1));
  if (s == "twiddle_im") return put(std::vector<double>(w.twIm.begin(), w.twIm.begin() + w.fftN - 1));
  if (s == "cf") return put(w.cf);
  if (s == "lowt") return put(w.loWt);
  if (s == "lochan") return put(w.loChan);
  if (s == "info") return put(std::vector<int>{w.fftN, w.n, w.klo, w.khi});
  if (s == "scalars") return put(std::vector<float>{w.fres, w.sqrt2var});
  fe_errf(err, "jamd_frontend_table: unknown table \"%s\"", name);
  return -1;
}

// ---------------------------------------------------------------------------------- counts
static inline long long fe_frames_raw(const jamd_frontend_desc &d, int64_t n) {
  if (n < d.framesize) return 0;
  return (n - d.framesize) / d.frameshift + 1;
}

// The samples of entry u of sample_off, or -1 with `err` set where sample_off is not in order there.  `noun` is what
// an entry is to the caller `who`: "utterance" or "channel".
static inline long long fe_span(const char *who, const char *noun, const int64_t *sample_off, int u, std::string &err) {
  if (sample_off[u] < 0 || sample_off[u + 1] < sample_off[u]) {
    fe_errf(err, "%s: sample_off is not non-decreasing from 0 at %s %d", who, noun, u);
    return -1;
  }
  return sample_off[u + 1] - sample_off[u];
}

struct LvCounts { long long Tb, Nf, To; bool reest; };

// The frame counts of one live segment of n samples (realtime-1stpass.c:290, :853-859, :1197-1287).
static inline LvCounts lv_counts(const jamd_frontend_desc &d, long long n) {
  LvCounts k{0, 0, 0, false};
  if (n >= (long long)d.framesize + 1) k.Tb = (n - d.framesize - 1) / d.frameshift + 1;
  long long Nd = k.Tb;
  if (d.delta && k.Tb < d.delWin) Nd = 0;
  k.Nf = Nd;
  long long holes = 0;
  if (d.acc) {
    if (Nd < d.accWin) k.Nf = 0;
    // a delta vector that the flush loop hands to an acceleration buffer still in its delay advances the reference's
    // frame counter without a vector being stored (:1249-1257): samplenum then differs from now.framenum
    const long long Md = k.Tb > d.delWin ? k.Tb - d.delWin : 0;
    const long long lim = Nd < d.accWin ? Nd : d.accWin;
    holes = lim > Md ? lim - Md : 0;
  }
  k.To = k.Nf - (d.splice - 1);
  if (k.To < 0) k.To = 0;
  k.reest = d.splice == 1 && k.Nf > 0 && holes == 0;
  return k;
}

// Frames out of the main loop for Tb base frames of a segment that has not ended, and rows those complete.
static inline long long lv_open_frames(const jamd_frontend_desc &d, long long Tb) {
  const long long L = (d.delta ? d.delWin : 0) + (d.acc ? d.accWin : 0);
  return Tb > L ? Tb - L : 0;
}
static inline long long lv_rows_of(const jamd_frontend_desc &d, long long frames) {
  return frames > d.splice - 1 ? frames - (d.splice - 1) : 0;
}

// One push of n samples onto a segment that holds n_old (0: the push opens it); `fin` ends the segment.  Before (_old)
// and after (_new): Tb base frames, F feature frames handed out, r samples behind the last whole window, which the
// device keeps.  `rows` is what this push delivers; `reest`: it ends the segment and the variance is re-estimated.
struct LvPush { long long Tb_old, Tb_new, F_old, F_new, r_old, r_new, rows; bool reest; };
static inline LvPush lv_push(const jamd_frontend_desc &d, long long n_old, long long n, bool fin) {
  const LvCounts ko = lv_counts(d, n_old), kn = lv_counts(d, n_old + n);
  LvPush q{ko.Tb, kn.Tb, lv_open_frames(d, ko.Tb), fin ? kn.Nf : lv_open_frames(d, kn.Tb), n_old - ko.Tb * d.frameshift,
           fin ? 0 : n_old + n - kn.Tb * d.frameshift, 0, fin && kn.reest};
  q.rows = lv_rows_of(d, q.F_new) - lv_rows_of(d, q.F_old);
  return q;
}
#endif  // JAMD_FRONTEND_TABLES_H
