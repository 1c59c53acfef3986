// cmn_file.h -- the cepstral mean / variance file of `-cmnload` / `-cmnsave` (read by CMN_load_from_file(), written by
// CMN_save_to_file(), libsent/src/wav2mfcc/wav2mfcc-pipe.c:514-696).  Plain C++ without device code, like ss_file.h:
// csrc/frontend_live_api.hip wraps the two functions in the C ABI (jamd_frontend_cmn_read / _write), and
// tests/cmn_file_check.cpp compiles them alone under the host sanitizers.  Two forms are read:
//   - the ASCII form (Julius >= 4.3): "<CEPSNORM> <>", "<MEAN> n" with n == veclen or n == mfcc_dim values (the rest of
//     the mean is zero), and an optional "<VARIANCE> veclen" block; tokens are split at "<> \t\r\n" as there (quoting,
//     which mystrtok_quote() would honour, does not occur in such a file and is not served);
//   - the old binary form: big-endian int32 veclen, veclen big-endian floats of mean, then, when the caller wants a
//     variance, veclen floats of variance.
// Gzipped files are not served.  The reader takes nothing in the file on trust: every index is checked against the
// caller's veclen before it is used.
#ifndef JAMD_CMN_FILE_H
#define JAMD_CMN_FILE_H
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// cmean [veclen] is always filled; cvar [veclen] (may be NULL) only where the file holds a variance.  Returns 1 when a
// variance was read, 0 when the file holds a mean only, -1 with `err` set when the reference would refuse the file.
static inline int cmnf_read(const char *path, int veclen, int mfcc_dim, bool want_var, float *cmean, float *cvar,
                            std::string &err) {
  if (veclen < 1) { err = "veclen < 1"; return -1; }
  FILE *fp = fopen(path, "rb");
  if (!fp) { err = std::string("failed to open \"") + path + "\""; return -1; }
  unsigned char ch[5];
  if (fread(ch, 1, 5, fp) != 5) {
    fclose(fp);
    err = std::string("failed to read CMN/CVN file \"") + path + "\"";
    return -1;
  }
  rewind(fp);
  auto is = [&](int i, char up) { return ch[i] == (unsigned char)up || ch[i] == (unsigned char)(up + 32); };
  if (ch[0] == '<' && is(1, 'C') && is(2, 'E') && is(3, 'P') && is(4, 'S')) {
    static const char *delim = "<> \t\r\n";
    char buf[4096];
    int mode = 0, d = 0, dv = 0, len = -1;      // (the reference leaves d / dv / len unset until their block)
    bool fail = false;
    while (!fail && fgets(buf, (int)sizeof buf, fp)) {
      char *save = nullptr;
      for (char *p = strtok_r(buf, delim, &save); p && !fail; p = strtok_r(nullptr, delim, &save)) {
        switch (mode) {
        case 0:
          if (!strcmp(p, "MEAN")) mode = 1;
          else if (!strcmp(p, "VARIANCE")) mode = 3;
          break;
        case 1:
          len = (int)atof(p);
          if (len != veclen && len != mfcc_dim) {
            err = "cepstral dimension mismatch: process = " + std::to_string(veclen) + " (" + std::to_string(mfcc_dim) +
                  "), file = " + std::to_string(len);
            fail = true;
            break;
          }
          for (int i = 0; i < veclen; i++) cmean[i] = 0.0f;
          d = 0;
          mode = 2;
          break;
        case 2:
          if (!strcmp(p, "VARIANCE")) mode = 3;
          else if (d >= len || d >= veclen) { err = "corrupted data (more mean values than declared)"; fail = true; }
          else cmean[d++] = (float)atof(p);
          break;
        case 3:
          len = (int)atof(p);
          if (len != veclen) {
            err = "cepstral dimension mismatch: process = " + std::to_string(veclen) + ", file = " + std::to_string(len);
            fail = true;
            break;
          }
          dv = 0;
          mode = 4;
          break;
        default:
          if (dv >= len) { err = "corrupted data (more variance values than declared)"; fail = true; }
          else { if (cvar) cvar[dv] = (float)atof(p); dv++; }
          break;
        }
      }
    }
    fclose(fp);
    if (fail) return -1;
    // the reference's closing test, `len` being the last block's count (wav2mfcc-pipe.c:606): a mean of mfcc_dim values
    // followed by a variance block is refused by it as well
    if (len < 0 || d != len || (mode >= 3 && dv != len)) { err = "corrupted data (fewer values than declared)"; return -1; }
    return mode >= 3 ? 1 : 0;
  }
  auto be32 = [&](uint32_t *v) {
    unsigned char b[4];
    if (fread(b, 1, 4, fp) != 4) return false;
    *v = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | (uint32_t)b[3];
    return true;
  };
  uint32_t n;
  if (!be32(&n)) { fclose(fp); err = "failed to read header"; return -1; }
  if (n != (uint32_t)veclen) {
    fclose(fp);
    err = "cepstral dimension mismatch: process = " + std::to_string(veclen) + ", file = " + std::to_string((int32_t)n);
    return -1;
  }
  for (int pass = 0; pass < (want_var ? 2 : 1); pass++) {
    for (int i = 0; i < veclen; i++) {
      uint32_t v;
      if (!be32(&v)) {
        fclose(fp);
        err = pass ? "failed to read variance for CVN" : "failed to read mean for CMN";
        return -1;
      }
      float *dst = pass ? cvar : cmean;
      if (dst) memcpy(dst + i, &v, 4);
    }
  }
  fclose(fp);
  return want_var ? 1 : 0;
}

// CMN_save_to_file(): the ASCII form, byte for byte.  cvar == NULL writes no <VARIANCE> block.
static inline int cmnf_write(const char *path, int veclen, const float *cmean, const float *cvar, std::string &err) {
  FILE *fp = fopen(path, "wb");
  if (!fp) { err = std::string("failed to open \"") + path + "\" for writing"; return -1; }
  bool ok = fprintf(fp, "<CEPSNORM> <>\n") > 0 && fprintf(fp, "<MEAN> %d\n", veclen) > 0;
  for (int d = 0; ok && d < veclen; d++) ok = fprintf(fp, " %e\n", cmean[d]) > 0;
  if (cvar) {
    ok = ok && fprintf(fp, "<VARIANCE> %d\n", veclen) > 0;
    for (int d = 0; ok && d < veclen; d++) ok = fprintf(fp, " %e\n", cvar[d]) > 0;
  }
  ok = (fclose(fp) == 0) && ok;
  if (!ok) { err = std::string("failed to write \"") + path + "\""; return -1; }
  return 0;
}
#endif  // JAMD_CMN_FILE_H
