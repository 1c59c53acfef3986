// ss_file.h -- the noise-spectrum file of `mkss` / `-ssload` (written by mkss/mkss.c:219-233, read by
// new_SS_load_from_file(), libsent/src/wav2mfcc/ss.c:65-96): a big-endian int32 count, then that many
// big-endian float32.  Plain C++ without device code: csrc/frontend_api.hip wraps the two functions in the C ABI
// (jamd_frontend_ss_read / _write), and tests/ss_file_check.cpp compiles them alone under the host sanitizers.
// The reader takes nothing in the file on trust: the count sizes no allocation, and the values are copied in
// fixed pieces up to the caller's capacity.
#ifndef JAMD_SS_FILE_H
#define JAMD_SS_FILE_H
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

// Returns the count the file declares (copies min(count, cap) values into out), or -1 with `err` set.  Bytes
// after the declared values are ignored, as the reference ignores them.
static inline int ssf_read(const char *path, float *out, int cap, std::string &err) {
  FILE *fp = fopen(path, "rb");
  if (!fp) { err = std::string("failed to open \"") + path + "\""; return -1; }
  unsigned char b[4 * 256];
  if (fread(b, 1, 4, fp) != 4) {
    fclose(fp);
    err = std::string("\"") + path + "\" is shorter than its count field";
    return -1;
  }
  const uint32_t cnt = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | (uint32_t)b[3];
  if (cnt > 0x7fffffffu) {
    fclose(fp);
    err = std::string("\"") + path + "\" declares a negative count";
    return -1;
  }
  const int n = (int)cnt;
  for (int done = 0; done < n;) {
    const int want = n - done < 256 ? n - done : 256;
    if (fread(b, 4, (size_t)want, fp) != (size_t)want) {
      fclose(fp);
      err = std::string("\"") + path + "\" is truncated: it declares " + std::to_string(n) + " values";
      return -1;
    }
    for (int i = 0; i < want && out && done + i < cap; i++) {
      const unsigned char *q = b + 4 * i;
      const uint32_t v = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3];
      memcpy(out + done + i, &v, 4);
    }
    done += want;
  }
  fclose(fp);
  return n;
}

static inline int ssf_write(const char *path, const float *noise, int n, std::string &err) {
  FILE *fp = fopen(path, "wb");
  if (!fp) { err = std::string("failed to open \"") + path + "\" for writing"; return -1; }
  bool ok = true;
  auto put = [&](uint32_t v) {
    const unsigned char b[4] = {(unsigned char)(v >> 24), (unsigned char)(v >> 16), (unsigned char)(v >> 8), (unsigned char)v};
    ok = ok && fwrite(b, 1, 4, fp) == 4;
  };
  put((uint32_t)n);
  for (int i = 0; i < n; i++) {
    uint32_t v;
    memcpy(&v, noise + i, 4);
    put(v);
  }
  ok = (fclose(fp) == 0) && ok;
  if (!ok) { err = std::string("failed to write \"") + path + "\""; return -1; }
  return 0;
}
#endif  // JAMD_SS_FILE_H
