// ss_file_check.cpp -- the reader and writer of the mkss / -ssload noise-spectrum file (julius_amd/csrc/ss_file.h,
// the only host code of the spectral subtraction that parses outside data) as a program of their own, so that
// tests/test_frontend_ss_host.py can build them with -fsanitize=address,undefined and run them over a good, an empty,
// a truncated and an over-long file, with buffers sized exactly (the heap checker sees one value too many).
//
//   ss_file_check DIR      writes its files under DIR; prints one line per case; exit 0 when every case behaved
#include "ss_file.h"

#include <cstdlib>
#include <vector>

static int failures = 0;
static void expect(bool ok, const char *what) {
  printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) failures++;
}

static void put_bytes(const std::string &path, const std::vector<unsigned char> &b) {
  FILE *fp = fopen(path.c_str(), "wb");
  if (!fp) { perror(path.c_str()); exit(2); }
  if (!b.empty() && fwrite(b.data(), 1, b.size(), fp) != b.size()) { perror(path.c_str()); exit(2); }
  fclose(fp);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  std::string err;

  // good: write 512 values, read them back into a buffer of exactly 512
  const int n = 512;
  std::vector<float> src(n);
  for (int i = 0; i < n; i++) src[i] = 1000.0f / (float)(i + 1) - 3.0f;
  const std::string good = dir + "/good.ss";
  expect(ssf_write(good.c_str(), src.data(), n, err) == 0, "write 512 values");
  {
    float *out = (float *)malloc(sizeof(float) * n);
    expect(ssf_read(good.c_str(), out, n, err) == n && memcmp(out, src.data(), sizeof(float) * n) == 0, "good file round trip");
    free(out);
  }
  {   // capacity below the count: the count comes back, only `cap` values are written
    float *out = (float *)malloc(sizeof(float) * 7);
    expect(ssf_read(good.c_str(), out, 7, err) == n && memcmp(out, src.data(), sizeof(float) * 7) == 0, "cap 7 of 512");
    free(out);
    expect(ssf_read(good.c_str(), nullptr, 0, err) == n, "cap 0, no buffer");
  }
  {   // a count of zero
    const std::string zero = dir + "/zero.ss";
    expect(ssf_write(zero.c_str(), src.data(), 0, err) == 0 && ssf_read(zero.c_str(), nullptr, 0, err) == 0, "count 0");
  }
  // empty: not even the count
  put_bytes(dir + "/empty.ss", {});
  expect(ssf_read((dir + "/empty.ss").c_str(), nullptr, 0, err) == -1 && !err.empty(), "empty file refused");
  put_bytes(dir + "/short_count.ss", {0, 0});
  expect(ssf_read((dir + "/short_count.ss").c_str(), nullptr, 0, err) == -1, "two bytes refused");
  // truncated: the count says 512, the file holds 300 values and 2 bytes
  {
    std::vector<unsigned char> b = {0, 0, 2, 0};
    b.resize(4 + 4 * 300 + 2, 0x3f);
    put_bytes(dir + "/trunc.ss", b);
    float *out = (float *)malloc(sizeof(float) * n);
    expect(ssf_read((dir + "/trunc.ss").c_str(), out, n, err) == -1 && !err.empty(), "truncated file refused");
    free(out);
  }
  // a count far beyond the file (and beyond any buffer), and a negative one
  {
    std::vector<unsigned char> b = {0x7f, 0xff, 0xff, 0xff, 1, 2, 3, 4};
    put_bytes(dir + "/huge.ss", b);
    float one[1];
    expect(ssf_read((dir + "/huge.ss").c_str(), one, 1, err) == -1, "count 2^31 - 1 over 4 bytes refused");
    b[0] = 0xff;
    put_bytes(dir + "/neg.ss", b);
    expect(ssf_read((dir + "/neg.ss").c_str(), one, 1, err) == -1, "negative count refused");
  }
  // over-long: 16 values declared, 40 in the file; the reference reads the 16 and ignores the rest
  {
    std::vector<unsigned char> b = {0, 0, 0, 16};
    for (int i = 0; i < 40 * 4; i++) b.push_back((unsigned char)(i * 7));
    put_bytes(dir + "/long.ss", b);
    float *out = (float *)malloc(sizeof(float) * 16);
    expect(ssf_read((dir + "/long.ss").c_str(), out, 16, err) == 16 && memcmp(out, "\x15\x0e\x07\x00", 4) == 0,
           "over-long file: the declared 16 values, big-endian");
    free(out);
  }
  expect(ssf_read((dir + "/missing.ss").c_str(), nullptr, 0, err) == -1, "missing file refused");
  expect(ssf_write((dir + "/no/such/dir.ss").c_str(), src.data(), 4, err) == -1, "unwritable path refused");
  return failures ? 1 : 0;
}
