// cmn_file_check.cpp -- the reader and writer of the -cmnload / -cmnsave file (julius_amd/csrc/cmn_file.h, the only
// host code of the live front end that parses outside data) as a program of their own, so that
// tests/test_frontend_live_host.py can build them with -fsanitize=address,undefined and run them over good, short,
// over-long and malformed files, with buffers sized exactly (the heap checker sees one value too many).
//
//   cmn_file_check DIR      writes its files under DIR; prints one line per case; exit 0 when every case behaved
#include "cmn_file.h"

#include <cmath>
#include <vector>

static int failures = 0;
static void expect(bool ok, const char *what) {
  printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) failures++;
}

static void put(const std::string &path, const std::string &b) {
  FILE *fp = fopen(path.c_str(), "wb");
  if (!fp) { perror(path.c_str()); exit(2); }
  if (!b.empty() && fwrite(b.data(), 1, b.size(), fp) != b.size()) { perror(path.c_str()); exit(2); }
  fclose(fp);
}

static std::string be(uint32_t v) {
  const char b[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v};
  return std::string(b, 4);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  std::string err;
  const int V = 39, M = 13;
  std::vector<float> cm(V), cv(V);
  for (int i = 0; i < V; i++) { cm[i] = 3.5f / (float)(i + 1) - 1.0f; cv[i] = 0.25f * (float)(i + 1); }

  // ASCII, mean and variance: round trip into buffers of exactly V floats
  const std::string both = dir + "/both.cmn";
  expect(cmnf_write(both.c_str(), V, cm.data(), cv.data(), err) == 0, "write mean + variance");
  {
    float *a = (float *)malloc(sizeof(float) * V), *b = (float *)malloc(sizeof(float) * V);
    expect(cmnf_read(both.c_str(), V, M, true, a, b, err) == 1, "read mean + variance");
    bool close = true;                        // (%e keeps 7 digits)
    for (int i = 0; i < V; i++) close = close && fabsf(a[i] - cm[i]) <= 1e-6f * fabsf(cm[i]) && fabsf(b[i] - cv[i]) <= 1e-6f * fabsf(cv[i]);
    expect(close, "values of the round trip");
    expect(cmnf_read(both.c_str(), V, M, false, a, nullptr, err) == 1, "variance present, none wanted, no buffer");
    expect(cmnf_read(both.c_str(), V + 1, M, true, a, b, err) == -1 && !err.empty(), "wrong veclen refused");
    free(a); free(b);
  }
  // ASCII, mean alone
  const std::string mean = dir + "/mean.cmn";
  expect(cmnf_write(mean.c_str(), V, cm.data(), nullptr, err) == 0, "write mean alone");
  {
    float *a = (float *)malloc(sizeof(float) * V);
    expect(cmnf_read(mean.c_str(), V, M, true, a, nullptr, err) == 0, "mean alone: no variance reported");
    free(a);
  }
  // a <MEAN> of mfcc_dim entries: the rest zero
  {
    std::string s = "<CEPSNORM> <MFCC_E_D_A_Z>\n<MEAN> 13\n";
    for (int i = 0; i < M; i++) s += " " + std::to_string(i + 0.5);
    s += "\n";
    put(dir + "/short_mean.cmn", s);
    float *a = (float *)malloc(sizeof(float) * V);
    bool ok = cmnf_read((dir + "/short_mean.cmn").c_str(), V, M, false, a, nullptr, err) == 0;
    for (int i = 0; ok && i < V; i++) ok = a[i] == (i < M ? (float)(i + 0.5) : 0.0f);
    expect(ok, "<MEAN> of mfcc_dim values, the rest zero");
    free(a);
  }
  // more mean values than declared; fewer; a truncated variance; more variance values than declared; no <MEAN> at all
  {
    float *a = (float *)malloc(sizeof(float) * 3), *b = (float *)malloc(sizeof(float) * 3);
    put(dir + "/over.cmn", "<CEPSNORM> <>\n<MEAN> 3\n 1 2 3 4 5 6 7 8\n");
    expect(cmnf_read((dir + "/over.cmn").c_str(), 3, 2, false, a, nullptr, err) == -1, "over-long mean refused");
    put(dir + "/under.cmn", "<CEPSNORM> <>\n<MEAN> 3\n 1 2\n");
    expect(cmnf_read((dir + "/under.cmn").c_str(), 3, 2, false, a, nullptr, err) == -1, "short mean refused");
    put(dir + "/truncvar.cmn", "<CEPSNORM> <>\n<MEAN> 3\n 1 2 3\n<VARIANCE> 3\n 1 2\n");
    expect(cmnf_read((dir + "/truncvar.cmn").c_str(), 3, 2, true, a, b, err) == -1, "truncated variance refused");
    put(dir + "/overvar.cmn", "<CEPSNORM> <>\n<MEAN> 3\n 1 2 3\n<VARIANCE> 3\n 1 2 3 4 5 6 7\n");
    expect(cmnf_read((dir + "/overvar.cmn").c_str(), 3, 2, true, a, b, err) == -1, "over-long variance refused");
    put(dir + "/nomean.cmn", "<CEPSNORM> <>\n");
    expect(cmnf_read((dir + "/nomean.cmn").c_str(), 3, 2, false, a, nullptr, err) == -1, "no <MEAN> refused");
    put(dir + "/varonly.cmn", "<CEPSNORM> <>\n<VARIANCE> 3\n 1 2 3\n");
    expect(cmnf_read((dir + "/varonly.cmn").c_str(), 3, 2, true, a, b, err) == -1, "variance without mean refused");
    put(dir + "/hugelen.cmn", "<CEPSNORM> <>\n<MEAN> 2000000000\n 1 2 3 4 5\n");
    expect(cmnf_read((dir + "/hugelen.cmn").c_str(), 3, 2, false, a, nullptr, err) == -1, "absurd count refused");
    put(dir + "/empty.cmn", "");
    expect(cmnf_read((dir + "/empty.cmn").c_str(), 3, 2, false, a, nullptr, err) == -1, "empty file refused");
    put(dir + "/four.cmn", "<CEP");
    expect(cmnf_read((dir + "/four.cmn").c_str(), 3, 2, false, a, nullptr, err) == -1, "four bytes refused");
    // binary form
    std::string bin = be(3);
    const float m3[3] = {1.5f, -2.0f, 0.125f}, v3[3] = {4.0f, 9.0f, 16.0f};
    for (int pass = 0; pass < 2; pass++)
      for (int i = 0; i < 3; i++) { uint32_t u; memcpy(&u, (pass ? v3 : m3) + i, 4); bin += be(u); }
    put(dir + "/bin.cmn", bin);
    expect(cmnf_read((dir + "/bin.cmn").c_str(), 3, 2, true, a, b, err) == 1 && !memcmp(a, m3, 12) && !memcmp(b, v3, 12),
           "binary form, mean and variance");
    expect(cmnf_read((dir + "/bin.cmn").c_str(), 3, 2, false, a, nullptr, err) == 0 && !memcmp(a, m3, 12), "binary form, mean alone");
    expect(cmnf_read((dir + "/bin.cmn").c_str(), 4, 2, false, a, nullptr, err) == -1, "binary form, wrong veclen refused");
    put(dir + "/binshort.cmn", bin.substr(0, 4 + 12 + 6));
    expect(cmnf_read((dir + "/binshort.cmn").c_str(), 3, 2, true, a, b, err) == -1, "binary form, truncated variance refused");
    put(dir + "/binneg.cmn", be(0xffffffffu) + bin.substr(4));
    expect(cmnf_read((dir + "/binneg.cmn").c_str(), 3, 2, false, a, nullptr, err) == -1, "binary form, negative count refused");
    free(a); free(b);
  }
  expect(cmnf_read((dir + "/missing.cmn").c_str(), 3, 2, false, cm.data(), nullptr, err) == -1, "missing file refused");
  return failures ? 1 : 0;
}
