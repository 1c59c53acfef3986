// adin_plan_check.cpp -- csrc/adin_plan.h as a stand-alone program, for the host sanitizers (tests/test_adin_host.py
// builds it with -fsanitize=address,undefined and runs it): the closed-form counts against a literal walk of
// do_filter()'s block / delay bookkeeping, what a push hands the kernels (every index the kernels form from it stays
// inside Z), the descriptor checks and the coefficient file reader on well-formed and hostile files.
// usage: adin_plan_check <writable dir>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "adin_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); failures++; } \
  } while (0)

// do_filter()'s counters alone (ds48to16.c:191-260): bp, count, delay -> outputs handed on by one call
struct Walk {
  int dec, intr, delay, bp = 0, count = 1;
  long long feed(long long len) {
    long long out = 0, s = 0;
    for (;;) {
      while (bp < kAdBlock && s < len) { bp++; s++; }
      if (bp < kAdBlock) break;
      int d = 0;
      for (int k = 0; k < bp; k++)
        for (int i = 0; i < intr; i++)
          if (--count == 0) { d++; count = dec; }
      if (delay) {
        if (d > delay) { out += d - delay; delay = 0; } else delay -= d;
      } else out += d;
      bp -= kAdBlock;
    }
    return out;
  }
};

static void write_file(const std::string &p, const std::string &s) {
  FILE *f = fopen(p.c_str(), "wb");
  fwrite(s.data(), 1, s.size(), f);
  fclose(f);
}

int main(int argc, char **argv) {
  if (argc < 2) { printf("usage: adin_plan_check <dir>\n"); return 2; }
  const std::string dir = argv[1];
  std::mt19937 rng(7);

  // ---- counts: every table length that changes a delay or a history, random cuts
  const int lens[][2] = {{217, 401}, {1, 1}, {2, 3}, {513, 513}, {7, 8}, {216, 400}, {5, 2}};
  for (auto &ln : lens) {
    const AdCascade c = ad_cascade(ln[0], ln[1]);
    Walk w[3];
    long long A[3] = {0, 0, 0}, total = 0;
    for (int s = 0; s < 3; s++) { w[s].dec = c.st[s].dec; w[s].intr = c.st[s].intr; w[s].delay = c.st[s].delay; }
    CHECK(c.st[0].hist <= 128 && c.st[1].hist <= 512 && c.st[0].hist % 2 == 0 && c.st[1].hist % 2 == 0, "hist");
    for (int push = 0; push < 400; push++) {
      long long n = (long long)(rng() % (push % 7 == 0 ? 5000 : 700));
      long long before = A[0];
      for (int s = 0; s < 3; s++) {
        const AdStage &g = c.st[s];
        const AdPush p = ad_push(g, A[s], n);
        const long long got = w[s].feed(n);
        CHECK(p.n_out == got, "tables %d/%d stage %d push %d: n_out %d, the walk gives %lld", ln[0], ln[1], s, push, p.n_out, got);
        CHECK(ad_emitted(g, A[s] + n) - ad_emitted(g, A[s]) == got, "ad_emitted stage %d", s);
        CHECK(p.pend >= 0 && p.pend < kAdBlock && p.adv % kAdBlock == 0 && p.pend + n - p.adv == w[s].bp, "pending");
        CHECK(p.t_b >= 0 && p.t_b < g.dec && p.drop >= 0 && p.drop <= p.n_raw, "t_b %d drop %d", p.t_b, p.drop);
        if (p.n_raw > 0) {
          // the newest input the last output reads is a consumed one; the oldest lies inside the history
          const long long tick = p.t_b + (long long)g.dec * (p.n_raw - 1), k = tick / g.intr;
          CHECK(k < p.adv, "stage %d reads input %lld of %d consumed", s, k, p.adv);
          CHECK((long long)g.dec * p.n_raw + p.t_b >= (long long)g.intr * p.adv, "stage %d leaves an output behind", s);
          CHECK((g.hdn_len - (int)(tick % g.intr)) / g.intr <= g.hist, "history too short");
        } else {
          CHECK(p.adv == 0 || g.intr * (long long)p.adv <= p.t_b, "no output from %d consumed", p.adv);
        }
        A[s] += n;
        n = got;
      }
      total += n;
      CHECK(ad_cascade_emitted(c, A[0]) == total, "cascade total");
      CHECK(ad_cascade_emitted(c, A[0]) - ad_cascade_emitted(c, before) == n, "cascade push");
    }
  }
  {
    const AdCascade c = ad_cascade(217, 401);
    const long long in[] = {767, 768, 4000, 48000, 100000}, want[] = {0, 28, 1052, 15772, 33052};
    for (int i = 0; i < 5; i++) CHECK(ad_cascade_emitted(c, in[i]) == want[i], "%lld samples", in[i]);
    CHECK(c.st[0].delay == 36 && c.st[1].delay == 100 && c.st[0].hist == 54 && c.st[1].hist == 400, "delays");
    CHECK(ad_cascade_emitted(c, 1LL << 40) > 0, "long streams");
  }
  printf("ok: counts\n");

  // ---- descriptor
  {
    std::string err;
    double t[513] = {0};
    jamd_adin_desc d{};
    d.level_coef = 1.0f; d.strip_zero = 1;
    CHECK(ad_check_desc(&d, true, err), "defaults");
    CHECK(!ad_check_desc(nullptr, true, err), "NULL");
    d.down48 = 1;
    CHECK(!ad_check_desc(&d, true, err) && err.find("tables") != std::string::npos, "no tables: %s", err.c_str());
    d.n_3to4 = 217; d.n_2to1 = 401;
    CHECK(!ad_check_desc(&d, true, err) && ad_check_desc(&d, false, err), "counts without pointers");
    d.fir_3to4 = t; d.fir_2to1 = t;
    CHECK(ad_check_desc(&d, true, err), "tables");
    d.n_2to1 = 514;
    CHECK(!ad_check_desc(&d, true, err), "514 entries");
    d.n_2to1 = 513; d.n_3to4 = 0;
    CHECK(!ad_check_desc(&d, true, err), "0 entries");
    d.n_3to4 = 1;
    CHECK(ad_check_desc(&d, true, err), "1 entry");
    for (float c : {65536.0f, -65536.0f, 1e30f}) { d.level_coef = c; CHECK(!ad_check_desc(&d, true, err), "coef %g", c); }
    d.level_coef = 0.0f / 1.0f; CHECK(ad_check_desc(&d, true, err), "coef 0");
    d.level_coef = 65535.996f; CHECK(ad_check_desc(&d, true, err), "coef below the bound");
    volatile float z = 0.f;
    d.level_coef = z / z; CHECK(!ad_check_desc(&d, true, err), "coef NaN");
  }
  printf("ok: descriptor\n");

  // ---- coefficient file
  {
    std::string err;
    std::vector<double> out(600, -1.0);
    CHECK(ad_fir_read((dir + "/missing").c_str(), out.data(), 513, err) == -1, "missing file");
    write_file(dir + "/empty", "");
    CHECK(ad_fir_read((dir + "/empty").c_str(), out.data(), 513, err) == -1, "empty file");
    write_file(dir + "/three", "1.5\n-2.25e-3\r\n  7 trailing\n");
    CHECK(ad_fir_read((dir + "/three").c_str(), out.data(), 513, err) == 3 && out[0] == 1.5 && out[1] == -2.25e-3 && out[2] == 7.0,
          "three entries");
    CHECK(ad_fir_read((dir + "/three").c_str(), out.data(), 2, err) == -1, "cap 2");
    write_file(dir + "/noeol", "1\n2");
    CHECK(ad_fir_read((dir + "/noeol").c_str(), out.data(), 513, err) == 2 && out[1] == 2.0, "no newline at the end");
    std::string many;
    for (int i = 0; i < 600; i++) many += std::to_string(i) + "\n";
    write_file(dir + "/many", many);
    out.assign(600, -1.0);
    CHECK(ad_fir_read((dir + "/many").c_str(), out.data(), 513, err) == 513 && out[512] == 512.0 && out[513] == -1.0,
          "stops at 513 entries as load_filter() does");
    write_file(dir + "/long", std::string(2000, '9') + "\n3\n");   // fgets(buf, 512) cuts the line in four
    CHECK(ad_fir_read((dir + "/long").c_str(), out.data(), 513, err) == 5 && out[4] == 3.0, "an over-long line");
    write_file(dir + "/binary", std::string("\0\xff\n\n", 4) + "x\n");
    CHECK(ad_fir_read((dir + "/binary").c_str(), out.data(), 513, err) == 3 && out[0] == 0.0, "not numbers: atof gives 0");
  }
  printf("ok: coefficient file\n");
  if (failures) printf("FAILED: %d checks\n", failures);
  return failures ? 1 : 0;
}
