// adin_cut_plan_check.cpp -- csrc/adin_cut_plan.h as a stand-alone program, for the host sanitizers
// (tests/test_adin_cut_host.py builds it with -fsanitize=address,undefined and runs it): the parameters of the defaults,
// descriptors at and beyond every limit (nothing may overflow an int or convert a float that does not fit), and what
// the kernels rely on for every accepted descriptor of a random sweep: the history reaches behind every range a push
// can deliver, the swap buffer never holds more than sbsize, and the bounds grow with the chunk.
#include <climits>
#include <cstdio>
#include <random>
#include <string>

#include "adin_cut_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); failures++; } \
  } while (0)

static jamd_adin_cut_desc desc(int sfreq, int lv, int zc, int head, int tail, int chunk) {
  jamd_adin_cut_desc d;
  d.sfreq = sfreq; d.level_thres = lv; d.zero_cross_num = zc; d.head_margin_msec = head; d.tail_margin_msec = tail;
  d.chunk_size = chunk;
  return d;
}

int main() {
  std::string err;
  AcParams p;
  {
    const jamd_adin_cut_desc d = desc(16000, 2000, 60, 300, 400, 1000);
    CHECK(ac_params(&d, p, err), "defaults: %s", err.c_str());
    CHECK(p.c_length == 4800 && p.noise_zerocross == 18 && p.nc_max == 8 && p.sbsize == 7840 && p.hist == 8840, "defaults");
    CHECK(ac_push_cap(&d, p, 4000) == 4000 + 999 + 4800 + 7840 && ac_parts_cap(&d, p, 4000) == 2, "bounds of a live push");
    CHECK(ac_blocks_cap(&d, 0) == 1 && ac_parts_cap(&d, p, 0) == 2, "an empty push with end of stream");
  }
  printf("ok: defaults\n");

  {
    const int big[] = {INT_MAX, INT_MAX - 1, 1 << 30, (1 << 24) + 1, 1 << 24, (1 << 24) - 1, 0, -1, INT_MIN};
    int accepted = 0;
    for (int sf : big) for (int zc : big) for (int hd : big) for (int tl : big) for (int ch : big) {
      const jamd_adin_cut_desc d = desc(sf, 2000, zc, hd, tl, ch);
      if (ac_params(&d, p, err)) {
        accepted++;
        CHECK(p.c_length >= ch && p.hist > 0 && p.sbsize >= 0 && p.nc_max >= 2, "an accepted extreme");
        CHECK(ac_push_cap(&d, p, 0x3fffffffLL) > 0 && ac_parts_cap(&d, p, 0x3fffffffLL) > 0, "bounds of the longest push");
      } else {
        CHECK(!err.empty(), "a refusal without a reason");
      }
    }
    CHECK(!ac_params(nullptr, p, err), "NULL");
    printf("ok: extremes (%d accepted)\n", accepted);
  }

  {
    std::mt19937 rng(11);
    int accepted = 0;
    for (int i = 0; i < 20000; i++) {
      const int rates[] = {8000, 11025, 16000, 22050, 44100, 48000};
      const jamd_adin_cut_desc d = desc(rates[rng() % 6], (int)(rng() % 9000), (int)(rng() % 400), (int)(rng() % 1000),
                                        (int)(rng() % 1500), 1 + (int)(rng() % 5000));
      if (!ac_params(&d, p, err)) continue;
      accepted++;
      // the tail as the block loop walks it: nc_max blocks, delivered while rest_tail lasts, then swapped
      int rest = p.sbsize - p.c_length, sblen = 0;
      for (int nc = 1; nc <= p.nc_max; nc++) {
        if (rest == 0) sblen += d.chunk_size;
        else rest = rest < d.chunk_size ? 0 : rest - d.chunk_size;
      }
      CHECK(sblen <= p.sbsize, "swap buffer: %d of %d", sblen, p.sbsize);
      // the oldest sample a block can deliver lies max(c_length, sblen + w) behind its end, the block ends at the most
      // chunk_size - 1 ... 0 samples into the carry: all of it inside the ring
      CHECK(p.hist >= p.c_length + d.chunk_size - 1 && p.hist >= sblen + d.chunk_size, "history");
      long long last_s = 0, last_p = 0;
      for (long long n : {0LL, 1LL, (long long)d.chunk_size, d.chunk_size + 4000LL, 227441LL, 0x3fffffffLL}) {
        const long long s = ac_push_cap(&d, p, n), q = ac_parts_cap(&d, p, n);
        CHECK(s >= last_s && q >= last_p && s >= n + p.c_length && q >= 2, "bounds at %lld", n);
        last_s = s; last_p = q;
      }
    }
    CHECK(accepted > 2000, "the sweep accepts %d", accepted);
    printf("ok: sweep (%d accepted)\n", accepted);
  }
  if (failures) printf("FAILED: %d checks\n", failures);
  return failures ? 1 : 0;
}
