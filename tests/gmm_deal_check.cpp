// gmm_deal_check.cpp -- csrc/gmm_deal.h alone (no HIP header), as a program of its own under the host sanitizers
// (tests/test_gmm_deal_host.py builds and runs it).  For every launch of 1 .. 41 state ranges x 1 .. 20 frame groups the
// eight shares are walked ticket by ticket: every (range, group) is named exactly once, a share ends where gd_len()
// says and names nothing behind its end, the lengths sum to ranges x groups, the full rounds stay on their XCD, and
// the leftover runs differ by at most one `per`.
#include <cstdio>
#include <vector>

#include "gmm_deal.h"

static int failures = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                                       \
  } while (0)

int main() {
  long long launches = 0, tiles = 0;
  for (int nstb = 1; nstb <= 41; nstb++)
    for (int nfw = 1; nfw <= 20; nfw++) {
      const GmmDeal d = gd_make(nstb, nfw);
      std::vector<int> seen((size_t)nstb * nfw, 0);
      long long sum = 0;
      int left_min = 1 << 30, left_max = 0;
      for (int x = 0; x < kGdShares; x++) {
        const int len = gd_len(d, x);
        CHECK(len >= d.full && len <= d.full + d.per, "nstb %d nfw %d share %d len %d", nstb, nfw, x, len);
        sum += len;
        const int left = len - d.full;
        if (left < left_min) left_min = left;
        if (left > left_max) left_max = left;
        int range = -1, group = -1;
        for (int n = 0; n < len; n++) {
          const bool ok = gd_ticket(d, x, n, range, group);
          CHECK(ok, "nstb %d nfw %d share %d ticket %d of %d not named", nstb, nfw, x, n, len);
          if (!ok) continue;
          CHECK(range >= 0 && range < nstb && group >= 0 && group < nfw, "nstb %d nfw %d share %d ticket %d -> (%d, %d)",
                nstb, nfw, x, n, range, group);
          if (range < 0 || range >= nstb || group < 0 || group >= nfw) continue;
          if (n < d.full) CHECK((range & 7) == x && range < d.k8, "nstb %d nfw %d: full-round range %d in share %d", nstb, nfw, range, x);
          else CHECK(range >= d.k8, "nstb %d nfw %d: leftover ticket %d names range %d", nstb, nfw, n, range);
          seen[(size_t)range * nfw + group]++;
        }
        // behind the end: nothing, however far a head has overshot
        for (int n = len; n < len + 3 * nfw + 70; n++)
          CHECK(!gd_ticket(d, x, n, range, group), "nstb %d nfw %d share %d names ticket %d behind its end %d", nstb, nfw, x, n, len);
        CHECK(!gd_ticket(d, x, 0x7fffffff, range, group) && !gd_ticket(d, x, -1, range, group), "nstb %d nfw %d share %d", nstb, nfw, x);
      }
      CHECK(sum == (long long)nstb * nfw, "nstb %d nfw %d: lengths sum to %lld", nstb, nfw, sum);
      CHECK(left_max - left_min <= d.per, "nstb %d nfw %d: leftover runs %d .. %d, per %d", nstb, nfw, left_min, left_max, d.per);
      CHECK(d.per <= nfw, "nstb %d nfw %d: per %d (a run would touch more than two ranges)", nstb, nfw, d.per);
      for (size_t i = 0; i < seen.size(); i++)
        CHECK(seen[i] == 1, "nstb %d nfw %d: (range %d, group %d) named %d times", nstb, nfw, (int)(i / nfw), (int)(i % nfw), seen[i]);
      launches++;
      tiles += (long long)nstb * nfw;
    }
  if (!failures) printf("ok: %lld launches, %lld tiles, each named once\n", launches, tiles);

  // the grid of a pull launch: a multiple of 8, at least 8, the override taken when given
  CHECK(gd_pull_grid(1024, 0) == 1024 && gd_pull_grid(1027, 0) == 1024 && gd_pull_grid(3, 0) == 8, "grid from capacity");
  CHECK(gd_pull_grid(1024, 8) == 8 && gd_pull_grid(1024, 20) == 16 && gd_pull_grid(1024, 5) == 8 && gd_pull_grid(1024, -4) == 1024, "grid override");
  if (!failures) printf("ok: grid choice\n");
  return failures ? 1 : 0;
}
