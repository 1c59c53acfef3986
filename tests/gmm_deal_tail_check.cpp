// gmm_deal_tail_check.cpp -- the deal with a fine-grained tail (csrc/gmm_deal.h: gd_tail_make, gd_tail_len,
// gd_tail_ticket) alone, no HIP header, as a program of its own under the host sanitizers
// (tests/test_gmm_deal_tail_host.py builds and runs it).  For every launch of 1 .. 41 state ranges x 1 .. 20 frame
// groups, Q in {0, 1, 3, len, len + 5} (len: the share's own length in tiles) and pieces of 2, 4 and 8 states, with S a
// multiple of 16 and not (the last range 1, 8 or 13 states), the eight shares are walked ticket by ticket: every
// (state, group) below S is covered exactly once, a ticket names states of its own range only, a share is as long as
// specified (len + (16 / sub - 1) min(Q, len)) and names nothing behind its end, the tail is tile-major with the piece
// fastest over the share's last min(Q, len) tiles, and Q = 0 is gd_ticket / gd_len ticket for ticket.
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

constexpr int kNsb = 16;

// one launch, one (Q rule, sub); qrule: 0, 1, 3 as they are, -1: len, -2: len + 5 -- Q is one number per launch, so
// the rules "len" and "len + 5" take the length of share `qshare`
static void walk(int nstb, int nfw, int S, int qrule, int qshare, int sub, long long &tickets, long long &empties) {
  const GmmDeal d = gd_make(nstb, nfw);
  const int Q = qrule >= 0 ? qrule : gd_len(d, qshare) + (qrule == -2 ? 5 : 0);
  const GmmTail t = gd_tail_make(Q, kNsb, sub);
  const int nper = kNsb / sub;
  CHECK(t.q == Q && t.nsb == kNsb && t.sub == sub && (1 << t.shift) == nper, "tail of Q %d sub %d: q %d sub %d shift %d", Q, sub, t.q, t.sub, t.shift);
  std::vector<int> seen((size_t)S * nfw, 0);
  for (int x = 0; x < kGdShares; x++) {
    const int len = gd_len(d, x);
    const int q = Q < len ? Q : len;
    const int tlen = gd_tail_len(d, t, x);
    CHECK(tlen == len + (nper - 1) * q, "nstb %d nfw %d Q %d sub %d share %d: %d tickets, %d tiles", nstb, nfw, Q, sub, x, tlen, len);
    for (int n = 0; n < tlen; n++) {
      int range = -1, group = -1, s0 = -1, ns = -1;
      const bool ok = gd_tail_ticket(d, t, x, n, range, group, s0, ns);
      CHECK(ok, "nstb %d nfw %d Q %d sub %d share %d ticket %d of %d not named", nstb, nfw, Q, sub, x, n, tlen);
      if (!ok) continue;
      // the tile this ticket belongs to, from the plain deal
      const int whole = len - q;
      const int tile = n < whole ? n : whole + (n - whole) / nper;
      int r2 = -1, g2 = -1;
      const bool ok2 = gd_ticket(d, x, tile, r2, g2);
      CHECK(ok2 && r2 == range && g2 == group, "nstb %d nfw %d Q %d sub %d share %d ticket %d: (%d, %d), tile %d is (%d, %d)",
            nstb, nfw, Q, sub, x, n, range, group, tile, r2, g2);
      if (n < whole) CHECK(s0 == 0 && ns == kNsb, "share %d ticket %d in front of the tail: states %d + %d", x, n, s0, ns);
      else CHECK(s0 == ((n - whole) % nper) * sub && ns == sub, "share %d ticket %d of the tail: states %d + %d", x, n, s0, ns);
      CHECK(range >= 0 && range < nstb && group >= 0 && group < nfw && s0 >= 0 && ns > 0 && s0 + ns <= kNsb,
            "nstb %d nfw %d Q %d sub %d share %d ticket %d -> (%d, %d, %d, %d)", nstb, nfw, Q, sub, x, n, range, group, s0, ns);
      if (range < 0 || range >= nstb || group < 0 || group >= nfw || s0 < 0 || ns <= 0 || s0 + ns > kNsb) continue;
      tickets++;
      const int sb = range * kNsb + s0;
      if (sb >= S) { empties++; continue; }            // a valid ticket with no work
      const int se = sb + ns < S ? sb + ns : S;        // (as the kernel cuts it)
      for (int s = sb; s < se; s++) seen[(size_t)s * nfw + group]++;
      if (Q == 0) CHECK(n < len && s0 == 0 && ns == kNsb, "Q 0: share %d ticket %d", x, n);
    }
    if (Q == 0) CHECK(tlen == len, "Q 0: share %d has %d tickets, gd_len %d", x, tlen, len);
    // behind the end: nothing, however far a head has overshot
    int a, b, c, e;
    for (int n = tlen; n < tlen + 3 * nfw + 70; n++)
      CHECK(!gd_tail_ticket(d, t, x, n, a, b, c, e), "nstb %d nfw %d Q %d sub %d share %d names ticket %d behind its end %d", nstb, nfw, Q, sub, x, n, tlen);
    CHECK(!gd_tail_ticket(d, t, x, 0x7fffffff, a, b, c, e) && !gd_tail_ticket(d, t, x, -1, a, b, c, e), "nstb %d nfw %d share %d", nstb, nfw, x);
  }
  for (size_t i = 0; i < seen.size(); i++)
    CHECK(seen[i] == 1, "nstb %d nfw %d S %d Q %d sub %d: (state %d, group %d) covered %d times", nstb, nfw, S, Q, sub, (int)(i / nfw), (int)(i % nfw), seen[i]);
}

int main() {
  long long launches = 0, tickets = 0, empties = 0;
  const int subs[3] = {2, 4, 8};
  const int last[4] = {16, 1, 8, 13};                 // states of the last range
  const int qrules[5] = {0, 1, 3, -1, -2};
  for (int nstb = 1; nstb <= 41; nstb++)
    for (int nfw = 1; nfw <= 20; nfw++)
      for (int li = 0; li < 4; li++) {
        const int S = (nstb - 1) * kNsb + last[li];
        for (int qi = 0; qi < 5; qi++)
          for (int si = 0; si < 3; si++) {
            // "len" differs between the shares of a launch: take the longest (share 0) and the shortest (share 7)
            walk(nstb, nfw, S, qrules[qi], 0, subs[si], tickets, empties);
            if (qrules[qi] < 0) walk(nstb, nfw, S, qrules[qi], kGdShares - 1, subs[si], tickets, empties);
            launches++;
          }
      }
  if (!failures) printf("ok: %lld launches, %lld tickets (%lld of them empty), each state and group covered once\n", launches, tickets, empties);

  // the tail's parameters: a piece that is no power of two or wider than the tile falls back to kGdSub, Q < 0 to none
  {
    const GmmTail a = gd_tail_make(7, 16, 4), b = gd_tail_make(-3, 16, 3), c = gd_tail_make(5, 16, 32), e = gd_tail_make(5, 16, 16), f = gd_tail_make(1, 16, 0);
    CHECK(a.q == 7 && a.sub == 4 && a.shift == 2, "plain");
    CHECK(b.q == 0 && b.sub == kGdSub && b.shift == 2, "sub 3, Q -3: %d %d %d", b.q, b.sub, b.shift);
    CHECK(c.sub == kGdSub && c.shift == 2, "sub 32: %d %d", c.sub, c.shift);
    CHECK(e.sub == 16 && e.shift == 0, "sub 16: %d %d", e.sub, e.shift);
    CHECK(f.sub == kGdSub && f.shift == 2, "sub 0: %d %d", f.sub, f.shift);
    CHECK(gd_tail_default(1024) == 1024 && gd_tail_default(8) == 8 && gd_tail_default(16) == 16 && gd_tail_default(24) == 24, "default Q");
    // Q = 0 against the plain deal at the bench shape, and the lengths with the default tail there
    const GmmDeal d = gd_make(188, 500);
    const GmmTail t0 = gd_tail_make(0, 16, 4), t = gd_tail_make(gd_tail_default(1024), 16, 4);
    for (int x = 0; x < kGdShares; x++) {
      CHECK(gd_tail_len(d, t0, x) == gd_len(d, x) && gd_tail_len(d, t, x) == gd_len(d, x) + 3 * 1024, "bench shape, share %d", x);
      for (int n = -2; n < gd_len(d, x) + 5; n++) {
        int r1 = -1, g1 = -1, r2 = -1, g2 = -1, s0 = -1, ns = -1;
        const bool k1 = gd_ticket(d, x, n, r1, g1), k2 = gd_tail_ticket(d, t0, x, n, r2, g2, s0, ns);
        CHECK(k1 == k2 && (!k1 || (r1 == r2 && g1 == g2 && s0 == 0 && ns == 16)), "bench shape, Q 0, share %d ticket %d", x, n);
      }
    }
  }
  if (!failures) printf("ok: tail parameters\n");
  return failures ? 1 : 0;
}
