// frontend_tables_check.cpp -- the device-free part of the audio front end (julius_amd/csrc/frontend_tables.h: the HTK
// config parser, the tables of WMP_work_new(), the frame and row counts of both front ends) as a program of its own, so
// that tests/test_frontend_host.py can build it with -fsanitize=address,undefined and run it over configs that end in
// CRLF, lack values or pass the line buffer, over the smallest and largest windows, band limits and VTLN, accepted and
// refused, and over every sample count of a short live segment cut at every point.  Values against the reference are
// in the Python tests; here every case has to behave, every table has to hold what its size says, and no report.
//
//   frontend_tables_check DIR      writes its files under DIR; prints one line per case; exit 0 when every case behaved
#include "frontend_tables.h"

static int failures = 0;
static void expect(bool ok, const std::string &what) {
  printf("%s: %s\n", ok ? "ok" : "FAILED", what.c_str());
  if (!ok) failures++;
}

static std::string put_text(const std::string &dir, const char *name, const std::string &text) {
  const std::string path = dir + "/" + name;
  FILE *fp = fopen(path.c_str(), "wb");
  if (!fp || fwrite(text.data(), 1, text.size(), fp) != text.size()) { perror(path.c_str()); exit(2); }
  fclose(fp);
  return path;
}

static jamd_frontend_desc desc(int framesize = 400, int frameshift = 160) {
  jamd_frontend_desc d;
  fe_default_desc(JAMD_F_MFCC | JAMD_F_E | JAMD_F_D | JAMD_F_A | JAMD_F_Z, 39, &d);
  d.framesize = framesize; d.frameshift = frameshift;
  return d;
}

// Every table as long as the descriptor says, every index a kernel would follow inside the table it points into.
static bool tables_sound(const jamd_frontend_desc &d, const FeTables &w) {
  bool ok = w.fftN >= d.framesize && w.fftN < 2 * d.framesize + 2 && (1 << w.n) == w.fftN && w.nv2 == w.fftN / 2;
  ok = ok && (int)w.ham.size() == d.framesize && (int)w.twRe.size() == w.fftN && (int)w.twIm.size() == w.fftN;
  ok = ok && (int)w.cf.size() == d.fbank_num + 2 && (int)w.loChan.size() == w.nv2 + 1 && (int)w.loWt.size() == w.nv2 + 1;
  ok = ok && (int)w.dct.size() == d.fbank_num * d.mfcc_dim && (int)w.wcep.size() == d.mfcc_dim;
  ok = ok && (int)w.kfirst.size() == d.fbank_num + 1 && (int)w.klast.size() == d.fbank_num + 1;
  ok = ok && w.klo >= 2 && w.khi <= w.nv2;
  for (int k = 1; ok && k <= w.nv2; k++)
    ok = k < w.klo || k > w.khi ? w.loChan[k] == -1 : (w.loChan[k] >= 0 && w.loChan[k] <= d.fbank_num);
  for (int b = 1; ok && b <= d.fbank_num; b++)
    ok = w.klast[b] < w.kfirst[b] || (w.kfirst[b] >= w.klo && w.klast[b] <= w.khi);
  return ok;
}

static void check_tables(const char *what, const jamd_frontend_desc &d, bool accepted) {
  FeTables w;
  std::string err;
  const bool got = fe_build_tables(&d, w, err);
  expect(got == accepted && (got ? tables_sound(d, w) : !err.empty()), std::string("tables: ") + what);
}

static void check_htkconf(const std::string &dir) {
  std::string err;
  // CRLF ends, a comment, a key without a value, a key followed by '=' only, and a comment that passes the 512-byte
  // line buffer (its later pieces read as keys without a value)
  const std::string good = "SOURCERATE = 1250\r\n# a comment = ignored\r\nNUMCHANS\r\nCEPLIFTER =\r\n  \t \r\n#" +
                           std::string(1500, 'x') + "\r\nWINDOWSIZE = 256000.0\r\nTARGETRATE=100000\r\nNUMCHANS = 20\r\n"
                           "USEHAMMING = T\r\nZMEANSOURCE = T\r\nTARGETKIND = MFCC_E_D_A_Z";
  jamd_frontend_desc d = desc();
  bool ok = fe_htkconf(put_text(dir, "good.conf", good).c_str(), &d, err);
  expect(ok && d.smp_period == 1250 && d.smp_freq == 8000 && d.framesize == 204 && d.frameshift == 80 && d.fbank_num == 20 &&
             d.lifter == 22 && d.zmeanframe == 1, "htkconf: CRLF, comment, missing values, over-long line");
  // a line of exactly the buffer's capacity and one byte more, without a newline at the end of the file
  for (int len : {510, 511, 512, 513, 1023}) {
    d = desc();
    ok = fe_htkconf(put_text(dir, "edge.conf", "NUMCHANS = 31\n#" + std::string(len - 1, 'y')).c_str(), &d, err);
    expect(ok && d.fbank_num == 31, "htkconf: last line of " + std::to_string(len) + " bytes");
  }
  d = desc();
  ok = fe_htkconf(put_text(dir, "empty.conf", "").c_str(), &d, err);
  expect(ok && d.smp_period == 625 && d.framesize == 0, "htkconf: empty file (default rate, window in samples)");
  const jamd_frontend_desc before = desc();
  d = before;
  ok = fe_htkconf(put_text(dir, "unknown.conf", "SOURCERATE = 1250\nSAVECOMPRESSED = T\n").c_str(), &d, err);
  expect(!ok && err.find("SAVECOMPRESSED") != std::string::npos && memcmp(&d, &before, sizeof d) == 0, "htkconf: unknown key refused");
  ok = fe_htkconf(put_text(dir, "hamming.conf", "NUMCHANS = 20\nUSEHAMMING = F\n").c_str(), &d, err);
  expect(!ok && err.find("USEHAMMING") != std::string::npos && memcmp(&d, &before, sizeof d) == 0, "htkconf: USEHAMMING = F refused");
  // the piece of an over-long line behind the buffer's end is a line of its own: a key the reference does not take
  ok = fe_htkconf(put_text(dir, "long.conf", "#" + std::string(600, 'z') + " Q = 1\n").c_str(), &d, err);
  expect(!ok && memcmp(&d, &before, sizeof d) == 0, "htkconf: key in the tail of an over-long line refused");
  expect(!fe_htkconf((dir + "/missing.conf").c_str(), &d, err) && !err.empty(), "htkconf: missing file refused");
}

static void check_all_tables() {
  check_tables("default", desc(), true);
  check_tables("framesize 2", desc(2, 1), true);
  check_tables("framesize 3", desc(3, 1), true);
  check_tables("framesize 4096", desc(4096, 1024), true);
  check_tables("framesize 1 refused", desc(1, 1), false);
  check_tables("framesize 4097 refused", desc(4097, 160), false);
  check_tables("frameshift 0 refused", desc(400, 0), false);
  jamd_frontend_desc d = desc();
  d.lopass = 200; d.hipass = 7000;
  check_tables("lopass 200, hipass 7000", d, true);
  d.lopass = 0; d.hipass = 9000;
  check_tables("lopass 0, hipass beyond the band", d, true);
  d.lopass = 7000; d.hipass = 200;
  check_tables("lopass above hipass: no index in the band", d, true);
  d = desc();
  d.vtln_alpha = 1.08f; d.vtln_lower = 250.0f; d.vtln_upper = 6500.0f;
  check_tables("VTLN 1.08", d, true);
  d.vtln_alpha = 0.5f; d.lopass = 100; d.hipass = 7600;
  check_tables("VTLN 0.5 (centre frequencies out of order) with band limits", d, true);
  d.vtln_upper = 9000.0f;
  check_tables("VTLN upper cut-off refused", d, false);
  d.vtln_upper = 6500.0f; d.vtln_lower = 50.0f;
  check_tables("VTLN lower cut-off refused", d, false);
  // the warp lifts an FFT index of the band above the last centre frequency: refused before cf[] is read at its channel
  d = desc(16, 1);
  d.fbank_num = 31; d.hipass = 3590; d.vtln_alpha = 1.2f; d.vtln_lower = 10.0f; d.vtln_upper = 3580.0f;
  check_tables("VTLN 1.2: FFT index above the last channel refused", d, false);
  d = desc();
  fe_set_kind(&d, JAMD_F_FBANK, 1);
  check_tables("fbank_num 1 (FBANK, vector size 1)", d, true);
  d = desc();
  d.fbank_num = 1;
  check_tables("fbank_num 1 (MFCC)", d, true);
  d.fbank_num = 0;
  check_tables("fbank_num 0 refused", d, false);
  // band limits at every few Hz, three windows, with and without VTLN: whatever is accepted is sound
  int accepted = 0, sound = 0;
  for (int fs : {16, 400, 1102})
    for (int hi = 1; hi <= 8200; hi += 97)
      for (int lo : {-1, 0, 63, hi - 1})
        for (float alpha : {1.0f, 0.8f, 1.2f}) {
          d = desc(fs, 1);
          d.fbank_num = 1 + hi % 40; d.lopass = lo; d.hipass = hi;
          d.vtln_alpha = alpha; d.vtln_lower = (float)(lo > 0 ? lo : 0) + 10.0f; d.vtln_upper = (float)hi - 10.0f;
          FeTables w;
          std::string err;
          if (!fe_build_tables(&d, w, err)) continue;
          accepted++;
          sound += tables_sound(d, w);
        }
  expect(accepted > 300 && sound == accepted, "tables: sweep of band limits: " + std::to_string(accepted) + " accepted, all sound");

  // jamd_frontend_table()'s body with buffers sized exactly: the count comes back, min(count, cap) values are written
  d = desc();
  std::string err;
  const int n = fe_table(&d, "hamming", nullptr, 0, err);
  double *ham = (double *)malloc(sizeof(double) * 400);
  short *few = (short *)malloc(sizeof(short) * 3);
  expect(n == 400 && fe_table(&d, "hamming", ham, 400, err) == 400 && ham[0] == 0.54 - 0.46, "table: hamming into 400");
  expect(fe_table(&d, "lochan", few, 3, err) == 257 && few[1] == -1 && few[2] == 0, "table: cap 3 of 257");
  expect(fe_table(&d, "twiddle_re", ham, 400, err) == 511 && ham[0] == 1.0, "table: twiddles, fftN - 1");
  expect(fe_table(&d, "lowt", ham, -5, err) == 257, "table: negative cap writes nothing");
  expect(fe_table(&d, "nothing", ham, 400, err) == -1 && err.find("nothing") != std::string::npos, "table: unknown name refused");
  free(ham); free(few);
}

static void check_counts() {
  std::string err;
  const int64_t off[4] = {0, 5, 5, 3};
  expect(fe_span("f", "utterance", off, 0, err) == 5 && fe_span("f", "utterance", off, 1, err) == 0, "span: in order");
  expect(fe_span("jamd_x", "channel", off, 2, err) == -1 && err == "jamd_x: sample_off is not non-decreasing from 0 at channel 2",
         "span: out of order, the message");
  const int64_t neg[2] = {-1, 4};
  expect(fe_span("f", "utterance", neg, 0, err) == -1, "span: negative start");
  jamd_frontend_desc d = desc();
  expect(fe_frames_raw(d, 399) == 0 && fe_frames_raw(d, 400) == 1 && fe_frames_raw(d, 559) == 1 && fe_frames_raw(d, 560) == 2,
         "frames: buffered");
  // live segments: every kind of window, every sample count, cut in two at every point
  long long cases = 0, bad_rows = 0, bad_sum = 0, bad_mono = 0;
  for (int geo = 0; geo < 2; geo++)
    for (int delta = 0; delta < 2; delta++)
      for (int acc = 0; acc <= delta; acc++)
        for (int splice : {1, 2, 5})
          for (int win : {1, 2, 3}) {
            d = geo ? desc(400, 160) : desc(25, 10);
            d.delta = delta; d.acc = acc; d.splice = splice; d.delWin = win; d.accWin = 4 - win;
            long long prev = 0;
            for (long long n = 0; n <= d.framesize + 6 * d.frameshift; n++) {
              const LvCounts k = lv_counts(d, n);
              const long long want = k.Nf - (splice - 1) > 0 ? k.Nf - (splice - 1) : 0;
              bad_rows += k.To != want || lv_push(d, 0, n, true).rows != k.To;
              bad_mono += k.To < prev || lv_rows_of(d, lv_open_frames(d, k.Tb)) > k.To;
              prev = k.To;
              for (long long a = 0; a <= n; a += geo ? 13 : 1, cases++) {   // (every point in the small geometry)
                const LvPush p1 = lv_push(d, 0, a, false), p2 = lv_push(d, a, n - a, true);
                bad_sum += p1.rows + p2.rows != k.To || p1.rows < 0 || p2.rows < 0 || p1.r_new != p2.r_old ||
                           p1.r_new > d.framesize || p1.Tb_new != p2.Tb_old || p1.F_new != p2.F_old || p2.Tb_new != k.Tb ||
                           p2.F_new != k.Nf || p2.reest != k.reest;
              }
            }
          }
  expect(bad_rows == 0, "live: To == max(0, Nf - (splice - 1)), and one final push delivers it");
  expect(bad_mono == 0, "live: rows never shrink with more samples, an open segment never leads its end");
  expect(bad_sum == 0, "live: " + std::to_string(cases) + " two-push splits deliver the rows of one final push, state handed on");
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
  check_htkconf(argv[1]);
  check_all_tables();
  check_counts();
  return failures ? 1 : 0;
}
