"""The deal of K1's pull form with a fine-grained tail (csrc/gmm_deal.h: gd_tail_make, gd_tail_len, gd_tail_ticket --
the last Q tiles of every share handed out in pieces of a few states) as a stand-alone program under the host
sanitizers.  No GPU."""
import subprocess

from julius_amd import lib


def test_tail_deal_under_sanitizers(tmp_path):
    """tests/gmm_deal_tail_check.cpp (its own main over csrc/gmm_deal.h, which includes no HIP header) built with
    -fsanitize=address,undefined, the runtimes linked statically: 1 .. 41 state ranges x 1 .. 20 frame groups x
    Q in {0, 1, 3, len, len + 5} x pieces of 2, 4, 8 states, S a multiple of 16 and not: every (state, group) covered
    exactly once over the eight shares, nothing named behind a share's end, the lengths as specified, Q = 0 identical
    to gd_ticket / gd_len; and the tail's parameters."""
    exe = tmp_path / "gmm_deal_tail_check"
    root = lib._PKG.parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    str(root / "tests" / "gmm_deal_tail_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 2 and "Sanitizer" not in r.stderr
