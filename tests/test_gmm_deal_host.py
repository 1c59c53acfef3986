"""The deal of K1's pull form (csrc/gmm_deal.h: which (state range, frame group) a ticket of a share names, how long a
share is, the grid of a pull launch) as a stand-alone program under the host sanitizers.  No GPU."""
import subprocess

from julius_amd import lib


def test_deal_under_sanitizers(tmp_path):
    """tests/gmm_deal_check.cpp (its own main over csrc/gmm_deal.h, which includes no HIP header) built with
    -fsanitize=address,undefined, the runtimes linked statically: 1 .. 41 state ranges x 1 .. 20 frame groups, every tile
    named exactly once over the eight shares, the lengths summing to ranges x groups, the leftover runs within one `per`
    of each other, nothing named behind a share's end; and the grid choice."""
    exe = tmp_path / "gmm_deal_check"
    root = lib._PKG.parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    str(root / "tests" / "gmm_deal_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 2 and "Sanitizer" not in r.stderr
