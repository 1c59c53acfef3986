"""What the silence cutting stage works out without a device (csrc/adin_cut_plan.h through the C ABI): the defaults, the
parameters of adin_setup_param() against a Python restatement (np.float32 where the reference computes in float) for
the defaults and a sweep of seeded descriptors, the refusals, and the two bounds of a push against what the reference
helper (adincutref.RefCut) delivers over seeded streams and cuts.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import adincutref as K
from julius_amd import lib

SMALL = dict(head_margin_msec=30, tail_margin_msec=40, chunk_size=100)


def _params(d):
    v = [C.c_int(-1) for _ in range(4)]
    rc = lib.load().jamd_adin_cut_params(C.byref(d), *[C.addressof(x) for x in v])
    return rc, tuple(x.value for x in v)


def _fields(d):
    return {f[0]: getattr(d, f[0]) for f in lib.AdinCutDesc._fields_}


def test_defaults_and_their_parameters():
    d = lib.AdinCutDesc()
    assert lib.load().jamd_adin_cut_default(C.byref(d)) == 0
    assert _fields(d) == dict(sfreq=16000, level_thres=2000, zero_cross_num=60, head_margin_msec=300,
                              tail_margin_msec=400, chunk_size=1000)
    assert _params(d) == (0, (4800, 18, 8, 7840))
    assert K.params() == (4800, 18, 8, 7840)
    assert 7840 - 4800 == 3040                               # the first rest_tail
    assert _params(lib.AdinCut.desc_for(**SMALL)) == (0, (480, 1, 8, 784))
    assert lib.load().jamd_abi_version() == 4                # symbols were added, nothing else


def test_params_sweep_of_seeded_descriptors():
    rng = np.random.default_rng(7)
    accepted = refused = 0
    for _ in range(200):
        f = dict(sfreq=int(rng.choice([8000, 11025, 16000, 22050, 44100, 48000])), level_thres=int(rng.integers(0, 9000)),
                 zero_cross_num=int(rng.integers(0, 300)), head_margin_msec=int(rng.integers(0, 900)),
                 tail_margin_msec=int(rng.integers(0, 1200)), chunk_size=int(rng.integers(1, 4000)))
        rc, got = _params(lib.AdinCut.desc_for(**f))
        want = K.params(**f)
        bad = f["chunk_size"] > want[0] or K.overflows(want[0], want[2], want[3], f["chunk_size"])
        assert (rc != 0) == bad, (f, want, rc)
        if bad:
            refused += 1
            assert rc == -1
        else:
            accepted += 1
            assert got == want, f
    assert accepted >= 50 and refused >= 20                  # the sweep reaches both sides


def test_refusals():
    L = lib.load()
    for f, word in ((dict(sfreq=0), b"sfreq"), (dict(sfreq=-16000), b"sfreq"), (dict(chunk_size=0), b"chunk_size"),
                    (dict(chunk_size=4801), b"header margin"), (dict(head_margin_msec=30, tail_margin_msec=40,
                                                                      chunk_size=480), b"swap buffer")):
        d = lib.AdinCut.desc_for(**f)
        assert _params(d)[0] == -1 and word in L.jamd_last_error(), f
        assert L.jamd_adin_cut_push_cap(C.byref(d), 100) == -1 and L.jamd_adin_cut_parts_cap(C.byref(d), 100) == -1
    assert _params(lib.AdinCut.desc_for(chunk_size=4800, tail_margin_msec=1000))[0] == 0   # chunk_size == c_length is allowed
    assert _params(lib.AdinCut.desc_for())[0] == 0
    d = lib.AdinCut.desc_for()
    assert L.jamd_adin_cut_push_cap(C.byref(d), -1) == -1 and L.jamd_adin_cut_parts_cap(C.byref(d), -1) == -1
    assert L.jamd_adin_cut_params(None, None, None, None, None) == -1


def _caps(d, n):
    return lib.load().jamd_adin_cut_push_cap(C.byref(d), n), lib.load().jamd_adin_cut_parts_cap(C.byref(d), n)


def test_cap_formulas():
    d = lib.AdinCut.desc_for()
    for n in (0, 1, 999, 1000, 4000, 8001, 9001, 9002, 227000):
        blocks = (n + 999) // 1000 + 1
        events = 1 + (blocks - 1) // 9
        assert _caps(d, n) == (n + 999 + 7840 + events * 4800, events + 1), n
    assert _caps(d, 4000)[0] == 4000 + 999 + 4800 + 7840      # one trigger: chunk + (chunk_size - 1) + c_length + sbsize


@pytest.mark.parametrize("desc", [SMALL, dict(SMALL, zero_cross_num=200, tail_margin_msec=20),
                                  dict(head_margin_msec=60, tail_margin_msec=10, chunk_size=50, zero_cross_num=190)])
def test_caps_bound_what_the_reference_delivers(ref, desc):
    d = lib.AdinCut.desc_for(**desc)
    rng = np.random.default_rng(11)
    most = 0.0
    for seed in range(1, 7):
        w = K.bursts(seed, 0.1)
        for top in (1, 150, 700, 3000, len(w)):
            r = K.RefCut(ref, 1, **desc)
            at = 0
            while at < len(w):
                n = min(int(rng.integers(0, top)) + 1, len(w) - at)
                parts = r.push([w[at:at + n]], [at + n == len(w)])[0]
                at += n
                samples, nparts = sum(len(p.data()) for p in parts), len(parts)
                cs, cp = _caps(d, n)
                assert samples <= cs and nparts <= cp, (seed, top, at, n, samples, cs, nparts, cp)
                most = max(most, nparts / cp)
            r.close()
    assert most == 1.0 or desc is not SMALL                  # the part bound is attained (with the first set)


def test_push_cap_is_nearly_attained_by_a_trigger_with_full_cycle_buffer_and_carry(ref):
    """Silence until the cycle buffer is full, then 99 samples of a loud square wave that wait for their block; the next
    push completes that block, which triggers and brings the whole head margin with it."""
    d = lib.AdinCut.desc_for(**SMALL)
    r = K.RefCut(ref, 1, **SMALL)
    loud = (6000 * (1 - 2 * ((np.arange(800) // 4) % 2))).astype(np.int16)
    assert r.push([np.concatenate([np.zeros(900, np.int16), loud[:99]])])[0] == []
    parts = r.push([loud[99:]])[0]
    got = sum(len(p.data()) for p in parts)
    assert r.events["trigger_head"] == 1 and len(parts) == 1
    assert got == 701 + 99 + 480 - 100                       # the push, the carry, c_length less the triggering block
    cap = _caps(d, 701)[0]
    assert cap == 701 + 99 + 480 + 784 and got == cap - 784 - 100   # short of the bound by the (empty) swap buffer and a block
    r.close()


def test_second_trigger_delivers_the_tail_again(ref):
    """Why the sample bound counts c_length once per trigger: with -zc 200 the tail margin is delivered almost whole, so
    the head margin of a segment that follows at once repeats it, and a push holds more than its own samples plus one
    c_length + sbsize would allow for."""
    desc = dict(SMALL, zero_cross_num=200, tail_margin_msec=20, chunk_size=20)
    c_length, nz, nc_max, sbsize = K.params(**desc)
    loud = (6000 * (1 - 2 * ((np.arange(200) // 2) % 2))).astype(np.int16)
    quiet = np.zeros(c_length + nc_max * 20, np.int16)
    w = np.concatenate([np.zeros(500, np.int16)] + [loud, quiet] * 12)
    r = K.RefCut(ref, 1, **desc)
    parts = r.push([w])[0]
    got = sum(len(p.data()) for p in parts)
    cs, cp = _caps(lib.AdinCut.desc_for(**desc), len(w))
    print(len(w), got, len(parts), cs, cp)
    assert r.events["end_silence"] == 12
    assert len(w) + 19 + c_length + sbsize < got <= cs and len(parts) <= cp
    r.close()


def test_plan_under_sanitizers(tmp_path):
    """tests/adin_cut_plan_check.cpp (its own main over csrc/adin_cut_plan.h, which includes no HIP header) built with
    -fsanitize=address,undefined, the runtimes linked statically: descriptors at and beyond every limit, and for a sweep
    of accepted ones the swap buffer, the history and the bounds the kernels rely on: every case as expected, no report."""
    exe = tmp_path / "adin_cut_plan_check"
    root = lib._PKG.parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", str(lib._PKG / "csrc"),
                    "-I", str(root / "include"), str(root / "tests" / "adin_cut_plan_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 3 and "Sanitizer" not in r.stderr
