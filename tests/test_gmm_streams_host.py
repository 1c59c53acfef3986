"""CPU: the host layer of jamd_gmm_ms -- what jamd_gmm_ms_create() refuses and what the binary HMM reader takes --
without a device.  Every refusal comes before the first device call, so a placeholder engine handle is enough
(as tests/test_cabi.py does for the lexicon); a description that passes every check fails only where the device is
selected (JAMD_ENODEV), or, on a machine that has one, is created."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import streamsref  # noqa: E402
from julius_amd import lib  # noqa: E402

EINVAL, ENODEV = -1, -2


def _fake_engine():
    return C.create_string_buffer(256)


def _create(model):
    L = lib.load()
    d, keep = lib.GmmStreams.make_desc(model)
    eng, h = _fake_engine(), C.c_void_p()
    rc = L.jamd_gmm_ms_create(C.cast(eng, C.c_void_p), C.byref(d), C.byref(h))
    msg = L.jamd_last_error().decode()
    if h.value:
        L.jamd_gmm_ms_destroy(h)
    return rc, msg


@pytest.mark.parametrize("name", list(streamsref.REFUSALS))
def test_create_refuses_before_any_device_call(name):
    import re
    change, pattern = streamsref.REFUSALS[name]
    rc, msg = _create(change(streamsref.refusal_model()))
    assert rc == EINVAL
    assert msg.startswith("jamd_gmm_ms_create: ") and re.search(pattern, msg), msg


@pytest.mark.parametrize("name", ["lay_26_13", "branches", "one_stream"])
def test_good_description_passes_every_check(name):
    rc, msg = _create(streamsref.load_case(name)[0])
    assert rc in (0, ENODEV), msg


def _load(path):
    L = lib.load()
    eng, h = _fake_engine(), C.c_void_p()
    rc = L.jamd_gmm_ms_load_binhmm(C.cast(eng, C.c_void_p), str(path).encode(), C.byref(h))
    msg = L.jamd_last_error().decode()
    if h.value:
        L.jamd_gmm_ms_destroy(h)
    return rc, msg


@pytest.mark.parametrize("name", streamsref.BINHMM_CASES)
def test_reader_takes_multi_stream_binhmm_and_refuses_damaged_ones(tmp_path, name):
    """The committed mkbinhmm files parse and pass jamd_gmm_ms_create()'s checks; cut short anywhere before the HMM
    section (which the reader does not need) or damaged in the header they are refused, never read past."""
    path = streamsref.load_binhmm(name, tmp_path / "binhmm")
    rc, msg = _load(path)
    assert rc in (0, ENODEV), msg
    raw = path.read_bytes()
    for k in range(1, 7):
        (tmp_path / "cut").write_bytes(raw[:len(raw) * k // 8])
        rc, msg = _load(tmp_path / "cut")
        assert rc == EINVAL, (k, msg)
    (tmp_path / "junk").write_bytes(b"JBINHMMV2\0_Q\0" + b"\0" * 64)
    assert _load(tmp_path / "junk")[0] == EINVAL
    (tmp_path / "noise").write_bytes(np.random.default_rng(0).integers(0, 256, 4096, dtype=np.uint8).tobytes())
    assert _load(tmp_path / "noise")[0] == EINVAL
    # the stream count of rd_opt(): the short after the header strings
    at = raw.index(b"\0", len(b"JBINHMMV2\0")) + 1 if raw.startswith(b"JBINHMMV2\0") else len(b"JBINHMM\n\0")
    for bad in (0, 51, -3):
        (tmp_path / "streams").write_bytes(raw[:at] + int(bad).to_bytes(2, "big", signed=True) + raw[at + 2:])
        rc, msg = _load(tmp_path / "streams")
        assert rc == EINVAL and "streams" in msg, msg
    assert _load(tmp_path / "absent")[0] == EINVAL


def test_single_stream_entries_keep_refusing_multi_stream_files(tmp_path):
    """jamd_binhmm_to_blob() shares the reader with the new entry and still refuses nstream != 1 with its text."""
    path = streamsref.load_binhmm("branches", tmp_path / "binhmm")
    L = lib.load()
    assert L.jamd_binhmm_to_blob(str(path).encode(), str(tmp_path / "x.am").encode()) == EINVAL
    assert "3 streams (the device path serves single-stream models)" in L.jamd_last_error().decode()
    one = streamsref.load_binhmm("one_stream", tmp_path / "one.binhmm")
    assert L.jamd_binhmm_to_blob(str(one).encode(), str(tmp_path / "one.am").encode()) == 0, L.jamd_last_error()
