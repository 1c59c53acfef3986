"""Writes the fixtures of the voice-activity detector (-fvad) from the reference: tests/golden/fvad_model.txt through
julius_amd/shim/jamd_fvad_export, and per stream of fvadref.STREAMS one tests/golden/<name>.npz with the int16 stream
itself (a normal generator is not promised to give the same numbers on every install) and, per mode 0 ... 3, libfvad's
raw value for every whole frame and the core's final state.  tests/test_fvad_ref.py proves the committed files equal a
fresh recording.

    python tests/make_golden_fvad.py
"""
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import fvadref as F   # noqa: E402


def export_model(tmp: Path, out: Path):
    subprocess.run(["make", "-s", "-C", str(F.ROOT / "julius_amd" / "shim"), f"JULIUS_SRC={F.REFERENCE}", f"BINDIR={tmp}",
                    "fvad_export"], check=True)
    subprocess.run([str(tmp / "jamd_fvad_export"), str(out)], check=True)


def main():
    with tempfile.TemporaryDirectory() as t:
        tmp = Path(t)
        export_model(tmp, F.MODEL)
        lib = F.build(tmp)
        for name in F.STREAMS:
            np.savez_compressed(F.GOLDEN / f"{name}.npz", **F.record(lib, name))
            print(name, (F.GOLDEN / f"{name}.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
