"""tests/test_gpu_sharpen_shapes.py without a GPU: the same shape table and the same batched frame case on
tools/libs360_emu.so, the library's sources compiled for the CPU with the kernels run wave by wave (see
tests/test_cpu_library_emulation.py). Each runs in a process whose Python binding points at the emulated library
(tests/conftest.py: S360_TEST_EMULATED_LIB=1). The frame is the quarter-size rig of tests/test_cpu_known_result.py: minutes of
host time otherwise."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so"])
    return os.path.join(ROOT, "tools", "libs360_emu.so")


def test_shape_table_on_the_emulated_library(emu_lib):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_sharpen_shapes.py"), "-q", "-m", "gpu",
                        "-k", "test_sharpen_shape", "-p", "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "30 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


_CHILD = r"""
import os, sys, pathlib
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "oracle")]
from surround360_amd import _capi
_capi.LIB_PATH = sys.argv[2]
import oracle_lib
import sharpen_shapes_cases as S
oracle_lib.lib()
S.CAM = 256
path = S.make_rig(os.path.join(root, "tests", "golden", "rig_17cam.json"), pathlib.Path(sys.argv[3]))
flags = dict(S.frame_flags(), eqr_width=504, eqr_height=252, final_eqr_width=481, final_eqr_height=504)
S.check_batch(path, 3, oracle_lib, cam=256, flags=flags)
print("BATCH_OK")
"""


def test_batch_sharpened_width_only_resize_on_the_emulated_library(emu_lib, tmp_path):
    """Three slots, sharpening 0.25, 504x252 eyes resized to 481x252 each (an odd width: the B,G,R rows end ragged and the
    reference's vector path ends inside a pixel): slot by slot the frame rendered alone, slot 0 the oracle's frame."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, emu_lib, str(tmp_path)], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0 and "BATCH_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
