"""tests/test_gpu_composite_poles.py without a GPU: the same cases on tools/libs360_emu.so, the library's sources compiled for the
CPU with the kernels run wave by wave (see tests/test_cpu_library_emulation.py), in a process whose Python binding points at the
emulated library (tests/conftest.py: S360_TEST_EMULATED_LIB=1). Eyes of 504x252: minutes of host time otherwise."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so"])
    return os.path.join(ROOT, "tools", "libs360_emu.so")


def test_composite_cases_on_the_emulated_library(emu_lib):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1", S360_COMPOSITE_CASES_EQR="504x252")
    e.pop("S360_COMPOSITE_FUSED", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_composite_poles.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "7 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
