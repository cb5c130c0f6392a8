"""host/TestRenderStereoPanorama with --enable_pole_removal on the fast input paths (include/s360_pole_inputs.h): --bin_list, which
refused pole removal before; --device_input_png and --device_input_jpeg, whose secondary bottom camera stayed on the host decoder;
and a secondary file the device decoder does not take. The masks are read once per run and handed to the contexts
(s360_set_pole_masks) in every mode, so the existing pole-removal digests of tests/test_gpu_zz_refprogram.py cover that path too.
The check functions are tests/pole_inputs_cases.py's: tests/test_cpu_pole_inputs.py runs them on the programs linked against the
emulated library."""
import os
import subprocess

import pytest

import pole_inputs_cases as PC
import rigutil  # noqa: F401  (tests/ on the path)
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

ROOT = PC.ROOT


@pytest.fixture(scope="module")
def programs(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host", "Unpacker"), os.path.join(ROOT, "host", "TestRenderStereoPanorama")


@pytest.fixture(scope="module")
def device_encoder(s360lib, tmp_path_factory):
    """B,G,R image -> the banded PNG file the device encoder writes (8 bits, as the case's files hold)."""
    c = R.Context(R.RigDescription(PC.small_rig(tmp_path_factory.mktemp("rig_pole_host"))), R.make_params(**PC.FLAGS))
    yield lambda a: bytes(c.encode_png(a))
    c.close()


def test_bin_list_with_pole_removal(tmp_path, programs):
    PC.check_bin_list_pole_removal(programs[0], programs[1], tmp_path)


def test_device_input_png_takes_the_secondary_camera(tmp_path, programs, device_encoder):
    PC.check_device_input_png(programs[1], tmp_path, device_encoder)


def test_device_input_jpeg_takes_the_secondary_camera(tmp_path, programs):
    PC.check_device_input_jpeg(programs[1], tmp_path)


def test_secondary_file_of_another_writer_takes_the_host_path(tmp_path, programs, device_encoder):
    PC.check_secondary_on_the_host_path(programs[1], tmp_path, device_encoder)
