"""A finished frame's equirect and cubemap as JPEG files encoded on the device (include/s360_frame_jpeg.h, the finish stage of
surround360_amd/csrc/render.hip, api_frame_jpeg.hip): byte equality against jpegio::encode and PIL of the pixels the library
downloads for the same frame. The cases and their reasons: tests/frame_jpeg_cases.py. The file also runs on the CPU emulation of
the library (S360_TEST_EMULATED_LIB=1, tests/test_cpu_frame_jpeg.py), except the 8K case."""
import pytest

import frame_jpeg_cases as FJ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(tmp_path_factory, rig_json, s360lib):
    return FJ.small_rig(tmp_path_factory.mktemp("rig_frame_jpeg"), rig_json)


@pytest.mark.parametrize("shape", list(FJ.SHAPES))
def test_small_frames(env, shape):
    FJ.check_small_frames(env, shape)


def test_png_and_jpeg_both_on(env):
    FJ.check_png_and_jpeg(env)


def test_two_slots_three_frames_each(env):
    FJ.check_slots_and_ages(env)


def test_refusals(env):
    FJ.check_refusals(env)


def test_capacity_through_the_tap(env):
    FJ.check_capacity(env)


def test_many_scan_groups_and_stream_tiles_through_the_tap(env):
    FJ.check_large_index(env)


@pytest.mark.fullsize
def test_8k_once(env):
    FJ.check_8k(env)
