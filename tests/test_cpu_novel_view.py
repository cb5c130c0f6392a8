"""View interpolation without a GPU: generateNovelView (NovelView.cpp:20-99, 156-172) as s360_generate_novel_views /
s360_interpolate_views, the Python mirror and both modes of host/TestOpticalFlow, on the CPU emulation of the library's own
sources (tools/libs360_emu.so, tools/emu/), against the recorded outputs of the reference's generateNovelView
(tests/golden/novel_view_golden.*, written by tests/golden/make_novel_view_golden.py). Byte equality, every pixel.
The checks themselves are tests/novel_view_checks.py: tests/test_gpu_novel_view.py runs the same ones on the MI355X."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import novel_view_cases as NV
import novel_view_checks as CK

ROOT = CK.ROOT
EMU = os.path.join(ROOT, "tools", "emu")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu_programs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return EMU


@pytest.fixture(scope="module")
def host_program():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "surround360_amd", "csrc"), "-j8", "-s"])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host", "TestOpticalFlow")


def test_header_binding_and_emulated_library_agree_on_the_new_entry_points(emu_programs):
    """include/s360.h declares them, surround360_amd/_capi.py lists them, the emulated library exports them (the product
    library: tests/test_cpu_abi.py goes over the whole list)."""
    import ctypes as C
    import re
    from surround360_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "s360.h")).read()
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for name in ("s360_generate_novel_views", "s360_interpolate_views"):
        assert re.search(r"^int %s\(s360_ctx\* ctx," % name, hdr, re.M), name
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name)
    names = set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert len(names) == len(_capi.SYMBOLS) == 96  # 94 before this operator


@pytest.mark.parametrize("check", list(CK.CHECKS))
def test_emulated_library_gives_the_reference_views(emu_programs, check):
    """Cases (a) and (b) through both entry points and the Python mirror; n = 1 against the slices of n = 4; null side outputs;
    interpolate_views' flows against compute_optical_flow's; the error paths."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "novel_view_checks.py"), check], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])))
    assert r.returncode == 0 and ("ok " + check) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_edge_case_populates_every_branch_of_the_blend():
    """What the generator asserted on the REFERENCE's fromL / fromR alphas when it recorded case (b): each of the four alpha
    cases of combineNovelViews (neither / only L / only R / both visible) holds at least 5 % of the pixels of a recorded view."""
    br = json.load(open(NV.GOLDEN_JSON))["branches"]["edge"]
    best = np.max(np.array(list(br.values())), axis=0)
    assert (best >= 0.05).all(), best


def test_generator_reproduces_the_committed_golden(tmp_path):
    if not os.path.isdir("/root/reference/surround360_render/source/optical_flow"):
        pytest.skip("needs the reference's sources to compile generateNovelView from")
    prefix = str(tmp_path / "regen")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "golden", "make_novel_view_golden.py"), prefix], timeout=1800)
    assert json.load(open(prefix + ".json")) == json.load(open(NV.GOLDEN_JSON))
    new, old = np.load(prefix + ".npz"), np.load(NV.GOLDEN_NPZ)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k
    assert os.path.getsize(NV.GOLDEN_NPZ) < (1 << 20)


def test_emulated_program_test_mode_writes_the_reference_views(tmp_path, emu_programs):
    CK.check_program_test_mode(os.path.join(emu_programs, "TestOpticalFlow"), str(tmp_path))


def test_emulated_program_middlebury_experiment_prints_the_reference_lines(tmp_path, emu_programs):
    CK.check_program_middlebury(os.path.join(emu_programs, "TestOpticalFlow"), str(tmp_path))


def test_rmse_addressing_is_the_reference_one():
    """imageDiffRMSE walks four-channel rows as three-byte elements: the recorded RMSE is that of the first 3w bytes of each row
    (alphas included, the last quarter of the columns not), and differs from the RMSE over B, G, R of every pixel."""
    a = np.zeros((4, 8, 4), np.uint8)
    b = a.copy()
    b[:, 6:, :3] = 200   # columns the reference never reads
    b[:, 0, 3] = 10      # an alpha it does read
    assert NV.image_diff_rmse(a, b) == float(np.sqrt(4 * 100.0 / (3 * 4 * 8)))


def test_program_argument_handling(tmp_path, host_program):
    """The real host/TestOpticalFlow (no GPU needed before the first image is read): the modes, the refusal of one view,
    requireArg order of the experiment mode (TestOpticalFlow.cpp:166-167)."""
    exe = host_program
    r = subprocess.run([exe, "--mode", "video"], capture_output=True, text=True)
    assert r.returncode != 0 and "Terminated with exception: unrecongized mode: video" in r.stderr
    common = ["--test_dir", str(tmp_path), "--left_img", "l.png", "--right_img", "r.png", "--flow_alg", "pixflow_low"]
    r = subprocess.run([exe, "--mode", "test", "--num_intermediate_views", "1"] + common, capture_output=True, text=True)
    assert r.returncode != 0 and "num_intermediate_views = 1" in r.stderr and "failed to load image" not in r.stderr
    r = subprocess.run([exe, "--mode", "test", "--num_intermediate_views=3", "--save_asymmetric_novel_views"] + common,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "failed to load image" in r.stderr  # flags accepted; the images do not exist
    r = subprocess.run([exe, "--mode", "middlebury_interpolation_experiment"], capture_output=True, text=True)
    assert r.returncode != 0 and "missing required command line argument: test_dir" in r.stderr
    r = subprocess.run([exe, "--mode", "middlebury_interpolation_experiment", "--test_dir", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "missing required command line argument: flow_alg" in r.stderr
    r = subprocess.run([exe, "--mode", "middlebury_interpolation_experiment", "--flow_alg", "pixflow_low"], capture_output=True, text=True)
    assert r.returncode != 0 and "missing required command line argument: test_dir" in r.stderr
    # a dataset without its files: the reference's imread failure
    open(str(tmp_path / "lonely_10.png"), "w").write("")
    r = subprocess.run([exe, "--mode", "middlebury_interpolation_experiment", "--test_dir", str(tmp_path), "--flow_alg", "pixflow_low",
                        "--show_interpolated_view"], capture_output=True, text=True)
    assert r.returncode != 0 and "Terminated with exception" in r.stderr


def test_morph_kernel_keeps_nothing_in_scratch(tmp_path):
    """k_morph_views for gfx950 with the product's flags: private_segment_fixed_size 0 (the loop over a block's views must not turn
    the tap registers into scratch), read from the code object's metadata as tests/test_cpu_isa.py does for the sweeps."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_loops
    out = str(tmp_path / "render_kernels.s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-S",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "surround360_amd", "csrc", "render_kernels.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = {k: v for k, v in isa_loops.kernel_meta(open(out).read()).items() if "k_morph_views" in k}
    assert len(meta) == 1, sorted(meta)
    (name, m), = meta.items()
    assert m["private_segment_fixed_size"] == 0 and m["scratch"] == 0, (name, m)
    assert m["next_free_vgpr"] <= 128, (name, m)  # four waves per SIMD or more
