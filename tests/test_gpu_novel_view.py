"""View interpolation on the MI355X: k_morph_views through s360_generate_novel_views / s360_interpolate_views (libs360.so), the
Python mirror and both modes of host/TestOpticalFlow against the recorded outputs of the reference's generateNovelView
(tests/golden/novel_view_golden.*). The checks are tests/novel_view_checks.py — the ones tests/test_cpu_novel_view.py runs on the
CPU emulation — plus the 2048 x 2048 pair of BASELINE configs[1] against recorded digests. Byte equality, every pixel."""
import json
import os
import subprocess

import numpy as np
import pytest

import novel_view_cases as NV
import novel_view_checks as CK

pytestmark = pytest.mark.gpu

HOST_DIR = os.path.join(CK.ROOT, "host")


@pytest.fixture(scope="module")
def ctx(gpu_rig):
    from surround360_amd import render as R
    return R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))


@pytest.fixture(scope="module")
def program(s360lib):
    subprocess.check_call(["make", "-C", HOST_DIR, "-s"])
    return os.path.join(HOST_DIR, "TestOpticalFlow")


@pytest.mark.parametrize("check", list(CK.CHECKS))
def test_device_gives_the_reference_views(ctx, s360lib, check):
    """Cases (a) synth pair with its real flows and (b) edge content, through both entry points and the Python mirror; n = 1
    against the slices of n = 4; null side outputs; interpolate_views' flows against compute_optical_flow's; error paths."""
    CK.CHECKS[check](ctx, s360lib)


def test_both_mappings_of_shifts_to_the_grid_give_the_same_bytes(gpu_rig):
    """shifts as grid.z slices and as a loop in the workgroup (S360_MORPH_VPB, what tools/morph_time.py compares) and a mixed
    grouping with a ragged last group, each in a process of its own: the same digests"""
    import sys
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import novel_view_cases as NV, novel_view_checks as CK\n"
            "m, l, r = CK.make_ctx().generate_novel_views(*NV.edge_case(), NV.ALL_SHIFTS, want_sides=True)\n"
            "print(NV.sha(m), NV.sha(l), NV.sha(r))\n") % (CK.ROOT, os.path.join(CK.ROOT, "tests"))
    outs = []
    for vpb in (None, "1", "4", "11"):
        env = dict(os.environ)
        env.pop("S360_MORPH_VPB", None)
        if vpb:
            env["S360_MORPH_VPB"] = vpb
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert len(set(outs)) == 1, outs


def test_program_test_mode(program, tmp_path):
    CK.check_program_test_mode(program, str(tmp_path))


def test_program_middlebury_experiment(program, tmp_path):
    CK.check_program_middlebury(program, str(tmp_path))


@pytest.mark.fullsize
def test_fullsize_pair_against_recorded_digests(ctx):
    """BASELINE configs[1]'s pair (2048 x 2048): flows computed on the device by interpolate_views, the merged views for shifts
    0.25 and 0.5 and both warped images for 0.5 against the digests of the reference's."""
    from surround360_amd import synth
    fs = NV.FULLSIZE
    meta = json.load(open(NV.GOLDEN_JSON))
    il, ir = synth.flow_pair(fs["w"], fs["h"], fs["seed"])
    want_in = meta["inputs"]["fullsize"]
    assert [NV.sha(il), NV.sha(ir)] == want_in[:2], "synth.flow_pair no longer produces the pair the digests were recorded from"
    shifts = sorted(set(fs["merged"]) | set(fs["sides"]))
    merged, from_l, from_r, f_lr, f_rl = ctx.interpolate_views(il, ir, shifts, want_sides=True, want_flows=True)
    assert [NV.sha(f_lr), NV.sha(f_rl)] == want_in[2:], "the device's flows of the pair differ from the reference's"
    for k, t in enumerate(shifts):
        if t in fs["merged"]:
            assert NV.sha(merged[k]) == meta["digests"][NV.key("fullsize", "merged", t)], ("merged", t)
        if t in fs["sides"]:
            assert NV.sha(from_l[k]) == meta["digests"][NV.key("fullsize", "fromL", t)], ("fromL", t)
            assert NV.sha(from_r[k]) == meta["digests"][NV.key("fullsize", "fromR", t)], ("fromR", t)
