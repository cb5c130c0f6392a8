"""The byte comparisons of the view-interpolation operator against the recorded outputs of the reference's generateNovelView
(tests/golden/novel_view_golden.*), written once and run twice: on the MI355X through libs360.so (tests/test_gpu_novel_view.py,
in process) and on the CPU emulation of the same sources, tools/libs360_emu.so (tests/test_cpu_novel_view.py starts
`python novel_view_checks.py <check>` per check: the emulated library gets a process of its own). Byte equality, every pixel."""
import ctypes as C
import json
import os
import sys

import numpy as np

import novel_view_cases as NV
import oracle_lib as O

ROOT = os.path.dirname(NV.HERE)
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = (dict(np.load(NV.GOLDEN_NPZ)), json.load(open(NV.GOLDEN_JSON)))
    return _golden


def make_ctx():
    from surround360_amd import render as R
    rig = R.RigDescription(os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
    return R.Context(rig, R.make_params(eqr_width=1008, eqr_height=504))


def same_as_golden(case, what, shift, got):
    """digest for every recorded view; where the image itself is recorded a mismatch names the pixel"""
    arrays, meta = golden()
    k = NV.key(case, what, shift)
    if k in arrays and not np.array_equal(got, arrays[k]):
        bad = np.argwhere(got != arrays[k])
        y, x, c = bad[0]
        raise AssertionError("%s: %d of %d bytes differ from the reference's, first at (y %d, x %d, channel %d): %d vs %d" % (
            k, len(bad), got.size, y, x, c, got[y, x, c], arrays[k][y, x, c]))
    assert NV.sha(got) == meta["digests"][k], "%s: digest differs from the reference's" % k


def inputs(case):
    if case == "edge":
        ins = NV.edge_case()
    else:
        il, ir = NV.synth_pair()
        ins = (il, ir) + tuple(NV.prepare_flows(O.compute_optical_flow, il, ir))
    want = golden()[1]["inputs"][case]
    assert [NV.sha(a) for a in ins] == want, "the inputs of case %r are not the ones the golden was recorded from" % case
    return ins


def check_generate(ctx, case):
    """s360_generate_novel_views through the Python mirror: all eleven shifts in one launch, merged + both warped images"""
    ins = inputs(case)
    merged, from_l, from_r = ctx.generate_novel_views(*ins, NV.ALL_SHIFTS, want_sides=True)
    for k, t in enumerate(NV.ALL_SHIFTS):
        same_as_golden(case, "merged", t, merged[k])
        same_as_golden(case, "fromL", t, from_l[k])
        same_as_golden(case, "fromR", t, from_r[k])
    # the four shifts the issue names, as literals
    m4 = ctx.generate_novel_views(*ins, NV.SHIFTS4)
    for k, t in enumerate(NV.SHIFTS4):
        same_as_golden(case, "merged", t, m4[k])
    return merged, m4


def check_slices(ctx, case):
    """n = 1 equals the corresponding slice of n = 4; leaving out fromL / fromR changes nothing in merged"""
    ins = inputs(case)
    m4, l4, r4 = ctx.generate_novel_views(*ins, NV.SHIFTS4, want_sides=True)
    assert np.array_equal(ctx.generate_novel_views(*ins, NV.SHIFTS4), m4)
    for k, t in enumerate(NV.SHIFTS4):
        m1, l1, r1 = ctx.generate_novel_views(*ins, [t], want_sides=True)
        assert np.array_equal(m1[0], m4[k]) and np.array_equal(l1[0], l4[k]) and np.array_equal(r1[0], r4[k]), t
        assert np.array_equal(ctx.generate_novel_views(*ins, t)[0], m4[k]), t


def check_c_abi(ctx, lib):
    """both entry points called as C would: one null side output, the other not"""
    il, ir, f_lr, f_rl = inputs("edge")
    h, w = il.shape[:2]
    sh = np.array(NV.SHIFTS4, np.float64)
    merged = np.zeros((4, h, w, 4), np.uint8)
    from_r = np.zeros_like(merged)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.s360_generate_novel_views(ctx.h, p(il), p(ir), p(f_lr), p(f_rl), w, h, p(sh), 4, p(merged), None, p(from_r))
    assert rc == 0
    for k, t in enumerate(NV.SHIFTS4):
        same_as_golden("edge", "merged", t, merged[k])
        same_as_golden("edge", "fromR", t, from_r[k])
    il, ir = NV.synth_pair()
    merged[:] = 0
    from_l = np.zeros_like(merged)
    rc = lib.s360_interpolate_views(ctx.h, b"pixflow_low", p(il), p(ir), w, h, p(sh), 4, p(merged), p(from_l), None, None, None)
    assert rc == 0
    for k, t in enumerate(NV.SHIFTS4):
        same_as_golden("synth", "merged", t, merged[k])
        same_as_golden("synth", "fromL", t, from_l[k])


def check_interpolate(ctx):
    """s360_interpolate_views: prepare + views; its flows are s360_compute_optical_flow's bit for bit"""
    il, ir = NV.synth_pair()
    merged, from_l, from_r, f_lr, f_rl = ctx.interpolate_views(il, ir, NV.ALL_SHIFTS, want_sides=True, want_flows=True)
    for k, t in enumerate(NV.ALL_SHIFTS):
        same_as_golden("synth", "merged", t, merged[k])
        same_as_golden("synth", "fromL", t, from_l[k])
        same_as_golden("synth", "fromR", t, from_r[k])
    w_lr, w_rl = NV.prepare_flows(ctx.compute_optical_flow, il, ir)
    assert np.array_equal(f_lr.view(np.uint32), w_lr.view(np.uint32)) and np.array_equal(f_rl.view(np.uint32), w_rl.view(np.uint32))
    assert np.array_equal(ctx.interpolate_views(il, ir, 0.5)[0], merged[NV.ALL_SHIFTS.index(0.5)])
    # edge content through the flow as well: whatever the flows are, the views must be generate_novel_views' of them
    el, er = NV.edge_case()[:2]
    m, fl, fr, e_lr, e_rl = ctx.interpolate_views(el, er, NV.SHIFTS4, want_sides=True, want_flows=True)
    m2, fl2, fr2 = ctx.generate_novel_views(el, er, e_lr, e_rl, NV.SHIFTS4, want_sides=True)
    assert np.array_equal(m, m2) and np.array_equal(fl, fl2) and np.array_equal(fr, fr2)


def check_errors(ctx, lib):
    """null images, n = 0, non-positive size, unknown algorithm: the existing codes, a message in s360_last_error"""
    from surround360_amd import _capi
    il, ir, f_lr, f_rl = NV.edge_case()
    h, w = il.shape[:2]
    sh = np.array([0.5], np.float64)
    out = np.zeros((1, h, w, 4), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    gen, itp = lib.s360_generate_novel_views, lib.s360_interpolate_views

    def msg():
        return lib.s360_last_error(ctx.h).decode()

    assert gen(ctx.h, None, p(ir), p(f_lr), p(f_rl), w, h, p(sh), 1, p(out), None, None) == _capi.ERR_INVALID_ARG and "null" in msg()
    assert gen(ctx.h, p(il), None, p(f_lr), p(f_rl), w, h, p(sh), 1, p(out), None, None) == _capi.ERR_INVALID_ARG
    assert gen(ctx.h, p(il), p(ir), None, p(f_rl), w, h, p(sh), 1, p(out), None, None) == _capi.ERR_INVALID_ARG
    assert gen(ctx.h, p(il), p(ir), p(f_lr), p(f_rl), w, h, None, 1, p(out), None, None) == _capi.ERR_INVALID_ARG
    assert gen(ctx.h, p(il), p(ir), p(f_lr), p(f_rl), w, h, p(sh), 1, None, None, None) == _capi.ERR_INVALID_ARG
    assert gen(ctx.h, p(il), p(ir), p(f_lr), p(f_rl), w, h, p(sh), 0, p(out), None, None) == _capi.ERR_INVALID_ARG and "shift" in msg()
    assert gen(ctx.h, p(il), p(ir), p(f_lr), p(f_rl), 0, h, p(sh), 1, p(out), None, None) == _capi.ERR_INVALID_ARG and "size" in msg()
    assert gen(ctx.h, p(il), p(ir), p(f_lr), p(f_rl), w, -3, p(sh), 1, p(out), None, None) == _capi.ERR_INVALID_ARG
    assert gen(None, p(il), p(ir), p(f_lr), p(f_rl), w, h, p(sh), 1, p(out), None, None) == _capi.ERR_INVALID_ARG
    assert itp(ctx.h, b"pixflow_low", None, p(ir), w, h, p(sh), 1, p(out), None, None, None, None) == _capi.ERR_INVALID_ARG
    assert itp(ctx.h, None, p(il), p(ir), w, h, p(sh), 1, p(out), None, None, None, None) == _capi.ERR_INVALID_ARG
    assert itp(ctx.h, b"pixflow_low", p(il), p(ir), w, h, p(sh), 0, p(out), None, None, None, None) == _capi.ERR_INVALID_ARG
    assert itp(ctx.h, b"pixflow_low", p(il), p(ir), 0, 0, p(sh), 1, p(out), None, None, None, None) == _capi.ERR_INVALID_ARG
    assert itp(ctx.h, b"no_such_flow", p(il), p(ir), w, h, p(sh), 1, p(out), None, None, None, None) == _capi.ERR_UNKNOWN_ALG
    from surround360_amd import render as R
    try:
        ctx.interpolate_views(il, ir, 0.5, alg="no_such_flow")
    except R.VrCamException as e:
        assert "unrecognized flow algorithm name" in str(e)
    else:
        raise AssertionError("unknown algorithm accepted")
    # the context is usable afterwards
    same_as_golden("edge", "merged", 0.5, ctx.generate_novel_views(il, ir, f_lr, f_rl, 0.5)[0])


CHECKS = {
    "generate-synth": lambda ctx, lib: check_generate(ctx, "synth"),
    "generate-edge": lambda ctx, lib: check_generate(ctx, "edge"),
    "slices-edge": lambda ctx, lib: check_slices(ctx, "edge"),
    "c-abi": check_c_abi,
    "interpolate": lambda ctx, lib: check_interpolate(ctx),
    "errors": check_errors,
}


# ---- the host program ---------------------------------------------------------------------------------------------------
def write_pair(path, img_l, img_r):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img_l[:, :, [2, 1, 0, 3]])).save(os.path.join(path, "left.png"))
    Image.fromarray(np.ascontiguousarray(img_r[:, :, [2, 1, 0, 3]])).save(os.path.join(path, "right.png"))


def read_bgra(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "RGBA", (path, im.mode)
    return np.ascontiguousarray(np.asarray(im)[:, :, [2, 1, 0, 3]])


def check_program_test_mode(exe, tmp):
    """--mode test --num_intermediate_views 5 --save_asymmetric_novel_views on the synth pair: 15 PNGs whose decoded pixels are
    the reference's views, stale files of novel_view/ gone (a sub-directory stays: `rm` without -r), the .bin flows and the log
    lines of the mode as they were."""
    import subprocess
    il, ir = NV.synth_pair()
    write_pair(tmp, il, ir)
    nv = os.path.join(tmp, "novel_view")
    os.makedirs(os.path.join(nv, "kept_dir"))
    for stale in ("000007.png", "novelFromL_000009.png", "notes.txt"):
        open(os.path.join(nv, stale), "w").write("stale")
    r = subprocess.run([exe, "--mode", "test", "--test_dir", tmp, "--left_img", "left.png", "--right_img", "right.png", "--flow_alg",
                        "pixflow_low", "--repetitions", "2", "--num_intermediate_views", str(NV.PROGRAM_VIEWS),
                        "--save_asymmetric_novel_views"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("RUNTIME (sec) = ") == 2 and r.stderr.count("---- repetition ") == 2
    names = ["%s%06d.png" % (pre, v) for v in range(NV.PROGRAM_VIEWS) for pre in ("", "novelFromL_", "novelFromR_")]
    assert sorted(os.listdir(nv)) == sorted(names + ["kept_dir"])
    for v, t in enumerate(NV.mode_test_shifts(NV.PROGRAM_VIEWS)):
        for pre, what in (("", "merged"), ("novelFromL_", "fromL"), ("novelFromR_", "fromR")):
            same_as_golden("synth", what, t, read_bgra(os.path.join(nv, "%s%06d.png" % (pre, v))))
    for name, a, b, hint in (("flowLtoR", il, ir, "LEFT"), ("flowRtoL", ir, il, "RIGHT")):
        path = os.path.join(tmp, "disparity", name + "_pixflow_low.bin")
        hdr = np.fromfile(path, dtype=np.int32, count=2)
        got = np.fromfile(path, dtype=np.float32, offset=8).reshape(int(hdr[0]), int(hdr[1]), 2)
        want = O.compute_optical_flow(a, b, "pixflow_low", hint)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert sorted(os.listdir(os.path.join(tmp, "disparity"))) == ["flowLtoR_pixflow_low.bin", "flowRtoL_pixflow_low.bin"]
    # without the flag: the merged views only, and the previous run's side views are gone
    r = subprocess.run([exe, "--mode", "test", "--test_dir", tmp, "--left_img", "left.png", "--right_img", "right.png", "--flow_alg",
                        "pixflow_low", "--num_intermediate_views", "2"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(nv)) == ["000000.png", "000001.png", "kept_dir"]
    same_as_golden("synth", "merged", 1.0, read_bgra(os.path.join(nv, "000001.png")))


def check_program_middlebury(exe, tmp):
    """--mode middlebury_interpolation_experiment on case (c): the lines as the reference prints them"""
    import subprocess
    NV.write_middlebury_dir(tmp)
    os.makedirs(os.path.join(tmp, ".hidden_10.png"))  # entries that start with '.' are no datasets
    r = subprocess.run([exe, "--mode", "middlebury_interpolation_experiment", "--test_dir", tmp, "--flow_alg", "pixflow_low",
                        "--show_interpolated_view"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rec = golden()[1]["middlebury"]
    assert sorted(rec) == sorted(NV.MIDDLEBURY)
    vals = [rec[k]["rmse"] for k in sorted(rec)]
    want = ["%s\t%s" % (k, rec[k]["printed"]) for k in sorted(rec)]
    want += ["min RMSE over all datasets = " + NV.fmt_g(min(vals)), "max RMSE over all datasets = " + NV.fmt_g(max(vals))]
    avg = 0.0
    for v in vals:  # (the reference's order of additions)
        avg += v
    want.append("avg RMSE over all datasets = " + NV.fmt_g(avg / float(len(vals))))
    assert [ln for ln in r.stderr.splitlines() if "RMSE" in ln or "\t" in ln] == want, r.stderr


def main(argv):
    from surround360_amd import _capi
    _capi.LIB_PATH = os.path.join(ROOT, "tools", "libs360_emu.so")  # (before the first _capi.lib())
    ctx = make_ctx()
    CHECKS[argv[1]](ctx, _capi.lib())
    print("ok " + argv[1])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main(sys.argv)
