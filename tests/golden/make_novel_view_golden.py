#!/usr/bin/env python
"""Writes tests/golden/novel_view_golden.npz + .json: what the REFERENCE's generateNovelView (optical_flow/NovelView.cpp:20-99,
156-172, compiled from /root/reference where it lies, over the stand-ins of oracle/ref_shim) returns for the cases of
tests/novel_view_cases.py. The driver below is this project's own text: it includes the reference's headers, fills imageL / imageR /
flowLtoR / flowRtoL of a NovelViewGeneratorAsymmetricFlow and calls generateNovelView per shift. imageDiffRMSE lives in the file
with the reference's main() and its visualisation calls, which do not link over the stand-ins: the driver RESTATES those twenty
lines (Vec3b addressing over four-channel images included) and applies them to the reference's own t = 0.5 view.
The flows are the reference's own PixFlow (oracle/_ref/libref_pixflow.so); the generator asserts that the oracle, which the GPU
machine has, computes the same bits.
Run in the build container, where /root/reference exists:  python tests/golden/make_novel_view_golden.py [out_prefix]"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import novel_view_cases as NV  # noqa: E402
import oracle_lib as O  # noqa: E402

REF = "/root/reference/surround360_render/source"
ORACLE = os.path.join(ROOT, "oracle")

DRIVER = r"""
// in: int32 w, h, n, hasTruth; imageL, imageR (w*h*4); flowLtoR, flowRtoL (w*h*2 float); n doubles; [truth w*h*4]
// out: per shift merged, fromL, fromR (w*h*4 each); [double rmse(truth, merged of shift 0)]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "CvUtil.h"
#include "MathUtil.h"
#include "NovelView.h"

using namespace cv;
using namespace surround360;
using namespace surround360::optical_flow;

// RESTATEMENT of imageDiffRMSE (test/TestOpticalFlow.cpp:145-163): Vec3b reads of whatever the Mats hold
static double imageDiffRMSE(const Mat& imageA, const Mat& imageB) {
  double sse = 0.0;
  for (int y = 0; y < imageA.rows; ++y) {
    for (int x = 0; x < imageA.cols; ++x) {
      const Vec3b colorA = imageA.at<Vec3b>(y, x);
      const Vec3b colorB = imageB.at<Vec3b>(y, x);
      sse += math_util::square(colorA[0] - colorB[0]) + math_util::square(colorA[1] - colorB[1]) +
             math_util::square(colorA[2] - colorB[2]);
    }
  }
  const double mse = sse / double(3 * imageA.rows * imageA.cols);
  return sqrt(mse);
}

int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  int32_t hd[4];
  if (!f || fread(hd, 4, 4, f) != 4) return 2;
  const int w = hd[0], h = hd[1], n = hd[2];
  const size_t px = (size_t)w * h;
  std::vector<uint8_t> L(px * 4), R(px * 4), T(px * 4);
  std::vector<float> flr(px * 2), frl(px * 2);
  std::vector<double> shifts(n);
  if (fread(L.data(), 1, px * 4, f) != px * 4 || fread(R.data(), 1, px * 4, f) != px * 4 || fread(flr.data(), 4, px * 2, f) != px * 2 ||
      fread(frl.data(), 4, px * 2, f) != px * 2 || fread(shifts.data(), 8, n, f) != (size_t)n)
    return 3;
  if (hd[3] && fread(T.data(), 1, px * 4, f) != px * 4) return 4;
  fclose(f);
  NovelViewGeneratorAsymmetricFlow gen("pixflow_low");
  gen.imageL = Mat(h, w, CV_8UC4, L.data());
  gen.imageR = Mat(h, w, CV_8UC4, R.data());
  gen.flowLtoR = Mat(h, w, CV_32FC2, flr.data());
  gen.flowRtoL = Mat(h, w, CV_32FC2, frl.data());
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  double rmse = 0;
  for (int v = 0; v < n; ++v) {
    Mat merged, fromL, fromR;
    gen.generateNovelView(shifts[v], merged, fromL, fromR);
    if (merged.type() != CV_8UC4 || merged.rows != h || merged.cols != w || fromL.type() != CV_8UC4 || fromR.type() != CV_8UC4) return 6;
    for (const Mat* m : {&merged, &fromL, &fromR})
      for (int y = 0; y < h; ++y) fwrite(m->ptr<uint8_t>(y), 1, (size_t)w * 4, o);
    if (v == 0 && hd[3]) rmse = imageDiffRMSE(Mat(h, w, CV_8UC4, T.data()), merged);
  }
  if (hd[3]) fwrite(&rmse, 8, 1, o);
  fclose(o);
  return 0;
}
"""


def build_driver(tmp):
    src = os.path.join(tmp, "novel_view_driver.cpp")
    exe = os.path.join(tmp, "novel_view_driver")
    open(src, "w").write(DRIVER)
    # (oracle/Makefile's REFFLAGS include paths, as a program)
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fno-fast-math", "-w", "-I" + os.path.join(ORACLE, "ref_shim"),
                           "-I" + REF, "-I" + REF + "/util", "-I" + REF + "/optical_flow", "-I" + ORACLE, "-o", exe, src,
                           REF + "/optical_flow/NovelView.cpp", REF + "/util/CvUtil.cpp",
                           os.path.join(ORACLE, "ref_shim", "ref_support.cpp"), "-lz"])
    return exe


def run_driver(exe, tmp, img_l, img_r, f_lr, f_rl, shifts, truth=None):
    h, w = img_l.shape[:2]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, len(shifts), 1 if truth is not None else 0], np.int32).tobytes())
        for a, t in ((img_l, np.uint8), (img_r, np.uint8), (f_lr, np.float32), (f_rl, np.float32), (shifts, np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
        if truth is not None:
            f.write(np.ascontiguousarray(truth, np.uint8).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    n = len(shifts)
    views = np.frombuffer(raw, np.uint8, n * 3 * h * w * 4).reshape(n, 3, h, w, 4)
    rmse = float(np.frombuffer(raw, np.float64, 1, n * 3 * h * w * 4)[0]) if truth is not None else None
    return views[:, 0], views[:, 1], views[:, 2], rmse


def branch_fractions(from_l, from_r):
    """shares of combineNovelViews' four alpha cases (neither / only L / only R / both visible), from the REFERENCE's warped images"""
    al, ar = from_l[..., 3] > 0, from_r[..., 3] > 0
    return [float(np.mean(~al & ~ar)), float(np.mean(al & ~ar)), float(np.mean(~al & ar)), float(np.mean(al & ar))]


def ref_flows(img_l, img_r):
    flows = NV.prepare_flows(O.ref_compute_optical_flow, img_l, img_r)
    mine = NV.prepare_flows(O.compute_optical_flow, img_l, img_r)
    for a, b in zip(flows, mine):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the oracle's flow differs from the reference's"
    return flows


def main(prefix):
    assert os.path.isdir(REF) and O.ref_lib("pixflow") is not None, "needs /root/reference (make -C oracle ref)"
    tmp = tempfile.mkdtemp()
    exe = build_driver(tmp)
    arrays, meta = {}, {"digests": {}, "inputs": {}, "branches": {}, "middlebury": {}}

    def record(case, ins, shifts):
        merged, from_l, from_r, _ = run_driver(exe, tmp, *ins, shifts)
        for k, t in enumerate(shifts):
            for what, a in (("merged", merged[k]), ("fromL", from_l[k]), ("fromR", from_r[k])):
                meta["digests"][NV.key(case, what, t)] = NV.sha(a)
                if t in (NV.FULL[case] if what == "merged" else NV.FULL_SIDES[case]):
                    arrays[NV.key(case, what, t)] = a
        meta["inputs"][case] = [NV.sha(a) for a in ins]
        meta["branches"][case] = {repr(t): branch_fractions(from_l[k], from_r[k]) for k, t in enumerate(shifts)}

    # (a)
    il, ir = NV.synth_pair()
    record("synth", (il, ir) + tuple(ref_flows(il, ir)), NV.RECORDED["synth"])
    # (b)
    record("edge", NV.edge_case(), NV.RECORDED["edge"])
    best = np.max(np.array(list(meta["branches"]["edge"].values())), axis=0)
    assert (best >= 0.05).all(), "a branch of combineNovelViews holds < 5 %% of the pixels in every recorded view: %s" % best
    # (c)
    for name in NV.MIDDLEBURY:
        f10, f11, mid = (NV.add_alpha(a) for a in NV.middlebury_dataset(name))
        merged, _, _, rmse = run_driver(exe, tmp, f10, f11, *ref_flows(f10, f11), [0.5], truth=mid)
        assert rmse == NV.image_diff_rmse(mid, merged[0])
        meta["middlebury"][name] = {"rmse": rmse, "printed": NV.fmt_g(rmse), "merged": NV.sha(merged[0])}
    # 2048 x 2048 (BASELINE configs[1]): digests only
    fs = NV.FULLSIZE
    from surround360_amd import synth
    il, ir = synth.flow_pair(fs["w"], fs["h"], fs["seed"])
    flows = ref_flows(il, ir)
    shifts = sorted(set(fs["merged"]) | set(fs["sides"]))
    merged, from_l, from_r, _ = run_driver(exe, tmp, il, ir, *flows, shifts)
    meta["inputs"]["fullsize"] = [NV.sha(a) for a in (il, ir) + tuple(flows)]
    for k, t in enumerate(shifts):
        if t in fs["merged"]:
            meta["digests"][NV.key("fullsize", "merged", t)] = NV.sha(merged[k])
        if t in fs["sides"]:
            meta["digests"][NV.key("fullsize", "fromL", t)] = NV.sha(from_l[k])
            meta["digests"][NV.key("fullsize", "fromR", t)] = NV.sha(from_r[k])
    np.savez_compressed(prefix + ".npz", **arrays)
    json.dump(meta, open(prefix + ".json", "w"), indent=1, sort_keys=True)
    print("wrote %d arrays, %d bytes; branches of the edge case (best view each): %s" % (len(arrays), os.path.getsize(prefix + ".npz"), best))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "novel_view_golden"))
