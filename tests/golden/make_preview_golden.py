#!/usr/bin/env python
"""Writes tests/golden/preview_golden.npz: what the REFERENCE's TestHyperPreview computes for the cases of tests/preview_cases.py —
its sources compiled from /root/reference where they lie, over the stand-ins of oracle/ref_shim. The driver below is this
project's own text. It includes test/TestHyperPreview.cpp itself with its main() renamed (never called) and links Camera.cpp,
RigDescription.cpp, ImageWarper.cpp and CvUtil.cpp, so the recorded numbers come from the reference's own

  PreviewRenderer()            RigDescription::findCameraByDirection / findLargestDistCamAxisToRigCenter,
                               Camera::createRescaledCamera, precomputeProjectionWarp -> projectEquirectToCam -> Camera::sees / pixel
  PreviewRenderer::simpleDemosaic, projectToEquirect (remap: cvlite's restatement behind the stand-in)
  radialAlphaFade, topDownAlphaFade, flattenLayersAlphaSoftmax (CvUtil.cpp)

Camera::createRescaledCamera (Camera.cpp:273-289) sits in the half of Camera.cpp that the stand-ins cannot compile (the rig
serialisation around it needs all of folly::dynamic; that half is switched off with -DSUPPRESS_RIG_IO as everywhere in oracle/):
the generator cuts that one function's text out of the reference's file AT RUN TIME into a temporary translation unit of its own
and compiles it there, unchanged. Nothing of it is kept.

What does not compile or link over the stand-ins is restated in the driver:
  * `src.size() / scale` (TestHyperPreview.cpp:167): cv::Size / int, an integer division of both members;
  * `outImage.ptr(0)` in the renamed main() (:258): the stand-in has only ptr<T>(); main() is never run;
  * render() (:143-161) ends in imwriteExceptionOnFail of a .jpg, which the stand-ins cannot write: its lines are restated in the
    driver up to the image handed to imwrite — cvtColor(BGR2BGRA) of a float image (alpha 1.0f; the stand-in converts 8-bit images
    only), `eqrImage * kNorm16to8` (the stand-in's Mat * double: a float multiply, as cv::Mat's scaled conversion of a float image
    is), and the saturate_cast<uchar> that imwrite's convertTo(CV_8U) applies (cvRound: round half to even, INT_MIN for NaN).
The raw images are handed over already widened to 16 bits (the unpacking loop lives in the reference's main(), :374-397; it is
restated in tests/preview_oracle.py: unpack, and in the library as k_isp_unpack has it).

The generator ASSERTS that tests/preview_oracle.py gives the same bits for everything recorded; that is what pins the restatement
the GPU tests are checked against. Run where /root/reference exists:  python tests/golden/make_preview_golden.py [out.npz]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import preview_cases as PC  # noqa: E402
import preview_oracle as PO  # noqa: E402

REF = "/root/reference/surround360_render/source"
ORACLE = os.path.join(ROOT, "oracle")

DRIVER = r"""
// driver <rig.json> <eqr_w> <eqr_h> <gamma> <softmax_coef> <raw_w> <raw_h> <raw16 x 3 file> <out file>
// out: per camera 6 doubles (resolution, principal, focal) + 32 bytes of id; 3 maps (eqr_h x eqr_w x 2 float);
//      per layer: demosaiced (hh x hw x 3 float), developed (hh x hw x 4), remapped (eqr_h x eqr_w x 4);
//      flattened (eqr_h x eqr_w x 3 float); bytes (eqr_h x eqr_w x 3)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "CvUtil.h"
#include "ImageWarper.h"
#include "RigDescription.h"

namespace cv {
inline Size operator/(const Size& s, int d) { return Size(s.width / d, s.height / d); }  // RESTATEMENT: cv::Size / int
}
#define main reference_main
#define ptr(x) data  /* outImage.ptr(0) in the renamed main(): see the docstring */
#include "test/TestHyperPreview.cpp"
#undef ptr
#undef main

static void put(FILE* o, const Mat& m, size_t elem) {
  for (int y = 0; y < m.rows; ++y) fwrite(m.data + (size_t)y * m.step, 1, (size_t)m.cols * elem, o);
}

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  FLAGS_rig_json_file = argv[1];
  FLAGS_eqr_width = atoi(argv[2]);
  FLAGS_eqr_height = atoi(argv[3]);
  FLAGS_gamma = atof(argv[4]);
  FLAGS_softmax_coef = atof(argv[5]);
  const int w = atoi(argv[6]), h = atoi(argv[7]);
  std::vector<uint16_t> raw((size_t)w * h * 3);
  FILE* f = fopen(argv[8], "rb");
  if (!f || fread(raw.data(), 2, raw.size(), f) != raw.size()) return 3;
  fclose(f);
  FILE* o = fopen(argv[9], "wb");
  if (!o) return 4;
  PreviewRenderer pr;
  for (const Camera& c : pr.cameras) {
    const double v[6] = {c.resolution.x(), c.resolution.y(), c.principal.x(), c.principal.y(), c.focal.x(), c.focal.y()};
    char id[32] = {0};
    strncpy(id, c.id.c_str(), 31);
    fwrite(v, 8, 6, o);
    fwrite(id, 1, 32, o);
  }
  for (const Mat& m : pr.warped) put(o, m, 8);
  // RESTATEMENT of render() (TestHyperPreview.cpp:143-161) around the reference's own functions
  std::vector<Mat> layers;
  for (int i = 0; i < 3; ++i) {
    const Mat rawImg(h, w, CV_16U, raw.data() + (size_t)i * w * h);
    Mat rgb = PreviewRenderer::simpleDemosaic(rawImg);
    put(o, rgb, 12);
    Mat bgra(rgb.rows, rgb.cols, CV_32FC4);  // cvtColor(rgb, rgb, CV_BGR2BGRA) of a float image: alpha 1.0f
    for (int y = 0; y < rgb.rows; ++y)
      for (int x = 0; x < rgb.cols; ++x) {
        const Vec3f c = rgb.at<Vec3f>(y, x);
        bgra.at<Vec4f>(y, x) = Vec4f(c[0], c[1], c[2], 1.0f);
      }
    if (i > 0) topDownAlphaFade(bgra);
    radialAlphaFade(bgra);
    put(o, bgra, 16);
    layers.push_back(pr.projectToEquirect(pr.cameras[i], bgra, pr.warped[i]));
    put(o, layers.back(), 16);
  }
  Mat eqrImage = flattenLayersAlphaSoftmax(layers, FLAGS_softmax_coef);
  put(o, eqrImage, 12);
  const Mat scaled = eqrImage * kNorm16to8;
  for (int y = 0; y < scaled.rows; ++y)
    for (int x = 0; x < scaled.cols; ++x)
      for (int k = 0; k < 3; ++k) {  // imwrite's convertTo(CV_8U): saturate_cast<uchar>(float) = cvRound, clamped
        const float v = scaled.at<Vec3f>(y, x)[k];
        const int r = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)__builtin_rintf(v) : (-2147483647 - 1);
        const unsigned char b = (unsigned char)(r < 0 ? 0 : r > 255 ? 255 : r);
        fwrite(&b, 1, 1, o);
      }
  fclose(o);
  return 0;
}
"""

# (shape, content, bits, gamma): the chains that are recorded
CHAINS = [("landscape", "spread", 12, 1.0), ("portrait", "checker", 8, 1.0), ("portrait", "dark", 12, 2.2)]


def build_driver(tmp):
    src, exe = os.path.join(tmp, "preview_driver.cpp"), os.path.join(tmp, "preview_driver")
    open(src, "w").write(DRIVER)
    cam = open(REF + "/render/Camera.cpp").read()
    a = cam.index("Camera Camera::createRescaledCamera(")
    b = cam.index("\n}\n", a) + 3
    rescale = os.path.join(tmp, "rescaled_camera.cpp")
    open(rescale, "w").write('#include "Camera.h"\nnamespace surround360 {\n' + cam[a:b] + "}\n")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fno-fast-math", "-w", "-DSUPPRESS_RIG_IO",
                           "-include", os.path.join(ORACLE, "ref_shim", "ref_prelude.h"), "-I" + os.path.join(ORACLE, "ref_shim"),
                           "-I" + REF, "-I" + REF + "/util", "-I" + REF + "/render", "-I" + REF + "/optical_flow", "-I" + ORACLE, "-o", exe, src,
                           REF + "/render/Camera.cpp", rescale, REF + "/render/RigDescription.cpp", REF + "/render/ImageWarper.cpp",
                           REF + "/util/CvUtil.cpp", REF + "/util/SystemUtil.cpp", REF + "/util/StringUtil.cpp",
                           os.path.join(ORACLE, "ref_shim", "ref_support.cpp"), "-lz", "-pthread"])
    return exe


def run_driver(exe, tmp, shape, content, bits, gamma, coef=30.0):
    raw_w, raw_h, W, H, _, _ = PC.SHAPES[shape]
    hw, hh = raw_w // 2, raw_h // 2
    rig = PC.write_rig(PC.small_rig(shape), os.path.join(tmp, "rig.json"))
    frames = PC.frames(shape, content, bits)
    raw = np.stack([PO.unpack(f, bits, raw_w, raw_h) for f in frames])
    fin, fout = os.path.join(tmp, "raw.bin"), os.path.join(tmp, "out.bin")
    raw.tofile(fin)
    subprocess.check_call([exe, rig, str(W), str(H), repr(gamma), repr(coef), str(raw_w), str(raw_h), fin, fout])
    b = open(fout, "rb").read()
    pos = [0]

    def take(dtype, *shp):
        n = int(np.prod(shp)) * np.dtype(dtype).itemsize
        a = np.frombuffer(b, dtype, int(np.prod(shp)), pos[0]).reshape(shp)
        pos[0] += n
        return a
    cams = []
    for _ in range(3):
        v = take(np.float64, 6)
        cams.append((v, take(np.uint8, 32).tobytes().split(b"\0")[0].decode()))
    out = {"cams": cams, "maps": [take(np.float32, H, W, 2) for _ in range(3)], "demosaic": [], "developed": [], "remapped": []}
    for _ in range(3):
        out["demosaic"].append(take(np.float32, hh, hw, 3))
        out["developed"].append(take(np.float32, hh, hw, 4))
        out["remapped"].append(take(np.float32, H, W, 4))
    out["flat"] = take(np.float32, H, W, 3)
    out["bytes"] = take(np.uint8, H, W, 3)
    assert pos[0] == len(b)
    return out, frames


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main(path):
    assert os.path.isdir(REF), "needs /root/reference"
    tmp = tempfile.mkdtemp()
    exe = build_driver(tmp)
    arrays = {}
    for shape, content, bits, gamma in CHAINS:
        ref, frames = run_driver(exe, tmp, shape, content, bits, gamma)
        raw_w, raw_h, W, H, _, _ = PC.SHAPES[shape]
        key = "%s/%s/%d/%g/" % (shape, content, bits, gamma)
        # the restatement on the same inputs, bit for bit
        poles = PC.pole_cameras(PC.small_rig(shape))
        assert [i for _, i in ref["cams"]] == list(PC.POLE_IDS), ref["cams"]
        for l in range(3):
            cj = PO.rescaled_camera_json(poles[l])
            assert list(ref["cams"][l][0]) == cj["resolution"] + cj["principal"] + cj["focal"], "createRescaledCamera, layer %d" % l
            assert same(PO.warp_map(cj, W, H), ref["maps"][l]), "warp map, layer %d" % l
            raw16 = PO.unpack(frames[l], bits, raw_w, raw_h)
            assert same(PO.simple_demosaic(raw16, gamma), ref["demosaic"][l]), "simpleDemosaic, layer %d" % l
            dev = PO.develop(frames[l], bits, raw_w, raw_h, l, gamma)
            assert same(dev, ref["developed"][l]), "fades, layer %d" % l
            assert same(PO.remap(dev, ref["maps"][l]), ref["remapped"][l]), "remap, layer %d" % l
        flat = PO.flatten_layers_alpha_softmax(ref["remapped"], 30.0)
        assert same(flat, ref["flat"]), "flattenLayersAlphaSoftmax"
        assert same(PO.to_u8(flat), ref["bytes"]), "8-bit conversion"
        assert np.isnan(ref["flat"]).any() == (shape == "portrait"), "the band no camera sees"
        r = PO.Renderer(poles, raw_w, raw_h, W, H, gamma)
        assert same(r.render(*frames, bits), ref["bytes"]), "the whole chain"
        arrays[key + "cams"] = np.stack([v for v, _ in ref["cams"]])
        if gamma == 1.0:
            for l in range(3):
                arrays[key + "map%d" % l] = ref["maps"][l]
        for l in range(3):
            arrays[key + "developed%d" % l] = ref["developed"][l]
        arrays[key + "remapped1"] = ref["remapped"][1]
        arrays[key + "flat"] = ref["flat"]
        arrays[key + "bytes"] = ref["bytes"]
        print(key, "recorded; NaN pixels: %d, saturated bytes: %.0f %%" % (np.isnan(ref["flat"]).any(axis=-1).sum(),
                                                                         100 * (ref["bytes"] == 255).mean()))
    np.savez_compressed(path, **arrays)
    print("wrote %d arrays, %d bytes" % (len(arrays), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "preview_golden.npz"))
