// TestPoleRemoval — the reference's stand-alone check of a rig's pole masks (source/test/TestPoleRemoval.cpp) on the GPU: reads the
// rig from --rig_json_file, the two bottom cameras' images <src_images_dir>/<camera id>/<frame_number>.png and their masks
// <pole_masks_dir>/<camera id>.png, merges the two images through the flow between them with the masked pole cut out
// (combineBottomImagesWithPoleRemoval, PoleRemoval.cpp:32-188, with prevFrameDataDir "NONE", saveDebugImages true,
// saveFlowDataForNextFrame false: one call of s360_pole_removal_combine, include/s360_debug_images.h) and writes the reference's
// four files bottomImage.png, bottomImage2.png, bottomWarp2.png and _bottomCombined.png into <output_dir>/debug/<frame_number>/,
// which it makes as the reference does (TestPoleRemoval.cpp:57). Same seven flags (TestPoleRemoval.cpp:30-36); the glog flags are
// accepted like the other programs'; --device is an addition. Images are read like imgs_dir files: PNG or baseline JPEG, by
// signature (png_io.hpp / jpeg_io.hpp).
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../include/s360.h"
#include "jpeg_io.hpp"
#include "png_io.hpp"

namespace {
[[noreturn]] void die(const std::string& m) {  // VrCamException -> terminate handler -> abort (SystemUtil.cpp:42-61)
  std::fprintf(stderr, "Terminated with exception: %s\n", m.c_str());
  std::abort();
}
pngio::Image load_bgr(const std::string& path) {  // imreadExceptionOnFail(path, CV_LOAD_IMAGE_COLOR)
  try {
    return jpegio::read_any(path, false);
  } catch (const std::exception& e) {
    die(e.what());
  }
}
void mkdirs(const std::string& path) {  // mkdir -p
  std::string cur;
  for (size_t i = 0; i <= path.size(); ++i) {
    if ((i == path.size() || path[i] == '/') && !cur.empty()) mkdir(cur.c_str(), 0775);
    if (i < path.size()) cur += path[i];
  }
}
}  // namespace

int main(int argc, char** argv) {
  std::map<std::string, std::string> F = {{"src_images_dir", ""}, {"frame_number", ""}, {"pole_masks_dir", ""}, {"output_dir", ""},
                                          {"rig_json_file", ""}, {"flow_alg", "pixflow_low"}, {"alpha_feather_size", "31"},
                                          {"device", "0"}, {"log_dir", ""}, {"stderrthreshold", "0"}, {"v", "0"}, {"logbuflevel", "0"},
                                          {"logtostderr", "false"}, {"alsologtostderr", "false"}};
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.size() < 2 || a[0] != '-') die("unexpected argument: " + a);
    a = a.substr(a[1] == '-' ? 2 : 1);
    std::string key = a, val = "true";
    const size_t eq = a.find('=');
    if (eq != std::string::npos) {
      key = a.substr(0, eq);
      val = a.substr(eq + 1);
    } else if (key != "logtostderr" && key != "alsologtostderr") {
      if (i + 1 >= argc) die("flag '" + key + "' is missing its argument");
      val = argv[++i];
    }
    if (!F.count(key)) {
      std::fprintf(stderr, "ERROR: unknown command line flag '%s'\n", key.c_str());
      return 1;
    }
    F[key] = val;
  }
  for (const char* k : {"src_images_dir", "frame_number", "pole_masks_dir", "output_dir", "rig_json_file", "flow_alg"})  // TestPoleRemoval.cpp:45-50
    if (F[k].empty()) die(std::string("missing required command line argument: ") + k);

  std::vector<s360_camera> cams(64);
  const int ncams = s360_rig_load_json(F["rig_json_file"].c_str(), cams.data(), (int)cams.size());
  if (ncams < 0) die(s360_last_error(nullptr));
  cams.resize((size_t)ncams);
  // TestPoleRemoval.cpp:52-55: the camera that looks down, and the one whose axis passes farthest from the rig's centre
  const int bi = s360_rig_find_bottom(cams.data(), ncams), b2 = s360_rig_find_bottom2(cams.data(), ncams);
  if (bi < 0 || b2 < 0) die("no bottom camera in the rig");
  const s360_camera& cam = cams[(size_t)bi];
  const s360_camera& cam2 = cams[(size_t)b2];
  const double* up = cam.rotation + 3;
  const double* up2 = cam2.rotation + 3;
  const bool flip180 = up[0] * up2[0] + up[1] * up2[1] + up[2] * up2[2] < 0;

  const std::string debugDir = F["output_dir"] + "/debug/" + F["frame_number"];
  mkdirs(debugDir);

  // PoleRemoval.cpp:49-66
  const std::string file = F["frame_number"] + ".png";
  const pngio::Image bottom = load_bgr(F["src_images_dir"] + "/" + cam.id + "/" + file);
  const pngio::Image bottom2 = load_bgr(F["src_images_dir"] + "/" + cam2.id + "/" + file);
  const std::string maskPath = F["pole_masks_dir"] + "/" + cam.id + ".png", maskPath2 = F["pole_masks_dir"] + "/" + cam2.id + ".png";
  const pngio::Image mask = load_bgr(maskPath), mask2 = load_bgr(maskPath2);
  if (mask.w == 0 || mask.h == 0 || mask2.w == 0 || mask2.h == 0) die("missing or bad pole mask:" + maskPath + "," + maskPath2);
  const int w = bottom.w, h = bottom.h;
  if (bottom2.w != w || bottom2.h != h || mask.w != w || mask.h != h || mask2.w != w || mask2.h != h)
    die("the two bottom images and their pole masks must have one size");

  s360_params P;
  std::memset(&P, 0, sizeof P);  // (the operator depends on none of the frame's flags)
  P.interpupilary_dist = 6.4;
  P.zero_parallax_dist = 10000;
  P.side_alpha_feather_size = 100;
  P.std_alpha_feather_size = std::atoi(F["alpha_feather_size"].c_str());
  P.eqr_width = 256;
  P.eqr_height = 128;
  std::strncpy(P.side_flow_alg, "pixflow_low", sizeof(P.side_flow_alg) - 1);
  std::strncpy(P.polar_flow_alg, "pixflow_low", sizeof(P.polar_flow_alg) - 1);
  std::strncpy(P.poleremoval_flow_alg, "pixflow_low", sizeof(P.poleremoval_flow_alg) - 1);
  s360_ctx* ctx = nullptr;
  if (s360_create(&ctx, std::atoi(F["device"].c_str()), cams.data(), ncams, &P) < 0) die(s360_last_error(nullptr));

  const size_t n = (size_t)w * h * 4;
  std::vector<uint8_t> out[4] = {std::vector<uint8_t>(n), std::vector<uint8_t>(n), std::vector<uint8_t>(n), std::vector<uint8_t>(n)};
  if (s360_pole_removal_combine(ctx, bottom.px.data(), bottom2.px.data(), mask.px.data(), mask2.px.data(), w, h,
                                s360_camera_usable_pixels_radius(&cam), s360_camera_usable_pixels_radius(&cam2), flip180 ? 1 : 0,
                                P.std_alpha_feather_size, F["flow_alg"].c_str(), out[0].data(), out[1].data(), out[2].data(),
                                out[3].data(), nullptr) < 0)
    die(s360_last_error(ctx));
  const char* const names[4] = {"bottomImage.png", "bottomImage2.png", "bottomWarp2.png", "_bottomCombined.png"};  // PoleRemoval.cpp:148-153, 185-187
  try {
    for (int k = 0; k < 4; ++k) pngio::write(debugDir + "/" + names[k], out[k].data(), w, h, 4);
  } catch (const std::exception& e) {
    die(e.what());
  }
  s360_destroy(ctx);
  return 0;
}
