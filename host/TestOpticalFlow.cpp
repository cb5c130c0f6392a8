// TestOpticalFlow — the reference's single-pair flow tool (source/test/TestOpticalFlow.cpp) on the GPU, both of its modes.
//
// --mode test (TestOpticalFlow.cpp:50-143): reads --left_img / --right_img (relative to --test_dir, loaded "unchanged" like
// imread(path, -1), alpha added when missing), runs NovelViewGeneratorAsymmetricFlow::prepare — flowLtoR = flow(L, R, LEFT) and
// flowRtoL = flow(R, L, RIGHT), NovelView.cpp:270-299 — --repetitions times and logs "RUNTIME (sec) = ..." per repetition
// exactly where the reference does (TestOpticalFlow.cpp:78-81: around prepare only). This is the harness shape of BASELINE
// configs[1] (one 2048x2048 pair). The flow fields are written in the reference's .bin format (CvUtil.cpp:159-199) to
// <test_dir>/disparity/flow{LtoR,RtoL}_<flow_alg>.bin. Then the morph between the two images: generateNovelView
// (NovelView.cpp:156-172) for shiftFromLeft = double(v) / double(n - 1), v = 0 .. n - 1, n = --num_intermediate_views (11),
// written to <test_dir>/novel_view/%06d.png and, with --save_asymmetric_novel_views, novelFromL_%06d.png / novelFromR_%06d.png
// (TestOpticalFlow.cpp:112-139). All n views are one call into the library, after the last repetition (the reference renders
// them in every repetition, each time over the previous ones). The reference empties novel_view/ with `rm` through system();
// here the directory's regular files are unlinked and the directory is created when absent. n = 1 divides zero by zero in the
// reference (a NaN shift); it is refused with a message.
//
// --mode middlebury_interpolation_experiment (TestOpticalFlow.cpp:165-226): datasets = the distinct prefixes before the first
// '_' of the entries of --test_dir, sorted; per dataset the t = 0.5 view between <p>_10.png and <p>_11.png (prepare +
// generateNovelView in one library call) against <p>_10i11.png, one line "<dataset>\t<rmse>" and the min / max / avg lines
// in the reference's wording. --show_interpolated_view is accepted and ignored (no window system).
//
// NOT produced: the reference's flow pictures <test_dir>/disparity/{LtoR,RtoL}_<flow_alg>.png (grey disparity, colour wheel,
// vector field: cv::line with CV_AA, normalize, HSV2BGR) and <test_dir>/colorwheel.png — debug visualisations nothing here
// could be checked against.
#include <dirent.h>
#include <unistd.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../include/s360.h"
#include "png_io.hpp"

namespace {
[[noreturn]] void die(const std::string& m) {  // VrCamException -> terminate handler -> abort (SystemUtil.cpp:42-61)
  std::fprintf(stderr, "Terminated with exception: %s\n", m.c_str());
  std::abort();
}
double now_sec() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
std::vector<uint8_t> load_bgra(const std::string& path, int* w, int* h) {
  pngio::Image im;
  try {
    im = pngio::read(path, true);
  } catch (const std::exception& e) {
    die(e.what());
  }
  *w = im.w;
  *h = im.h;
  if (im.c == 4) return std::vector<uint8_t>(im.px.begin(), im.px.end());
  std::vector<uint8_t> out((size_t)im.w * im.h * 4);  // cvtColor(BGR2BGRA): alpha = 255 (TestOpticalFlow.cpp:60-66)
  for (size_t i = 0, n = (size_t)im.w * im.h; i < n; ++i) {
    out[4 * i] = im.px[3 * i];
    out[4 * i + 1] = im.px[3 * i + 1];
    out[4 * i + 2] = im.px[3 * i + 2];
    out[4 * i + 3] = 255;
  }
  return out;
}
// the flow and view operators need no rig: a one-camera placeholder carries the context
s360_ctx* make_context(int w, int h, int device) {
  s360_camera cam;
  const double o[3] = {20, 0, 0}, fwd[3] = {1, 0, 0}, up[3] = {0, 0, 1}, right[3] = {0, -1, 0};
  const double res[2] = {(double)w, (double)h}, focal[2] = {1000, -1000};
  if (s360_camera_init(&cam, S360_CAM_RECTILINEAR, o, fwd, up, right, res, nullptr, nullptr, focal, nullptr, "side camera",
                       "cam0") < 0)
    die(s360_last_error(nullptr));
  s360_params P;
  std::memset(&P, 0, sizeof P);
  P.interpupilary_dist = 6.4;
  P.zero_parallax_dist = 10000;
  P.side_alpha_feather_size = 100;
  P.std_alpha_feather_size = 31;
  P.eqr_width = 256;
  P.eqr_height = 128;
  std::strncpy(P.side_flow_alg, "pixflow_low", sizeof(P.side_flow_alg) - 1);
  std::strncpy(P.polar_flow_alg, "pixflow_low", sizeof(P.polar_flow_alg) - 1);
  s360_ctx* ctx = nullptr;
  if (s360_create(&ctx, device, &cam, 1, &P) < 0) die(s360_last_error(nullptr));
  return ctx;
}
// getFilesInDir(dir, false) (SystemUtil.h:69-94): every entry whose name does not start with '.'
std::vector<std::string> files_in_dir(const std::string& dir) {
  std::vector<std::string> out;
  DIR* d = opendir(dir.c_str());
  if (!d) return out;
  while (dirent* e = readdir(d))
    if (e->d_name[0] != '.') out.push_back(e->d_name);
  closedir(d);
  return out;
}
// imageDiffRMSE (TestOpticalFlow.cpp:145-163) as the reference computes it: it reads both FOUR-channel images through
// at<Vec3b>(y, x), i.e. element x of a row is the three bytes at offset 3 * x of that row — the first three quarters of each
// row's bytes, alphas included, the last quarter of the columns never. The printed number is the interface, so exactly
// that addressing is reproduced.
double image_diff_rmse(const uint8_t* a, const uint8_t* b, int w, int h) {
  double sse = 0.0;
  for (int y = 0; y < h; ++y) {
    const uint8_t* ra = a + (size_t)y * w * 4;
    const uint8_t* rb = b + (size_t)y * w * 4;
    for (int x = 0; x < w; ++x)
      for (int k = 0; k < 3; ++k) {
        const int d = (int)ra[3 * x + k] - (int)rb[3 * x + k];
        sse += d * d;
      }
  }
  return std::sqrt(sse / double(3 * h * w));
}
int middlebury_interpolation_experiment(std::map<std::string, std::string>& F) {
  for (const char* k : {"test_dir", "flow_alg"})
    if (F[k].empty()) die(std::string("missing required command line argument: ") + k);
  std::set<std::string> datasets;
  for (const std::string& f : files_in_dir(F["test_dir"])) datasets.insert(f.substr(0, f.find('_')));  // stringSplit(f, '_')[0]
  double minRMSE = std::numeric_limits<double>::max(), maxRMSE = -std::numeric_limits<double>::max(), avgRMSE = 0.0;
  s360_ctx* ctx = nullptr;
  for (const std::string& dataset : datasets) {
    const std::string base = F["test_dir"] + "/" + dataset;
    int w, h, w1, h1, wm, hm;
    const std::vector<uint8_t> I0 = load_bgra(base + "_10.png", &w, &h);
    const std::vector<uint8_t> I1 = load_bgra(base + "_11.png", &w1, &h1);
    const std::vector<uint8_t> mid = load_bgra(base + "_10i11.png", &wm, &hm);
    if (w1 != w || h1 != h || wm != w || hm != h) die("images of dataset " + dataset + " differ in size");
    if (!ctx) ctx = make_context(w, h, std::atoi(F["device"].c_str()));
    std::vector<uint8_t> merged((size_t)w * h * 4);
    const double kShift = 0.5;
    if (s360_interpolate_views(ctx, F["flow_alg"].c_str(), I0.data(), I1.data(), w, h, &kShift, 1, merged.data(), nullptr, nullptr,
                               nullptr, nullptr) < 0)
      die(s360_last_error(ctx));
    const double rmse = image_diff_rmse(mid.data(), merged.data(), w, h);
    minRMSE = std::min(minRMSE, rmse);
    maxRMSE = std::max(maxRMSE, rmse);
    avgRMSE += rmse;
    std::fprintf(stderr, "%s\t%g\n", dataset.c_str(), rmse);
  }
  avgRMSE /= double(datasets.size());
  std::fprintf(stderr, "min RMSE over all datasets = %g\n", minRMSE);
  std::fprintf(stderr, "max RMSE over all datasets = %g\n", maxRMSE);
  std::fprintf(stderr, "avg RMSE over all datasets = %g\n", avgRMSE);
  if (ctx) s360_destroy(ctx);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  std::map<std::string, std::string> F = {{"mode", ""}, {"test_dir", ""}, {"left_img", ""}, {"right_img", ""},
                                          {"num_intermediate_views", "11"}, {"flow_alg", ""}, {"repetitions", "1"},
                                          {"save_asymmetric_novel_views", "false"}, {"show_interpolated_view", "false"},
                                          {"device", "0"}, {"log_dir", ""}, {"stderrthreshold", "0"}, {"v", "0"},
                                          {"logbuflevel", "0"}};
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.size() < 2 || a[0] != '-') die("unexpected argument: " + a);
    a = a.substr(a[1] == '-' ? 2 : 1);
    std::string key = a, val = "true";
    const size_t eq = a.find('=');
    if (eq != std::string::npos) {
      key = a.substr(0, eq);
      val = a.substr(eq + 1);
    } else if (key != "save_asymmetric_novel_views" && key != "show_interpolated_view") {
      if (i + 1 >= argc) die("flag '" + key + "' is missing its argument");
      val = argv[++i];
    }
    if (!F.count(key)) {
      std::fprintf(stderr, "ERROR: unknown command line flag '%s'\n", key.c_str());
      return 1;
    }
    F[key] = val;
  }
  auto require = [&](const char* k) {
    if (F[k].empty()) die(std::string("missing required command line argument: ") + k);
  };
  require("mode");
  if (F["mode"] == "middlebury_interpolation_experiment") return middlebury_interpolation_experiment(F);
  if (F["mode"] != "test") die("unrecongized mode: " + F["mode"]);  // TestOpticalFlow.cpp:238
  require("test_dir");
  require("left_img");
  require("right_img");
  require("flow_alg");
  const int numViews = std::atoi(F["num_intermediate_views"].c_str());
  if (numViews == 1) die("num_intermediate_views = 1: shiftFromLeft = double(0) / double(0) is not a number; ask for 2 or more views (or 0 for none)");

  int wl, hl, wr, hr;
  const std::vector<uint8_t> L = load_bgra(F["test_dir"] + "/" + F["left_img"], &wl, &hl);
  const std::vector<uint8_t> R = load_bgra(F["test_dir"] + "/" + F["right_img"], &wr, &hr);
  if (wl != wr || hl != hr) die("left and right images differ in size");
  s360_ctx* ctx = make_context(wl, hl, std::atoi(F["device"].c_str()));

  std::vector<float> flowLtoR((size_t)wl * hl * 2), flowRtoL((size_t)wl * hl * 2);
  const int reps = std::max(1, std::atoi(F["repetitions"].c_str()));
  const char* alg = F["flow_alg"].c_str();
  for (int rep = 0; rep < reps; ++rep) {
    std::fprintf(stderr, "---- repetition %d\n", rep);
    const double t0 = now_sec();
    // NovelViewGeneratorAsymmetricFlow::prepare (NovelView.cpp:282-297)
    if (s360_compute_optical_flow(ctx, alg, L.data(), R.data(), wl, hl, nullptr, nullptr, nullptr, S360_HINT_LEFT,
                                  flowLtoR.data()) < 0 ||
        s360_compute_optical_flow(ctx, alg, R.data(), L.data(), wl, hl, nullptr, nullptr, nullptr, S360_HINT_RIGHT,
                                  flowRtoL.data()) < 0)
      die(s360_last_error(ctx));
    std::fprintf(stderr, "RUNTIME (sec) = %g\n", now_sec() - t0);
  }
  const std::string dir = F["test_dir"] + "/disparity";
  mkdir(dir.c_str(), 0775);
  if (s360_save_flow_to_file((dir + "/flowLtoR_" + F["flow_alg"] + ".bin").c_str(), flowLtoR.data(), wl, hl) < 0 ||
      s360_save_flow_to_file((dir + "/flowRtoL_" + F["flow_alg"] + ".bin").c_str(), flowRtoL.data(), wl, hl) < 0)
    die(s360_last_error(nullptr));
  const std::string nvDir = F["test_dir"] + "/novel_view";
  mkdir(nvDir.c_str(), 0775);
  for (const std::string& f : files_in_dir(nvDir)) {  // `rm <test_dir>/novel_view/*` (TestOpticalFlow.cpp:110): regular files only
    struct stat sb;
    const std::string p = nvDir + "/" + f;
    if (lstat(p.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) unlink(p.c_str());
  }
  if (numViews > 0) {  // TestOpticalFlow.cpp:112-139
    const bool sides = F["save_asymmetric_novel_views"] != "false" && F["save_asymmetric_novel_views"] != "0";
    const size_t bytes = (size_t)wl * hl * 4;
    std::vector<double> shifts(numViews);
    for (int v = 0; v < numViews; ++v) shifts[v] = double(v) / double(numViews - 1);
    std::vector<uint8_t> merged(bytes * numViews), fromL(sides ? bytes * numViews : 0), fromR(sides ? bytes * numViews : 0);
    if (s360_generate_novel_views(ctx, L.data(), R.data(), flowLtoR.data(), flowRtoL.data(), wl, hl, shifts.data(), numViews,
                                  merged.data(), sides ? fromL.data() : nullptr, sides ? fromR.data() : nullptr) < 0)
      die(s360_last_error(ctx));
    try {
      for (int v = 0; v < numViews; ++v) {
        char idx[16];
        std::snprintf(idx, sizeof idx, "%06d", v);
        pngio::write(nvDir + "/" + idx + ".png", merged.data() + bytes * v, wl, hl, 4);
        if (sides) {
          pngio::write(nvDir + "/novelFromL_" + idx + ".png", fromL.data() + bytes * v, wl, hl, 4);
          pngio::write(nvDir + "/novelFromR_" + idx + ".png", fromR.data() + bytes * v, wl, hl, 4);
        }
      }
    } catch (const std::exception& e) {
      die(e.what());
    }
  }
  s360_destroy(ctx);
  return 0;
}
