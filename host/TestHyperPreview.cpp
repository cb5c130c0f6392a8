// TestHyperPreview — the reference's footage preview (source/test/TestHyperPreview.cpp; scripts/preview.py drives it and pipes
// its frames into ffmpeg) on the GPU: reads the capture's .bin containers (footage.hpp), takes only the top camera and the two
// bottom cameras, and writes one equirect preview per frame to <preview_dest>/%06d.jpg. The per-frame work — crude half-resolution
// demosaic, fades, float bicubic projection, alpha softmax — is libs360's preview object (include/s360_preview.h); this program
// reads, feeds and encodes:
//   * the flags of TestHyperPreview.cpp:40-55 with their names and defaults (image_width / image_height and
//     enable_pole_removal are defined and never read there: accepted, ignored) and the four glog flags preview.py passes;
//     additions, opt-in only: --preview_ext jpg|png (png: the same pixels losslessly), --jpeg_threads N (8, at most 16), --device,
//     --device_jpeg (no value, or =true / =false; S360_PREVIEW_DEVICE_JPEG=1 in the environment switches it on for a caller that
//     cannot be changed — a flag on the command line, =false included, wins over it, and with --preview_ext png it is ignored): the .jpg files are encoded on the device behind the compose kernel (s360_preview_set_jpeg, quality 95:
//     the same bytes), the finished file travels to the host instead of the pixels and the pool's threads only write;
//   * files <binary_prefix>/<i>.bin, i < file_count, with the reference's header checks (magic, file index, file count, sizes
//     consistent across files; its comparison of the never-initialised timestamps[] is NOT restated); global camera c lives in
//     file c % file_count; the serial numbers (second 32-bit word of each frame of the first frame set) are sorted AS DECIMAL
//     STRINGS, and the three *_cam_index flags index that list (:305-321, :344-347);
//   * frames from start_frame for frame_count frames (0 = all). Only whole frame sets common to all files are rendered (the
//     reference's EOF bookkeeping for files of unequal length is not restated);
//   * reading + upload of frame k + 1, rendering of frame k and encoding + writing of earlier frames overlap: page-locked
//     frame buffers, s360_preview_submit_packed / _fetch, a pool of encoder threads (jpeg_io.hpp: what cv::imwrite writes
//     through libjpeg at OpenCV's defaults).
// S360_PREVIEW_TIMES=1 in the environment (developer switch, tools/preview_time.py): where the wall time went, on stderr at the end.
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../include/s360_preview.h"
#include "footage.hpp"
#include "jpeg_io.hpp"
#include "png_io.hpp"

namespace {
[[noreturn]] void die(const std::string& m) {
  std::fprintf(stderr, "Terminated with exception: %s\n", m.c_str());
  std::abort();
}

// encoder threads: jobs run in any order; the first failure is kept and reported by wait()
struct Pool {
  std::vector<std::thread> threads;
  std::deque<std::function<void()>> jobs;
  std::mutex mu;
  std::condition_variable cvJob, cvIdle;
  int running = 0;
  bool stop = false;
  std::string error;
  explicit Pool(int n) {
    for (int i = 0; i < n; ++i)
      threads.emplace_back([this] {
        for (;;) {
          std::function<void()> job;
          {
            std::unique_lock<std::mutex> lk(mu);
            cvJob.wait(lk, [this] { return stop || !jobs.empty(); });
            if (jobs.empty()) return;
            job = std::move(jobs.front());
            jobs.pop_front();
            ++running;
          }
          std::string err;
          try { job(); } catch (const std::exception& e) { err = e.what(); }
          std::lock_guard<std::mutex> lk(mu);
          if (!err.empty() && error.empty()) error = err;
          --running;
          cvIdle.notify_all();
        }
      });
  }
  void add(std::function<void()> job) {
    { std::lock_guard<std::mutex> lk(mu); jobs.push_back(std::move(job)); }
    cvJob.notify_one();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cvIdle.wait(lk, [this] { return jobs.empty() && running == 0; });
    if (!error.empty()) throw std::runtime_error(error);
  }
  ~Pool() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cvJob.notify_all();
    for (auto& t : threads) t.join();
  }
};
}  // namespace

int main(int argc, char** argv) {
  std::map<std::string, std::string> F = {
      {"image_width", "2048"}, {"image_height", "2048"}, {"binary_prefix", ""}, {"file_count", "2"}, {"start_frame", "0"},
      {"frame_count", "0"}, {"rig_json_file", ""}, {"eqr_width", "2048"}, {"eqr_height", "1024"}, {"preview_dest", ""},
      {"gamma", "1.0"}, {"top_cam_index", "0"}, {"bottom_cam_index", "15"}, {"bottom_cam2_index", "16"},
      {"enable_pole_removal", "true"}, {"softmax_coef", "30.0"}, {"preview_ext", "jpg"}, {"jpeg_threads", "8"}, {"device", "0"},
      {"device_jpeg", ""},
      {"log_dir", ""}, {"stderrthreshold", "0"}, {"v", "0"}, {"logbuflevel", "0"}};
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.size() < 2 || a[0] != '-') die("unexpected argument: " + a);
    a = a.substr(a[1] == '-' ? 2 : 1);
    std::string key = a, val;
    const size_t eq = a.find('=');
    if (eq != std::string::npos) { key = a.substr(0, eq); val = a.substr(eq + 1); }
    else if (key == "device_jpeg") val = "true";
    else { if (i + 1 >= argc) die("flag '" + key + "' is missing its argument"); val = argv[++i]; }
    if (!F.count(key)) { std::fprintf(stderr, "ERROR: unknown command line flag '%s'\n", key.c_str()); return 1; }
    F[key] = val;
  }
  for (const char* k : {"binary_prefix", "rig_json_file", "preview_dest"})
    if (F[k].empty()) die(std::string("missing required command line argument: ") + k);
  const int fileCount = std::atoi(F["file_count"].c_str());
  const long startFrame = std::atol(F["start_frame"].c_str()), frameCountFlag = std::atol(F["frame_count"].c_str());
  const int eqrW = std::atoi(F["eqr_width"].c_str()), eqrH = std::atoi(F["eqr_height"].c_str());
  const int jpegThreads = std::max(1, std::min(16, std::atoi(F["jpeg_threads"].c_str())));
  const bool png = F["preview_ext"] == "png";
  if (!png && F["preview_ext"] != "jpg") die("--preview_ext is jpg or png");
  const char* envJpeg = std::getenv("S360_PREVIEW_DEVICE_JPEG");
  const bool flagGiven = !F["device_jpeg"].empty();  // a flag on the command line decides; the environment only where there is none
  const bool flagJpeg = F["device_jpeg"] == "true" || F["device_jpeg"] == "1";
  if (flagGiven && !flagJpeg && F["device_jpeg"] != "false" && F["device_jpeg"] != "0") die("--device_jpeg is true or false");
  if (flagJpeg && png) die("--device_jpeg encodes .jpg files: it does not go with --preview_ext png");
  // (the environment switch is for .jpg output: with --preview_ext png it changes nothing, where the flag is refused)
  const bool deviceJpeg = flagGiven ? flagJpeg : (!png && envJpeg && envJpeg[0] == '1');
  if (fileCount < 1 || fileCount > 4096) die("--file_count must be at least 1");
  if (startFrame < 0 || frameCountFlag < 0) die("--start_frame and --frame_count must not be negative");

  try {
    // the containers and the reference's checks of their metadata pages (:212-253)
    std::vector<std::unique_ptr<footage::Footage>> files;
    uint32_t cameraCount = 0;
    for (int i = 0; i < fileCount; ++i) {
      files.emplace_back(new footage::Footage);
      footage::Footage& ff = *files.back();
      ff.path = F["binary_prefix"] + "/" + std::to_string(i) + ".bin";
      try {
        ff.open(false);
      } catch (const std::exception& e) {
        throw std::runtime_error(std::string("error opening binary file. err: ") + e.what() + " filename: " + ff.path);
      }
    }
    for (int i = 0; i < fileCount; ++i) {  // (every file is opened before the first header is looked at, as in the reference)
      footage::Footage& ff = *files[i];
      if (ff.md.magic != 0xfaceb00cu) throw std::runtime_error("binary file not tagged: " + ff.path);
      if (ff.md.fileIndex != (uint32_t)i) throw std::runtime_error("binary file name in metadata != loaded .bin file");
      if (ff.md.fileCount != (uint32_t)fileCount) throw std::runtime_error("binary file count in metadata != num .bin files");
      if (i > 0 && (ff.md.width != files[0]->md.width || ff.md.height != files[0]->md.height ||
                    ff.md.bitsPerPixel != files[0]->md.bitsPerPixel))
        throw std::runtime_error("metadata not consistent across binary files!");
      cameraCount += ff.md.numberOfCameras;
    }
    const int w = (int)files[0]->md.width, h = (int)files[0]->md.height, bits = (int)files[0]->md.bitsPerPixel;
    if (cameraCount == 0) throw std::runtime_error("no cameras in the binary files");
    for (int i = 0; i < fileCount; ++i)  // camera c is frame c / file_count of a frame set of file c % file_count
      if (files[i]->md.numberOfCameras != cameraCount / fileCount + ((uint32_t)i < cameraCount % fileCount ? 1 : 0))
        throw std::runtime_error("cameras are not dealt round-robin over the binary files: " + files[i]->path);
    std::fprintf(stderr, "Reading binary files...\n");
    size_t totalFrames = (size_t)-1;
    for (auto& ff : files) totalFrames = std::min(totalFrames, ff->frames());
    if (totalFrames == 0) throw std::runtime_error("no whole frame set in the binary files");
    const auto frame_of = [&](size_t f, uint32_t cam) { return files[cam % fileCount]->frame(f, cam / fileCount); };

    // serial numbers as decimal strings, sorted as strings (:305-321)
    std::vector<std::string> serials;
    for (uint32_t c = 0; c < cameraCount; ++c) {
      uint32_t s;
      std::memcpy(&s, frame_of(0, c) + 4, 4);
      serials.push_back(std::to_string(s));
    }
    std::vector<std::string> sorted(serials);
    std::sort(sorted.begin(), sorted.end());
    uint32_t camOf[3];
    const char* idxFlag[3] = {"top_cam_index", "bottom_cam_index", "bottom_cam2_index"};
    for (int l = 0; l < 3; ++l) {
      const long idx = std::atol(F[idxFlag[l]].c_str());
      if (idx < 0 || idx >= (long)sorted.size()) throw std::runtime_error(std::string("--") + idxFlag[l] + " is not an index into the " + std::to_string(sorted.size()) + " cameras");
      camOf[l] = (uint32_t)(std::find(serials.begin(), serials.end(), sorted[idx]) - serials.begin());
    }

    long first = startFrame, count = frameCountFlag == 0 ? (long)totalFrames - startFrame : frameCountFlag;
    if (first >= (long)totalFrames) {
      std::fprintf(stderr, "Start frame (%ld) past the %zu whole frame sets: nothing to render\n", first, totalFrames);
      count = 0;
    } else if (first + count > (long)totalFrames) {
      std::fprintf(stderr, "Reached EOF: rendering %ld frames instead of %ld\n", (long)totalFrames - first, count);
      count = (long)totalFrames - first;
    }

    std::fprintf(stderr, "Generating previews...\n");
    std::vector<s360_camera> cams(256);
    const int ncams = s360_rig_load_json(F["rig_json_file"].c_str(), cams.data(), (int)cams.size());
    if (ncams < 0) throw std::runtime_error(s360_last_error(nullptr));
    s360_preview* pv = nullptr;
    if (s360_preview_create(&pv, cams.data(), ncams, std::atoi(F["device"].c_str()), w, h, eqrW, eqrH, std::atof(F["gamma"].c_str()),
                            std::atof(F["softmax_coef"].c_str())) < 0)
      throw std::runtime_error(s360_last_error(nullptr));
    mkdir(F["preview_dest"].c_str(), 0755);
    if (deviceJpeg && s360_preview_set_jpeg(pv, 1, 95) < 0) throw std::runtime_error(s360_last_error(nullptr));

    const size_t frameBytes = files[0]->frame_size(), outBytes = deviceJpeg ? s360_preview_jpeg_bound(pv) : (size_t)eqrW * eqrH * 3;
    uint8_t* in[2][3];
    for (auto& set : in)
      for (auto& p : set)
        if (!(p = static_cast<uint8_t*>(s360_host_alloc(frameBytes)))) throw std::runtime_error(s360_last_error(nullptr));
    // output buffers: one per encoder thread and two more, so that fetching never waits for an encoder unless all are busy
    std::vector<uint8_t*> freeOut;
    std::mutex outMu;
    std::condition_variable outCv;
    for (int i = 0; i < jpegThreads + 2; ++i) {
      uint8_t* p = static_cast<uint8_t*>(s360_host_alloc(outBytes));
      if (!p) throw std::runtime_error(s360_last_error(nullptr));
      freeOut.push_back(p);
    }
    std::vector<uint8_t*> allOut(freeOut);
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    double tRead = 0, tSubmit = 0, tFetch = 0;
    std::atomic<long long> encodeUs{0};
    const auto tStart = now();
    {
      Pool pool(jpegThreads);
      const auto fetch_and_encode = [&](long frame) {
        uint8_t* buf;
        {
          std::unique_lock<std::mutex> lk(outMu);
          outCv.wait(lk, [&] { return !freeOut.empty(); });
          buf = freeOut.back();
          freeOut.pop_back();
        }
        const auto f0 = now();  // (waiting for a free output buffer counts as encoding, not as fetching)
        size_t fileBytes = 0;
        if ((deviceJpeg ? s360_preview_fetch_jpeg(pv, buf, outBytes, &fileBytes) : s360_preview_fetch(pv, buf)) < 0)
          throw std::runtime_error(s360_last_error(nullptr));
        tFetch += secs(f0, now());
        char name[32];
        std::snprintf(name, sizeof name, "/%06ld.%s", frame, png ? "png" : "jpg");
        const std::string path = F["preview_dest"] + name;
        pool.add([&, buf, path, fileBytes] {
          struct Release {
            std::vector<uint8_t*>& v; std::mutex& m; std::condition_variable& c; uint8_t* b;
            ~Release() { { std::lock_guard<std::mutex> lk(m); v.push_back(b); } c.notify_one(); }
          } rel{freeOut, outMu, outCv, buf};
          const auto e0 = std::chrono::steady_clock::now();
          if (deviceJpeg) {  // the file is finished: only written
            pngio::OutFile f(path);
            f.put(buf, fileBytes);
            f.close();
          } else if (png) pngio::write(path, buf, eqrW, eqrH, 3, 1, 1);
          else jpegio::write(path, buf, eqrW, eqrH);
          encodeUs += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - e0).count();
        });
      };
      for (long k = 0; k < count; ++k) {
        const long frame = first + k;
        uint8_t** set = in[k & 1];
        const auto r0 = now();
        for (int l = 0; l < 3; ++l) std::memcpy(set[l], frame_of((size_t)frame, camOf[l]), frameBytes);
        const auto r1 = now();
        std::fprintf(stderr, "Rendering frame %ld...\n", frame);
        if (s360_preview_submit_packed(pv, set[0], set[1], set[2], bits) < 0) throw std::runtime_error(s360_last_error(nullptr));
        tRead += secs(r0, r1);
        tSubmit += secs(r1, now());
        if (k > 0) fetch_and_encode(frame - 1);
      }
      if (count > 0) fetch_and_encode(first + count - 1);
      pool.wait();
    }
    const char* times = std::getenv("S360_PREVIEW_TIMES");
    if (times && times[0] == '1' && count > 0) {
      const double wall = secs(tStart, now()), enc = encodeUs.load() * 1e-6;
      std::fprintf(stderr, "preview times: %ld frames in %.3f s (%.1f frames/s); feeding thread: reading %.3f s, submit %.3f s, waiting in fetch %.3f s; "
                   "encoding + writing %.3f thread-seconds on %d threads (%.3f s of wall time if spread evenly)\n",
                   count, wall, count / wall, tRead, tSubmit, tFetch, enc, jpegThreads, enc / jpegThreads);
    }
    std::fprintf(stderr, "Closing binary files...\n");
    s360_preview_destroy(pv);
    for (auto& set : in)
      for (auto& p : set) s360_host_free(p);
    for (uint8_t* p : allOut) s360_host_free(p);
  } catch (const std::exception& e) {
    die(e.what());
  }
  return 0;
}
