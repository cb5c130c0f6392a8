// TestRenderStereoPanorama — drop-in host binary for the per-frame stereo-panorama render of surround360_render
// (reference: source/test/TestRenderStereoPanorama.cpp). Same flags (TRSP:44-70), same rig JSON, same input /
// output / state-file layout, so scripts/batch_process_video.py can call it unmodified; the work between
// "decoded images" and "stacked equirect" runs on one MI355X through the C ABI of libs360 (include/s360.h).
//
// Kept on the host, as in the reference: flag parsing, the rig loader (inside libs360: rig.cpp), directory
// scanning, PNG decode/encode (png_io.hpp instead of cv::imread/imwrite) and the flow-state files.
// --save_debug_images writes the reference's debug images under <output_data_dir>/debug/<frame>/ (write_debug_images below): one
// frame per process or --num_frames, on one GPU.
// Opt-in additions: --num_gpus G (one frame sharded over G GPUs, native RCCL strip gather) and --num_frames N (a
// stream of N consecutive frames in one process: device-resident temporal state, overlapped I/O).
#include <dirent.h>
#include <malloc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <sstream>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../include/s360.h"
#include "jpeg_io.hpp"
#include "footage.hpp"
#include "png_io.hpp"

namespace {

struct Flags {
  std::map<std::string, std::string> v;
  Flags() {
    // DEFINE_* of TRSP:44-70
    v = {{"rig_json_file", ""}, {"imgs_dir", ""}, {"frame_number", ""}, {"output_data_dir", ""},
         {"prev_frame_data_dir", "NONE"}, {"output_cubemap_path", ""}, {"output_equirect_path", ""},
         {"interpupilary_dist", "6.4"}, {"side_alpha_feather_size", "100"}, {"std_alpha_feather_size", "31"},
         {"save_debug_images", "false"}, {"sharpening", "0.0"}, {"enable_top", "false"}, {"enable_bottom", "false"},
         {"enable_pole_removal", "false"}, {"bottom_pole_masks_dir", ""}, {"side_flow_alg", "pixflow_low"},
         {"polar_flow_alg", "pixflow_low"}, {"poleremoval_flow_alg", "pixflow_low"}, {"zero_parallax_dist", "10000"},
         {"eqr_width", "256"}, {"eqr_height", "128"}, {"final_eqr_width", "3480"}, {"final_eqr_height", "960"},
         {"cubemap_width", "1536"}, {"cubemap_height", "1536"}, {"cubemap_format", "video"},
         // glog flags the caller passes (batch_process_video.py:31-34); accepted, only --v is used
         {"log_dir", ""}, {"stderrthreshold", "0"}, {"v", "0"}, {"logbuflevel", "0"}, {"logtostderr", "false"},
         {"alsologtostderr", "false"},
         // additions of this implementation (opt-in)
         {"device", "0"}, {"write_state", "true"},
         // --device_png (default on): the output equirect's PNG is filtered and deflated on the GPU behind the frame's last kernel
         // (s360_set_png_encode / s360_frame_download_png) and this program only writes the bytes; false: the frame's pixels come
         // back and host threads encode them (png_io.hpp). Same pixels in the file either way.
         {"device_png", "true"},
         // --device_state_png (default off; S360_DEVICE_STATE_PNG=1 in the environment switches it on too, for a per-frame caller
         // that cannot be changed): the state IMAGES behind a stream's last frame are encoded on the GPU that holds them — one
         // batched launch sequence per context (s360_frame_encode_state_pngs) — and this program only writes the files' bytes;
         // off: their pixels come back raw and host threads deflate them (png_io.hpp). Same pixels in the files either way.
         {"device_state_png", "false"},
         // --device_state_read (default off; S360_DEVICE_STATE_READ=1 in the environment switches it on too): the state IMAGES of
         // --prev_frame_data_dir are read as bytes and inflated and unfiltered on the GPU that takes them — one batched decode per
         // context (s360_frame_set_prev_images_png), the flows through s360_frame_set_prev_flow — instead of host threads
         // inflating them (png_io.hpp) and their pixels being uploaded. A file the device decoder does not take (cv::imwrite's,
         // the reference program's) takes the host path for its pair or unit. Same state on the device either way.
         {"device_state_read", "false"},
         // --device_input_png (default off; S360_DEVICE_INPUT_PNG=1 in the environment switches it on too): the camera images of
         // imgs_dir are read as bytes, and those the device decoder takes with colour type 2 (s360_input_png_decodable: the banded
         // files Unpacker --device_png and Raw2Rgb --device_png write, 16- or 8-bit) go to every GPU context that needs them in
         // ONE s360_frame_upload_png, which writes the frame's source slots from the files, instead of host threads inflating them
         // and their pixels being uploaded. Every other file (cv::imwrite's, RGBA, JPEG, interlaced) takes the host decoder and
         // the pixel upload as before, file by file. Same files written either way. Ignored with --bin_list.
         {"device_input_png", "false"},
         // --device_input_jpeg (default off; S360_DEVICE_INPUT_JPEG=1 in the environment switches it on, a flag on the command line
         // wins over the environment): the same for camera images that are baseline JPEG files — what a .jpg imgs_dir holds. The
         // files s360_input_jpeg_decodable takes (8-bit YCbCr, 4:2:0 / 4:2:2 / 4:4:4, one scan, no restart markers) go to every GPU
         // context that needs them in ONE s360_frame_upload_jpeg; every other file (greyscale, restart markers, PNG)
         // takes the host decoder and the pixel upload as before, file by file. May be combined with --device_input_png: a
         // directory may hold either kind. Same files written either way. Ignored with --bin_list.
         {"device_input_jpeg", "false"},
         // --device_jpeg (default off; S360_DEVICE_JPEG=1 in the environment switches it on, a flag on the command line wins over
         // the environment): an --output_equirect_path / --output_cubemap_path that ends in .jpg, .jpeg or .jpe names a JPEG file, as
         // it does for cv::imwrite. Without this flag host threads encode it (jpegio::encode, quality 95: the reference's way, a
         // thread-second per 8K frame); with it the file is encoded on the GPU behind the frame's last kernel (s360_set_jpeg_encode /
         // s360_frame_download_jpeg) and this program only writes the bytes. Same bytes in the file either way. Ignored for PNG
         // outputs, whose switch is --device_png; the two may be combined when one output is .png and the other .jpg. The state
         // images stay PNG files (they are read back with their alpha).
         {"device_jpeg", "false"},
         // --num_gpus G: the 14 side pairs of the frame sharded over G GPUs, one RCCL strip gather
         {"num_gpus", "1"},
         // --num_frames N: frames frame_number .. +N-1 as ONE stream in this process (temporal state stays on the
         // device, decode/upload/render/download/encode overlapped); output_equirect_path must contain %s or {frame}, and so
         // must output_cubemap_path, which then names the cubemap of EVERY frame (rendered with the frame)
         // (the state files are written after the LAST frame only: that is what a later run resumes from)
         {"num_frames", "1"},
         // --num_streams S: the --num_frames frames as S independent streams, stream s = the s-th contiguous segment of the
         // frame range on GPU device + s (modulo the GPUs there are) — exactly what S invocations with that segment's
         // --frame_number / --num_frames on S GPUs produce (each segment's first frame has no previous frame, except the
         // first one's --prev_frame_data_dir), in one process. One stream cannot use more than one GPU: its pole flows
         // are one serial chain per frame and every frame needs its predecessor's flows
         {"num_streams", "1"},
         // ... on at most this many GPUs (0 = all there are). Streams that share a GPU are rendered as the FRAME SLOTS of one
         // context: frame k of all of them in one launch sequence, every stream's temporal state resident in its slot
         {"stream_gpus", "0"},
         // --bin_list a.bin,b.bin --isp_dir D: the cameras' frames come straight from the capture's .bin containers through the
         // ISP on the device ("the ISP feeding the GPU directly from .bin") instead of imgs_dir/<cam>/<frame>.png:
         // what `Unpacker --bin_list .. --isp_dir D --output_dir imgs_dir` followed by this program writes, with no file in
         // between. Cameras map as Unpacker names them: the n-th smallest serial number is the rig's camera "cam<n>"; D holds
         // <serial>.json; frame_number is the frame's index in the containers. --soft_isp as in host/Unpacker.
         {"bin_list", ""}, {"isp_dir", ""}, {"soft_isp", "false"}};
  }
  static bool is_bool(const std::string& k) {
    static const char* b[] = {"save_debug_images", "enable_top", "enable_bottom", "enable_pole_removal", "logtostderr",
                              "alsologtostderr", "write_state", "soft_isp", "device_png", "device_state_png", "device_state_read",
                              "device_input_png", "device_input_jpeg", "device_jpeg"};
    for (auto s : b)
      if (k == s) return true;
    return false;
  }
  // gflags syntax: --k=v, --k v, -k ..., --bool, --nobool. Unknown flags are an error, like gflags.
  void parse(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
      std::string a = argv[i];
      if (a.size() < 2 || a[0] != '-') fail("unexpected argument: " + a);
      a = a.substr(a[1] == '-' ? 2 : 1);
      std::string key = a, val;
      bool has = false;
      const size_t eq = a.find('=');
      if (eq != std::string::npos) { key = a.substr(0, eq); val = a.substr(eq + 1); has = true; }
      if (key == "help") { usage(); std::exit(0); }
      if (!v.count(key)) {
        if (key.rfind("no", 0) == 0 && v.count(key.substr(2)) && is_bool(key.substr(2)) && !has) {
          v[key.substr(2)] = "false";
          given.insert(key.substr(2));
          continue;
        }
        fail("unknown command line flag '" + key + "'");
      }
      if (!has) {
        if (is_bool(key)) {
          // "--flag true/false" is accepted too when the next token is a literal boolean
          if (i + 1 < argc && (!std::strcmp(argv[i + 1], "true") || !std::strcmp(argv[i + 1], "false") ||
                               !std::strcmp(argv[i + 1], "1") || !std::strcmp(argv[i + 1], "0")))
            val = argv[++i];
          else val = "true";
        } else {
          if (i + 1 >= argc) fail("flag '" + key + "' is missing its argument");
          val = argv[++i];
        }
      }
      v[key] = val;
      given.insert(key);
    }
  }
  std::set<std::string> given;  // the flags the command line named
  std::string s(const std::string& k) const { return v.at(k); }
  double d(const std::string& k) const { return std::atof(v.at(k).c_str()); }
  int i(const std::string& k) const { return std::atoi(v.at(k).c_str()); }
  bool b(const std::string& k) const { const std::string& x = v.at(k); return x == "true" || x == "1" || x == "t" || x == "yes"; }
  [[noreturn]] static void fail(const std::string& m) {
    std::fprintf(stderr, "ERROR: %s\n", m.c_str());
    std::exit(1);
  }
  void usage() const {
    std::printf("TestRenderStereoPanorama (surround360_amd / MI355X): flags and defaults\n");
    for (auto& kv : v) std::printf("  --%s (default: \"%s\")\n", kv.first.c_str(), kv.second.c_str());
  }
};

double now_sec() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
[[noreturn]] void die(const std::string& m) {  // VrCamException -> terminate handler -> abort (SystemUtil.cpp:42-61)
  std::fprintf(stderr, "Terminated with exception: %s\n", m.c_str());
  std::abort();
}
void require_arg(const std::string& v, const char* name) {  // SystemUtil.h:45-49
  if (v.empty()) die(std::string("missing required command line argument: ") + name);
}
void ck(int rc, s360_ctx* ctx) {
  if (rc < 0) die(s360_last_error(ctx));
}
// getImageFileExtension (SystemUtil.h:96-105): extension of the first file in the camera's directory
std::string image_extension(const std::string& dir) {
  DIR* d = opendir(dir.c_str());
  if (!d) die("failed to read directory: " + dir);
  std::vector<std::string> names;
  while (dirent* e = readdir(d))
    if (e->d_name[0] != '.') names.push_back(e->d_name);
  closedir(d);
  if (names.empty()) die("no files in directory: " + dir);
  std::sort(names.begin(), names.end());
  const size_t dot = names[0].rfind('.');
  return dot == std::string::npos ? "" : names[0].substr(dot);
}
void mkdirs(const std::string& path) {
  std::string cur;
  for (size_t i = 0; i <= path.size(); ++i) {
    if (i == path.size() || path[i] == '/') {
      if (!cur.empty()) mkdir(cur.c_str(), 0775);
    }
    if (i < path.size()) cur += path[i];
  }
}
// imread: the decoder is chosen by the file's signature — PNG (every colour type / depth) or baseline JPEG (jpeg_io.hpp)
pngio::Image load_png(const std::string& path, bool keep_alpha) {
  try {
    return jpegio::read_any(path, keep_alpha);
  } catch (const std::exception& e) {
    die(e.what());
  }
}
void load_png_into(const std::string& path, bool keep_alpha, pngio::Image& im) {
  try {
    jpegio::read_any_into(path, keep_alpha, im);
  } catch (const std::exception& e) {
    die(e.what());
  }
}
// Deflate threads of one PNG encoder. A stream keeps up to three encoders running beside 51 decoder threads and the HIP
// runtime's own threads, which feed the GPU its ~1000 launches per frame: unbounded (one thread per 2 MB band, ~100 for an 8K
// equirect) the encoders crowd those out and the GPU waits for its host — on the GPU boxes the process has 16 CPUs of a
// 256-thread machine (profiles/r04_v2_end_to_end_*).
static bool g_fast_exit = false;
static int g_png_threads = 0;  // 0 = one per band, up to the hardware threads
// a PNG the device has encoded: nothing left to do but write the bytes (a short write leaves no file behind, like save_png)
void save_bytes(const std::string& path, const uint8_t* data, size_t n) {
  try {
    pngio::OutFile f(path);
    f.put(data, n);
    f.close();
  } catch (const std::exception& e) {
    die(e.what());
  }
}
void save_png(const std::string& path, const uint8_t* px, int w, int h, int c) {
  try {
    pngio::write(path, px, w, h, c, 1, g_png_threads);
  } catch (const std::exception& e) {
    die(e.what());
  }
}

// ---- the codec of an output file ----------------------------------------------------------------------------------------------
// imwriteExceptionOnFail is cv::imwrite (CvUtil.h), and cv::imwrite chooses its encoder by the path's extension: .jpg, .jpeg and
// .jpe (in either case) give a JPEG file at OpenCV's defaults — quality 95, 4:2:0: the file jpegio::encode writes — and everything
// else this program writes stays a PNG. The equirect's path and the cubemap's decide independently. Each codec has a device
// encoder behind a flag of its own (--device_png, --device_jpeg): with it the fetch returns the finished file and the writer
// threads only write bytes; without it the pixels come back and the writer threads encode them.
enum class OutMode { PngHost, PngDevice, JpegHost, JpegDevice };
bool is_jpeg_path(const std::string& path) {
  const size_t dot = path.rfind('.');
  if (dot == std::string::npos || path.find('/', dot) != std::string::npos) return false;
  std::string e = path.substr(dot);
  for (char& ch : e) ch = (char)std::tolower((unsigned char)ch);
  return e == ".jpg" || e == ".jpeg" || e == ".jpe";
}
bool device_jpeg(const Flags& F) {
  if (F.given.count("device_jpeg")) return F.b("device_jpeg");
  const char* e = std::getenv("S360_DEVICE_JPEG");
  return e && !std::strcmp(e, "1");
}
OutMode out_mode(const Flags& F, const std::string& path) {
  if (is_jpeg_path(path)) return device_jpeg(F) ? OutMode::JpegDevice : OutMode::JpegHost;
  return F.b("device_png") ? OutMode::PngDevice : OutMode::PngHost;
}
bool is_file(OutMode m) { return m == OutMode::PngDevice || m == OutMode::JpegDevice; }  // the fetch returns the file, not pixels
const char* mode_name(OutMode m) {
  return m == OutMode::PngDevice ? "PNG encoded on the device" : m == OutMode::PngHost ? "PNG encoded on the host"
       : m == OutMode::JpegDevice ? "JPEG encoded on the device" : "JPEG encoded on the host";
}
// --v 1: which path each output took
void report_output_paths(OutMode eq, bool cube, OutMode cm) {
  std::fprintf(stderr, "output files:            equirect %s", mode_name(eq));
  if (cube) std::fprintf(stderr, ", cubemap %s", mode_name(cm));
  std::fprintf(stderr, "\n");
}
// the device encoders the two outputs need, switched on for the frames rendered from now on
void enable_output_encoders(s360_ctx* ctx, OutMode eq, bool cube, OutMode cm) {
  const auto any = [&](OutMode m) { return eq == m || (cube && cm == m); };
  if (any(OutMode::PngDevice)) ck(s360_set_png_encode(ctx, 1), ctx);
  if (any(OutMode::JpegDevice)) ck(s360_set_jpeg_encode(ctx, 1, 95), ctx);
}
// what the buffer of an output must hold: the file's bound, or its w x h pixels
size_t output_buffer_bytes(s360_ctx* ctx, OutMode m, bool cubemap, int w, int h) {
  if (m == OutMode::PngDevice) return cubemap ? s360_frame_cubemap_png_bound(ctx) : s360_frame_png_bound(ctx);
  if (m == OutMode::JpegDevice) return cubemap ? s360_frame_cubemap_jpeg_bound(ctx) : s360_frame_jpeg_bound(ctx);
  return (size_t)w * h * 3;
}
// a finished output of slot `slot` (-1: the selected one) into buf: the file (*n its size) or the pixels
void fetch_output(s360_ctx* ctx, OutMode m, bool cubemap, int slot, int age, uint8_t* buf, size_t cap, size_t* n) {
  int rc;
  if (m == OutMode::PngDevice) {
    rc = cubemap ? (slot < 0 ? s360_frame_download_cubemap_png(ctx, age, buf, cap, n) : s360_frame_download_cubemap_png_slot(ctx, slot, age, buf, cap, n))
                 : (slot < 0 ? s360_frame_download_png(ctx, age, buf, cap, n) : s360_frame_download_png_slot(ctx, slot, age, buf, cap, n));
  } else if (m == OutMode::JpegDevice) {
    rc = cubemap ? (slot < 0 ? s360_frame_download_cubemap_jpeg(ctx, age, buf, cap, n) : s360_frame_download_cubemap_jpeg_slot(ctx, slot, age, buf, cap, n))
                 : (slot < 0 ? s360_frame_download_jpeg(ctx, age, buf, cap, n) : s360_frame_download_jpeg_slot(ctx, slot, age, buf, cap, n));
  } else {
    rc = cubemap ? (slot < 0 ? s360_frame_download_cubemap(ctx, age, buf) : s360_frame_download_cubemap_slot(ctx, slot, age, buf))
                 : (slot < 0 ? s360_frame_download_equirect_of(ctx, age, buf) : s360_frame_download_equirect_slot(ctx, slot, age, buf));
  }
  ck(rc, ctx);
}
void save_jpeg(const std::string& path, const uint8_t* px, int w, int h) {
  std::vector<uint8_t> file;
  try {
    file = jpegio::encode(px, w, h, 95);  // cv::imwrite's default quality
  } catch (const std::exception& e) {
    die(e.what());
  }
  save_bytes(path, file.data(), file.size());
}
// ... and onto the disk, on a writer thread: n bytes of a file, or w x h pixels through the path's host encoder
void write_output(OutMode m, const std::string& path, const uint8_t* data, size_t n, int w, int h) {
  if (is_file(m)) save_bytes(path, data, n);
  else if (m == OutMode::JpegHost) save_jpeg(path, data, w, h);
  else save_png(path, data, w, h, 3);
}

// One decoded frame of the rig (rig.loadSideCameraImages: one thread per camera, RigDescription.cpp:80-108)
struct FrameInputs {
  std::string frame;
  std::vector<pngio::Image> side;
  pngio::Image top, bottom, bottom2;  // (bottom2: --enable_pole_removal's secondary bottom camera; the masks are the run's, below)
  // --device_input_png: the file of a camera whose image the device decodes (its pngio::Image then holds the size only); else empty
  std::vector<std::vector<uint8_t>> sideFile;
  std::vector<uint8_t> topFile, bottomFile, bottom2File;
  long binFrame = -1;  // --bin_list: the frame's index in the containers (nothing is decoded on the host)
};
// --bin_list: where a rig camera's frames are, and the ISP that develops them
struct BinCamera {
  const footage::Footage* file = nullptr;
  size_t cam = 0;
  uint32_t serial = 0;
  s360_isp* isp = nullptr;
};

struct Job {
  Flags F;
  std::vector<s360_camera> cams;
  std::vector<int> sideIdx;
  int P = 0, ncams = 0, ti = -1, bi = -1, b2 = -1;
  s360_params prm;
  s360_geometry g;
  std::vector<s360_ctx*> ctx;  // one per GPU; ctx[0] is the root (composite, output)
  std::vector<int> bounds;     // pairs [bounds[r], bounds[r+1]) are rendered by ctx[r]
  int owner[4] = {-1, -1, -1, -1};  // GPU of pole unit u (top_left, top_right, bottom_left, bottom_right); -1 = not enabled
  std::vector<int> unitMask, need;  // per GPU: its pole units; the eyes whose complete strips it assembles
  int extW = 0;
  std::vector<std::unique_ptr<footage::Footage>> bins;  // --bin_list
  std::map<std::string, BinCamera> binCam;              // rig camera id -> its frames
  bool from_bins() const { return !bins.empty(); }
  s360_ctx* owner_ctx(int u) const { return ctx[owner[u] < 0 ? 0 : owner[u]]; }
  int bottom_gpu() const { return owner[2] >= 0 ? owner[2] : 0; }
};

// Pole unit -> GPU (the reference runs the four units as four threads, TRSP:811-860). 4 or more GPUs: unit u
// on GPU u — with pole removal both bottom units on GPU 2, where the merged bottom image is then computed once. 2 or 3
// GPUs: the top units on GPU 0, the bottom units on GPU 1 (each needs one pole image, one FlowEngine batch of two flows).
void assign_pole_units(Job& J) {
  const int G = (int)J.ctx.size();
  J.unitMask.assign(G, 0);
  J.need.assign(G, 0);
  for (int u = 0; u < 4; ++u) {
    const bool on = u < 2 ? J.prm.enable_top : J.prm.enable_bottom;
    if (!on) { J.owner[u] = -1; continue; }
    int r = 0;
    if (G >= 4) r = (J.prm.enable_pole_removal && u == 3) ? 2 : u;
    else if (G >= 2) r = u < 2 ? 0 : 1;
    J.owner[u] = r;
    J.unitMask[r] |= 1 << u;
    J.need[r] |= 1 << (u & 1);  // poleToSideFlowThread reads the whole side panorama of its eye
  }
  J.need[0] = 3;  // the root composites both eyes
}

// --enable_pole_removal: the two red masks are properties of the rig, not of a frame (PoleRemoval.cpp:48-66 reads them with every
// frame). They are read ONCE per run, whatever the mode, and handed to every context that renders pole removal
// (s360_set_pole_masks: the library computes pole removal's alpha planes once); a frame brings only the secondary camera's image.
struct PoleMasks { pngio::Image m1, m2; };
pngio::Image load_png(const std::string& path, bool keep_alpha);
std::string pole_mask_message(const Job& J) {
  return "missing or bad pole mask:" + J.F.s("bottom_pole_masks_dir") + "/" + J.cams[J.bi].id + ".png," + J.F.s("bottom_pole_masks_dir") + "/" + J.cams[J.b2].id + ".png";
}
const PoleMasks& pole_masks(const Job& J) {
  static std::once_flag once;
  static PoleMasks pm;
  std::call_once(once, [&] {
    const std::string masks = J.F.s("bottom_pole_masks_dir");
    std::thread second([&] { pm.m2 = load_png(masks + "/" + J.cams[J.b2].id + ".png", false); });
    pm.m1 = load_png(masks + "/" + J.cams[J.bi].id + ".png", false);
    second.join();
  });
  return pm;
}
void hand_pole_masks(const Job& J) {
  if (!J.prm.enable_pole_removal) return;
  const PoleMasks& pm = pole_masks(J);
  if (pm.m1.w <= 0 || pm.m1.h <= 0 || pm.m2.w != pm.m1.w || pm.m2.h != pm.m1.h) die(pole_mask_message(J));
  for (size_t r = 0; r < J.ctx.size(); ++r)
    if (J.unitMask[r] & 12) ck(s360_set_pole_masks(J.ctx[r], pm.m1.px.data(), pm.m2.px.data(), pm.m1.w, pm.m1.h), J.ctx[r]);
}

// --device_input_png / --device_input_jpeg: how many camera files took which path (--v 1)
std::atomic<int> g_inputOnDevice(0), g_inputJpegOnDevice(0), g_inputOnHost(0);
bool device_input_png(const Flags& F) {
  const char* e = std::getenv("S360_DEVICE_INPUT_PNG");
  return F.s("bin_list").empty() && (F.b("device_input_png") || (e && !std::strcmp(e, "1")));
}
bool device_input_jpeg(const Flags& F) {
  if (!F.s("bin_list").empty()) return false;
  if (F.given.count("device_input_jpeg")) return F.b("device_input_jpeg");
  const char* e = std::getenv("S360_DEVICE_INPUT_JPEG");
  return e && !std::strcmp(e, "1");
}
// --v 1: one line for the camera files, whichever of the two flags are on (the host count is of the files neither decoder took)
void report_input_paths(const Flags& F) {
  const bool p = device_input_png(F), j = device_input_jpeg(F);
  if (!p && !j) return;
  std::fprintf(stderr, "camera images:           %d files decoded on the device, %d on the host (%s)\n",
               (p ? g_inputOnDevice.load() : 0) + (j ? g_inputJpegOnDevice.load() : 0), g_inputOnHost.load(),
               p && j ? "--device_input_png --device_input_jpeg" : p ? "--device_input_png" : "--device_input_jpeg");
}
// which of the two a kept file is: JPEG files begin with SOI
bool is_jpeg_file(const std::vector<uint8_t>& f) { return f.size() >= 2 && f[0] == 0xFF && f[1] == 0xD8; }
std::vector<uint8_t> read_bytes(const std::string& path);
// One camera's image: with --device_input_png / --device_input_jpeg its file's bytes if that device decoder takes them as a
// 3-channel image (`file` keeps them, `im` gets the size only), else the pixels as the host decodes them.
void load_camera_image(bool devicePng, bool deviceJpeg, const std::string& path, pngio::Image& im, std::vector<uint8_t>& file) {
  file.clear();
  if (devicePng || deviceJpeg) {
    file = read_bytes(path);
    int info[6] = {0, 0, 0, 0, 0, 0};
    if (devicePng && s360_input_png_decodable(file.data(), file.size(), info) == S360_OK && info[2] == 3) {
      im.w = info[0]; im.h = info[1]; im.c = 3;  // (the size is known, e.g. to the pole-removal check; no pixels on the host)
      ++g_inputOnDevice;
      return;
    }
    if (deviceJpeg && s360_input_jpeg_decodable(file.data(), file.size(), info) == S360_OK) {
      im.w = info[0]; im.h = info[1]; im.c = 3;
      ++g_inputJpegOnDevice;
      return;
    }
    file.clear();
    ++g_inputOnHost;
  }
  load_png_into(path, false, im);
}

// `recycled`: the inputs of an earlier frame whose pixel buffers are reused (stream mode)
FrameInputs load_frame(const Job& J, const std::string& frame, FrameInputs recycled = FrameInputs()) {
  FrameInputs in = std::move(recycled);
  in.frame = frame;
  if (J.from_bins()) {  // the frames stay where they are (mmap); upload_frame sends their packed bytes
    char* end = nullptr;
    in.binFrame = std::strtol(frame.c_str(), &end, 10);
    if (end == frame.c_str() || *end || in.binFrame < 0) die("--bin_list: frame_number must be a frame index, got '" + frame + "'");
    return in;
  }
  in.side.resize(J.P);
  in.sideFile.resize(J.P);
  const bool dev = device_input_png(J.F), devJ = device_input_jpeg(J.F);
  const std::string imgs = J.F.s("imgs_dir");
  std::vector<std::thread> th;
  for (int k = 0; k < J.P; ++k)
    th.emplace_back([&, k] {
      const std::string dir = imgs + "/" + J.cams[J.sideIdx[k]].id;
      load_camera_image(dev, devJ, dir + "/" + frame + image_extension(dir), in.side[k], in.sideFile[k]);
    });
  if (J.prm.enable_top) th.emplace_back([&] { load_camera_image(dev, devJ, imgs + "/" + J.cams[J.ti].id + "/" + frame + ".png", in.top, in.topFile); });  // TRSP:652
  if (J.prm.enable_bottom) {
    th.emplace_back([&] { load_camera_image(dev, devJ, imgs + "/" + J.cams[J.bi].id + "/" + frame + ".png", in.bottom, in.bottomFile); });  // TRSP:602
    if (J.prm.enable_pole_removal)  // PoleRemoval.cpp:48-66 (the secondary camera's image; a camera file like the others)
      th.emplace_back([&] { load_camera_image(dev, devJ, imgs + "/" + J.cams[J.b2].id + "/" + frame + ".png", in.bottom2, in.bottom2File); });
  }
  for (auto& t : th) t.join();
  if (J.prm.enable_pole_removal) {
    const pngio::Image& im = in.bottom;
    const PoleMasks& pm = pole_masks(J);
    if (in.bottom2.w != im.w || in.bottom2.h != im.h || pm.m1.w != im.w || pm.m1.h != im.h || pm.m2.w != im.w || pm.m2.h != im.h) die(pole_mask_message(J));
  }
  return in;
}

// every GPU gets the side images its pairs touch and the pole images of its pole units (asynchronous: upload stream)
void upload_frame(const Job& J, const FrameInputs& in) {
  const int G = (int)J.ctx.size();
  if (J.from_bins()) {
    auto send = [&](const std::string& id, int camera) {
      const BinCamera& bc = J.binCam.at(id);
      const footage::Header& md = bc.file->md;
      const uint8_t* fr = nullptr;
      try {
        fr = bc.file->frame((size_t)in.binFrame, bc.cam);
      } catch (const std::exception& e) {
        die(e.what());
      }
      ck(s360_frame_upload_packed(J.ctx[0], bc.isp, camera, fr, (int)md.bitsPerPixel, (int)md.width, (int)md.height), J.ctx[0]);
    };
    for (int k = 0; k < J.P; ++k) send(J.cams[J.sideIdx[k]].id, k);
    if (J.prm.enable_top) send(J.cams[J.ti].id, S360_CAMERA_TOP);
    if (J.prm.enable_bottom) send(J.cams[J.bi].id, S360_CAMERA_BOTTOM);
    if (J.prm.enable_pole_removal) send(J.cams[J.b2].id, S360_CAMERA_BOTTOM2);
    return;
  }
  for (int r = 0; r < G; ++r) {
    std::vector<char> need(J.P, 0);
    for (int p = J.bounds[r]; p < J.bounds[r + 1]; ++p) need[p] = need[(p + 1) % J.P] = 1;
    // --device_input_png / --device_input_jpeg: the cameras of this GPU whose files the device decodes, in one call per kind
    // (synchronous; a damaged file dies here like a file the host decoder cannot read)
    std::vector<int> cams, camsJ;
    std::vector<const uint8_t*> files, filesJ;
    std::vector<size_t> bytes, bytesJ;
    auto by_file = [&](int camera, const std::vector<uint8_t>& f) {
      if (f.empty()) return false;
      const bool j = is_jpeg_file(f);
      (j ? camsJ : cams).push_back(camera); (j ? filesJ : files).push_back(f.data()); (j ? bytesJ : bytes).push_back(f.size());
      return true;
    };
    for (int k = 0; k < J.P; ++k)
      if (need[k] && !by_file(k, in.sideFile[k]))
        ck(s360_frame_upload_side(J.ctx[r], k, in.side[k].px.data(), in.side[k].w, in.side[k].h, in.side[k].c), J.ctx[r]);
    if (J.unitMask[r] & 3) by_file(S360_CAMERA_TOP, in.topFile);
    if (J.unitMask[r] & 12) by_file(S360_CAMERA_BOTTOM, in.bottomFile);
    if ((J.unitMask[r] & 12) && J.prm.enable_pole_removal) by_file(S360_CAMERA_BOTTOM2, in.bottom2File);
    if (!cams.empty()) ck(s360_frame_upload_png(J.ctx[r], (int)cams.size(), cams.data(), files.data(), bytes.data()), J.ctx[r]);
    if (!camsJ.empty()) ck(s360_frame_upload_jpeg(J.ctx[r], (int)camsJ.size(), camsJ.data(), filesJ.data(), bytesJ.data()), J.ctx[r]);
  }
  for (int r = 0; r < G; ++r) {  // the pole images go to the GPUs that run units of that pole
    s360_ctx* c = J.ctx[r];
    if ((J.unitMask[r] & 3) && in.topFile.empty()) ck(s360_frame_upload_top(c, in.top.px.data(), in.top.w, in.top.h), c);
    if (J.unitMask[r] & 12) {
      if (in.bottomFile.empty()) ck(s360_frame_upload_bottom(c, in.bottom.px.data(), in.bottom.w, in.bottom.h), c);
      if (J.prm.enable_pole_removal && in.bottom2File.empty()) ck(s360_frame_upload_bottom2(c, in.bottom2.px.data(), in.bottom2.w, in.bottom2.h), c);
    }
  }
}

const char* const kEyeNames[4] = {"top_left", "top_right", "bottom_left", "bottom_right"};

// fn(0) .. fn(n - 1) on up to `workers` threads (file reads / PNG codecs of the per-frame state: 68 files per frame)
template <class Fn>
void parallel_items(int n, int workers, Fn fn) {
  std::atomic<int> next(0);
  std::vector<std::thread> th;
  for (int w = 0; w < std::max(1, std::min(workers, n)); ++w)
    th.emplace_back([&] {
      for (int i = next++; i < n; i = next++) fn(i);
    });
  for (auto& t : th) t.join();
}
int state_workers() { return std::max(2, std::min(16, pngio::available_cpus())); }

// tasks pushed by one thread, run by a pool (the state files of a frame are coded and written while the next ones are fetched)
class TaskQueue {
 public:
  explicit TaskQueue(int workers) {
    for (int w = 0; w < std::max(1, workers); ++w)
      th_.emplace_back([this] {
        for (;;) {
          std::function<void()> t;
          {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return closed_ || !q_.empty(); });
            if (q_.empty()) return;
            t = std::move(q_.front());
            q_.pop_front();
          }
          t();
        }
      });
  }
  void push(std::function<void()> t) {
    { std::lock_guard<std::mutex> lk(mu_); q_.push_back(std::move(t)); }
    cv_.notify_one();
  }
  ~TaskQueue() {
    { std::lock_guard<std::mutex> lk(mu_); closed_ = true; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
 private:
  std::deque<std::function<void()>> q_;
  bool closed_ = false;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::thread> th_;
};

// fn(i) for i in [0, n) on a pool of threads in the background; wait(i) blocks until item i is done (the caller consumes the
// items in order while the later ones are still being produced)
class ItemPool {
 public:
  template <class Fn>
  ItemPool(int n, int workers, Fn fn) : done_(n) {
    for (auto& d : done_) d.store(false);
    for (int w = 0; w < std::max(1, std::min(workers, n)); ++w)
      th_.emplace_back([this, n, fn] {
        for (int i = next_++; i < n; i = next_++) {
          fn(i);
          { std::lock_guard<std::mutex> lk(mu_); done_[i].store(true); }
          cv_.notify_all();
        }
      });
  }
  void wait(int i) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return done_[i].load(); });
  }
  ~ItemPool() { for (auto& t : th_) t.join(); }
 private:
  std::vector<std::atomic<bool>> done_;
  std::atomic<int> next_{0};
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::thread> th_;
};

// previous frame's state from files (TRSP:215-235, 421-436), each pair to the GPU that renders it. The 68 files of an 8K frame
// (1.2 GB of flows, 0.9 GB of images behind their PNG coding) are read and decoded by a pool of threads — the reference reads
// them inside its per-pair / per-unit threads, TRSP:215-235 —, then handed to the library in order.
void load_prev_state_device(const Job& J, const std::string& prev);
bool device_state_read(const Flags& F);
void load_prev_state(const Job& J, const std::string& prev) {
  if (device_state_read(J.F)) return load_prev_state_device(J, prev);
  const s360_geometry& g = J.g;
  const std::string outData = J.F.s("output_data_dir");
  const std::string flowPrevDir = outData + "/flow/" + prev, imgPrevDir = outData + "/debug/" + prev + "/flow_images/";
  const size_t on = (size_t)g.overlap_image_width * g.cam_image_height;
  struct PairState { std::vector<float> fl, fr; pngio::Image L, R; };
  struct UnitState { std::vector<float> pf; pngio::Image S, Fi; bool on = false; };
  std::vector<PairState> pairs(J.P);
  UnitState units[4];
  for (int u = 0; u < 4; ++u) units[u].on = !((u < 2 && !J.prm.enable_top) || (u >= 2 && !J.prm.enable_bottom));
  // the pole units' files first (the largest: 85 MB images, 170 MB flows), then the pairs in the order they are handed over
  ItemPool pool(J.P + 4, state_workers(), [&](int it) {
    const int item = it < 4 ? J.P + it : it - 4;
    if (item < J.P) {
      const int i = item;
      PairState& ps = pairs[i];
      ps.fl.resize(on * 2);
      ps.fr.resize(on * 2);
      int w = 0, h = 0;
      if (s360_read_flow_from_file((flowPrevDir + "/flowLtoR_" + std::to_string(i) + ".bin").c_str(), ps.fl.data(), &w, &h, ps.fl.size()) < 0 ||
          w != g.overlap_image_width || h != g.cam_image_height)
        die("bad previous flow file for pair " + std::to_string(i) + ": " + s360_last_error(nullptr));
      if (s360_read_flow_from_file((flowPrevDir + "/flowRtoL_" + std::to_string(i) + ".bin").c_str(), ps.fr.data(), &w, &h, ps.fr.size()) < 0 ||
          w != g.overlap_image_width || h != g.cam_image_height)
        die("bad previous flow file for pair " + std::to_string(i) + ": " + s360_last_error(nullptr));
      ps.L = load_png(imgPrevDir + "/overlap_" + std::to_string(i) + "_L.png", true);
      ps.R = load_png(imgPrevDir + "/overlap_" + std::to_string(i) + "_R.png", true);
      if (ps.L.c != 4 || ps.R.c != 4 || ps.L.w != g.overlap_image_width || ps.L.h != g.cam_image_height || ps.R.w != ps.L.w || ps.R.h != ps.L.h)
        die("previous overlap images have the wrong size/channels");
    } else {
      const int u = item - J.P;
      UnitState& us = units[u];
      if (!us.on) return;
      const int rows = u < 2 ? g.top_rows : g.bottom_rows;
      us.pf.resize((size_t)J.extW * rows * 2);
      int w = 0, h = 0;
      if (s360_read_flow_from_file((flowPrevDir + "/flow_" + kEyeNames[u] + ".bin").c_str(), us.pf.data(), &w, &h, us.pf.size()) < 0 || w != J.extW || h != rows)
        die(std::string("bad previous pole flow file: ") + kEyeNames[u]);
      us.S = load_png(imgPrevDir + "/extendedSideSpherical_" + kEyeNames[u] + ".png", true);
      us.Fi = load_png(imgPrevDir + "/extendedFisheyeSpherical_" + kEyeNames[u] + ".png", true);
      if (us.S.c != 4 || us.Fi.c != 4 || us.S.w != J.extW || us.S.h != rows || us.Fi.w != J.extW || us.Fi.h != rows)
        die("previous extended pole images have the wrong size/channels");
    }
  });
  for (size_t r = 0; r < J.ctx.size(); ++r) {
    ck(s360_frame_set_partition(J.ctx[r], J.bounds[r], J.bounds[r + 1]), J.ctx[r]);
    for (int i = J.bounds[r]; i < J.bounds[r + 1]; ++i) {
      pool.wait(4 + i);  // (handed to the device while the later pairs are still being read)
      PairState& ps = pairs[i];
      ck(s360_frame_set_prev_side(J.ctx[r], i, ps.fl.data(), ps.fr.data(), ps.L.px.data(), ps.R.px.data()), J.ctx[r]);
      ps = PairState();
    }
  }
  if (J.prm.enable_pole_removal) {  // PoleRemoval.cpp:95-110
    s360_ctx* root = J.ctx[J.bottom_gpu()];  // the GPU that merges the bottom cameras
    int w = 0, h = 0;
    if (s360_read_flow_from_file((flowPrevDir + "/flow_bottom_secondary.bin").c_str(), nullptr, &w, &h, 0) < 0)
      die(std::string("bad previous flow file: flow_bottom_secondary.bin: ") + s360_last_error(nullptr));
    std::vector<float> pf((size_t)w * h * 2);
    if (s360_read_flow_from_file((flowPrevDir + "/flow_bottom_secondary.bin").c_str(), pf.data(), &w, &h, pf.size()) < 0)
      die(std::string("bad previous flow file: flow_bottom_secondary.bin: ") + s360_last_error(nullptr));
    const pngio::Image b1 = load_png(imgPrevDir + "/bottomImage.png", true), b2 = load_png(imgPrevDir + "/bottomImage2.png", true);
    if (b1.c != 4 || b2.c != 4 || b1.w != w || b1.h != h || b2.w != w || b2.h != h)
      die("previous bottomImage / bottomImage2 have the wrong size/channels");
    ck(s360_frame_set_prev_pole_removal(root, pf.data(), b1.px.data(), b2.px.data(), w, h), root);
  }
  for (int u = 0; u < 4; ++u) {
    UnitState& us = units[u];
    pool.wait(u);
    if (!us.on) continue;
    ck(s360_frame_set_prev_pole(J.owner_ctx(u), u, us.pf.data(), us.S.px.data(), us.Fi.px.data()), J.owner_ctx(u));  // a unit's state lives where it runs
    us = UnitState();
  }
}

// --device_state_read: the same state, its images decoded on the device. The image files are read as bytes (a pool of threads);
// those of a pair / pole unit / the pole removal whose files the device decoder takes go in ONE s360_frame_set_prev_images_png per
// context — a pair on the rank of its partition, a pole unit on its owner, the pole-removal images on the bottom GPU — while the
// pool reads the 1.2 GB of flow files (S360_STATE_READ_ORDER=batch, developer switch: the decode waits for them instead); the
// flows follow through s360_frame_set_prev_flow. A pair or unit with a file the decoder does not take goes the way of
// load_prev_state. A file the device finds damaged dies with the host reader's message.
struct PrevTimes { double files = 0, decode = 0, flows = 0; int onDevice = 0, onHost = 0; bool used = false; };  // seconds of the loading thread; images
PrevTimes g_prevTimes;
bool device_state_read(const Flags& F) {
  const char* e = std::getenv("S360_DEVICE_STATE_READ");
  return F.b("device_state_read") || (e && !std::strcmp(e, "1"));
}
std::vector<uint8_t> read_bytes(const std::string& path) {
  std::vector<uint8_t> b;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) die("failed to load image: " + path);
  if (std::fseek(f, 0, SEEK_END) == 0) {
    const long sz = std::ftell(f);
    std::rewind(f);
    if (sz > 0) {
      b.resize((size_t)sz);
      b.resize(std::fread(b.data(), 1, (size_t)sz, f));
    }
  }
  std::fclose(f);
  return b;
}
void load_prev_state_device(const Job& J, const std::string& prev) {
  const s360_geometry& g = J.g;
  const std::string outData = J.F.s("output_data_dir");
  const std::string flowPrevDir = outData + "/flow/" + prev, imgPrevDir = outData + "/debug/" + prev + "/flow_images/";
  const char* ord = std::getenv("S360_STATE_READ_ORDER");
  const bool overlap = !(ord && !std::strcmp(ord, "batch"));
  const bool pr = J.prm.enable_pole_removal;
  // groups: pairs 0..P-1, pole units P..P+3, pole removal P+4; every group's image files and flow files
  struct Img { std::string path, name; int idx = 0, group = 0; std::vector<uint8_t> bytes; int whc[3] = {0, 0, 0}; bool ours = false; };
  struct Flow { std::string path, name; int idx = 0, group = 0, w = 0, h = 0; std::vector<float> px; };
  std::vector<Img> imgs;
  std::vector<Flow> flows;
  auto add_img = [&](int group, const std::string& file, const char* name, int idx) {
    Img m; m.path = imgPrevDir + "/" + file; m.name = name; m.idx = idx; m.group = group;
    imgs.push_back(std::move(m));
  };
  auto add_flow = [&](int group, const std::string& file, const char* name, int idx, int w, int h) {
    Flow f; f.path = flowPrevDir + "/" + file; f.name = name; f.idx = idx; f.group = group; f.w = w; f.h = h;
    flows.push_back(std::move(f));
  };
  bool unitOn[4];
  for (int u = 0; u < 4; ++u) {  // (the largest files first)
    unitOn[u] = !((u < 2 && !J.prm.enable_top) || (u >= 2 && !J.prm.enable_bottom));
    if (!unitOn[u]) continue;
    add_img(J.P + u, std::string("extendedSideSpherical_") + kEyeNames[u] + ".png", "extended_side", u);
    add_img(J.P + u, std::string("extendedFisheyeSpherical_") + kEyeNames[u] + ".png", "extended_fisheye", u);
    add_flow(J.P + u, std::string("flow_") + kEyeNames[u] + ".bin", "flow_pole", u, J.extW, u < 2 ? g.top_rows : g.bottom_rows);
  }
  if (pr) {
    add_img(J.P + 4, "bottomImage.png", "bottom_image", 0);
    add_img(J.P + 4, "bottomImage2.png", "bottom_image2", 0);
    add_flow(J.P + 4, "flow_bottom_secondary.bin", "flow_bottom_secondary", 0, 0, 0);
  }
  for (int i = 0; i < J.P; ++i) {
    add_img(i, "overlap_" + std::to_string(i) + "_L.png", "overlap_l", i);
    add_img(i, "overlap_" + std::to_string(i) + "_R.png", "overlap_r", i);
    add_flow(i, "flowLtoR_" + std::to_string(i) + ".bin", "flow_l_to_r", i, g.overlap_image_width, g.cam_image_height);
    add_flow(i, "flowRtoL_" + std::to_string(i) + ".bin", "flow_r_to_l", i, g.overlap_image_width, g.cam_image_height);
  }
  const double t0 = now_sec();
  parallel_items((int)imgs.size(), state_workers(), [&](int k) {
    Img& m = imgs[k];
    m.bytes = read_bytes(m.path);
    int rows = 0;
    m.ours = s360_png_decodable(m.bytes.data(), m.bytes.size(), m.whc, &rows) == S360_OK;
  });
  auto read_flow = [&](int k) {
    Flow& f = flows[k];
    if (f.w == 0) {  // flow_bottom_secondary: its size is the file's (PoleRemoval.cpp:95-110)
      if (s360_read_flow_from_file(f.path.c_str(), nullptr, &f.w, &f.h, 0) < 0)
        die(std::string("bad previous flow file: flow_bottom_secondary.bin: ") + s360_last_error(nullptr));
      f.px.resize((size_t)f.w * f.h * 2);
      if (s360_read_flow_from_file(f.path.c_str(), f.px.data(), &f.w, &f.h, f.px.size()) < 0)
        die(std::string("bad previous flow file: flow_bottom_secondary.bin: ") + s360_last_error(nullptr));
      return;
    }
    f.px.resize((size_t)f.w * f.h * 2);
    int w = 0, h = 0;
    if (s360_read_flow_from_file(f.path.c_str(), f.px.data(), &w, &h, f.px.size()) < 0 || w != f.w || h != f.h) {
      if (f.group < J.P) die("bad previous flow file for pair " + std::to_string(f.idx) + ": " + s360_last_error(nullptr));
      die(std::string("bad previous pole flow file: ") + kEyeNames[f.idx]);
    }
  };
  const double t1 = now_sec();
  std::unique_ptr<ItemPool> flowPool;
  if (overlap) flowPool.reset(new ItemPool((int)flows.size(), state_workers(), read_flow));
  else parallel_items((int)flows.size(), state_workers(), read_flow);
  const double t2 = now_sec();
  // which groups go to the device decoder: every image of the group is a file it takes, of the size the state has
  std::vector<char> dev((size_t)J.P + 5, 1);
  for (const Img& m : imgs) {
    if (!m.ours) { dev[(size_t)m.group] = 0; continue; }
    if (m.group < J.P) {
      if (m.whc[2] != 4 || m.whc[0] != g.overlap_image_width || m.whc[1] != g.cam_image_height) die("previous overlap images have the wrong size/channels");
    } else if (m.group < J.P + 4) {
      const int rows = m.idx < 2 ? g.top_rows : g.bottom_rows;
      if (m.whc[2] != 4 || m.whc[0] != J.extW || m.whc[1] != rows) die("previous extended pole images have the wrong size/channels");
    }
  }
  if (pr && dev[(size_t)J.P + 4])  // PoleRemoval.cpp:95-110: the two images have the size of the flow between them
    for (size_t k = 0; k < flows.size(); ++k)
      if (flows[k].group == J.P + 4) {
        if (flowPool) flowPool->wait((int)k);
        for (const Img& m : imgs)
          if (m.group == J.P + 4 && (m.whc[2] != 4 || m.whc[0] != flows[k].w || m.whc[1] != flows[k].h))
            die("previous bottomImage / bottomImage2 have the wrong size/channels");
      }
  auto ctx_of = [&](int group) -> s360_ctx* {
    if (group < J.P) {
      for (size_t r = 0; r < J.ctx.size(); ++r)
        if (group >= J.bounds[r] && group < J.bounds[r + 1]) return J.ctx[r];
      return J.ctx[0];
    }
    return group < J.P + 4 ? J.owner_ctx(group - J.P) : J.ctx[J.bottom_gpu()];
  };
  for (size_t r = 0; r < J.ctx.size(); ++r) ck(s360_frame_set_partition(J.ctx[r], J.bounds[r], J.bounds[r + 1]), J.ctx[r]);
  for (s360_ctx* c : J.ctx) {  // one batched decode per context
    std::vector<const char*> names;
    std::vector<int> idx;
    std::vector<const uint8_t*> files;
    std::vector<size_t> bytes;
    std::vector<const Img*> which;
    for (const Img& m : imgs)
      if (dev[(size_t)m.group] && ctx_of(m.group) == c) {
        names.push_back(m.name.c_str()); idx.push_back(m.idx); files.push_back(m.bytes.data()); bytes.push_back(m.bytes.size());
        which.push_back(&m);
      }
    if (names.empty()) continue;
    if (s360_frame_set_prev_images_png(c, (int)names.size(), names.data(), idx.data(), files.data(), bytes.data()) != S360_OK) {
      const std::string e = s360_last_error(c);
      int image = -1, reason = S360_PNG_DECODE_FAILURE_NONE;
      (void)s360_png_decode_failure(c, &image, &reason);
      if (reason == S360_PNG_DECODE_FAILURE_DAMAGED && image >= 0 && (size_t)image < which.size())
        die("corrupt PNG data: " + which[(size_t)image]->path);  // (the host reader's message)
      die(e);
    }
  }
  const double t3 = now_sec();
  // the flows; and the groups that take the host path: their images through png_io.hpp, handed in by the calls of load_prev_state
  auto flow_of = [&](int group, const char* name) -> Flow& {
    for (size_t k = 0; k < flows.size(); ++k)
      if (flows[k].group == group && flows[k].name == name) {
        if (flowPool) flowPool->wait((int)k);
        return flows[k];
      }
    die("internal: no such flow");
    return flows[0];
  };
  auto host_decode = [&](int group, const char* name) -> pngio::Image {  // (the file's bytes are in memory already)
    for (const Img& m : imgs)
      if (m.group == group && m.name == name) {
        try {
          return jpegio::decode_any(m.bytes, m.path, true);
        } catch (const std::exception& e) {
          die(e.what());
        }
      }
    die("internal: no such image");
  };
  for (int grp = 0; grp < J.P + 5; ++grp) {
    if (grp >= J.P && grp < J.P + 4 && !unitOn[grp - J.P]) continue;
    if (grp == J.P + 4 && !pr) continue;
    s360_ctx* c = ctx_of(grp);
    if (dev[(size_t)grp]) {
      for (size_t k = 0; k < flows.size(); ++k)
        if (flows[k].group == grp) {
          if (flowPool) flowPool->wait((int)k);
          ck(s360_frame_set_prev_flow(c, flows[k].name.c_str(), flows[k].idx, flows[k].px.data()), c);
          std::vector<float>().swap(flows[k].px);
        }
      continue;
    }
    if (grp < J.P) {
      const pngio::Image L = host_decode(grp, "overlap_l"), R = host_decode(grp, "overlap_r");
      if (L.c != 4 || R.c != 4 || L.w != g.overlap_image_width || L.h != g.cam_image_height || R.w != L.w || R.h != L.h)
        die("previous overlap images have the wrong size/channels");
      ck(s360_frame_set_prev_side(c, grp, flow_of(grp, "flow_l_to_r").px.data(), flow_of(grp, "flow_r_to_l").px.data(), L.px.data(), R.px.data()), c);
    } else if (grp < J.P + 4) {
      const int u = grp - J.P, rows = u < 2 ? g.top_rows : g.bottom_rows;
      const pngio::Image S = host_decode(grp, "extended_side"), Fi = host_decode(grp, "extended_fisheye");
      if (S.c != 4 || Fi.c != 4 || S.w != J.extW || S.h != rows || Fi.w != J.extW || Fi.h != rows)
        die("previous extended pole images have the wrong size/channels");
      ck(s360_frame_set_prev_pole(c, u, flow_of(grp, "flow_pole").px.data(), S.px.data(), Fi.px.data()), c);
    } else {
      Flow& f = flow_of(grp, "flow_bottom_secondary");
      const pngio::Image b1 = host_decode(grp, "bottom_image"), b2 = host_decode(grp, "bottom_image2");
      if (b1.c != 4 || b2.c != 4 || b1.w != f.w || b1.h != f.h || b2.w != f.w || b2.h != f.h)
        die("previous bottomImage / bottomImage2 have the wrong size/channels");
      ck(s360_frame_set_prev_pole_removal(c, f.px.data(), b1.px.data(), b2.px.data(), f.w, f.h), c);
    }
  }
  const double t4 = now_sec();
  g_prevTimes.used = true;
  for (const Img& m : imgs) ++(dev[(size_t)m.group] ? g_prevTimes.onDevice : g_prevTimes.onHost);
  g_prevTimes.files += (t1 - t0) + (overlap ? 0.0 : t2 - t1);
  g_prevTimes.decode += t3 - t2;
  g_prevTimes.flows += t4 - t3;
}

// Enqueue one frame. One GPU: the whole frame on its stream. G GPUs (TRSP:320-385): every GPU renders its
// block of pairs, ONE grouped RCCL exchange hands the strips to the GPUs that assemble an eye (the root: both; the owner
// of a pole unit: its eye), the pole units run where assign_pole_units put them, a second grouped exchange returns their
// warped layers to the root, the root composites. One host thread per GPU for the collective calls (single-process RCCL).
void render_frame(const Job& J, bool usePrev) {
  const int G = (int)J.ctx.size();
  if (G == 1) {
    ck(s360_frame_render(J.ctx[0], usePrev ? 1 : 0), J.ctx[0]);
    return;
  }
  std::vector<std::thread> th;
  for (int r = 0; r < G; ++r)
    th.emplace_back([&, r] {
      s360_ctx* c = J.ctx[r];
      ck(s360_frame_render_pairs(c, J.bounds[r], J.bounds[r + 1], usePrev ? 1 : 0), c);
      ck(s360_frame_exchange_strips(c, J.bounds.data(), J.need.data()), c);  // exchange 1: strips to whoever assembles that eye
      if (J.unitMask[r] || r == 0) ck(s360_frame_pole_units(c, J.unitMask[r], usePrev ? 1 : 0), c);
      ck(s360_frame_gather_pole_layers(c, J.owner, 0), c);                    // exchange 2: warped pole layers to the root
      if (r == 0) ck(s360_frame_composite(c, 15), c);
    });
  for (auto& t : th) t.join();
}

// state for the next frame: always written by the reference (TRSP:201-208, 247-255, 413-416, 451-452). Fetched from the device
// in order, PNG-coded / written by a pool of threads (36 images and 32 flow files per 8K frame: 2 GB).
// --device_state_png: the images are encoded where they lie, one batched encode per context enqueued up front (a pair on the rank
// of its partition, a pole unit on its owner, the pole-removal images on the bottom GPU), and the pool only writes bytes.
struct StateTimes { double images = 0, flows = 0, writers = 0; };  // host-thread seconds: fetching images / flows, waiting for the pool
StateTimes g_stateTimes;
bool device_state_png(const Flags& F) {
  const char* e = std::getenv("S360_DEVICE_STATE_PNG");
  return F.b("device_state_png") || (e && !std::strcmp(e, "1"));
}
void write_state(const Job& J, const std::string& frame) {
  const std::string outData = J.F.s("output_data_dir");
  const std::string flowDir = outData + "/flow/" + frame, flowImagesDir = outData + "/debug/" + frame + "/flow_images";
  mkdirs(flowDir);
  mkdirs(flowImagesDir);
  const bool devState = device_state_png(J.F);
  double tImages = 0, tFlows = 0;
  struct Item {
    std::string path; std::vector<uint8_t> img; std::vector<float> fl; int w = 0, h = 0;
    std::unique_ptr<uint8_t[]> file; size_t fileBytes = 0;  // a finished file (its buffer has the file's BOUND and is not zero-filled: only the pages the file reaches are touched)
  };
  struct DevImage { s360_ctx* c; std::string what; int idx; std::string path; };
  std::vector<DevImage> devImages;  // (--device_state_png) in the order the images are asked for
  const double t00 = now_sec();
  auto coders = std::make_unique<TaskQueue>(state_workers());  // (joined before this function returns: every file is complete then)
  bool flowsNow = false;  // (get_flow: fetch now, do not defer)
  auto hand_over = [&](std::shared_ptr<Item> it) {
    coders->push([it] {
      if (it->file) {
        save_bytes(it->path, it->file.get(), it->fileBytes);
      } else if (!it->img.empty()) {
        try {
          // (the pool is the parallelism; only the pole units' 85 MB images get deflate threads of their own)
          pngio::write(it->path, it->img.data(), it->w, it->h, 4, 1, it->img.size() > ((size_t)32 << 20) ? 4 : 1);
        } catch (const std::exception& e) {
          die(e.what());
        }
      } else {
        ck(s360_save_flow_to_file(it->path.c_str(), it->fl.data(), it->w, it->h), nullptr);
      }
    });
  };
  auto get_img = [&](s360_ctx* c, const char* what, int idx, const std::string& path) {
    if (devState) { devImages.push_back({c, what, idx, path}); return; }
    const double t0 = now_sec();
    int whc[3];
    ck(s360_frame_get_u8(c, what, idx, whc, nullptr), c);
    auto it = std::make_shared<Item>();
    it->path = path; it->w = whc[0]; it->h = whc[1];
    it->img.resize((size_t)whc[0] * whc[1] * 4);
    ck(s360_frame_get_u8(c, what, idx, whc, it->img.data()), c);
    hand_over(std::move(it));
    tImages += now_sec() - t0;
  };
  struct DevFlow { s360_ctx* c; std::string what; int idx; std::string path; };
  std::vector<DevFlow> laterFlows;  // (--device_state_png) the flows follow the images: their fetch waits for the context's stream
  auto get_flow = [&](s360_ctx* c, const char* what, int idx, const std::string& path) {
    if (devState && !flowsNow) { laterFlows.push_back({c, what, idx, path}); return; }
    const double t0 = now_sec();
    struct Add { double& t; double t0; ~Add() { t += now_sec() - t0; } } add{tFlows, t0};
    int whc[3];
    ck(s360_frame_get_f32(c, what, idx, whc, nullptr), c);
    auto it = std::make_shared<Item>();
    it->path = path; it->w = whc[0]; it->h = whc[1];
    it->fl.resize((size_t)whc[0] * whc[1] * 2);
    ck(s360_frame_get_f32(c, what, idx, whc, it->fl.data()), c);
    hand_over(std::move(it));
  };
  // the pole units first: their images (85 MB each at 8K) take longest to code
  for (int u = 0; u < 4; ++u) {
    if ((u < 2 && !J.prm.enable_top) || (u >= 2 && !J.prm.enable_bottom)) continue;
    s360_ctx* root = J.owner_ctx(u);
    get_img(root, "extended_side", u, flowImagesDir + "/extendedSideSpherical_" + kEyeNames[u] + ".png");
    get_img(root, "extended_fisheye", u, flowImagesDir + "/extendedFisheyeSpherical_" + kEyeNames[u] + ".png");
    get_flow(root, "flow_pole", u, flowDir + "/flow_" + kEyeNames[u] + ".bin");
  }
  if (J.prm.enable_pole_removal) {  // PoleRemoval.cpp:118-126 (kSaveDataNextFrame, TRSP:581)
    s360_ctx* root = J.ctx[J.bottom_gpu()];
    get_img(root, "bottom_image", 0, flowImagesDir + "/bottomImage.png");
    get_img(root, "bottom_image2", 0, flowImagesDir + "/bottomImage2.png");
    get_flow(root, "flow_bottom_secondary", 0, flowDir + "/flow_bottom_secondary.bin");
  }
  for (size_t r = 0; r < J.ctx.size(); ++r) {
    s360_ctx* c = J.ctx[r];
    for (int i = J.bounds[r]; i < J.bounds[r + 1]; ++i) {
      get_img(c, "overlap_l", i, flowImagesDir + "/overlap_" + std::to_string(i) + "_L.png");
      get_img(c, "overlap_r", i, flowImagesDir + "/overlap_" + std::to_string(i) + "_R.png");
      get_flow(c, "flow_l_to_r", i, flowDir + "/flowLtoR_" + std::to_string(i) + ".bin");
      get_flow(c, "flow_r_to_l", i, flowDir + "/flowRtoL_" + std::to_string(i) + ".bin");
    }
  }
  if (devState) {
    const double t0 = now_sec();
    // one batched encode per context, all of them enqueued before the first file is fetched
    std::vector<s360_ctx*> ctxs;
    for (const DevImage& d : devImages)
      if (std::find(ctxs.begin(), ctxs.end(), d.c) == ctxs.end()) ctxs.push_back(d.c);
    std::vector<std::vector<size_t>> mine(ctxs.size());
    for (size_t k = 0; k < ctxs.size(); ++k) {
      std::vector<const char*> names;
      std::vector<int> idx;
      for (size_t j = 0; j < devImages.size(); ++j)
        if (devImages[j].c == ctxs[k]) { mine[k].push_back(j); names.push_back(devImages[j].what.c_str()); idx.push_back(devImages[j].idx); }
      ck(s360_frame_encode_state_pngs(ctxs[k], (int)names.size(), names.data(), idx.data()), ctxs[k]);
    }
    for (size_t k = 0; k < ctxs.size(); ++k)
      for (size_t i = 0; i < mine[k].size(); ++i) {
        auto it = std::make_shared<Item>();
        it->path = devImages[mine[k][i]].path;
        const size_t cap = s360_frame_state_png_bound(ctxs[k], (int)i);
        it->file.reset(new uint8_t[cap]);
        ck(s360_frame_download_state_png(ctxs[k], (int)i, it->file.get(), cap, &it->fileBytes), ctxs[k]);
        hand_over(std::move(it));
      }
    tImages += now_sec() - t0;
    flowsNow = true;
    for (const DevFlow& f : laterFlows) get_flow(f.c, f.what.c_str(), f.idx, f.path);
  }
  coders.reset();
  g_stateTimes.images += tImages;
  g_stateTimes.flows += tFlows;
  g_stateTimes.writers += now_sec() - t00 - tImages - tFlows;
}

// --save_debug_images: the reference's files under <output_data_dir>/debug/<frame>/ (TRSP:177-184, 548-560, 639-643, 680-684,
// 792-801, 896-911; PoleRemoval.cpp:148-153, 185-187), names and order from the library (include/s360_debug_images.h). The frame
// was rendered with s360_set_debug_images on. Directories are the caller's (batch_process_video.py:132-135): a missing one is the
// write error it is in the reference. Old projections/* files are removed first (TRSP:766-770). Default: the images' pixels come
// back raw and the pool of write_state's kind encodes them (png_io.hpp); --device_state_png (or its environment switch): they are
// encoded where they lie, ONE batched launch sequence for all of them (s360_frame_encode_debug_pngs), and the pool only writes bytes.
struct DebugTimes { int files = 0; size_t bytes = 0; double seconds = 0; bool device = false; };
DebugTimes g_debugTimes;
void write_debug_images(const Job& J, const std::string& frame) {
  const double t0 = now_sec();
  s360_ctx* c = J.ctx[0];
  const std::string debugDir = J.F.s("output_data_dir") + "/debug/" + frame;
  const std::string projDir = debugDir + "/projections";
  if (DIR* d = opendir(projDir.c_str())) {  // rm -f projections/*
    std::vector<std::string> old;
    while (dirent* e = readdir(d))
      if (std::strcmp(e->d_name, ".") && std::strcmp(e->d_name, "..")) old.push_back(e->d_name);
    closedir(d);
    for (const std::string& n : old) (void)unlink((projDir + "/" + n).c_str());
  }
  const int n = s360_frame_debug_image_count(c);
  ck(n, c);
  const bool dev = device_state_png(J.F);
  if (dev) ck(s360_frame_encode_debug_pngs(c), c);
  std::atomic<size_t> bytes(0);
  {
    TaskQueue coders(state_workers());  // (joined at the end of this block: every file is complete then)
    for (int i = 0; i < n; ++i) {
      char name[96];
      int whc[3];
      ck(s360_frame_debug_image_info(c, i, name, whc), c);
      const std::string path = debugDir + "/" + name;
      if (dev) {
        const size_t cap = s360_frame_debug_png_bound(c, i);
        std::shared_ptr<uint8_t> file(new uint8_t[cap], std::default_delete<uint8_t[]>());
        size_t nb = 0;
        ck(s360_frame_download_debug_png(c, i, file.get(), cap, &nb), c);
        coders.push([path, file, nb, &bytes] { save_bytes(path, file.get(), nb); bytes += nb; });
      } else {
        auto px = std::make_shared<std::vector<uint8_t>>((size_t)whc[0] * whc[1] * whc[2]);
        ck(s360_frame_get_debug_image(c, i, px->data()), c);
        const int w = whc[0], h = whc[1], ch = whc[2];
        coders.push([path, px, w, h, ch, &bytes] {
          save_png(path, px->data(), w, h, ch);
          struct stat st;
          if (stat(path.c_str(), &st) == 0) bytes += (size_t)st.st_size;
        });
      }
    }
  }
  g_debugTimes.files += n;
  g_debugTimes.bytes += bytes.load();
  g_debugTimes.seconds += now_sec() - t0;
  g_debugTimes.device = dev;
}

// "000123" + 1 -> "000124" (same width); frame names of the reference's datasets are zero-padded decimal numbers
std::string next_frame_name(const std::string& f) {
  char buf[64];
  std::snprintf(buf, sizeof buf, "%0*lld", (int)f.size(), std::atoll(f.c_str()) + 1);
  return buf;
}
// output path of one frame in stream mode: "%s" (or "{frame}") in the flag value is replaced by the frame name
std::string frame_path(const std::string& pattern, const std::string& frame) {
  std::string out = pattern;
  for (const char* key : {"%s", "{frame}"}) {
    const size_t at = out.find(key);
    if (at != std::string::npos) { out.replace(at, std::strlen(key), frame); return out; }
  }
  return out;
}

}  // namespace

// --bin_list: opens the containers, finds every camera's serial number (the second word of its frames), names the cameras
// like Unpacker (Unpacker.cpp:203-219: directories sorted by serial number become cam0, cam1, ...) and creates one ISP per
// rig camera from <isp_dir>/<serial>.json — the arithmetic Unpacker runs (CameraIspPipe at 16 bits; --soft_isp: CameraIsp).
static void open_bins(Job& J) {
  const Flags& F = J.F;
  if (J.ctx.size() != 1) die("--bin_list feeds one GPU (an ISP object feeds one context): not with --num_gpus");
  std::istringstream list(F.s("bin_list"));
  std::string path;
  std::map<uint32_t, std::pair<const footage::Footage*, size_t>> bySerial;
  try {
    while (std::getline(list, path, ',')) {
      std::unique_ptr<footage::Footage> ff(new footage::Footage);
      ff->path = path;
      ff->open(false);
      if (ff->md.numberOfCameras == 0) continue;
      if (ff->md.bitsPerPixel != 8 && ff->md.bitsPerPixel != 12) throw std::runtime_error("unsupported bits per pixel in " + path);
      for (size_t cam = 0; cam < ff->md.numberOfCameras; ++cam) {
        uint32_t serial;
        std::memcpy(&serial, ff->frame(0, cam) + 4, 4);
        bySerial[serial] = {ff.get(), cam};
      }
      J.bins.push_back(std::move(ff));
    }
  } catch (const std::exception& e) {
    die(e.what());
  }
  if (J.bins.empty()) die("--bin_list: no camera in " + F.s("bin_list"));
  size_t ordinal = 0;
  for (const auto& kv : bySerial) {
    BinCamera bc;
    bc.file = kv.second.first;
    bc.cam = kv.second.second;
    bc.serial = kv.first;
    J.binCam["cam" + std::to_string(ordinal++)] = bc;
  }
  auto want = [&](int idx) {
    const std::string id = J.cams[idx].id;
    auto it = J.binCam.find(id);
    if (it == J.binCam.end()) die("--bin_list: the containers hold " + std::to_string(J.binCam.size()) + " cameras, none becomes '" + id + "'");
    BinCamera& bc = it->second;
    if (bc.isp) return;
    const std::string json_path = F.s("isp_dir") + "/" + std::to_string(bc.serial) + ".json";
    std::ifstream js(json_path);
    if (!js) die("--bin_list: no ISP configuration " + json_path);
    std::stringstream ss;
    ss << js.rdbuf();
    s360_isp_config cfg;
    s360_isp_config_defaults(&cfg);
    cfg.output_bpp = 16;                  // kOutputBpp (Unpacker.cpp:167)
    cfg.pipe = F.b("soft_isp") ? 0 : 1;   // CameraIspPipe, kFast = false (Unpacker.cpp:166-168)
    if (s360_isp_config_from_json(ss.str().c_str(), &cfg) < 0) die(s360_last_error(nullptr));
    if (s360_isp_create(&bc.isp, F.i("device"), &cfg) < 0) die(s360_last_error(nullptr));
  };
  for (int k = 0; k < J.P; ++k) want(J.sideIdx[k]);
  if (J.prm.enable_top) want(J.ti);
  if (J.prm.enable_bottom) want(J.bi);
  if (J.prm.enable_pole_removal) want(J.b2);  // the secondary bottom camera: its container and ISP configuration too
}

// Flags -> rig, parameters, required arguments (TRSP:717-721): common to a job and to a batch of streams
static void init_job(Job& J, const Flags& flags) {
  J.F = flags;
  Flags& F = J.F;
  require_arg(F.s("rig_json_file"), "rig_json_file");  // TRSP:717-721
  if (F.s("bin_list").empty()) require_arg(F.s("imgs_dir"), "imgs_dir");
  else require_arg(F.s("isp_dir"), "isp_dir");
  require_arg(F.s("frame_number"), "frame_number");
  require_arg(F.s("output_data_dir"), "output_data_dir");
  require_arg(F.s("output_equirect_path"), "output_equirect_path");

  J.cams.resize(64);
  J.ncams = s360_rig_load_json(F.s("rig_json_file").c_str(), J.cams.data(), (int)J.cams.size());
  if (J.ncams < 0) die(s360_last_error(nullptr));
  J.cams.resize(J.ncams);
  for (int i = 0; i < J.ncams; ++i)
    if (J.cams[i].is_side) J.sideIdx.push_back(i);
  J.P = (int)J.sideIdx.size();

  s360_params& prm = J.prm;
  std::memset(&prm, 0, sizeof prm);
  prm.interpupilary_dist = F.d("interpupilary_dist");
  prm.zero_parallax_dist = F.d("zero_parallax_dist");
  prm.sharpening = F.d("sharpening");
  prm.side_alpha_feather_size = F.i("side_alpha_feather_size");
  prm.std_alpha_feather_size = F.i("std_alpha_feather_size");
  prm.enable_top = F.b("enable_top");
  prm.enable_bottom = F.b("enable_bottom");
  prm.eqr_width = F.i("eqr_width");
  prm.eqr_height = F.i("eqr_height");
  prm.final_eqr_width = F.i("final_eqr_width");
  prm.final_eqr_height = F.i("final_eqr_height");
  std::strncpy(prm.side_flow_alg, F.s("side_flow_alg").c_str(), sizeof(prm.side_flow_alg) - 1);
  std::strncpy(prm.polar_flow_alg, F.s("polar_flow_alg").c_str(), sizeof(prm.polar_flow_alg) - 1);
  prm.enable_pole_removal = F.b("enable_pole_removal") && F.b("enable_bottom");
  std::strncpy(prm.poleremoval_flow_alg, F.s("poleremoval_flow_alg").c_str(), sizeof(prm.poleremoval_flow_alg) - 1);
  if (prm.enable_pole_removal) require_arg(F.s("bottom_pole_masks_dir"), "bottom_pole_masks_dir");  // TRSP:571
  if (prm.enable_top && (J.ti = s360_rig_find_top(J.cams.data(), J.ncams)) < 0) die("no top camera in the rig");
  if (prm.enable_bottom && (J.bi = s360_rig_find_bottom(J.cams.data(), J.ncams)) < 0) die("no bottom camera in the rig");
  if (prm.enable_pole_removal) J.b2 = s360_rig_find_bottom2(J.cams.data(), J.ncams);
}

// One job = what one invocation of the reference's program does, or (--num_frames) one stream of consecutive frames.
static int run_job(const Flags& flags) {
  Job J;
  const double startTime = now_sec();
  init_job(J, flags);
  Flags& F = J.F;
  s360_params& prm = J.prm;
  const int verbose = F.i("v");
  const double rigTime = now_sec();
  // the first frame's 17 images are decoded (one thread per camera) while HIP starts up and the context is made: a process
  // per frame — how batch_process_video.py:29-62 runs the program — pays both for every frame
  std::string frame = F.s("frame_number");
  std::future<FrameInputs> firstDecode;
  if (F.s("bin_list").empty()) firstDecode = std::async(std::launch::async, [&J, frame] { return load_frame(J, frame); });

  // ---- GPUs: --num_gpus G uses devices device .. device+G-1 (never more GPUs than pairs)
  const int G = std::max(1, std::min(F.i("num_gpus"), J.P));
  const int numFrames = std::max(1, F.i("num_frames"));
  if (G > 1 && numFrames > 1) die("--num_gpus and --num_frames are separate modes (a stream keeps its temporal state on one GPU)");
  if (G > s360_device_count() - F.i("device")) die("--num_gpus: not that many HIP devices");
  J.ctx.resize(G, nullptr);
  for (int r = 0; r < G; ++r)
    if (s360_create(&J.ctx[r], F.i("device") + r, J.cams.data(), J.ncams, &prm) < 0) die(s360_last_error(nullptr));
  ck(s360_get_geometry(J.ctx[0], &J.g), J.ctx[0]);
  J.extW = int(float(prm.eqr_width) * 1.2f);
  J.bounds.assign(1, 0);
  for (int r = 0; r < G; ++r) J.bounds.push_back(J.bounds.back() + J.P / G + (r < J.P % G ? 1 : 0));  // 14 over 8 -> 2,2,2,2,2,2,1,1
  assign_pole_units(J);
  hand_pole_masks(J);
  if (G > 1) {
    if (s360_comm_init_all(J.ctx.data(), G) < 0) die(s360_last_error(nullptr));
    for (int r = 0; r < G; ++r) ck(s360_frame_set_partition(J.ctx[r], J.bounds[r], J.bounds[r + 1]), J.ctx[r]);
  }
  // --save_debug_images: every frame keeps the reference's debug images until they are written, so the frames of a stream are
  // rendered one at a time — no frame pipelining, frame k + 1 is enqueued when frame k's files are out (main refuses several GPUs)
  const bool debugImages = F.b("save_debug_images");
  if (debugImages) ck(s360_set_debug_images(J.ctx[0], 1), J.ctx[0]);
  if (numFrames > 1 && !debugImages) {
    ck(s360_set_frame_pipelining(J.ctx[0], 1), J.ctx[0]);  // pole stage of frame k overlaps side stage of k+1
  }
  if (!F.s("bin_list").empty()) open_bins(J);
  const s360_geometry& g = J.g;
  const std::string prev = F.s("prev_frame_data_dir");
  const bool cube = F.i("cubemap_width") > 0 && F.i("cubemap_height") > 0 && !F.s("output_cubemap_path").empty();
  const OutMode eqMode = out_mode(F, F.s("output_equirect_path")), cmMode = out_mode(F, F.s("output_cubemap_path"));
  // a stream leaves the cubemap of EVERY frame (the reference's caller asks for one beside every equirect,
  // batch_process_video.py:40-47): rendered with the frame, fetched and written beside its equirect; so does a single frame whose
  // cubemap the device encodes as a JPEG (the encoder sits behind the frame's last kernel)
  const bool cubeStream = cube && (numFrames > 1 || cmMode == OutMode::JpegDevice);
  enable_output_encoders(J.ctx[0], eqMode, cubeStream, cmMode);  // (the root composites and holds the output)
  if (verbose >= 1) report_output_paths(eqMode, cube, cubeStream || cmMode == OutMode::JpegHost ? cmMode : OutMode::PngHost);
  int cubeWhc[3] = {0, 0, 0};
  if (cubeStream) {
    ck(s360_set_cubemap_output(J.ctx[0], F.i("cubemap_width"), F.i("cubemap_height"), F.s("cubemap_format").c_str()), J.ctx[0]);
    ck(s360_frame_cubemap_size(J.ctx[0], cubeWhc), J.ctx[0]);
  }

  // ---- frame 0: decode, upload, previous-frame state from files, render
  const double ctxTime = now_sec();
  FrameInputs in = firstDecode.valid() ? firstDecode.get() : load_frame(J, frame);
  const double decodeTime = now_sec();
  upload_frame(J, in);
  const double loadTime = now_sec();
  if (prev != "NONE") load_prev_state(J, prev);
  const double renderStart = now_sec();
  render_frame(J, prev != "NONE");

  // Up to two finished frames are PNG-encoded and written while the next one renders (one encoder per frame, parallel
  // deflate inside it): an 8192 x 8192 file takes longer to encode and write than the frame takes to render.
  const size_t outBytes = output_buffer_bytes(J.ctx[0], eqMode, false, g.out_width, g.out_height);
  constexpr int kMaxEncoders = 4;
  const char* encEnv = std::getenv("S360_ENCODERS");  // (developer switch)
  const int kEncoders = std::max(1, std::min(kMaxEncoders, encEnv ? std::atoi(encEnv) : 3));
  // (page-locked in stream mode: the finished frame comes back in one DMA transfer instead of through the runtime's
  // staging buffers — 201 MB per 8K frame)
  pngio::Pixels outBuf[kMaxEncoders + 1];
  std::thread encoder[kMaxEncoders + 1];  // encoder[i] owns outBuf[i] while it runs
  for (int i = 0; i <= kEncoders; ++i) outBuf[i].resize(numFrames > 1 || i == 0 ? outBytes : 0);
  const size_t cubeBytes = !cubeStream ? 0 : output_buffer_bytes(J.ctx[0], cmMode, true, cubeWhc[0], cubeWhc[1]);
  pngio::Pixels cubeBuf[kMaxEncoders + 1];  // the frame's cubemap travels with its equirect: same fetch, same writer thread
  for (int i = 0; i <= kEncoders && cubeStream; ++i) cubeBuf[i].resize(cubeBytes);
  int cur = 0;  // the buffer the next download goes to
  double renderEnd = renderStart, stateEnd = renderStart;
  double tDecode = 0, tUpload = 0, tFetch = 0, tJoin = 0;  // where the host thread of a stream spends its time (--v 1)
  double tSteadyStart = 0;                                  // ... from its fourth frame on (the first ones build maps and buffers)
  int steadyFrames = 0;
  // A stream decodes ahead: the PNGs of up to three coming frames are read and decoded by threads of their own (17 per
  // frame) while this thread feeds and drains the GPU — decoding one 8K frame's inputs takes longer than rendering it.
  std::deque<std::future<FrameInputs>> decoding;
  std::string decodeCursor = frame;
  int decodesStarted = 0;
  std::vector<FrameInputs> spare;  // uploaded frames: their pixel buffers go to the next decodes
  std::vector<FrameInputs> leaving;  // enqueued uploads may still read these (page-locked buffers are sent in place)
  auto decode_ahead = [&] {
    while (decodesStarted < numFrames - 1 && decoding.size() < 3) {
      decodeCursor = next_frame_name(decodeCursor);
      auto recycled = std::make_shared<FrameInputs>();
      if (!spare.empty()) { *recycled = std::move(spare.back()); spare.pop_back(); }
      decoding.push_back(std::async(std::launch::async, [&J, name = decodeCursor, recycled] { return load_frame(J, name, std::move(*recycled)); }));
      ++decodesStarted;
    }
  };
  if (numFrames > 1) {
    // Page-locking memory costs ~0.4 ms per MB: the buffers of the frames that will be in flight (three decoding ahead, one
    // uploading, one whose uploads may still run) are made once, here, while the GPU works on frame 0 — not by the decoder
    // threads of the first frames one image at a time (they serialise on the runtime's allocation lock: measured, the host
    // thread of a 20-frame stream waited 71 ms per frame for its decoders).
    for (int i = 0; i < 4 && i < numFrames - 1; ++i) {
      FrameInputs fi;
      fi.side.resize(in.side.size());
      for (size_t k = 0; k < in.side.size(); ++k) fi.side[k].px.resize(in.side[k].px.size());
      fi.top.px.resize(in.top.px.size());
      fi.bottom.px.resize(in.bottom.px.size());
      fi.bottom2.px.resize(in.bottom2.px.size());
      spare.push_back(std::move(fi));
    }
  }
  decode_ahead();
  for (int k = 0; k < numFrames; ++k) {
    const bool last = k + 1 == numFrames;
    if (k == 3 && numFrames > 4) { tDecode = tUpload = tFetch = tJoin = 0; tSteadyStart = now_sec(); }
    if (k >= 3) ++steadyFrames;
    std::string nextName;
    auto feed_next = [&] {  // frame k+1
      nextName = next_frame_name(frame);
      const double t0 = now_sec();
      FrameInputs nin = decoding.front().get();
      decoding.pop_front();
      decode_ahead();
      const double t1 = now_sec();
      upload_frame(J, nin);     // upload stream: overlaps frame k
      render_frame(J, true);    // temporal state stays on the device
      leaving.push_back(std::move(nin));  // (sent in place: recycled once the uploads have run, below)
      tDecode += t1 - t0;
      tUpload += now_sec() - t1;
    };
    if (!last && !debugImages) feed_next();  // behind frame k: the GPU never waits for the host
    const double tf = now_sec();
    size_t pngBytes = 0;
    const int age = last || debugImages ? 0 : 1;  // the latest enqueued frame is k+1, except at the end and with --save_debug_images
    if (!is_file(eqMode) && last) ck(s360_frame_download_equirect(J.ctx[0], outBuf[cur].data()), J.ctx[0]);
    else fetch_output(J.ctx[0], eqMode, false, -1, age, outBuf[cur].data(), outBuf[cur].size(), &pngBytes);  // frame k, while k+1 renders
    size_t cubePngBytes = 0;
    if (cubeStream) fetch_output(J.ctx[0], cmMode, true, -1, age, cubeBuf[cur].data(), cubeBuf[cur].size(), &cubePngBytes);
    if (!leaving.empty()) {  // frame k is complete, so frame k+1's uploads (enqueued before it rendered) are long done
      ck(s360_frame_uploads_complete(J.ctx[0]), J.ctx[0]);
      for (auto& fi : leaving) spare.push_back(std::move(fi));
      leaving.clear();
    }
    renderEnd = now_sec();
    tFetch += renderEnd - tf;
    // (%s / {frame} in the path stands for the frame name — needed by streams, harmless for a single frame: a stream
    // segment of one frame is named like the others)
    const std::string outPath = frame_path(F.s("output_equirect_path"), frame);
    const uint8_t* px = outBuf[cur].data();
    const std::string cubePath = cubeStream ? frame_path(F.s("output_cubemap_path"), frame) : std::string();
    const uint8_t* cpx = cubeStream ? cubeBuf[cur].data() : nullptr;
    const int cw = cubeWhc[0], chh = cubeWhc[1];
    encoder[cur] = std::thread([=, &g] {
      write_output(eqMode, outPath, px, pngBytes, g.out_width, g.out_height);   // TRSP:961
      if (cpx) write_output(cmMode, cubePath, cpx, cubePngBytes, cw, chh);  // TRSP:935
    });
    // the reference writes the state of every frame; a stream only needs it to resume after its last frame. (Beside the
    // equirect's encoder, not in front of it.)
    if (F.b("write_state") && last) write_state(J, frame);
    if (debugImages) write_debug_images(J, frame);
    stateEnd = now_sec();
    if (last && cube && !cubeStream) {  // optional stereo cubemap (TRSP:917-935)
      int whc[3];
      ck(s360_frame_cubemap(J.ctx[0], F.i("cubemap_width"), F.i("cubemap_height"), F.s("cubemap_format").c_str(), whc, nullptr), J.ctx[0]);
      std::vector<uint8_t> cubeImg((size_t)whc[0] * whc[1] * 3);
      ck(s360_frame_cubemap(J.ctx[0], F.i("cubemap_width"), F.i("cubemap_height"), F.s("cubemap_format").c_str(), whc, cubeImg.data()), J.ctx[0]);
      // (a stream segment of one frame is named like the others; pixels in hand: the path's host encoder)
      write_output(cmMode == OutMode::JpegHost ? cmMode : OutMode::PngHost, frame_path(F.s("output_cubemap_path"), frame), cubeImg.data(), 0, whc[0], whc[1]);
    }
    cur = numFrames > 1 ? (cur + 1) % (kEncoders + 1) : 0;
    const double tj = now_sec();
    if (encoder[cur].joinable()) encoder[cur].join();  // the oldest encoder: its buffer takes the next frame
    if (last)
      for (auto& e : encoder)
        if (e.joinable()) e.join();
    tJoin += now_sec() - tj;
    if (!last && debugImages) feed_next();  // frame k's debug images are out: the next render may overwrite them
    frame = nextName;
  }
  const double endTime = now_sec();
  if (verbose >= 1) {  // the reference's VLOG(1) runtime breakdown, TRSP:964-971
    std::fprintf(stderr, "--- Runtime breakdown (sec) ---\n");
    std::fprintf(stderr, "load + decode + upload:  %.3f  (flags + rig %.3f, HIP start-up + context %.3f beside the PNG decodes, waiting for them %.3f, upload %.3f)\n",
                 loadTime - startTime, rigTime - startTime, ctxTime - rigTime, decodeTime - ctxTime, loadTime - decodeTime);
    if (g_prevTimes.used)
      std::fprintf(stderr, "previous-frame state:    %.3f  (reading the image files %.3f, device decode %.3f, flows %.3f; %d images decoded on the device, %d on the host)\n",
                   renderStart - loadTime, g_prevTimes.files, g_prevTimes.decode, g_prevTimes.flows, g_prevTimes.onDevice, g_prevTimes.onHost);
    else
      std::fprintf(stderr, "previous-frame state:    %.3f\n", renderStart - loadTime);
    if (numFrames == 1) {
      std::fprintf(stderr, "GPU render + download:   %.3f  (%d GPU%s)\n", renderEnd - renderStart, G, G > 1 ? "s, RCCL strip gather" : "");
      std::fprintf(stderr, "state files:             %.3f  (beside the equirect's PNG encoder)\n", stateEnd - renderEnd);
      std::fprintf(stderr, "state files, images:     %.3f  (%s)\n", g_stateTimes.images,
                   device_state_png(F) ? "encoded on the device, fetched as files" : "fetched raw, deflated by the writers");
      std::fprintf(stderr, "state files, flows:      %.3f  (fetched)\n", g_stateTimes.flows);
      std::fprintf(stderr, "state files, writers:    %.3f  (waiting for the pool to finish the files)\n", g_stateTimes.writers);
      std::fprintf(stderr, "equirect PNG encode:     %.3f  (what was left of it)\n", endTime - stateEnd);
    } else {
      std::fprintf(stderr, "stream of %d frames:      %.3f  (%.3f per frame: decode, upload, render, download, encode overlapped)\n",
                   numFrames, endTime - renderStart, (endTime - renderStart) / numFrames);
      const int nf = tSteadyStart > 0 ? steadyFrames : numFrames;
      const double per = tSteadyStart > 0 ? (endTime - tSteadyStart) / nf : (endTime - renderStart) / nf;
      std::fprintf(stderr, "host thread per frame:   decode %.3f  upload+enqueue %.3f  wait+fetch %.3f  wait for the encoder %.3f  other %.3f  of %.3f  (frames %d..%d; decode = waiting for the decode-ahead threads)\n",
                   tDecode / nf, tUpload / nf, tFetch / nf, tJoin / nf, per - (tDecode + tUpload + tFetch + tJoin) / nf, per,
                   numFrames - nf, numFrames - 1);
    }
    report_input_paths(F);
    if (debugImages)
      std::fprintf(stderr, "debug images:            %d files, %.1f MB, %.3f  (%s)\n", g_debugTimes.files, g_debugTimes.bytes / 1e6, g_debugTimes.seconds,
                   g_debugTimes.device ? "encoded on the device in one batch per frame, written as bytes" : "fetched raw, encoded by the writers");
    std::fprintf(stderr, "TOTAL:                   %.3f\n", endTime - startTime);
  }
  if (g_fast_exit) return 0;  // main leaves the process at once (one frame per process): the device memory goes with it
  for (auto& kv : J.binCam)
    if (kv.second.isp) s360_isp_destroy(kv.second.isp);
  for (s360_ctx* c : J.ctx) s360_destroy(c);
  return 0;
}

// --num_streams with more streams than GPUs: the streams that share a GPU are the FRAME SLOTS of one context there. Step k renders
// frame k of every stream that still has one as ONE launch sequence (s360_frame_render_slots): per-frame kernels slot by slot, the
// 28 side flows of every stream in one batch of the flow kernels, the 4 pole flows of every stream in another — each frame
// regularised toward its own stream's device-resident previous flows and images (TRSP:215-235, 421-436; PixFlow.h:101-118,
// 185-193). A single stream is bound by the latency of its pole flows' serial chain; S of them in one
// launch sequence share that chain's time. Every stream writes, file for file, what an invocation of its own with that segment's
// --frame_number / --num_frames writes: its equirects, and the state files behind its last frame.
// While step k renders, step k+1's images are decoded (one task per stream, one thread per camera inside it) and uploaded, and
// step k-1's equirects are PNG-encoded.
struct Segment { std::string first; int n = 0; std::string prev = "NONE"; };
static int run_stream_batch(const Flags& flags, const std::vector<Segment>& segs, int device) {
  Job J;
  const double startTime = now_sec();
  init_job(J, flags);
  Flags& F = J.F;
  const int verbose = F.i("v");
  const bool cube = F.i("cubemap_width") > 0 && F.i("cubemap_height") > 0 && !F.s("output_cubemap_path").empty();
  const int S = (int)segs.size();
  J.ctx.assign(1, nullptr);
  if (s360_create(&J.ctx[0], device, J.cams.data(), J.ncams, &J.prm) < 0) die(s360_last_error(nullptr));
  s360_ctx* ctx = J.ctx[0];
  ck(s360_get_geometry(ctx, &J.g), ctx);
  J.extW = int(float(J.prm.eqr_width) * 1.2f);
  J.bounds = {0, J.P};
  assign_pole_units(J);
  hand_pole_masks(J);
  ck(s360_set_frame_slots(ctx, S), ctx);
  ck(s360_set_output_double_buffer(ctx, 1), ctx);  // step k is fetched while step k+1 renders
  if (!F.s("bin_list").empty()) {  // every stream's frames straight from the capture's containers: no PNG is inflated
    F.v["device"] = std::to_string(device);  // (open_bins makes the ISP objects on the job's device)
    open_bins(J);
  }
  ck(s360_set_sweep_mode(ctx, "throughput"), ctx);  // many flows per launch: the kernel with the fewest instructions per pixel
  const s360_geometry& g = J.g;
  const OutMode eqMode = out_mode(F, F.s("output_equirect_path")), cmMode = out_mode(F, F.s("output_cubemap_path"));
  enable_output_encoders(ctx, eqMode, cube, cmMode);
  if (verbose >= 1) report_output_paths(eqMode, cube, cmMode);
  const size_t outBytes = output_buffer_bytes(ctx, eqMode, false, g.out_width, g.out_height);
  std::vector<size_t> pngBytes(S, 0);
  // the cubemap of every frame of every stream (batch_process_video.py:40-47), rendered for all slots of a step in one launch
  int cubeWhc[3] = {0, 0, 0};
  if (cube) {
    ck(s360_set_cubemap_output(ctx, F.i("cubemap_width"), F.i("cubemap_height"), F.s("cubemap_format").c_str()), ctx);
    ck(s360_frame_cubemap_size(ctx, cubeWhc), ctx);
  }
  const size_t cubeBytes = !cube ? 0 : output_buffer_bytes(ctx, cmMode, true, cubeWhc[0], cubeWhc[1]);
  std::vector<size_t> cubePngBytes(S, 0);
  std::vector<pngio::Pixels> cubeBuf(cube ? S : 0);
  for (auto& b : cubeBuf) b.resize(cubeBytes);

  int steps = 0;
  for (const Segment& sg : segs) steps = std::max(steps, sg.n);
  std::vector<std::string> name(S);  // the frame stream s renders in the current step
  for (int s = 0; s < S; ++s) name[s] = segs[s].first;
  std::vector<FrameInputs> cur(S), spare(S);
  std::vector<std::future<FrameInputs>> decoding(S);
  auto start_decode = [&](int k) {  // step k's frames
    for (int s = 0; s < S; ++s)
      if (k < segs[s].n) {
        auto recycled = std::make_shared<FrameInputs>(std::move(spare[s]));
        std::string nm = segs[s].first;
        for (int i = 0; i < k; ++i) nm = next_frame_name(nm);
        decoding[s] = std::async(std::launch::async, [&J, nm, recycled] { return load_frame(J, nm, std::move(*recycled)); });
      }
  };
  std::mutex selMu;
  auto upload_step = [&](int k, std::vector<FrameInputs>& into) {
    for (int s = 0; s < S; ++s)
      if (k < segs[s].n) {
        into[s] = decoding[s].get();
        std::lock_guard<std::mutex> sel(selMu);  // (slot selection is context state: the fetching thread selects too, for the state files)
        ck(s360_select_frame_slot(ctx, s), ctx);
        upload_frame(J, into[s]);
      }
  };
  auto render_step = [&](int k) {
    std::vector<int> resumed, rest;
    for (int s = 0; s < S; ++s)
      if (k < segs[s].n) (k == 0 && segs[s].prev != "NONE" ? resumed : rest).push_back(s);
    for (int s : resumed) {  // a stream whose first frame resumes from state files: that slot alone, with its state
      ck(s360_select_frame_slot(ctx, s), ctx);
      load_prev_state(J, segs[s].prev);
      ck(s360_frame_render_slots(ctx, &s, 1, 1), ctx);
    }
    if (!rest.empty()) ck(s360_frame_render_slots(ctx, rest.data(), (int)rest.size(), k > 0 ? 1 : 0), ctx);
  };
  std::vector<pngio::Pixels> outBuf(S);
  for (auto& b : outBuf) b.resize(outBytes);
  std::vector<std::thread> encoder(S);
  double tGpuWait = 0, tEncWait = 0, tDecWait = 0, tEnqueue = 0, tDrainWait = 0, tStep0 = 0;
  start_decode(0);
  std::vector<FrameInputs> next(S);
  upload_step(0, cur);
  render_step(0);
  start_decode(1);
  // Two host threads. THIS one feeds: step k+1 is uploaded and enqueued while step k renders — every slot has two output buffers
  // (s360_set_output_double_buffer), so the GPU goes from step k straight into step k+1. The OTHER one drains: it fetches step k's
  // frames (age 1: the slot's latest enqueued frame is k+1 by then) with the slot named, not selected, and hands them to the file
  // writers. (Measured on 8 streams from containers: fetch then enqueue on one thread 14 frames per second — the GPU idle for the
  // length of the fetch —, enqueue then fetch on one thread 31, the device renders 41.) Step k+1 is enqueued only when step k-1 has
  // been fetched: it composites into the buffers step k-1 left.
  std::mutex mu;
  std::condition_variable cv;
  int enqueued = 0, drained = -1;  // highest step enqueued / fetched
  std::thread drain([&] {
    for (int k = 0; k < steps; ++k) {
      const bool more = k + 1 < steps;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return enqueued >= std::min(k + 1, steps - 1); });
      }
      const double t1 = now_sec();
      for (auto& e : encoder)
        if (e.joinable()) e.join();  // step k-1's files are written: their buffers take step k's frames
      const double t2 = now_sec();
      tEncWait += t2 - t1;
      for (int s = 0; s < S; ++s)
        if (k < segs[s].n) {
          const int age = (more && k + 1 < segs[s].n) ? 1 : 0;  // the slot's latest enqueued frame is k+1 unless its stream has ended
          // (the first fetch of a step waits for the step)
          fetch_output(ctx, eqMode, false, s, age, outBuf[s].data(), outBuf[s].size(), &pngBytes[s]);
          if (cube) fetch_output(ctx, cmMode, true, s, age, cubeBuf[s].data(), cubeBuf[s].size(), &cubePngBytes[s]);
          if (F.b("write_state") && k + 1 == segs[s].n) {
            std::lock_guard<std::mutex> sel(selMu);
            ck(s360_select_frame_slot(ctx, s), ctx);
            write_state(J, name[s]);
          }
        }
      tGpuWait += now_sec() - t2;
      if (k == 0) tStep0 = now_sec();  // the first step's frames have arrived: the steady state is measured from here
      {
        std::lock_guard<std::mutex> lk(mu);
        drained = k;
      }
      cv.notify_all();
      for (int s = 0; s < S; ++s)
        if (k < segs[s].n) {
          const std::string outPath = frame_path(F.s("output_equirect_path"), name[s]);
          const uint8_t* px = outBuf[s].data();
          const size_t nb = pngBytes[s];
          const std::string cubePath = cube ? frame_path(F.s("output_cubemap_path"), name[s]) : std::string();
          const uint8_t* cpx = cube ? cubeBuf[s].data() : nullptr;
          const size_t cnb = cubePngBytes[s];
          const int cw = cubeWhc[0], chh = cubeWhc[1];
          encoder[s] = std::thread([=, &g] {
            write_output(eqMode, outPath, px, nb, g.out_width, g.out_height);
            if (cpx) write_output(cmMode, cubePath, cpx, cnb, cw, chh);
          });
          name[s] = next_frame_name(name[s]);
        }
    }
  });
  for (int k = 0; k < steps; ++k) {
    const bool more = k + 1 < steps;
    const double t0 = now_sec();
    if (more) upload_step(k + 1, next);  // (the uploads wait, on their own stream, for step k's projections)
    const double t1 = now_sec();
    tDecWait += t1 - t0;
    if (more) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return drained >= k - 1; });
      }
      const double t1a = now_sec();
      tDrainWait += t1a - t1;
      render_step(k + 1);
      {
        std::lock_guard<std::mutex> lk(mu);
        enqueued = k + 1;
      }
      cv.notify_all();
      tEnqueue += now_sec() - t1a;
      ck(s360_frame_uploads_complete(ctx), ctx);
    }
    for (int s = 0; s < S; ++s)
      if (k < segs[s].n) spare[s] = std::move(cur[s]);  // its uploads have run (s360_frame_uploads_complete of the previous round)
    std::swap(cur, next);
    if (k + 2 < steps) start_decode(k + 2);
  }
  drain.join();
  for (auto& e : encoder)
    if (e.joinable()) e.join();
  const double endTime = now_sec();
  if (verbose >= 1) {
    int frames = 0;
    for (const Segment& sg : segs) frames += sg.n;
    std::fprintf(stderr, "--- Runtime breakdown (sec) ---\n");
    std::fprintf(stderr, "%d streams as frame slots of one context, %d steps, %d frames: %.3f  (%.3f per frame)\n", S, steps, frames,
                 endTime - startTime, (endTime - startTime) / frames);
    std::fprintf(stderr, "host thread per step:    decode + upload %.3f  wait for the encoders %.3f  wait for the GPU + fetch %.3f  enqueue %.3f  wait for the fetching thread %.3f  (feeding thread: decode + upload, enqueue, wait for the fetching thread; fetching thread: the rest)\n",
                 tDecWait / steps, tEncWait / steps, tGpuWait / steps, tEnqueue / steps, tDrainWait / steps);
    int later = 0;  // frames of the steps behind the first one (which pays for maps, buffers and kernel loading)
    for (const Segment& sg : segs) later += std::max(0, sg.n - 1);
    if (later > 0 && endTime > tStep0)
      std::fprintf(stderr, "steady state:            %d frames of steps 1..%d in %.3f  (%.2f frames per second, files written)\n", later, steps - 1,
                   endTime - tStep0, later / (endTime - tStep0));
    report_input_paths(flags);
    std::fprintf(stderr, "TOTAL:                   %.3f\n", endTime - startTime);
  }
  for (auto& kv : J.binCam)
    if (kv.second.isp) s360_isp_destroy(kv.second.isp);
  s360_destroy(ctx);
  return 0;
}

int main(int argc, char** argv) {
  // glibc: keep freed blocks of up to 32 MB (decoded camera images, PNG scanline bands) in the heap instead of handing
  // every one back to the kernel — a stream's decoder and encoder threads would spend their time in page faults
  mallopt(M_MMAP_THRESHOLD, 32 << 20);
  mallopt(M_TRIM_THRESHOLD, 1 << 30);
  Flags F;
  F.parse(argc, argv);
  const int streams = std::max(1, F.i("num_streams")), frames = std::max(1, F.i("num_frames"));
  if (F.b("save_debug_images") && (streams > 1 || F.i("num_gpus") > 1))  // (before any GPU work)
    Flags::fail("--save_debug_images is not available with --num_streams or --num_gpus above 1: the images of one frame live on several contexts");
  if (frames > 1 && F.i("cubemap_width") > 0 && F.i("cubemap_height") > 0 && !F.s("output_cubemap_path").empty() &&
      frame_path(F.s("output_cubemap_path"), "0") == frame_path(F.s("output_cubemap_path"), "1"))
    die("--output_cubemap_path must contain %s or {frame} with --num_frames > 1: " + std::to_string(frames) +
        " frames would be written to one file, " + F.s("output_cubemap_path"));
  if (frames > 1) {
    const char* e = std::getenv("S360_PNG_THREADS");  // (developer switch)
    // three encoders and 51 decoder threads share the CPUs the process may use: half of them per encoder
    g_png_threads = e ? std::atoi(e) : std::max(2, pngio::available_cpus() / 2);
  }
  // (S360_HOST_PINNED=0: developer switch for timing the two ways against each other; the pixels do not depend on it)
  const char* pinEnv = std::getenv("S360_HOST_PINNED");
  if (frames > 1 && !(pinEnv && pinEnv[0] == '0')) {
    // a stream's decoders write into page-locked memory: the uploads are DMA transfers straight from the decoded images
    // (set once, before the first image exists; every pngio::Image of this process then lives in such memory)
    pngio::g_pixel_alloc = s360_host_alloc;
    pngio::g_pixel_free = s360_host_free;
  }
  if (streams == 1) {
    // One frame per process is how the reference's caller runs this program (batch_process_video.py:29-62). Every file is closed
    // and every device result fetched when run_job returns; freeing 12 GB of device memory buffer by buffer and unloading the
    // runtime only to exit costs ~0.2 s per frame, so run_job skips its destroy calls and the process leaves at once with
    // _exit — which runs no atexit handlers and no library destructors: S360_CLEAN_EXIT=1 tears down normally, and is what a
    // leak checker, rocprofv3 or any other tracer that flushes its output at exit needs.
    const char* ce = std::getenv("S360_CLEAN_EXIT");
    g_fast_exit = frames == 1 && !(ce && ce[0] == '1');
    const int rc = run_job(F);
    if (g_fast_exit) {
      std::fflush(nullptr);
      _exit(rc);
    }
    return rc;
  }
  if (F.i("num_gpus") > 1) die("--num_streams and --num_gpus are separate modes");
  if (streams > frames) die("--num_streams: more streams than frames");
  require_arg(F.s("frame_number"), "frame_number");
  const int devices = s360_device_count();
  if (devices < 1) die("no HIP device");
  // stream s = the s-th contiguous segment; streams go round the GPUs (--stream_gpus limits them); a GPU with one stream runs it
  // as a job (frame pipelining inside the stream), a GPU with several runs them as the frame slots of one context
  const int useDev = std::max(1, std::min(devices, F.i("stream_gpus") > 0 ? F.i("stream_gpus") : devices));
  std::vector<std::vector<Segment>> perDev(useDev);
  std::string first = F.s("frame_number");
  for (int s = 0; s < streams; ++s) {
    Segment sg;
    sg.first = first;
    sg.n = frames / streams + (s < frames % streams ? 1 : 0);
    sg.prev = s == 0 ? F.s("prev_frame_data_dir") : "NONE";
    perDev[s % useDev].push_back(sg);
    for (int k = 0; k < sg.n; ++k) first = next_frame_name(first);
  }
  const int perEncoder = std::max(1, (int)perDev[0].size());  // encoders running at once per GPU
  if (perEncoder > 1) g_png_threads = std::max(1, pngio::available_cpus() / std::min(perEncoder * useDev, 8));
  std::vector<std::thread> th;
  for (int d = 0; d < useDev; ++d) {
    const int dev = (F.i("device") + d) % devices;
    if (perDev[d].size() == 1) {
      Flags Fs = F;
      Fs.v["num_streams"] = "1";
      Fs.v["frame_number"] = perDev[d][0].first;
      Fs.v["num_frames"] = std::to_string(perDev[d][0].n);
      Fs.v["device"] = std::to_string(dev);
      Fs.v["prev_frame_data_dir"] = perDev[d][0].prev;
      th.emplace_back([Fs] { run_job(Fs); });  // (errors abort the process, like the reference's)
    } else if (!perDev[d].empty()) {
      th.emplace_back([&F, &perDev, d, dev] { run_stream_batch(F, perDev[d], dev); });
    }
  }
  for (auto& t : th) t.join();
  return 0;
}
