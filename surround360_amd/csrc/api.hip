// api.hip — the C ABI of libs360 (include/s360.h): lifecycle, rig, settings, the frame (uploads, render, previous state, getters),
// the sharded frame, profile, flow files. Thin: argument checks, host<->device copies, exception -> error-code translation
// (api_guard.hpp). No CPU fallback anywhere. The rest of the ABI by area: api_ops.hip (operators), api_png.hip (downloads and the
// PNG family), api_taps.hip (test taps), api_isp.hip (the soft ISP); preview.hip and jpeg.hip carry their objects' entry points.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <sstream>

#include "../../include/s360.h"
#include "api_internal.hpp"
#include "isp.hpp"

using namespace s360;

static thread_local std::string g_err;
namespace {
// live contexts by uid
std::mutex g_ctxMu;
std::vector<unsigned long long> g_ctxLive;
unsigned long long g_ctxNext = 0;
// buffers handed out by s360_host_alloc (page-locked host memory)
std::mutex g_pinMu;
std::vector<std::pair<const char*, size_t>> g_pinBlocks;
}  // namespace

// The sharded frame's split phases (exchange / pole units / gather / composite: comm.cpp) enqueue their RCCL calls on the
// main stream while frame pipelining runs the pole stage and the composite on the second one: nothing orders the two, so
// the combination is refused instead of racing (a stream keeps its temporal state on ONE GPU anyway: DESIGN.md section 7).
static void no_pipelining(s360_ctx* c) {
  if (c->pipeline) throw Error(S360_ERR_STATE, "the sharded (multi-GPU) frame is not available while frame pipelining is on (s360_set_frame_pipelining)");
}
namespace s360 {
// the calling thread's last error (api_guard.hpp)
void set_thread_error(const std::string& m) { g_err = m; }
bool context_alive(unsigned long long uid) {
  std::lock_guard<std::mutex> lk(g_ctxMu);
  return std::find(g_ctxLive.begin(), g_ctxLive.end(), uid) != g_ctxLive.end();
}
bool host_is_pinned(const void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pinMu);
  const char* q = static_cast<const char*>(p);
  for (const auto& b : g_pinBlocks)
    if (q >= b.first && q + bytes <= b.first + b.second) return true;
  return false;
}
// A non-zero snapshot of a finished frame is reported once: the engines' cumulative error words are reset, so that the frames
// enqueued from now on are judged on their own sweeps (frames already in flight carry the snapshot they took).
void check_sweep_error(s360_ctx* c, const unsigned* frame_words) {
  if (frame_words && !(frame_words[0] | frame_words[1] | frame_words[2])) return;
  unsigned e = 0;
  for (FlowEngine* f : {c->flow.get(), c->flow_pole.get(), c->flow_pr.get()})
    if (f) e |= f->take_error(c->st);
  if (e || frame_words) throw Error(S360_ERR_HIP, "banded sweep timed out waiting for a neighbour band (results invalid)");
}
// The previous-frame half of the double buffer is laid out like frame_render_pairs lays out the block [p0, p1) this context
// renders (s360_frame_set_partition; default all pairs): `pair` is pair j of that block.
PrevLayout prev_side_block(s360_ctx* c, FrameState& F, int pair, int& j) {
  need(pair >= 0 && pair < F.P, "pair_idx out of range");
  if (!F.partition_declared) { F.side_p0 = 0; F.side_p1 = F.P; }
  need(pair >= F.side_p0 && pair < F.side_p1, "pair_idx outside the block declared with s360_frame_set_partition");
  j = pair - F.side_p0;
  return PrevLayout(c, F.side_p0, F.side_p1);
}
// A set of previous-state halves is complete: mark the state as handed in, exactly as s360_frame_set_prev_side / _pole /
// _pole_removal leave it.
void prev_side_arrived(FrameState& F, int pair, unsigned bits) {
  if (F.prevSideGot.size() < (size_t)F.P) F.prevSideGot.resize((size_t)F.P, 0);
  unsigned char& g = F.prevSideGot[(size_t)pair];
  g |= (unsigned char)bits;
  if (g == 15) { g = 0; F.have_prev_side = true; }
}
void prev_pole_arrived(s360_ctx* c, FrameState& F, int unit, unsigned bits) {
  unsigned char& g = F.prevPoleGot[unit];
  g |= (unsigned char)bits;
  if (g == 7) {
    g = 0;
    PrevLayout(c).stamp_pole(F);
    F.have_prev_pole = true;
  }
}
void prev_pr_arrived(FrameState& F, unsigned bits) {
  F.prevPrGot |= (unsigned char)bits;
  if (F.prevPrGot == 7) { F.prevPrGot = 0; F.have_prev_pr = true; }
}
// Where the named 8-bit intermediate of the selected slot's latest frame lies on the device (the names of s360_frame_get_u8).
// `pack_eye`: eye_l / eye_r are packed to B,G,R into op_f (the caller wants their pixels, not only their size).
const void* frame_u8_source(s360_ctx* c, FrameState& F, const std::string& n, int idx, bool pack_eye, int& w, int& h, int& ch) {
  const s360_geometry& g = c->g;
  const int W = c->P.eqr_width, H = c->P.eqr_height, P = F.P;
  const void* src = nullptr;
  w = 0; h = 0; ch = 4;
  const PrevLayout L(c, F.side_p0, F.side_p1);
  if (n == "projection") {
    need(idx >= 0 && idx < P && F.sc->proj.p, "projection not available");
    w = g.cam_image_width; h = g.cam_image_height;
    src = F.sc->proj.as<uchar4>() + (size_t)w * h * idx;
  } else if (n == "overlap_l" || n == "overlap_r") {
    need(idx >= F.side_p0 && idx < F.side_p1 && F.overlaps[F.last_side].p, "overlap not available");
    w = g.overlap_image_width; h = g.cam_image_height;
    src = F.overlaps[F.last_side].as<uchar4>() + (n == "overlap_r" ? L.right(idx - L.p0) : L.left(idx - L.p0));
  } else if (n == "side_pano_l" || n == "side_pano_r") {
    const int e = n == "side_pano_r";
    need(F.panoDbg[e].p, "enable keep_intermediates before rendering");
    w = W; h = H; src = F.panoDbg[e].p;
  } else if (n == "top_spherical") {
    need(F.sc->topSph.p, "not available"); w = W; h = g.top_rows; src = F.sc->topSph.p;
  } else if (n == "bottom_spherical") {
    need(F.sc->botSph.p, "not available"); w = W; h = g.bottom_rows; src = F.sc->botSph.p;
  } else if (n == "pole_warped") {
    need(idx >= 0 && idx < 4 && F.sc->poleWarped[idx].p, "not available"); w = W; h = H; src = F.sc->poleWarped[idx].p;
  } else if (n == "extended_side" || n == "extended_fisheye") {
    need(idx >= 0 && idx < 4 && F.extImgs[F.last_pole].p, "not available");
    w = F.extW; h = idx < 2 ? F.poleRowsT : F.poleRowsB;
    src = F.extImgs[F.last_pole].as<uchar4>() + (n == "extended_side" ? L.side(idx) : L.fisheye(idx));
  } else if (n == "bottom_image" || n == "bottom_image2") {
    need(F.prImgs[F.last_pr].p && F.have_prev_pr, "not available (pole removal not run)");
    w = F.poleW; h = F.poleH;
    src = F.prImgs[F.last_pr].as<uchar4>() + (n == "bottom_image2" ? (size_t)w * h : 0);
  } else if (n == "eye_l" || n == "eye_r") {
    const int e = n == "eye_r";
    need(F.pano[e].p, "not available");
    w = W; h = H; ch = 3;
    if (pack_eye) {
      c->op_f.ensure((size_t)w * h * 3);
      wait_finish_stream(c);  // the pack kernel reads the composited panorama
      launch_pack_bgr(c->st, F.pano[e].as<uchar4>(), w, h, c->op_f.as<uint8_t>());
      src = c->op_f.p;
    }
  } else {
    throw Error(S360_ERR_INVALID_ARG, "unknown intermediate name: " + n);
  }
  return src;
}
}  // namespace s360

extern "C" {

const char* s360_version(void) { return "surround360_amd 0.1 (gfx950)"; }
int s360_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
const char* s360_last_error(const s360_ctx* ctx) {
  if (!ctx) return g_err.c_str();
  // a copy per calling thread: another thread's failing call may replace ctx->err at any time
  static thread_local std::string copy;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  copy = ctx->err;
  return copy.c_str();
}

// ---- rig -------------------------------------------------------------------------------------
int s360_rig_load_json(const char* path, s360_camera* cams, int max_cams) {
  int n = 0;
  const int rc = guard([&] {
    need(path && cams, "null argument");
    std::ifstream f(path);
    if (!f) throw Error(S360_ERR_IO, std::string("could not read JSON file: ") + path);
    std::stringstream ss;
    ss << f.rdbuf();
    std::vector<s360_camera> v = parse_rig_json(ss.str());
    need((int)v.size() <= max_cams, "rig has more cameras than max_cams");
    for (size_t i = 0; i < v.size(); ++i) cams[i] = v[i];
    n = (int)v.size();
  });
  return rc == S360_OK ? n : rc;
}
int s360_camera_init(s360_camera* out, int type, const double origin[3], const double forward[3], const double up[3],
                     const double right[3], const double resolution[2], const double* principal,
                     const double* distortion, const double focal[2], const double* fov, const char* group,
                     const char* id) {
  return guard([&] {
    need(out && origin && forward && up && right && resolution && focal, "null argument");
    need(type == S360_CAM_FTHETA || type == S360_CAM_RECTILINEAR, "bad camera type");
    std::memset(out, 0, sizeof(*out));
    out->type = type;
    if (id) std::strncpy(out->id, id, sizeof(out->id) - 1);
    for (int i = 0; i < 3; ++i) out->position[i] = origin[i];
    camera_set_rotation(out, forward, up, right);
    for (int i = 0; i < 2; ++i) {
      out->resolution[i] = resolution[i];
      out->principal[i] = principal ? principal[i] : resolution[i] / 2;
      out->distortion[i] = distortion ? distortion[i] : 0.0;
      out->focal[i] = focal[i];
    }
    if (fov) camera_set_fov(out, *fov); else camera_set_default_fov(out);
    out->is_side = (group && std::strstr(group, "side")) ? 1 : 0;
  });
}
void s360_camera_pixel(const s360_camera* cam, const double rig_point[3], double pixel_out[2]) {
  camera_pixel(cam, rig_point, pixel_out);
}
double s360_camera_get_fov(const s360_camera* cam) { return camera_get_fov(cam); }
static int find_dir(const s360_camera* cams, int n, double z) {
  Rig r;
  r.all.assign(cams, cams + n);
  const double d[3] = {0, 0, z};
  return r.find_by_direction(d);
}
int s360_rig_find_top(const s360_camera* cams, int n) { return find_dir(cams, n, 1.0); }
int s360_rig_find_bottom(const s360_camera* cams, int n) { return find_dir(cams, n, -1.0); }
int s360_rig_find_bottom2(const s360_camera* cams, int n) {
  if (!cams || n <= 0) return -1;
  Rig r;
  r.all.assign(cams, cams + n);
  return r.find_largest_axis_dist();
}
float s360_camera_usable_pixels_radius(const s360_camera* cam) { return cam ? approximate_usable_pixels_radius(cam) : 0.f; }

int s360_derive_geometry(const s360_camera* cams, int n_cams, const s360_params* params, s360_geometry* out) {
  return guard([&] {
    need(cams && params && out && n_cams > 0, "null argument");
    Rig r;
    r.all.assign(cams, cams + n_cams);
    r.finalize();
    need(!r.side.empty(), "rig has no side cameras");
    *out = derive_geometry(r, *params);
  });
}
int s360_pole_ramp(const s360_camera* cams, int n_cams, float out4[4]) {
  return guard([&] {
    need(cams && out4 && n_cams > 0, "null argument");
    Rig r;
    r.all.assign(cams, cams + n_cams);
    r.finalize();
    const double down[3] = {0, 0, -1};
    need(!r.side.empty() && r.find_by_direction(down) >= 0, "rig needs side cameras and a bottom camera");
    const PoleRamp p = pole_ramp(r);
    out4[0] = p.poleCameraRadius; out4[1] = p.phiRampStart; out4[2] = p.phiMid; out4[3] = p.phiRampEnd;
  });
}

// ---- context -----------------------------------------------------------------------------------
int s360_create(s360_ctx** out, int device, const s360_camera* cams, int n_cams, const s360_params* params) {
  if (!out) return S360_ERR_INVALID_ARG;
  *out = nullptr;
  s360_ctx* c = nullptr;
  const int rc = guard([&] {
    need(cams && params && n_cams > 0, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      throw Error(S360_ERR_NO_DEVICE, "no HIP device available (libs360 has no CPU path)");
    need(device >= 0 && device < ndev, "device index out of range");
    c = new s360_ctx;
    c->device = device;
    S360_HIP(hipSetDevice(device));
    S360_HIP(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    c->st_user = c->st;
    c->prof.st = c->st;
    c->rig.all.assign(cams, cams + n_cams);
    c->rig.finalize();
    need(!c->rig.side.empty(), "rig has no side cameras");  // RigDescription.cpp:27 CHECK_NE
    c->P = *params;
    pixflow_consts_by_name(c->P.side_flow_alg);   // validate early (throws S360_ERR_UNKNOWN_ALG)
    pixflow_consts_by_name(c->P.polar_flow_alg);
    if (c->P.enable_pole_removal && c->P.poleremoval_flow_alg[0]) pixflow_consts_by_name(c->P.poleremoval_flow_alg);
    c->g = derive_geometry(c->rig, c->P);
    const double up[3] = {0, 0, 1}, down[3] = {0, 0, -1};
    c->top_idx = c->rig.find_by_direction(up);
    c->bottom_idx = c->rig.find_by_direction(down);
    // Sizes no frame can have (the reference runs into OpenCV's assertions somewhere inside the frame, TRSP aborts):
    // every stage indexes pixels with 32-bit integers and sizes its buffers from these numbers. The operator-level
    // entry points (flows, remaps, blends) do not depend on them, so the context is still created; every s360_frame_*
    // call of such a context fails with this message (frame_guard).
    auto frame_needs = [&](bool ok, const char* what) {
      if (!ok && c->frame_invalid.empty()) c->frame_invalid = what;
    };
    frame_needs(c->P.eqr_width >= 1 && c->P.eqr_height >= 1 && c->P.eqr_width <= 65536 && c->P.eqr_height <= 65536,
                "eqr_width / eqr_height must be in 1..65536");
    frame_needs(c->P.final_eqr_width >= 0 && c->P.final_eqr_height >= 0 && c->P.final_eqr_width <= 65536 && c->P.final_eqr_height <= 65536,
                "final_eqr_width / final_eqr_height must be in 0..65536 (0 = no final resize)");
    frame_needs(c->g.cam_image_width >= 1 && c->g.cam_image_height >= 1 && c->g.overlap_image_width >= 1 && c->g.num_novel_views >= 1,
                "eqr_width / eqr_height too small for this rig: a side projection, its overlap or its strip would be empty");
    frame_needs(c->g.out_width >= 1 && c->g.out_height >= 2, "final_eqr_width / final_eqr_height leave no output pixels");
    {  // the flows of a frame run on overlap_image_width x cam_image_height and (eqr_width x 1.2) x pole rows images
      const PixFlowConsts ps = pixflow_consts_by_name(c->P.side_flow_alg), pp = pixflow_consts_by_name(c->P.polar_flow_alg);
      frame_needs(int(c->g.overlap_image_width * ps.downscaleFactor) >= 2 && int(c->g.cam_image_height * ps.downscaleFactor) >= 2,
                  "eqr_width / eqr_height too small for this rig: the side flows need overlap images of at least 2 x 2 pixels after the entry downscale");
      const int extW = extended_width(c->P.eqr_width);
      frame_needs(!c->P.enable_top || c->top_idx < 0 || (int(extW * pp.downscaleFactor) >= 2 && int(c->g.top_rows * pp.downscaleFactor) >= 2),
                  "eqr_width / eqr_height too small for this rig: the top pole flows need at least 2 x 2 pixels after the entry downscale");
      frame_needs(!c->P.enable_bottom || c->bottom_idx < 0 || (int(extW * pp.downscaleFactor) >= 2 && int(c->g.bottom_rows * pp.downscaleFactor) >= 2),
                  "eqr_width / eqr_height too small for this rig: the bottom pole flows need at least 2 x 2 pixels after the entry downscale");
    }
    if (c->bottom_idx >= 0) c->ramp = pole_ramp(c->rig);
    { c->flow.reset(new FlowEngine(&c->prof)); c->flow->set_sweep_mode(c->sweep_mode); }
  });
  if (rc != S360_OK) {
    delete c;
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_ctxMu);
    c->uid = ++g_ctxNext;
    g_ctxLive.push_back(c->uid);
  }
  *out = c;
  return S360_OK;
}
void s360_destroy(s360_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stUp) (void)hipStreamSynchronize(c->stUp);
  if (c->st) (void)hipStreamSynchronize(c->st);
  if (c->st2) (void)hipStreamSynchronize(c->st2);
  {  // (behind the waits: an ISP object bound to this context may be taken over by another one from here on)
    std::lock_guard<std::mutex> lk(g_ctxMu);
    g_ctxLive.erase(std::remove(g_ctxLive.begin(), g_ctxLive.end(), c->uid), g_ctxLive.end());
  }
  comm_destroy(c);
  c->slots.clear();
  c->slotScratch.reset();
  c->flow.reset();
  c->flow_pole.reset();
  c->flow_pr.reset();
  if (c->st) (void)hipStreamDestroy(c->st);
  if (c->st2) {
    (void)hipStreamDestroy(c->st2);
    (void)hipEventDestroy(c->evSideDone);
    (void)hipEventDestroy(c->evStripsFree);
  }
  if (c->evPoleSrcFree) (void)hipEventDestroy(c->evPoleSrcFree);
  if (c->stDown) (void)hipStreamDestroy(c->stDown);
  for (s360_ctx::PackedCache* pc : {&c->sidePk, &c->topPk, &c->botPk})
    for (auto& e : pc->e)
      if (e->ready) (void)hipEventDestroy(e->ready);
  if (c->evMaps) (void)hipEventDestroy(c->evMaps);
  if (c->evDown) (void)hipEventDestroy(c->evDown);
  for (s360_ctx::PngBatch* B : {&c->statePng, &c->opPng, &c->debugPng})
    if (B->events) { (void)hipEventDestroy(B->evEnc); (void)hipEventDestroy(B->evRead); (void)hipEventDestroy(B->evAfter); }
  if (c->evUpHost) (void)hipEventDestroy(c->evUpHost);
  if (c->stUp) {
    (void)hipStreamDestroy(c->stUp);
    (void)hipEventDestroy(c->evUploaded);
    (void)hipEventDestroy(c->evSideSrcFree);
    for (int i = 0; i < s360_ctx::kPinChunks; ++i) {
      if (c->pin[i]) (void)hipHostFree(c->pin[i]);
      if (c->pinEv[i]) (void)hipEventDestroy(c->pinEv[i]);
    }
  }
  delete c;
}
int s360_get_geometry(const s360_ctx* c, s360_geometry* out) {
  if (!c || !out) return S360_ERR_INVALID_ARG;
  *out = c->g;
  return S360_OK;
}
void* s360_stream(s360_ctx* c) { return c ? (void*)c->st_user : nullptr; }  // (immutable after s360_create: no lock needed)
int s360_synchronize(s360_ctx* c) {
  return guard(c, [&] {
    need(c, "null ctx");
    if (c->stUp) S360_HIP(hipStreamSynchronize(c->stUp));
    S360_HIP(hipStreamSynchronize(c->st));
    if (c->st2) S360_HIP(hipStreamSynchronize(c->st2));
    check_sweep_error(c);
  });
}
int s360_set_frame_pipelining(s360_ctx* c, int on) {
  return guard(c, [&] {
    need(c, "null ctx");
    if (on && c->debug_images) throw Error(S360_ERR_STATE, "frame pipelining is not available while s360_set_debug_images is on (frames are rendered one at a time)");
    c->make_current();
    S360_HIP(hipStreamSynchronize(c->st));
    if (c->st2) S360_HIP(hipStreamSynchronize(c->st2));
    if (on && !c->st2) {
      S360_HIP(hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking));
      S360_HIP(hipEventCreateWithFlags(&c->evSideDone, hipEventDisableTiming));
      S360_HIP(hipEventCreateWithFlags(&c->evStripsFree, hipEventDisableTiming));
      if (!c->evPoleSrcFree) S360_HIP(hipEventCreateWithFlags(&c->evPoleSrcFree, hipEventDisableTiming));
    }
    c->pipeline = on != 0;
    c->haveStripsFree = false;
    flow_engines_follow_pipelining(c);  // (the streams are idle: the finish stage's engines change buffer sets)
  });
}
int s360_set_output_double_buffer(s360_ctx* c, int on) {
  return guard(c, [&] {
    need(c, "null ctx");
    c->make_current();
    S360_HIP(hipStreamSynchronize(c->st));
    if (c->st2) S360_HIP(hipStreamSynchronize(c->st2));
    c->two_outputs = on != 0;
  });
}
int s360_set_sharpening(s360_ctx* c, double sharpening) {
  return guard(c, [&] {
    need(c && sharpening >= 0.0, "bad argument");
    c->P.sharpening = sharpening;  // read by the next frame_finish (TRSP:901-915)
  });
}
int s360_set_keep_intermediates(s360_ctx* c, int on) {
  return guard(c, [&] { need(c, "null ctx"); frame_state(c).keep_intermediates = on != 0; });
}

// ---- frame level ------------------------------------------------------------------------------------
int s360_frame_upload_side(s360_ctx* c, int side_idx, const uint8_t* img, int w, int h, int channels) {
  return frame_guard(c, [&] { need(c && img && w > 0 && h > 0, "bad argument"); frame_upload_side(c, side_idx, img, w, h, channels); });
}
int s360_frame_upload_top(s360_ctx* c, const uint8_t* bgr, int w, int h) {
  return frame_guard(c, [&] { need(c && bgr && w > 0 && h > 0, "bad argument"); frame_upload_pole(c, true, bgr, w, h); });
}
int s360_frame_upload_bottom(s360_ctx* c, const uint8_t* bgr, int w, int h) {
  return frame_guard(c, [&] { need(c && bgr && w > 0 && h > 0, "bad argument"); frame_upload_pole(c, false, bgr, w, h); });
}
int s360_frame_upload_raw(s360_ctx* c, s360_isp* isp, int camera, const uint16_t* raw16, int w, int h) {
  return frame_guard(c, [&] { need(c && isp && raw16 && w > 0 && h > 0, "bad argument"); frame_upload_raw(c, isp, camera, raw16, 16, w, h); });
}
int s360_frame_upload_packed(s360_ctx* c, s360_isp* isp, int camera, const uint8_t* frame, int bits, int w, int h) {
  return frame_guard(c, [&] {
    need(c && isp && frame && w > 0 && h > 0, "bad argument");
    need(bits == 8 || bits == 12, "packed frames are 8 or 12 bits per pixel");
    frame_upload_raw(c, isp, camera, frame, bits, w, h);
  });
}
int s360_frame_upload_pole_removal(s360_ctx* c, const uint8_t* bottom2, const uint8_t* mask, const uint8_t* mask2, int w,
                                   int h) {
  return frame_guard(c, [&] {
    need(c && bottom2 && mask && mask2 && w > 0 && h > 0, "bad argument");
    frame_upload_pole_removal(c, bottom2, mask, mask2, w, h);
  });
}
/* ---- include/s360_pole_inputs.h ---- */
int s360_frame_upload_bottom2(s360_ctx* c, const uint8_t* bgr, int w, int h) {
  return frame_guard(c, [&] { need(c && bgr && w > 0 && h > 0, "bad argument"); frame_upload_bottom2(c, bgr, w, h); });
}
int s360_set_pole_masks(s360_ctx* c, const uint8_t* mask, const uint8_t* mask2, int w, int h) {
  return frame_guard(c, [&] {
    need(c && ((mask && mask2 && w > 0 && h > 0) || (!mask && !mask2 && w == 0 && h == 0)), "bad argument");
    set_pole_masks(c, mask, mask2, w, h);
  });
}
int s360_frame_set_prev_pole_removal(s360_ctx* c, const float* flow, const uint8_t* bottom_image, const uint8_t* bottom_image2,
                                     int w, int h) {
  return frame_guard(c, [&] {
    need(c && flow && bottom_image && bottom_image2 && w > 0 && h > 0, "bad argument");
    FrameState& F = frame_state(c);
    const size_t n = (size_t)w * h;
    const int prv = F.last_pr;  // becomes "the previous frame" of the next render
    F.prImgs[prv].ensure(2 * n * sizeof(uchar4));
    F.prFlow[prv].ensure(n * sizeof(float2));
    h2d(c, F.prImgs[prv].as<uchar4>(), bottom_image, n * sizeof(uchar4));
    h2d(c, F.prImgs[prv].as<uchar4>() + n, bottom_image2, n * sizeof(uchar4));
    h2d(c, F.prFlow[prv].p, flow, n * sizeof(float2));
    S360_HIP(hipStreamSynchronize(c->st));
    F.have_prev_pr = true;
    F.prevPrGot = 0;  // (halves handed in through s360_frame_set_prev_images_png / _flow are superseded)
  });
}
int s360_frame_render_pairs(s360_ctx* c, int p0, int p1, int use_prev) {
  return frame_guard(c, [&] { need(c, "null ctx"); frame_render_pairs(c, p0, p1, use_prev); });
}
int s360_frame_finish(s360_ctx* c, int pole_mask, int use_prev) {
  return frame_guard(c, [&] { need(c, "null ctx"); frame_finish(c, pole_mask, use_prev); });
}
int s360_frame_render(s360_ctx* c, int use_prev) {
  return frame_guard(c, [&] {
    need(c, "null ctx");
    frame_render_pairs(c, 0, (int)c->rig.side.size(), use_prev);
    frame_finish(c, 15, use_prev);
  });
}
int s360_set_frame_slots(s360_ctx* c, int n) {
  return frame_guard(c, [&] { need(c, "null ctx"); set_frame_slots(c, n); });
}
int s360_select_frame_slot(s360_ctx* c, int k) {
  return frame_guard(c, [&] {
    need(c, "null ctx");
    need(k >= 0 && k < (int)std::max<size_t>(c->slots.size(), 1), "frame slot out of range");
    c->slot = k;
  });
}
int s360_frame_render_batch(s360_ctx* c, int use_prev) {
  return frame_guard(c, [&] { need(c, "null ctx"); frame_render_batch(c, use_prev); });
}
int s360_frame_render_slots(s360_ctx* c, const int* slots, int n, int use_prev) {
  return frame_guard(c, [&] {
    need(c && slots && n > 0, "bad argument");
    frame_render_slots(c, slots, n, use_prev);
  });
}
int s360_frame_set_prev_side(s360_ctx* c, int pair, const float* flow_l_to_r, const float* flow_r_to_l,
                             const uint8_t* overlap_l, const uint8_t* overlap_r) {
  return frame_guard(c, [&] {
    need(c && flow_l_to_r && flow_r_to_l && overlap_l && overlap_r, "bad argument");
    FrameState& F = frame_state(c);
    int j = 0;
    const PrevLayout L = prev_side_block(c, F, pair, j);
    const int prv = F.last_side;  // becomes "the previous frame" of the next render
    F.overlaps[prv].ensure(L.overlaps_bytes());
    F.sideFlows.ensure(L.side_flows_bytes());
    h2d(c, F.overlaps[prv].as<uchar4>() + L.left(j), overlap_l, L.on * sizeof(uchar4));
    h2d(c, F.overlaps[prv].as<uchar4>() + L.right(j), overlap_r, L.on * sizeof(uchar4));
    h2d(c, F.sideFlows.as<float2>() + L.left(j), flow_l_to_r, L.on * sizeof(float2));
    h2d(c, F.sideFlows.as<float2>() + L.right(j), flow_r_to_l, L.on * sizeof(float2));
    S360_HIP(hipStreamSynchronize(c->st));  // the caller's buffers may be reused as soon as this returns
    if ((size_t)pair < F.prevSideGot.size()) F.prevSideGot[(size_t)pair] = 0;  // (halves of this pair handed in as files are superseded)
    F.have_prev_side = true;
  });
}
int s360_frame_set_prev_pole(s360_ctx* c, int unit, const float* flow, const uint8_t* ext_side,
                             const uint8_t* ext_fisheye) {
  return frame_guard(c, [&] {
    need(c && flow && ext_side && ext_fisheye && unit >= 0 && unit < 4, "bad argument");
    FrameState& F = frame_state(c);
    const PrevLayout L(c);
    const size_t xn = L.unit_pixels(unit);  // one image / flow of this unit
    const int prv = F.last_pole;  // becomes "the previous frame" of the next render
    F.extImgs[prv].ensure(L.ext_bytes());
    F.poleFlows.ensure(L.pole_flows_bytes());
    h2d(c, F.extImgs[prv].as<uchar4>() + L.side(unit), ext_side, xn * sizeof(uchar4));
    h2d(c, F.extImgs[prv].as<uchar4>() + L.fisheye(unit), ext_fisheye, xn * sizeof(uchar4));
    h2d(c, F.poleFlows.as<float2>() + L.side(unit), flow, xn * sizeof(float2));
    S360_HIP(hipStreamSynchronize(c->st));  // the caller's buffers may be reused as soon as this returns
    L.stamp_pole(F);
    F.have_prev_pole = true;
    F.prevPoleGot[unit] = 0;  // (halves of this unit handed in as files are superseded)
  });
}
int s360_comm_get_unique_id(void* id_out) {
  return guard([&] { need(id_out, "null argument"); comm_unique_id(id_out); });
}
const char* s360_comm_library_path(void) {
  const char* p = nullptr;
  (void)guard([&] { p = comm_library_path(); });
  return p;
}
int s360_comm_init_rank(s360_ctx* c, const void* id, int rank, int nranks) {
  return guard(c, [&] { need(c && id, "null argument"); comm_init_rank(c, id, rank, nranks); });
}
int s360_comm_init_all(s360_ctx* const* ctxs, int n) {
  return guard([&] { need(ctxs && n > 0, "bad argument"); comm_init_all(ctxs, n); });
}
int s360_comm_destroy(s360_ctx* c) {
  return guard(c, [&] { need(c, "null ctx"); S360_HIP(hipStreamSynchronize(c->st)); comm_destroy(c); });
}
int s360_comm_size(s360_ctx* c) {
  int n = -1;
  (void)guard(c, [&] { need(c, "null ctx"); n = comm_size(c); });
  return n;
}
int s360_comm_rank(s360_ctx* c) {
  int r = -1;
  (void)guard(c, [&] { need(c, "null ctx"); r = comm_rank(c); });
  return r;
}
int s360_comm_stats(s360_ctx* c, int which, unsigned long long out[3]) {
  return guard(c, [&] {
    need(c && out, "null argument");
    need(which == 0 || which == 1, "which: 0 = strips exchange, 1 = pole-layer gather");
    out[0] = c->comm_stats[which].calls;
    out[1] = c->comm_stats[which].sent;
    out[2] = c->comm_stats[which].received;
  });
}
int s360_frame_gather_strips(s360_ctx* c, const int* bounds, int root) {
  return frame_guard(c, [&] { need(c && bounds, "null argument"); no_pipelining(c); frame_gather_strips(c, bounds, root); });
}
int s360_frame_exchange_strips(s360_ctx* c, const int* bounds, const int* need_mask) {
  return frame_guard(c, [&] { need(c && bounds && need_mask, "null argument"); no_pipelining(c); frame_exchange_strips(c, bounds, need_mask); });
}
int s360_frame_gather_pole_layers(s360_ctx* c, const int owner[4], int root) {
  return frame_guard(c, [&] { need(c && owner, "null argument"); no_pipelining(c); frame_gather_pole_layers(c, owner, root); });
}
int s360_frame_pole_units(s360_ctx* c, int pole_mask, int use_prev) {
  return frame_guard(c, [&] { need(c, "null ctx"); no_pipelining(c); frame_pole_units(c, pole_mask, use_prev); });
}
int s360_frame_composite(s360_ctx* c, int pole_mask) {
  return frame_guard(c, [&] { need(c, "null ctx"); no_pipelining(c); frame_composite(c, pole_mask); });
}
int s360_comm_loopback(s360_ctx* c, int src_pair, int dst_pair) {
  return guard(c, [&] { need(c, "null ctx"); comm_loopback(c, src_pair, dst_pair); });
}
int s360_frame_set_partition(s360_ctx* c, int p0, int p1) {
  return frame_guard(c, [&] {
    need(c, "null ctx");
    FrameState& F = frame_state(c);
    need(p0 >= 0 && p1 <= F.P && p0 <= p1, "bad pair range");
    if (F.side_p0 != p0 || F.side_p1 != p1) F.have_prev_side = false;  // state of another block is of no use
    F.side_p0 = p0;
    F.side_p1 = p1;
    F.partition_declared = true;
  });
}
int s360_frame_strip_ptr(s360_ctx* c, int eye, void** dev_ptr, size_t* bytes_per_pair) {
  return frame_guard(c, [&] {
    need(c && dev_ptr && (eye == 0 || eye == 1), "bad argument");
    FrameState& F = frame_state(c);
    const int P = F.P, camH = c->g.cam_image_height, stripW = c->P.eqr_width / P;
    const size_t per = (size_t)camH * stripW * sizeof(uchar4);
    F.strips.ensure(2 * P * per);
    *dev_ptr = F.strips.as<uint8_t>() + (size_t)eye * P * per;
    if (bytes_per_pair) *bytes_per_pair = per;
  });
}
int s360_frame_equirect_dev(s360_ctx* c, void** dev_ptr, size_t* bytes) {
  return frame_guard(c, [&] {
    need(c && dev_ptr, "bad argument");
    FrameState& F = frame_state(c);
    need(F.frames_done > 0, "no frame rendered yet");
    *dev_ptr = F.outBGR[F.out_cur].p;
    if (bytes) *bytes = (size_t)c->g.out_width * c->g.out_height * 3;
  });
}
int s360_frame_download_equirect(s360_ctx* c, uint8_t* out_bgr) {
  return frame_guard(c, [&] {
    need(c && out_bgr, "bad argument");
    FrameState& F = frame_state(c);
    need(F.frames_done > 0, "no frame rendered yet");
    d2h(c, out_bgr, F.outBGR[F.out_cur].p, (size_t)c->g.out_width * c->g.out_height * 3);
  });
}
/* ---- page-locked host buffers for streaming hosts ---- */
void* s360_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    g_err = "s360_host_alloc: hipHostMalloc failed";
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(g_pinMu);
  g_pinBlocks.emplace_back(static_cast<const char*>(p), bytes);
  return p;
}
void s360_host_free(void* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_pinMu);
    for (size_t i = 0; i < g_pinBlocks.size(); ++i)
      if (g_pinBlocks[i].first == p) { g_pinBlocks.erase(g_pinBlocks.begin() + i); break; }
  }
  (void)hipHostFree(p);
}
int s360_frame_uploads_complete(s360_ctx* c) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    if (!c->haveUploaded) return;
    if (!c->evUpHost) S360_HIP(hipEventCreateWithFlags(&c->evUpHost, hipEventDisableTiming | hipEventBlockingSync));
    S360_HIP(hipEventRecord(c->evUpHost, c->stUp));
    const hipEvent_t ev = c->evUpHost;
    lk.unlock();
    const hipError_t rc = hipEventSynchronize(ev);
    lk.lock();
    S360_HIP(rc);
  });
}

/* ---- the stereo cubemap of every frame (TRSP:917-935 for a stream or a batch) ---- */
static bool cubemap_is_video(const char* format) {
  const std::string f(format);
  if (f != "video" && f != "photo")  // CvUtil.cpp:134-137
    throw Error(S360_ERR_INVALID_ARG, "unexpected cubemap format: " + f + ". valid formats are: video,photo");
  return f == "video";
}
int s360_set_cubemap_output(s360_ctx* c, int face_w, int face_h, const char* format) {
  return frame_guard(c, [&] {
    need(c, "null ctx");
    if (face_w == 0 || face_h == 0) { c->cube_fw = c->cube_fh = 0; return; }
    need(format, "bad argument");
    const bool video = cubemap_is_video(format);
    need(face_w > 0 && face_h > 0 && face_w <= 16384 && face_h <= 16384, "cubemap face size must be in 1..16384 (0 = off)");
    (void)cube_maps(c, face_w, face_h, video);  // maps + prepared form now (a host wait), not inside a frame
    c->cube_fw = face_w; c->cube_fh = face_h; c->cube_video = video;
  });
}
int s360_frame_cubemap_size(s360_ctx* c, int whc[3]) {
  return guard(c, [&] {
    need(c && whc, "bad argument");
    if (c->cube_fw <= 0 || c->cube_fh <= 0) throw Error(S360_ERR_STATE, "the cubemap output is off (s360_set_cubemap_output)");
    whc[0] = c->cube_video ? 3 * c->cube_fw : c->cube_fw;
    whc[1] = c->cube_video ? 4 * c->cube_fh : 12 * c->cube_fh;
    whc[2] = 3;
  });
}
int s360_frame_cubemap(s360_ctx* c, int face_w, int face_h, const char* format, int whc[3], uint8_t* out_bgr) {
  return frame_guard(c, [&] {
    need(c && format && whc, "bad argument");
    const bool video = cubemap_is_video(format);
    need(face_w > 0 && face_h > 0 && face_w <= 16384 && face_h <= 16384, "cubemap face size must be in 1..16384");
    whc[0] = video ? 3 * face_w : face_w;
    whc[1] = video ? 4 * face_h : 12 * face_h;
    whc[2] = 3;
    if (!out_bgr) return;
    int ow = 0, oh = 0;
    wait_finish_stream(c);  // the cubemap kernel reads the composited panoramas
    frame_cubemap(c, face_w, face_h, video, &ow, &oh);
    d2h(c, out_bgr, frame_state(c).cubeOut.p, (size_t)ow * oh * 3);
  });
}
int s360_frame_get_u8(s360_ctx* c, const char* name, int idx, int whc[3], uint8_t* dst) {
  return frame_guard(c, [&] {
    need(c && name && whc, "bad argument");
    int w = 0, h = 0, ch = 4;
    const void* src = frame_u8_source(c, frame_state(c), name, idx, dst != nullptr, w, h, ch);
    whc[0] = w; whc[1] = h; whc[2] = ch;
    if (dst) d2h(c, dst, src, (size_t)w * h * ch);
  });
}
int s360_frame_set_prev_flow(s360_ctx* c, const char* name, int idx, const float* flow) {
  return frame_guard(c, [&] {
    need(c && name && flow, "bad argument");
    FrameState& F = frame_state(c);
    const std::string nm(name);
    if (nm == "flow_l_to_r" || nm == "flow_r_to_l") {
      int j = 0;
      const PrevLayout L = prev_side_block(c, F, idx, j);
      F.sideFlows.ensure(L.side_flows_bytes());
      h2d(c, F.sideFlows.as<float2>() + (nm == "flow_r_to_l" ? L.right(j) : L.left(j)), flow, L.on * sizeof(float2));
      S360_HIP(hipStreamSynchronize(c->st));
      prev_side_arrived(F, idx, nm == "flow_r_to_l" ? 8u : 4u);
    } else if (nm == "flow_pole") {
      need(idx >= 0 && idx < 4, "pole unit out of range");
      const PrevLayout L(c);
      F.poleFlows.ensure(L.pole_flows_bytes());
      h2d(c, F.poleFlows.as<float2>() + L.side(idx), flow, L.unit_pixels(idx) * sizeof(float2));
      S360_HIP(hipStreamSynchronize(c->st));
      prev_pole_arrived(c, F, idx, 4u);
    } else if (nm == "flow_bottom_secondary") {
      need(c->P.enable_pole_removal != 0, "this context does not run pole removal");
      const int w = F.prevPrW > 0 ? F.prevPrW : F.poleW, h = F.prevPrW > 0 ? F.prevPrH : F.poleH;
      if (w <= 0 || h <= 0) throw Error(S360_ERR_STATE, "flow_bottom_secondary: the bottom images' size is not known yet (hand bottom_image / bottom_image2 in first)");
      const size_t pn = (size_t)w * h;
      F.prFlow[F.last_pr].ensure(pn * sizeof(float2));
      h2d(c, F.prFlow[F.last_pr].p, flow, pn * sizeof(float2));
      S360_HIP(hipStreamSynchronize(c->st));
      prev_pr_arrived(F, 4u);
    } else {
      throw Error(S360_ERR_INVALID_ARG, "not a previous-state flow name: " + nm);
    }
  });
}
int s360_frame_get_f32(s360_ctx* c, const char* name, int idx, int whc[3], float* dst) {
  return frame_guard(c, [&] {
    need(c && name && whc, "bad argument");
    FrameState& F = frame_state(c);
    const s360_geometry& g = c->g;
    const std::string n(name);
    const void* src = nullptr;
    int w = 0, h = 0;
    const PrevLayout L(c, F.side_p0, F.side_p1);
    if (n == "flow_l_to_r" || n == "flow_r_to_l") {
      need(idx >= F.side_p0 && idx < F.side_p1 && F.sideFlows.p, "flow not available");
      w = g.overlap_image_width; h = g.cam_image_height;
      src = F.sideFlows.as<float2>() + (n == "flow_r_to_l" ? L.right(idx - L.p0) : L.left(idx - L.p0));
    } else if (n == "flow_bottom_secondary") {
      need(F.prFlow[F.last_pr].p && F.have_prev_pr, "not available (pole removal not run)");
      w = F.poleW; h = F.poleH;
      src = F.prFlow[F.last_pr].p;
    } else if (n == "flow_pole") {
      need(idx >= 0 && idx < 4 && F.poleFlows.p, "flow not available");
      w = F.extW; h = idx < 2 ? F.poleRowsT : F.poleRowsB;
      src = F.poleFlows.as<float2>() + L.side(idx);
    } else {
      throw Error(S360_ERR_INVALID_ARG, "unknown intermediate name: " + n);
    }
    whc[0] = w; whc[1] = h; whc[2] = 2;
    if (dst) d2h(c, dst, src, (size_t)w * h * sizeof(float2));
  });
}

int s360_set_sweep_mode(s360_ctx* c, const char* mode) {
  return guard(c, [&] {
    need(c && mode, "bad argument");
    const std::string m(mode);
    if (m == "latency") c->sweep_mode = 2;
    else if (m == "throughput") c->sweep_mode = 3;
    else throw Error(S360_ERR_INVALID_ARG, "sweep mode must be \"latency\" or \"throughput\"");
    if (c->flow) c->flow->set_sweep_mode(c->sweep_mode);
    if (c->flow_pole) c->flow_pole->set_sweep_mode(c->sweep_mode);
    if (c->flow_pr) c->flow_pr->set_sweep_mode(c->sweep_mode);
  });
}

// ---- measurement -----------------------------------------------------------------------------------
int s360_profile_enable(s360_ctx* c, int on) {
  return guard(c, [&] {
    need(c, "null ctx");
    S360_HIP(hipStreamSynchronize(c->st));
    c->prof.clear();
    c->prof.on = on != 0;
  });
}
int s360_profile_get(s360_ctx* c, char* names_out, size_t names_cap, float* ms_out, int* launches_out, int cap) {
  int n = 0;
  const int rc = guard(c, [&] {
    need(c && names_out && ms_out, "bad argument");
    std::vector<float> ms;
    std::vector<int> cnt;
    c->prof.collect(ms, cnt);
    std::string names;
    for (size_t i = 0; i < c->prof.names.size() && (int)i < cap; ++i) {
      if (i) names += ';';
      names += c->prof.names[i];
      ms_out[i] = ms[i];
      if (launches_out) launches_out[i] = cnt[i];
      n = (int)i + 1;
    }
    need(names.size() + 1 <= names_cap, "names buffer too small");
    std::memcpy(names_out, names.c_str(), names.size() + 1);
  });
  return rc == S360_OK ? n : rc;
}

// ---- flow state files (CvUtil.cpp:159-199) -----------------------------------------------------------
int s360_save_flow_to_file(const char* path, const float* flow, int w, int h) {
  return guard([&] {
    need(path && flow && w > 0 && h > 0, "bad argument");
    FILE* f = std::fopen(path, "wb");
    if (!f) throw Error(S360_ERR_IO, std::string("file not found: ") + path);
    const int rows = h, cols = w;
    bool ok = std::fwrite(&rows, sizeof(rows), 1, f) == 1 && std::fwrite(&cols, sizeof(cols), 1, f) == 1;
    ok = ok && std::fwrite(flow, sizeof(float) * 2, (size_t)w * h, f) == (size_t)w * h;
    std::fclose(f);
    if (!ok) throw Error(S360_ERR_IO, std::string("short write: ") + path);
  });
}
int s360_read_flow_from_file(const char* path, float* flow_out, int* w, int* h, size_t cap_floats) {
  return guard([&] {
    need(path && w && h, "bad argument");
    FILE* f = std::fopen(path, "rb");
    if (!f) throw Error(S360_ERR_IO, std::string("file not found: ") + path);
    int rows = 0, cols = 0;
    bool ok = std::fread(&rows, sizeof(rows), 1, f) == 1 && std::fread(&cols, sizeof(cols), 1, f) == 1;
    if (ok && rows > 0 && cols > 0) {
      *w = cols; *h = rows;
      if (flow_out) {
        const size_t n = (size_t)rows * cols * 2;
        if (n > cap_floats) { std::fclose(f); throw Error(S360_ERR_INVALID_ARG, "flow_out too small"); }
        ok = std::fread(flow_out, sizeof(float), n, f) == n;
      }
    } else ok = false;
    std::fclose(f);
    if (!ok) throw Error(S360_ERR_IO, std::string("bad flow file: ") + path);
  });
}


}  // extern "C"
