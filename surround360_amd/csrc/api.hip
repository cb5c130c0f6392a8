// api.hip — the C ABI of libs360 (include/s360.h). Thin: argument checks, host<->device copies for
// the operator-level calls, exception -> error-code translation. No CPU fallback anywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <sstream>

#include "../../include/s360.h"
#include "../../include/s360_debug.h"
#include "../../include/s360_debug_final_flow.h"
#include "../../include/s360_debug_flow_level.h"
#include "../../include/s360_debug_flow_pyramid.h"
#include "../../include/s360_debug_isp.h"
#include "../../include/s360_debug_cubemap.h"
#include "../../include/s360_debug_remap.h"
#include "ctx.hpp"
#include "isp.hpp"
#include "render.hpp"

using namespace s360;

static thread_local std::string g_err;
namespace s360 {
// for the objects whose entry points live in files of their own (preview.hip): the calling thread's last error
void set_thread_error(const std::string& m) { g_err = m; }
}  // namespace s360

// live contexts by uid
namespace {
std::mutex g_ctxMu;
std::vector<unsigned long long> g_ctxLive;
unsigned long long g_ctxNext = 0;
}  // namespace
namespace s360 {
bool context_alive(unsigned long long uid) {
  std::lock_guard<std::mutex> lk(g_ctxMu);
  return std::find(g_ctxLive.begin(), g_ctxLive.end(), uid) != g_ctxLive.end();
}
}  // namespace s360
// buffers handed out by s360_host_alloc (page-locked host memory)
namespace {
std::mutex g_pinMu;
std::vector<std::pair<const char*, size_t>> g_pinBlocks;
}  // namespace
namespace s360 {
bool host_is_pinned(const void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pinMu);
  const char* q = static_cast<const char*>(p);
  for (const auto& b : g_pinBlocks)
    if (q >= b.first && q + bytes <= b.first + b.second) return true;
  return false;
}
}  // namespace s360

template <typename F>
static int guard(s360_ctx* c, F&& f) {
  // thread-safe per context: concurrent callers of one context are serialised here
  std::unique_lock<std::recursive_mutex> lk;
  if (c) lk = std::unique_lock<std::recursive_mutex>(c->mu);
  try {
    if (c) c->make_current();
    f();
    return S360_OK;
  } catch (const Error& e) {
    (c ? c->err : g_err) = e.what();
    g_err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    (c ? c->err : g_err) = e.what();
    g_err = e.what();
    return S360_ERR_STATE;
  }
}
// Entry points that BLOCK on the device (a finished frame's download, waiting for uploads) give the context back while
// they wait: f receives the held lock and may unlock / relock it around the wait, so that another host thread can feed
// the next frame meanwhile (a stream's uploader beside the thread that fetches and encodes).
template <typename F>
static int guard_l(s360_ctx* c, F&& f, bool needs_frame = true /* false: operator-level calls work on a context whose flags describe no frame */) {
  std::unique_lock<std::recursive_mutex> lk(c->mu);
  try {
    c->make_current();
    if (needs_frame && !c->frame_invalid.empty()) throw Error(S360_ERR_INVALID_ARG, c->frame_invalid);
    f(lk);
    if (!lk.owns_lock()) lk.lock();
    return S360_OK;
  } catch (const Error& e) {
    if (!lk.owns_lock()) lk.lock();
    c->err = e.what();
    g_err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    if (!lk.owns_lock()) lk.lock();
    c->err = e.what();
    g_err = e.what();
    return S360_ERR_STATE;
  }
}
// s360_frame_* entry points: as guard, and refused when the context's flags describe no renderable frame (s360_create)
template <typename F>
static int frame_guard(s360_ctx* c, F&& f) {
  return guard(c, [&] {
    if (c && !c->frame_invalid.empty()) throw Error(S360_ERR_INVALID_ARG, c->frame_invalid);
    f();
  });
}
static void need(bool ok, const char* what) {
  if (!ok) throw Error(S360_ERR_INVALID_ARG, what);
}
// The sharded frame's split phases (exchange / pole units / gather / composite: comm.cpp) enqueue their RCCL calls on the
// main stream while frame pipelining runs the pole stage and the composite on the second one: nothing orders the two, so
// the combination is refused instead of racing (a stream keeps its temporal state on ONE GPU anyway: DESIGN.md section 7).
static void no_pipelining(s360_ctx* c) {
  if (c->pipeline) throw Error(S360_ERR_STATE, "the sharded (multi-GPU) frame is not available while frame pipelining is on (s360_set_frame_pipelining)");
}
static void h2d(s360_ctx* c, void* d, const void* h, size_t n) {
  S360_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->st));
}
static void check_sweep_error(s360_ctx* c) {
  unsigned e = 0;
  if (c->flow) e |= c->flow->take_error(c->st);
  if (c->flow_pole) e |= c->flow_pole->take_error(c->st);
  if (c->flow_pr) e |= c->flow_pr->take_error(c->st);
  if (e) throw Error(S360_ERR_HIP, "banded sweep timed out waiting for a neighbour band (results invalid)");
}
// Frame pipelining: frame_finish runs on st2. Anything enqueued on st that READS what frame_finish writes (panoramas,
// warped poles, extended pole images, the stacked equirect) must be ordered after it: the host waits for st2 first.
static void wait_finish_stream(s360_ctx* c) {
  if (c->st2) S360_HIP(hipStreamSynchronize(c->st2));
}
static void d2h(s360_ctx* c, void* h, const void* d, size_t n) {
  if (c->st2) S360_HIP(hipStreamSynchronize(c->st2));  // frame pipelining: the data may come from the finish stream
  S360_HIP(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->st));
  S360_HIP(hipStreamSynchronize(c->st));
  check_sweep_error(c);
}

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
  const int rc = guard(nullptr, [&] {
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
  return guard(nullptr, [&] {
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
  return guard(nullptr, [&] {
    need(cams && params && out && n_cams > 0, "null argument");
    Rig r;
    r.all.assign(cams, cams + n_cams);
    r.finalize();
    need(!r.side.empty(), "rig has no side cameras");
    *out = derive_geometry(r, *params);
  });
}
int s360_pole_ramp(const s360_camera* cams, int n_cams, float out4[4]) {
  return guard(nullptr, [&] {
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
  const int rc = guard(nullptr, [&] {
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
      const int extW = int(float(c->P.eqr_width) * 1.2f);
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
  if (c->downErr) (void)hipHostFree(c->downErr);
  if (c->pngMetaHost) (void)hipHostFree(c->pngMetaHost);
  for (s360_ctx::PngBatch* B : {&c->statePng, &c->opPng}) {
    if (B->tabHost) (void)hipHostFree(B->tabHost);
    if (B->metaHost) (void)hipHostFree(B->metaHost);
    if (B->events) { (void)hipEventDestroy(B->evEnc); (void)hipEventDestroy(B->evRead); (void)hipEventDestroy(B->evAfter); }
  }
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

// ---- operator level ------------------------------------------------------------------------------
int s360_compute_optical_flow_batch(s360_ctx* c, const char* alg, int batch, const uint8_t* i0, const uint8_t* i1,
                                    int w, int h, const float* prev_flow, const uint8_t* prev_i0,
                                    const uint8_t* prev_i1, int hint, float* flow_out) {
  return guard(c, [&] {
    need(c && alg && i0 && i1 && flow_out, "null argument");
    need(w >= 4 && h >= 4, "image too small: the reference's bilinear taps need a 2x2 image after the x0.5 entry downscale (PixFlow.h:457-475)");
    need(batch >= 1 && batch <= kMaxFlows, "batch out of range");
    need(hint >= 0 && hint <= 4, "bad direction hint");
    need(!prev_flow || (prev_i0 && prev_i1), "prev_flow given without previous images");
    const PixFlowConsts pc = pixflow_consts_by_name(alg);
    const size_t n = (size_t)w * h, B = batch;
    c->op_a.ensure(2 * B * n * 4);
    c->op_b.ensure(B * n * sizeof(float2));
    h2d(c, c->op_a.p, i0, B * n * 4);
    h2d(c, c->op_a.as<uint8_t>() + B * n * 4, i1, B * n * 4);
    const uchar4* pimg = nullptr;
    const float2* pflow = nullptr;
    if (prev_flow) {
      c->op_c.ensure(2 * B * n * 4);
      c->op_d.ensure(B * n * sizeof(float2));
      h2d(c, c->op_c.p, prev_i0, B * n * 4);
      h2d(c, c->op_c.as<uint8_t>() + B * n * 4, prev_i1, B * n * 4);
      h2d(c, c->op_d.p, prev_flow, B * n * sizeof(float2));
      pimg = c->op_c.as<uchar4>();
      pflow = c->op_d.as<float2>();
    }
    FlowBatch fb;
    fb.add_images(c->op_a.as<uchar4>(), 2 * batch, n);
    if (pimg) fb.add_prev_images(pimg, 2 * batch, n);
    for (int b = 0; b < batch; ++b) fb.add_flow(b, batch + b, c->op_b.as<float2>() + n * b, pflow ? pflow + n * b : nullptr);
    c->flow->compute(c->st, pc, fb, w, h, hint);
    d2h(c, flow_out, c->op_b.p, B * n * sizeof(float2));
  });
}
int s360_compute_optical_flow(s360_ctx* c, const char* alg, const uint8_t* i0, const uint8_t* i1, int w, int h,
                              const float* prev_flow, const uint8_t* prev_i0, const uint8_t* prev_i1, int hint,
                              float* flow_out) {
  return s360_compute_optical_flow_batch(c, alg, 1, i0, i1, w, h, prev_flow, prev_i0, prev_i1, hint, flow_out);
}
// test tap: flow after every pyramid level (coarsest first) of the last single-pair call configuration
int s360_debug_flow_levels(s360_ctx* c, const char* alg, const uint8_t* i0, const uint8_t* i1, int w, int h, int hint,
                           float* levels_out, size_t cap_floats, int* n_levels) {
  return guard(c, [&] {
    need(c && alg && i0 && i1 && levels_out, "null argument");
    const PixFlowConsts pc = pixflow_consts_by_name(alg);
    const size_t n = (size_t)w * h;
    c->op_a.ensure(2 * n * 4);
    c->op_b.ensure(n * sizeof(float2));
    h2d(c, c->op_a.p, i0, n * 4);
    h2d(c, c->op_a.as<uint8_t>() + n * 4, i1, n * 4);
    FlowBatch fb;
    fb.add_images(c->op_a.as<uchar4>(), 2, n);
    fb.add_flow(0, 1, c->op_b.as<float2>());
    std::vector<std::vector<float>> lv;
    c->flow->capture_levels = &lv;
    try {
      c->flow->compute(c->st, pc, fb, w, h, hint);
    } catch (...) {
      c->flow->capture_levels = nullptr;
      throw;
    }
    c->flow->capture_levels = nullptr;
    S360_HIP(hipStreamSynchronize(c->st));
    size_t off = 0;
    for (auto& v : lv) {
      need(off + v.size() <= cap_floats, "levels_out too small");
      std::memcpy(levels_out + off, v.data(), v.size() * sizeof(float));
      off += v.size();
    }
    if (n_levels) *n_levels = (int)lv.size();
  });
}
// test tap: PixFlow's entry (downscale, grey and alpha planes) alone on caller-made images of any size
int s360_debug_entry_downscale(s360_ctx* c, const uint8_t* src, int sw, int sh, int batch, int dw, int dh, int generic,
                               uint8_t* down_out, float* gray_out, float* alpha_out, int* tiled) {
  return guard(c, [&] {
    need(c && src && gray_out && alpha_out, "null argument");
    need(sw > 0 && sh > 0 && dw > 0 && dh > 0 && batch >= 1 && batch <= kMaxFlows, "bad size");
    need(!generic || down_out, "the generic pair always stores the image");
    const size_t ns = (size_t)sw * sh, nd = (size_t)dw * dh, B = batch;
    c->op_a.ensure(B * ns * 4);
    c->op_b.ensure(2 * B * nd * 4);  // the image, and the scratch copy of the fallback
    c->op_c.ensure(2 * B * nd * sizeof(float));
    c->op_d.ensure(B * sizeof(void*));
    h2d(c, c->op_a.p, src, B * ns * 4);
    uchar4* down = c->op_b.as<uchar4>();
    float* gray = c->op_c.as<float>();
    float* alpha = gray + B * nd;
    std::vector<const uchar4*> tab(B);  // (lives until the downloads below have synchronised the stream)
    if (generic) {
      launch_resize_cubic_u8c4_generic(c->st, c->op_a.as<uchar4>(), sw, sh, ns, down, dw, dh, nd, batch);
      launch_gray_alpha(c->st, down, nd, nd, gray, alpha, nd, batch);
    } else {  // as FlowEngine::compute launches it: the sources through a table of pointers
      for (size_t b = 0; b < B; ++b) tab[b] = c->op_a.as<uchar4>() + ns * b;
      h2d(c, c->op_d.p, tab.data(), B * sizeof(void*));
      S360_HIP(hipMemsetAsync(down, 0x5a, B * nd * 4, c->st));  // (an image that is not stored stays this)
      launch_entry_downscale(c->st, nullptr, sw, sh, 0, down_out ? down : nullptr, down + B * nd, dw, dh, nd, batch,
                             c->op_d.as<const uchar4*>(), gray, alpha, nd);
    }
    if (down_out) d2h(c, down_out, down, B * nd * 4);
    d2h(c, gray_out, gray, B * nd * sizeof(float));
    d2h(c, alpha_out, alpha, B * nd * sizeof(float));
    if (tiled) *tiled = resize_cubic_u8c4_tiled_fits(sw, sh, dw, dh) ? 1 : 0;
  });
}
// test tap: PixFlow's final upscale + scalar + 3x3 blur alone on caller-made flows of any size
int s360_debug_upscale_blur(s360_ctx* c, const float* src, int sw, int sh, int batch, int dw, int dh, float post_scale, int generic,
                            float* out, int* tiled) {
  return guard(c, [&] {
    need(c && src && out, "null argument");
    need(sw > 0 && sh > 0 && dw > 0 && dh > 0 && batch >= 1 && batch <= kMaxFlows, "bad size");
    const size_t ns = (size_t)sw * sh, nd = (size_t)dw * dh, B = batch;
    c->op_a.ensure(B * ns * sizeof(float2));
    c->op_d.ensure(B * sizeof(void*));
    h2d(c, c->op_a.p, src, B * ns * sizeof(float2));
    // as FlowEngine::compute launches it: the destinations through a table of pointers, here one allocation per flow
    std::vector<DevBuf> outs(B);
    std::vector<float*> tab(B);  // (lives until the downloads below have synchronised the stream)
    for (size_t b = 0; b < B; ++b) {
      outs[b].ensure(nd * sizeof(float2));
      tab[b] = outs[b].as<float>();
    }
    h2d(c, c->op_d.p, tab.data(), B * sizeof(void*));
    launch_upscale_blur(c->st, c->op_a.as<float2>(), sw, sh, ns, nullptr, dw, dh, nd, batch, post_scale, gaussian_taps(3, 1.0f),
                        c->op_d.as<float*>(), generic != 0);
    for (size_t b = 0; b < B; ++b) d2h(c, out + 2 * nd * b, outs[b].p, nd * sizeof(float2));
    if (tiled) *tiled = (!generic && upscale_blur_tiled_fits(sw, sh, dw, dh)) ? 1 : 0;
  });
}
// test tap (include/s360_debug_flow_level.h): one pyramid level of the flow engine on caller-made planes, stage by stage
int s360_debug_flow_level(s360_ctx* c, const float* gray, const float* alpha, int n_images, int w, int h, const int* i0, const int* i1,
                          int n_flows, const float* initial_flow, const char* alg, int hint, const float* prev_flow, const float* motion,
                          float prev_scale, const s360_flow_level_out* out, int* info) {
  static_assert(S360_FLI_COUNT == kFlowLevelInfoCount, "info block");
  return guard(c, [&] {
    need(c && gray && alpha && i0 && i1 && alg, "null argument");
    need(w >= 2 && h >= 2, "level too small: the reference's bilinear taps need a 2x2 image (PixFlow.h:457-475)");
    need(n_images >= 1 && n_flows >= 1 && n_flows <= kMaxFlows, "batch out of range");
    need(hint >= 0 && hint <= 4, "bad direction hint");
    for (int b = 0; b < n_flows; ++b)
      need(i0[b] >= 0 && i0[b] < n_images && i1[b] >= 0 && i1[b] < n_images, "image index out of range");
    need((prev_flow != nullptr) == (motion != nullptr), "previous flow and motion planes must be given together");
    need(!(prev_flow && out && out->diffused), "with previous state the diffusion and the adjustment are one launch: no diffused flow");
    const PixFlowConsts pc = pixflow_consts_by_name(alg);
    FlowLevelTaps t;
    if (out) {
      t.gradients = out->gradients; t.initial_flow = out->initial_flow; t.blurred_flow = out->blurred_flow;
      t.updated = out->updated; t.row_flags = out->row_flags; t.sweep_forward = out->sweep_forward;
      t.median_first = out->median_first; t.sweep_backward = out->sweep_backward; t.median_second = out->median_second;
      t.diffused = out->diffused; t.final_flow = out->final_flow;
    }
    c->flow->debug_level(c->st, pc, n_images, n_flows, w, h, gray, alpha, i0, i1, initial_flow, hint, prev_flow, motion, prev_scale, t,
                         info);
  });
}

// test taps (include/s360_debug_flow_pyramid.h): the flow engine's preparation on caller-made images, and the pyramids' two resizes on
// caller-made planes. Buffers of the call's own; a resize's output is uploaded first, so a word no thread stores comes back as the
// caller left it.
int s360_debug_flow_prepare(s360_ctx* c, const uint8_t* images, int n_images, int w, int h, const int* i0, const int* i1, int n_flows,
                            const uint8_t* prev_images, const float* prev_flows, const char* alg, int fill,
                            const s360_flow_prepare_out* out) {
  return guard(c, [&] {
    need(c && images && i0 && i1 && alg && out, "null argument");
    need(w > 0 && h > 0 && n_images >= 1 && n_images <= kMaxFlows && n_flows >= 1 && n_flows <= kMaxFlows, "bad size");
    need((prev_images != nullptr) == (prev_flows != nullptr), "previous images and previous flows must be given together");
    need(fill >= -1 && fill <= 255, "bad fill byte");
    const PixFlowConsts pc = pixflow_consts_by_name(alg);
    const size_t n = (size_t)w * h, N = n_images, B = n_flows;
    DevBuf dimg;
    dimg.ensure(N * n * 4);
    h2d(c, dimg.p, images, N * n * 4);
    std::vector<DevBuf> pimg(prev_images ? N : 0), pflow(prev_flows ? B : 0);  // one allocation each, as a frame's state arrives
    FlowBatch fb;
    fb.add_images(dimg.as<uchar4>(), n_images, n);
    for (size_t k = 0; k < pimg.size(); ++k) {
      pimg[k].ensure(n * 4);
      h2d(c, pimg[k].p, prev_images + k * n * 4, n * 4);
      fb.prev_images.push_back(pimg[k].as<uchar4>());
    }
    for (size_t b = 0; b < B; ++b) {
      if (prev_flows) {
        pflow[b].ensure(n * sizeof(float2));
        h2d(c, pflow[b].p, prev_flows + b * n * 2, n * sizeof(float2));
      }
      fb.add_flow(i0[b], i1[b], nullptr, prev_flows ? pflow[b].as<float2>() : nullptr);
    }
    FlowPrepareTaps t;
    t.cap_levels = out->cap_levels; t.cap_pixels = out->cap_pixels;
    t.level_w = out->level_w; t.level_h = out->level_h; t.n_levels = out->n_levels; t.factors = out->factors;
    t.pyr_images = out->pyr_images; t.prev_pyr = out->prev_pyr; t.motion_pyr = out->motion_pyr;
    c->flow->debug_prepare(c->st, pc, fb, w, h, fill, t);
  });
}
int s360_debug_resize_linear_f32(s360_ctx* c, const float* src, int sw, int sh, int cn, int planes, int dw, int dh, float post_scale,
                                 int do_scale, float* dst, int* tiled) {
  return guard(c, [&] {
    need(!dst || (c && src), "null argument");
    need(sw > 0 && sh > 0 && dw > 0 && dh > 0 && planes >= 1 && planes <= kMaxFlows && (cn == 1 || cn == 2), "bad size");
    if (tiled) *tiled = resize_linear_f32_tiled(sw, sh, dw, dh, cn) ? 1 : 0;
    if (!dst) return;
    const size_t ns = (size_t)sw * sh, nd = (size_t)dw * dh, B = planes;
    DevBuf dsrc, ddst;
    dsrc.ensure(B * ns * cn * sizeof(float)); ddst.ensure(B * nd * cn * sizeof(float));
    h2d(c, dsrc.p, src, B * ns * cn * sizeof(float));
    h2d(c, ddst.p, dst, B * nd * cn * sizeof(float));
    launch_resize_linear_f32(c->st, dsrc.as<float>(), sw, sh, ns, ddst.as<float>(), dw, dh, nd, cn, planes, post_scale, do_scale);
    d2h(c, dst, ddst.p, B * nd * cn * sizeof(float));
  });
}
int s360_debug_resize_cubic_flow(s360_ctx* c, const float* src, int sw, int sh, int n_flows, int dw, int dh, float post_scale,
                                 int through_table, float* dst, int* tiled) {
  return guard(c, [&] {
    need(!dst || (c && src), "null argument");
    need(sw > 0 && sh > 0 && dw > 0 && dh > 0 && n_flows >= 1 && n_flows <= kMaxFlows, "bad size");
    if (tiled) *tiled = resize_cubic_f32c2_tiled(sw, sh, dw, dh, through_table != 0) ? 1 : 0;
    if (!dst) return;
    const size_t ns = (size_t)sw * sh, nd = (size_t)dw * dh, B = n_flows;
    DevBuf dsrc, ddst, dtab;
    std::vector<DevBuf> srcs(through_table ? B : 0);
    std::vector<const float2*> tab(B);  // (lives until the download below has synchronised the stream)
    ddst.ensure(B * nd * sizeof(float2));
    h2d(c, ddst.p, dst, B * nd * sizeof(float2));
    if (through_table) {
      for (size_t b = 0; b < B; ++b) {
        srcs[b].ensure(ns * sizeof(float2));
        h2d(c, srcs[b].p, src + b * ns * 2, ns * sizeof(float2));
        tab[b] = srcs[b].as<float2>();
      }
      dtab.ensure(B * sizeof(void*));
      h2d(c, dtab.p, tab.data(), B * sizeof(void*));
      launch_resize_cubic_f32c2(c->st, nullptr, sw, sh, 0, ddst.as<float2>(), dw, dh, nd, n_flows, post_scale, dtab.as<const float2*>());
    } else {
      dsrc.ensure(B * ns * sizeof(float2));
      h2d(c, dsrc.p, src, B * ns * sizeof(float2));
      launch_resize_cubic_f32c2(c->st, dsrc.as<float2>(), sw, sh, ns, ddst.as<float2>(), dw, dh, nd, n_flows, post_scale);
    }
    d2h(c, dst, ddst.p, B * nd * sizeof(float2));
  });
}

// test taps (include/s360_debug_remap.h): the frame's bicubic remap launchers on caller-made sources, maps and flows. Buffers of the
// call's own; the outputs are uploaded first, so a word no workgroup stores comes back as the caller left it.
int s360_debug_remap_packed(s360_ctx* c, const uint8_t* src, int sw, int sh, const float* map, int dw, int dh, int batch, int alpha_mode,
                            int y_feather_start, int feather_size, int weights, uint8_t* dst, uint32_t* packed, int32_t* tiles) {
  return guard(c, [&] {
    need(c && src && map && dst && packed && tiles, "null argument");
    need(sw > 0 && sh > 0 && dw > 0 && dh > 0 && batch >= 1 && batch <= 65535, "bad size");
    need(alpha_mode >= 0 && alpha_mode <= 2 && weights >= 0 && weights <= 2, "bad mode");
    need(alpha_mode == 0 || feather_size > 0, "the feather needs a positive size");
    FrameState& F = frame_state(c);
    need(weights != 2 || F.tab.dev.bicubic_res, "the host's rebuild of the weight table failed: no rebuilt weights");
    const size_t B = batch, sn = (size_t)sw * sh, dn = (size_t)dw * dh, nt = remap_packed_tiles(dw, dh);
    DevBuf dsrc, dmap, ddst, dpk, dtl;
    dsrc.ensure(B * sn * 4); dmap.ensure(B * dn * sizeof(float2)); ddst.ensure(B * dn * 4); dpk.ensure(B * dn * 4); dtl.ensure(B * nt * 16);
    h2d(c, dsrc.p, src, B * sn * 4);
    h2d(c, dmap.p, map, B * dn * sizeof(float2));
    h2d(c, ddst.p, dst, B * dn * 4);
    h2d(c, dpk.p, packed, B * dn * 4);
    h2d(c, dtl.p, tiles, B * nt * 16);
    launch_remap_pack_map(c->st, dmap.as<float2>(), sw, sh, dw, dh, dpk.as<unsigned>(), dtl.p, batch);
    launch_remap_cubic_u8c4_packed(c->st, dsrc.as<uchar4>(), sw, sh, dmap.as<float2>(), dpk.as<unsigned>(), dtl.p, ddst.as<uchar4>(), dw, dh,
                                   F.tab.dev, alpha_mode, y_feather_start, feather_size, batch, weights);
    d2h(c, dst, ddst.p, B * dn * 4);
    d2h(c, packed, dpk.p, B * dn * 4);
    d2h(c, tiles, dtl.p, B * nt * 16);
  });
}
int s360_debug_pole_warp_packed(s360_ctx* c, const uint8_t* ext_fisheye, int ext_w, int rows, const float* flow, float pole_camera_radius,
                                float phi_ramp_start, float phi_mid, float phi_ramp_end, uint8_t* warped, uint32_t* packed, int32_t* tiles) {
  return guard(c, [&] {
    need(c && ext_fisheye && flow && warped && packed && tiles, "null argument");
    need(ext_w > 0 && rows > 0, "bad size");
    FrameState& F = frame_state(c);
    const size_t n = (size_t)ext_w * rows, nt = remap_packed_tiles(ext_w, rows);
    PoleWarpParams pw{};
    pw.cols = pw.extW = ext_w;
    pw.rows = rows;
    pw.poleCameraRadius = pole_camera_radius; pw.phiRampStart = phi_ramp_start; pw.phiMid = phi_mid; pw.phiRampEnd = phi_ramp_end;
    DevBuf dsrc, dflow, ddst, dpk, dtl;
    dsrc.ensure(n * 4); dflow.ensure(n * sizeof(float2)); ddst.ensure(n * 4); dpk.ensure(n * 4); dtl.ensure(nt * 16);
    h2d(c, dsrc.p, ext_fisheye, n * 4);
    h2d(c, dflow.p, flow, n * sizeof(float2));
    h2d(c, ddst.p, warped, n * 4);
    h2d(c, dpk.p, packed, n * 4);
    h2d(c, dtl.p, tiles, nt * 16);
    launch_pole_warp_packed(c->st, dsrc.as<uchar4>(), dflow.as<float2>(), ddst.as<uchar4>(), pw, F.tab.dev, dpk.as<unsigned>(), dtl.p);
    d2h(c, warped, ddst.p, n * 4);
    d2h(c, packed, dpk.p, n * 4);
    d2h(c, tiles, dtl.p, nt * 16);
  });
}
int s360_debug_remap_by_flow(s360_ctx* c, const uint8_t* src, int w, int h, const float* flow, uint8_t* dst) {
  return guard(c, [&] {
    need(c && src && flow && dst, "null argument");
    need(w > 0 && h > 0, "bad size");
    FrameState& F = frame_state(c);
    const size_t n = (size_t)w * h;
    DevBuf dsrc, dflow, ddst;
    dsrc.ensure(n * 4); dflow.ensure(n * sizeof(float2)); ddst.ensure(n * 4);
    h2d(c, dsrc.p, src, n * 4);
    h2d(c, dflow.p, flow, n * sizeof(float2));
    h2d(c, ddst.p, dst, n * 4);
    launch_remap_by_flow(c->st, dsrc.as<uchar4>(), w, h, dflow.as<float2>(), ddst.as<uchar4>(), F.tab.dev);
    d2h(c, dst, ddst.p, n * 4);
  });
}

// test taps (include/s360_debug_cubemap.h): the frame's stereo cubemap launchers on caller-made eyes, through the face maps the
// frame builds (cube_face_maps). Buffers of the call's own; the outputs are uploaded first, as above.
static void debug_cubemap_impl(s360_ctx* c, const uint8_t* eyes, int n_slots, int sw, int sh, int fw, int fh, int video, int lds_pixels,
                               uint8_t* out, float* maps, uint32_t* packed, int32_t* tiles, bool tiled) {
  need(c && eyes && out && maps && (!tiled || (packed && tiles)), "null argument");
  need(sw > 0 && sh > 0 && fw > 0 && fh > 0 && sw <= 16384 && sh <= 16384 && fw <= 16384 && fh <= 16384, "bad size");
  need(n_slots >= 1 && n_slots <= 64, "bad number of slots");
  need(video == 0 || video == 1, "bad format");
  need(!tiled || lds_pixels == 4096 || lds_pixels == 2560, "the box of a tile holds 4096 or 2560 pixels");
  FrameState& F = frame_state(c);
  const size_t en = (size_t)sw * sh * 4, px = (size_t)6 * fw * fh, on = 2 * px * 3, nt = cubemap_tile_count(fw, fh);
  const std::vector<float> m = cube_face_maps(sw, sh, fw, fh);
  DevBuf deyes, dmaps, dout, dpk, dtl;
  deyes.ensure(2 * (size_t)n_slots * en); dmaps.ensure(px * sizeof(float2)); dout.ensure((size_t)n_slots * on);
  h2d(c, deyes.p, eyes, 2 * (size_t)n_slots * en);
  h2d(c, dmaps.p, m.data(), px * sizeof(float2));
  h2d(c, dout.p, out, (size_t)n_slots * on);
  std::vector<const uchar4*> ep(2 * (size_t)n_slots);
  std::vector<uint8_t*> op(n_slots);
  for (size_t k = 0; k < ep.size(); ++k) ep[k] = reinterpret_cast<const uchar4*>(static_cast<const uint8_t*>(deyes.p) + k * en);
  for (int k = 0; k < n_slots; ++k) op[k] = static_cast<uint8_t*>(dout.p) + (size_t)k * on;
  if (tiled) {
    dpk.ensure(px * sizeof(unsigned)); dtl.ensure(nt * 16);
    h2d(c, dpk.p, packed, px * sizeof(unsigned));
    h2d(c, dtl.p, tiles, nt * 16);
    launch_cubemap_pack(c->st, dmaps.as<float2>(), sw, sh, fw, fh, video, lds_pixels, dpk.as<unsigned>(), dtl.p);
    launch_cubemap_tiles(c->st, ep.data(), op.data(), n_slots, sw, sh, dmaps.as<float2>(), dpk.as<unsigned>(), dtl.p, fw, fh, video,
                         lds_pixels, F.tab.dev);
  } else {
    for (int k = 0; k < n_slots; ++k)
      launch_cubemap(c->st, ep[2 * k], ep[2 * k + 1], sw, sh, dmaps.as<float2>(), fw, fh, video, op[k], F.tab.dev);
  }
  d2h(c, out, dout.p, (size_t)n_slots * on);  // (synchronises the stream: `m` and the pointer lists live until here)
  d2h(c, maps, dmaps.p, px * sizeof(float2));
  if (tiled) {
    d2h(c, packed, dpk.p, px * sizeof(unsigned));
    d2h(c, tiles, dtl.p, nt * 16);
  }
}
int s360_debug_cubemap_tiles(s360_ctx* c, const uint8_t* eyes, int n_slots, int sw, int sh, int fw, int fh, int video, int lds_pixels,
                             uint8_t* out, float* maps, uint32_t* packed, int32_t* tiles) {
  return guard(c, [&] { debug_cubemap_impl(c, eyes, n_slots, sw, sh, fw, fh, video, lds_pixels, out, maps, packed, tiles, true); });
}
int s360_debug_cubemap(s360_ctx* c, const uint8_t* eyes, int n_slots, int sw, int sh, int fw, int fh, int video, uint8_t* out,
                       float* maps) {
  return guard(c, [&] { debug_cubemap_impl(c, eyes, n_slots, sw, sh, fw, fh, video, 0, out, maps, nullptr, nullptr, false); });
}

int s360_spherical_warp_map(s360_ctx* c, float* map_out, int dw, int dh, const s360_camera* cam, float l, float r,
                            float t, float b) {
  return guard(c, [&] {
    need(c && map_out && cam && dw > 0 && dh > 0, "bad argument");
    c->op_a.ensure((size_t)dw * dh * sizeof(float2));
    build_spherical_map(c, c->op_a.as<float2>(), dw, dh, *cam, l, r, t, b);
    d2h(c, map_out, c->op_a.p, (size_t)dw * dh * sizeof(float2));
  });
}
int s360_bicubic_remap_to_spherical(s360_ctx* c, uint8_t* dst, int dw, int dh, int dc, const uint8_t* src, int sw,
                                    int sh, int sc, const s360_camera* cam, float l, float r, float t, float b) {
  return guard(c, [&] {
    need(c && dst && src && cam, "null argument");
    need((dc == 3 || dc == 4) && (sc == 3 || sc == 4), "channels must be 3 or 4");
    need(!(sc == 4 && dc == 3), "4-channel source: the reference's remap() re-creates the destination with the source's type (ImageWarper.cpp:173) - pass a 4-channel destination");
    FrameState& F = frame_state(c);
    const size_t sn = (size_t)sw * sh, dn = (size_t)dw * dh;
    c->op_a.ensure(dn * sizeof(float2));
    c->op_b.ensure(sn * 4);
    c->op_c.ensure(sn * sizeof(uchar4));
    c->op_d.ensure(dn * sizeof(uchar4));
    build_spherical_map(c, c->op_a.as<float2>(), dw, dh, *cam, l, r, t, b);
    h2d(c, c->op_b.p, src, sn * sc);
    launch_bgr_to_bgra(c->st, c->op_b.as<uint8_t>(), sc, c->op_c.as<uchar4>(), sn);
    launch_remap_cubic_u8c4(c->st, c->op_c.as<uchar4>(), sw, sh, c->op_a.as<float2>(), c->op_d.as<uchar4>(), dw, dh,
                            F.tab.dev, 0, 0, 1);
    if (dc == 4) {
      d2h(c, dst, c->op_d.p, dn * 4);
    } else {
      c->op_e.ensure(dn * 3);
      launch_pack_bgr(c->st, c->op_d.as<uchar4>(), dw, dh, c->op_e.as<uint8_t>());
      d2h(c, dst, c->op_e.p, dn * 3);
    }
  });
}
int s360_combine_lazy_novel_views(s360_ctx* c, const uint8_t* image_l, const uint8_t* image_r, const float* flow_l_to_r,
                                  const float* flow_r_to_l, uint8_t* chunk_l, uint8_t* chunk_r) {
  return guard(c, [&] {
    need(c && image_l && image_r && flow_l_to_r && flow_r_to_l && chunk_l && chunk_r, "null argument");
    FrameState& F = frame_state(c);
    const s360_geometry& g = c->g;
    const int P = F.P, ow = g.overlap_image_width, camH = g.cam_image_height, stripW = c->P.eqr_width / P;
    const size_t on = (size_t)ow * camH, sn = (size_t)stripW * camH;
    c->op_a.ensure(2 * on * 4);
    c->op_b.ensure(2 * on * sizeof(float2));
    c->op_c.ensure(2 * sn * 4);
    h2d(c, c->op_a.p, image_l, on * 4);
    h2d(c, c->op_a.as<uint8_t>() + on * 4, image_r, on * 4);
    h2d(c, c->op_b.p, flow_l_to_r, on * sizeof(float2));
    h2d(c, c->op_b.as<float2>() + on, flow_r_to_l, on * sizeof(float2));
    NovelViewParams nv;
    nv.overlapW = ow; nv.camH = camH; nv.stripW = stripW; nv.numNovelViews = g.num_novel_views;
    nv.numPairs = 1; nv.numLocal = 1;
    nv.camImageWidthHalf = float(g.cam_image_width) * 0.5f;
    nv.disp = g.verge_at_infinity_slab_displacement;
    launch_novel_view(c->st, c->op_a.as<uchar4>(), c->op_b.as<float2>(), c->op_c.as<uchar4>(), nv, 0, 1, F.tab.dev);
    d2h(c, chunk_l, c->op_c.p, sn * 4);
    d2h(c, chunk_r, c->op_c.as<uint8_t>() + sn * 4, sn * 4);
  });
}
// generateNovelView for n shifts of the pair whose images are op_a[0], op_a[1] and whose flows are op_b[0] (LtoR), op_b[1] (RtoL)
static void morph_views_resident(s360_ctx* c, int w, int h, const double* shifts, int n, uint8_t* out_merged, uint8_t* out_from_l,
                                 uint8_t* out_from_r) {
  FrameState& F = frame_state(c);
  const size_t px = (size_t)w * h, V = n;
  c->op_c.ensure(V * px * 4 * (1 + (out_from_l ? 1 : 0) + (out_from_r ? 1 : 0)));
  c->op_d.ensure(V * sizeof(double));
  h2d(c, c->op_d.p, shifts, V * sizeof(double));
  uchar4* merged = c->op_c.as<uchar4>();
  uchar4* fromL = out_from_l ? merged + V * px : nullptr;
  uchar4* fromR = out_from_r ? merged + V * px * (out_from_l ? 2 : 1) : nullptr;
  // (developer switch S360_MORPH_VPB: views per grid.z slice, for tools/morph_time.py's comparison of the two mappings; same bytes either way)
  const char* e = std::getenv("S360_MORPH_VPB");
  {
    ProfScope ps(c->prof, "morph_views");
    launch_morph_views(c->st, c->op_a.as<uchar4>(), c->op_a.as<uchar4>() + px, c->op_b.as<float2>(), c->op_b.as<float2>() + px, w, h,
                       c->op_d.as<double>(), n, merged, fromL, fromR, F.tab.dev, e ? std::atoi(e) : 0);
  }
  d2h(c, out_merged, merged, V * px * 4);
  if (fromL) d2h(c, out_from_l, fromL, V * px * 4);
  if (fromR) d2h(c, out_from_r, fromR, V * px * 4);
}
int s360_generate_novel_views(s360_ctx* c, const uint8_t* image_l, const uint8_t* image_r, const float* flow_l_to_r,
                              const float* flow_r_to_l, int w, int h, const double* shifts, int n, uint8_t* out_merged,
                              uint8_t* out_from_l, uint8_t* out_from_r) {
  return guard(c, [&] {
    need(c && image_l && image_r && flow_l_to_r && flow_r_to_l && shifts && out_merged, "null argument");
    need(w > 0 && h > 0, "image size must be positive");
    need(n >= 1, "at least one shift is required");
    const size_t px = (size_t)w * h;
    c->op_a.ensure(2 * px * 4);
    c->op_b.ensure(2 * px * sizeof(float2));
    h2d(c, c->op_a.p, image_l, px * 4);
    h2d(c, c->op_a.as<uint8_t>() + px * 4, image_r, px * 4);
    h2d(c, c->op_b.p, flow_l_to_r, px * sizeof(float2));
    h2d(c, c->op_b.as<float2>() + px, flow_r_to_l, px * sizeof(float2));
    morph_views_resident(c, w, h, shifts, n, out_merged, out_from_l, out_from_r);
  });
}
int s360_interpolate_views(s360_ctx* c, const char* alg, const uint8_t* image_l, const uint8_t* image_r, int w, int h,
                           const double* shifts, int n, uint8_t* out_merged, uint8_t* out_from_l, uint8_t* out_from_r,
                           float* out_flow_l_to_r, float* out_flow_r_to_l) {
  return guard(c, [&] {
    need(c && alg && image_l && image_r && shifts && out_merged, "null argument");
    need(w >= 4 && h >= 4, "image too small: the reference's bilinear taps need a 2x2 image after the x0.5 entry downscale (PixFlow.h:457-475)");
    need(n >= 1, "at least one shift is required");
    const PixFlowConsts pc = pixflow_consts_by_name(alg);
    const size_t px = (size_t)w * h;
    c->op_a.ensure(2 * px * 4);
    c->op_b.ensure(2 * px * sizeof(float2));
    h2d(c, c->op_a.p, image_l, px * 4);
    h2d(c, c->op_a.as<uint8_t>() + px * 4, image_r, px * 4);
    // NovelViewGeneratorAsymmetricFlow::prepare (NovelView.cpp:270-299): (L, R, LEFT) then (R, L, RIGHT), no previous frame
    for (int d = 0; d < 2; ++d) {
      FlowBatch fb;
      fb.add_images(c->op_a.as<uchar4>(), 2, px);
      fb.add_flow(d, 1 - d, c->op_b.as<float2>() + px * d);
      c->flow->compute(c->st, pc, fb, w, h, d == 0 ? S360_HINT_LEFT : S360_HINT_RIGHT);
    }
    morph_views_resident(c, w, h, shifts, n, out_merged, out_from_l, out_from_r);
    if (out_flow_l_to_r) d2h(c, out_flow_l_to_r, c->op_b.p, px * sizeof(float2));
    if (out_flow_r_to_l) d2h(c, out_flow_r_to_l, c->op_b.as<float2>() + px, px * sizeof(float2));
  });
}
int s360_flatten_layers_deghost_prefer_base(s360_ctx* c, const uint8_t* bottom_layer, const uint8_t* top_layer, int w,
                                            int h, uint8_t* out) {
  return guard(c, [&] {
    need(c && bottom_layer && top_layer && out && w > 0 && h > 0, "bad argument");
    FrameState& F = frame_state(c);
    const size_t n = (size_t)w * h;
    c->op_a.ensure(n * 4); c->op_b.ensure(n * 4); c->op_c.ensure(n * 4);
    h2d(c, c->op_a.p, bottom_layer, n * 4);
    h2d(c, c->op_b.p, top_layer, n * 4);
    launch_flatten(c->st, c->op_a.as<uchar4>(), c->op_b.as<uchar4>(), c->op_c.as<uchar4>(), w, h, 0, F.tab.dev);
    d2h(c, out, c->op_c.p, n * 4);
  });
}
int s360_offset_horizontal_wrap(s360_ctx* c, const uint8_t* src, int w, int h, int channels, float offset,
                                uint8_t* out) {
  return guard(c, [&] {
    need(c && src && out && w > 0 && h > 0, "bad argument");
    need(channels == 3 || channels == 4, "channels must be 3 or 4");
    const size_t n = (size_t)w * h;
    c->op_a.ensure(n * 4); c->op_b.ensure(n * 4);
    if (channels == 4) {
      h2d(c, c->op_a.p, src, n * 4);
    } else {  // BGR: through the BGRA kernels, alpha dropped again
      c->op_c.ensure(n * 3);
      h2d(c, c->op_c.p, src, n * 3);
      launch_bgr_to_bgra(c->st, c->op_c.as<uint8_t>(), 3, c->op_a.as<uchar4>(), n);
    }
    // one "strip" of the full width, no padding: pure offsetHorizontalWrap
    launch_assemble_pano(c->st, c->op_a.as<uchar4>(), 1, h, w, offset, c->op_b.as<uchar4>(), w, h);
    if (channels == 4) {
      d2h(c, out, c->op_b.p, n * 4);
    } else {
      launch_pack_bgr(c->st, c->op_b.as<uchar4>(), w, h, c->op_c.as<uint8_t>());
      d2h(c, out, c->op_c.p, n * 3);
    }
  });
}
int s360_feather_alpha_channel(s360_ctx* c, const uint8_t* src, int w, int h, int erode_size, uint8_t* out) {
  return guard(c, [&] {
    need(c && src && out && w > 0 && h > 0, "bad argument");
    need(erode_size >= 1 && erode_size <= 32, "erode_size must be in 1..32");
    need(erode_size % 2 == 1, "erode_size must be odd (it is the GaussianBlur kernel size, CvUtil.cpp:151)");
    const size_t n = (size_t)w * h;
    c->op_a.ensure(n * 4); c->op_b.ensure(n * 4);
    h2d(c, c->op_a.p, src, n * 4);
    if (erode_size == c->P.std_alpha_feather_size) {
      dev_feather_alpha_to_ext(c, c->op_a.as<uchar4>(), w, h, c->op_b.as<uchar4>(), w);
    } else {
      const std::vector<int> taps = feather_gauss_taps(erode_size);
      c->op_e.ensure(taps.size() * sizeof(int));
      h2d(c, c->op_e.p, taps.data(), taps.size() * sizeof(int));
      dev_feather_alpha_to_ext(c, c->op_a.as<uchar4>(), w, h, c->op_b.as<uchar4>(), w, erode_size, c->op_e.as<int>());
    }
    d2h(c, out, c->op_b.p, n * 4);
  });
}
int s360_pole_to_side_flow(s360_ctx* c, const uint8_t* side, const uint8_t* pole, int pole_rows, uint8_t* warped_out,
                           float* flow_out) {
  return guard(c, [&] {
    need(c && side && pole && warped_out && pole_rows > 0, "bad argument");
    need(c->bottom_idx >= 0, "rig has no bottom camera (pole ramp uses its fov, TRSP:461)");
    const int W = c->P.eqr_width, H = c->P.eqr_height;
    need(pole_rows <= H, "pole_rows larger than eqr_height");
    const int extW = int(float(W) * 1.2f);
    const size_t en = (size_t)W * H, pn = (size_t)W * pole_rows, xn = (size_t)extW * pole_rows;
    c->op_a.ensure(en * 4); c->op_b.ensure(pn * 4); c->op_c.ensure(2 * xn * 4); c->op_d.ensure(xn * sizeof(float2));
    c->op_e.ensure(en * 4);
    h2d(c, c->op_a.p, side, en * 4);
    h2d(c, c->op_b.p, pole, pn * 4);
    uchar4* ext = c->op_c.as<uchar4>();
    dev_feather_alpha_to_ext(c, c->op_a.as<uchar4>(), W, pole_rows, ext, extW);
    launch_extend_wrap(c->st, c->op_b.as<uchar4>(), nullptr, W, pole_rows, ext + xn, extW);
    (void)flow_engine(c, 1);
    FlowBatch fb;
    fb.add_images(ext, 2, xn);
    fb.add_flow(0, 1, c->op_d.as<float2>());
    c->flow_pole->compute(c->st, pixflow_consts_by_name(c->P.polar_flow_alg), fb, extW, pole_rows, S360_HINT_DOWN);
    dev_pole_unit_post(c, ext + xn, c->op_d.as<float2>(), W, pole_rows, extW, c->op_e.as<uchar4>(), H);
    d2h(c, warped_out, c->op_e.p, en * 4);
    if (flow_out) d2h(c, flow_out, c->op_d.p, xn * sizeof(float2));
  });
}
int s360_sharpen(s360_ctx* c, uint8_t* bgr, int w, int h, float sharpening) {
  return guard(c, [&] {
    need(c && bgr && w > 1 && h > 1, "bad argument");
    const size_t n = (size_t)w * h;
    c->op_a.ensure(n * 3); c->op_b.ensure(n * 4); c->op_c.ensure(n * 4); c->op_d.ensure(sharpen_scratch_bytes(w, h));
    h2d(c, c->op_a.p, bgr, n * 3);
    launch_bgr_to_bgra(c->st, c->op_a.as<uint8_t>(), 3, c->op_b.as<uchar4>(), n);
    launch_sharpen(c->st, c->op_b.as<uchar4>(), c->op_c.as<uchar4>(), c->op_d.as<float>(), w, h, 1.0f + sharpening);
    launch_pack_bgr(c->st, c->op_b.as<uchar4>(), w, h, c->op_a.as<uint8_t>());
    d2h(c, bgr, c->op_a.p, n * 3);
  });
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
    const int P = F.P;
    need(pair >= 0 && pair < P, "pair_idx out of range");
    const size_t on = (size_t)c->g.overlap_image_width * c->g.cam_image_height;
    // previous-frame slot of the double buffer, laid out like frame_render_pairs lays out the block [p0, p1) this
    // context renders (s360_frame_set_partition; default all pairs): L images / LtoR flows of the block first, then
    // R images / RtoL flows
    if (!F.partition_declared) { F.side_p0 = 0; F.side_p1 = P; }
    const int p0 = F.side_p0, n = F.side_p1 - F.side_p0;
    need(pair >= p0 && pair < F.side_p1, "pair_idx outside the block declared with s360_frame_set_partition");
    const int j = pair - p0;
    const int prv = F.last_side;  // becomes "the previous frame" of the next render
    F.overlaps[prv].ensure(2 * n * on * sizeof(uchar4));
    F.sideFlows.ensure(2 * n * on * sizeof(float2));
    h2d(c, F.overlaps[prv].as<uchar4>() + on * j, overlap_l, on * sizeof(uchar4));
    h2d(c, F.overlaps[prv].as<uchar4>() + on * (n + j), overlap_r, on * sizeof(uchar4));
    h2d(c, F.sideFlows.as<float2>() + on * j, flow_l_to_r, on * sizeof(float2));
    h2d(c, F.sideFlows.as<float2>() + on * (n + j), flow_r_to_l, on * sizeof(float2));
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
    const int extW = int(float(c->P.eqr_width) * 1.2f);
    const int rows = unit < 2 ? c->g.top_rows : c->g.bottom_rows;
    const size_t xn = (size_t)extW * rows;                                       // one image / flow of this unit
    const size_t xs = (size_t)extW * std::max(c->g.top_rows, c->g.bottom_rows);  // slot stride (frame_finish)
    const int prv = F.last_pole;  // becomes "the previous frame" of the next render
    F.extImgs[prv].ensure(6 * xs * sizeof(uchar4));
    F.poleFlows.ensure(4 * xs * sizeof(float2));
    h2d(c, F.extImgs[prv].as<uchar4>() + xs * unit, ext_side, xn * sizeof(uchar4));
    h2d(c, F.extImgs[prv].as<uchar4>() + xs * (unit < 2 ? 4 : 5), ext_fisheye, xn * sizeof(uchar4));
    h2d(c, F.poleFlows.as<float2>() + xs * unit, flow, xn * sizeof(float2));
    S360_HIP(hipStreamSynchronize(c->st));  // the caller's buffers may be reused as soon as this returns
    F.extW = extW;
    F.extStride = xs;
    F.poleRowsT = c->g.top_rows;
    F.poleRowsB = c->g.bottom_rows;
    F.have_prev_pole = true;
    F.prevPoleGot[unit] = 0;  // (halves of this unit handed in as files are superseded)
  });
}
int s360_comm_get_unique_id(void* id_out) {
  return guard(nullptr, [&] { need(id_out, "null argument"); comm_unique_id(id_out); });
}
const char* s360_comm_library_path(void) {
  const char* p = nullptr;
  (void)guard(nullptr, [&] { p = comm_library_path(); });
  return p;
}
int s360_comm_init_rank(s360_ctx* c, const void* id, int rank, int nranks) {
  return guard(c, [&] { need(c && id, "null argument"); comm_init_rank(c, id, rank, nranks); });
}
int s360_comm_init_all(s360_ctx* const* ctxs, int n) {
  return guard(nullptr, [&] { need(ctxs && n > 0, "bad argument"); comm_init_all(ctxs, n); });
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
// the state of frame slot `slot` (-1: the selected one) without touching the selection: a fetching thread names its slot, so that
// the thread that feeds the context can go on selecting slots for its uploads
static FrameState& slot_state(s360_ctx* c, int slot) {
  if (slot < 0) return frame_state(c);
  need(slot < (int)std::max<size_t>(c->slots.size(), 1), "frame slot out of range");
  const int saved = c->slot;
  c->slot = slot;
  struct Restore { s360_ctx* c; int s; ~Restore() { c->slot = s; } } restore{c, saved};
  return frame_state(c);
}
static int download_equirect_impl(s360_ctx* c, int slot, int age, uint8_t* out_bgr) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(out_bgr && (age == 0 || age == 1), "bad argument (age is 0 = latest enqueued frame or 1 = the one before)");
    FrameState& F = slot_state(c, slot);
    need(F.frames_done > age, "that frame has not been rendered");
    need(age == 0 || ((c->pipeline || c->two_outputs) && F.outBGR[F.out_cur ^ 1].p),
         "age 1 needs two output buffers (s360_set_frame_pipelining or s360_set_output_double_buffer)");
    const int b = age == 0 ? F.out_cur : F.out_cur ^ 1;
    // wait for THAT frame only (its event sits behind its last kernel), then copy on a stream of its own so that the
    // transfer does not queue behind the kernels of the frame enqueued after it
    if (!c->stDown) S360_HIP(hipStreamCreateWithFlags(&c->stDown, hipStreamNonBlocking));
    if (!c->evDown) S360_HIP(hipEventCreateWithFlags(&c->evDown, hipEventDisableTiming | hipEventBlockingSync));
    if (!c->downErr) {
      S360_HIP(hipHostMalloc((void**)&c->downErr, 4 * sizeof(unsigned), hipHostMallocDefault));
      std::memset(c->downErr, 0, 4 * sizeof(unsigned));
    }
    if (!F.downRead[b]) S360_HIP(hipEventCreateWithFlags(&F.downRead[b], hipEventDisableTiming));
    S360_HIP(hipStreamWaitEvent(c->stDown, F.outDone[b], 0));
    S360_HIP(hipMemcpyAsync(out_bgr, F.outBGR[b].p, (size_t)c->g.out_width * c->g.out_height * 3, hipMemcpyDeviceToHost, c->stDown));
    // the frame's error words travel with it (a later frame's finish stage rewrites them as soon as downRead[b] has fired): a device
    // -> page-locked host copy on the download's own stream (a host -> host "async" copy would block this thread with the lock held)
    if (F.outErrDev[b].p) S360_HIP(hipMemcpyAsync(c->downErr, F.outErrDev[b].p, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stDown));
    S360_HIP(hipEventRecord(F.downRead[b], c->stDown));
    S360_HIP(hipEventRecord(c->evDown, c->stDown));
    const hipEvent_t ev = c->evDown;
    const unsigned* errw = F.outErrDev[b].p ? c->downErr : nullptr;  // (nothing of the slot is touched after the lock is back: it may be gone)
    // The wait is most of a frame long: the context is free meanwhile (the next frame's uploads and enqueue need it).
    // One fetching thread per context: evDown is re-recorded by the next call.
    lk.unlock();
    const hipError_t rc = hipEventSynchronize(ev);
    lk.lock();
    S360_HIP(rc);
    // the frame's sweep error words were snapshotted in front of outDone[b] (render.hpp): a timed-out banded sweep
    // fails THIS frame's download, before the host hands the pixels to an encoder
    if (errw && (errw[0] | errw[1] | errw[2])) {
      // reported once: the engines' cumulative error words are reset, so that the frames enqueued from now on are judged on
      // their own sweeps (frames already in flight carry the snapshot they took)
      for (FlowEngine* e : {c->flow.get(), c->flow_pole.get(), c->flow_pr.get()})
        if (e) (void)e->take_error(c->st);
      throw Error(S360_ERR_HIP, "banded sweep timed out waiting for a neighbour band (results invalid)");
    }
  });
}
int s360_frame_download_equirect_of(s360_ctx* c, int age, uint8_t* out_bgr) { return download_equirect_impl(c, -1, age, out_bgr); }
int s360_frame_download_equirect_slot(s360_ctx* c, int slot, int age, uint8_t* out_bgr) {
  if (slot < 0) return S360_ERR_INVALID_ARG;
  return download_equirect_impl(c, slot, age, out_bgr);
}
/* ---- the equirect as a PNG file, encoded on the device (png.hip; replaces imwriteExceptionOnFail, TRSP:938-961) ---- */
static int png_crc_threads() {
  const char* e = std::getenv("S360_PNG_CRC_THREADS");
  const int n = e ? std::atoi(e) : 4;
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}
int s360_set_png_encode(s360_ctx* c, int on) {
  return guard(c, [&] { need(c, "null ctx"); c->png_encode = on != 0; });
}
size_t s360_png_bound(int w, int h) {
  size_t n = 0;
  (void)guard(nullptr, [&] { n = PngPlan::make(w, h).file_bound; });
  return n;
}
size_t s360_frame_png_bound(s360_ctx* c) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] { n = PngPlan::make(c->g.out_width, c->g.out_height).file_bound; });
  return n;
}
// band table to the host (event wait with the context released), then the file image's bytes, then the CRCs off the lock
static void png_fetch(s360_ctx* c, std::unique_lock<std::recursive_mutex>& lk, const PngPlan& plan, const DevBuf& meta, const DevBuf& file,
                      hipEvent_t after /* nullable: what the copy waits for */, hipEvent_t readDone /* nullable: recorded behind the copies */,
                      const void* errDev, uint8_t* out, size_t cap, size_t* n_out, bool release = true) {
  if (!c->stDown) S360_HIP(hipStreamCreateWithFlags(&c->stDown, hipStreamNonBlocking));
  if (!c->evDown) S360_HIP(hipEventCreateWithFlags(&c->evDown, hipEventDisableTiming | hipEventBlockingSync));
  if (!c->downErr) {
    S360_HIP(hipHostMalloc((void**)&c->downErr, 4 * sizeof(unsigned), hipHostMallocDefault));
    std::memset(c->downErr, 0, 4 * sizeof(unsigned));
  }
  const size_t mbytes = ((size_t)plan.nbands + 1) * sizeof(PngBandMeta);
  if (c->pngMetaHostBytes < mbytes) {
    if (c->pngMetaHost) (void)hipHostFree(c->pngMetaHost);
    c->pngMetaHost = nullptr;
    c->pngMetaHostBytes = 0;
    S360_HIP(hipHostMalloc(&c->pngMetaHost, mbytes, hipHostMallocDefault));
    c->pngMetaHostBytes = mbytes;
  }
  if (after) S360_HIP(hipStreamWaitEvent(c->stDown, after, 0));
  S360_HIP(hipMemcpyAsync(c->pngMetaHost, meta.p, mbytes, hipMemcpyDeviceToHost, c->stDown));
  if (errDev) S360_HIP(hipMemcpyAsync(c->downErr, errDev, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stDown));
  S360_HIP(hipEventRecord(c->evDown, c->stDown));
  hipEvent_t ev = c->evDown;
  if (release) lk.unlock();
  hipError_t rc = hipEventSynchronize(ev);
  if (release) lk.lock();
  S360_HIP(rc);
  std::vector<PngBandMeta> m((size_t)plan.nbands + 1);
  std::memcpy(m.data(), c->pngMetaHost, mbytes);
  const unsigned errw = errDev ? (c->downErr[0] | c->downErr[1] | c->downErr[2]) : 0u;
  const size_t end_bands = (size_t)m[plan.nbands].file_off;
  if (end_bands > plan.file_bound || end_bands + 28 > cap) {
    if (readDone) S360_HIP(hipEventRecord(readDone, c->stDown));
    throw Error(S360_ERR_INVALID_ARG, "png: output buffer too small (s360_frame_png_bound / s360_png_bound give the size to allocate)");
  }
  S360_HIP(hipMemcpyAsync(out, file.p, end_bands, hipMemcpyDeviceToHost, c->stDown));
  if (readDone) S360_HIP(hipEventRecord(readDone, c->stDown));
  S360_HIP(hipEventRecord(c->evDown, c->stDown));
  ev = c->evDown;
  if (release) lk.unlock();
  rc = hipEventSynchronize(ev);
  if (rc != hipSuccess) { if (release) lk.lock(); S360_HIP(rc); }
  if (errw) {
    if (release) lk.lock();
    for (FlowEngine* e : {c->flow.get(), c->flow_pole.get(), c->flow_pr.get()})
      if (e) (void)e->take_error(c->st);
    throw Error(S360_ERR_HIP, "banded sweep timed out waiting for a neighbour band (results invalid)");
  }
  // the file's frame around the bands and the chunks' CRCs: host work on the caller's buffer, the context stays free meanwhile
  const size_t n = png_finish_host(out, cap, plan, m.data(), png_crc_threads());
  if (release) lk.lock();
  *n_out = n;
}
static int download_png_impl(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(out && n_out && (age == 0 || age == 1), "bad argument (age is 0 = latest enqueued frame or 1 = the one before)");
    FrameState& F = slot_state(c, slot);
    need(F.frames_done > age, "that frame has not been rendered");
    need(age == 0 || ((c->pipeline || c->two_outputs) && F.outBGR[F.out_cur ^ 1].p),
         "age 1 needs two output buffers (s360_set_frame_pipelining or s360_set_output_double_buffer)");
    const int b = age == 0 ? F.out_cur : F.out_cur ^ 1;
    if (F.pngFrame[b] != F.frames_done - 1 - age || !F.pngFile[b].p)
      throw Error(S360_ERR_STATE, "that frame was rendered without s360_set_png_encode");
    if (!F.downRead[b]) S360_HIP(hipEventCreateWithFlags(&F.downRead[b], hipEventDisableTiming));
    png_fetch(c, lk, F.pngPlan[b], F.pngMeta[b], F.pngFile[b], F.outDone[b], F.downRead[b], F.outErrDev[b].p, out, cap, n_out);
  });
}
int s360_frame_download_png(s360_ctx* c, int age, uint8_t* out, size_t cap, size_t* n_out) { return download_png_impl(c, -1, age, out, cap, n_out); }
int s360_frame_download_png_slot(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  if (slot < 0) return S360_ERR_INVALID_ARG;
  return download_png_impl(c, slot, age, out, cap, n_out);
}
int s360_encode_png(s360_ctx* c, const uint8_t* bgr, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(bgr && out && n_out && w > 0 && h > 0, "bad argument");
    const PngPlan plan = PngPlan::make(w, h);
    const size_t nb = (size_t)w * h * 3;
    c->op_a.ensure((nb + 3) & ~(size_t)3);
    c->op_b.ensure(plan.file_bound);
    S360_HIP(hipMemcpyAsync(c->op_a.p, bgr, nb, hipMemcpyHostToDevice, c->st));
    png_encode_enqueue(c->st, c->op_a.as<uint8_t>(), plan, c->op_c, c->op_d, c->op_b.as<uint8_t>());
    S360_HIP(hipStreamSynchronize(c->st));
    png_fetch(c, lk, plan, c->op_d, c->op_b, nullptr, nullptr, nullptr, out, cap, n_out, false);  // (the operator scratch stays locked)
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
int s360_set_cubemap_output(s360_ctx* c, int face_w, int face_h, const char* format) {
  return frame_guard(c, [&] {
    need(c, "null ctx");
    if (face_w == 0 || face_h == 0) { c->cube_fw = c->cube_fh = 0; return; }
    need(format, "bad argument");
    const std::string f(format);
    if (f != "video" && f != "photo")  // CvUtil.cpp:134-137
      throw Error(S360_ERR_INVALID_ARG, "unexpected cubemap format: " + f + ". valid formats are: video,photo");
    need(face_w > 0 && face_h > 0 && face_w <= 16384 && face_h <= 16384, "cubemap face size must be in 1..16384 (0 = off)");
    (void)cube_maps(c, face_w, face_h, f == "video");  // maps + prepared form now (a host wait), not inside a frame
    c->cube_fw = face_w; c->cube_fh = face_h; c->cube_video = f == "video";
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
// what the fetches of one output buffer share: the download stream and its events (download_equirect_impl)
static void ensure_download_stream(s360_ctx* c) {
  if (!c->stDown) S360_HIP(hipStreamCreateWithFlags(&c->stDown, hipStreamNonBlocking));
  if (!c->evDown) S360_HIP(hipEventCreateWithFlags(&c->evDown, hipEventDisableTiming | hipEventBlockingSync));
  if (!c->downErr) {
    S360_HIP(hipHostMalloc((void**)&c->downErr, 4 * sizeof(unsigned), hipHostMallocDefault));
    std::memset(c->downErr, 0, 4 * sizeof(unsigned));
  }
}
static int cube_buffer(s360_ctx* c, FrameState& F, int age) {
  need(F.frames_done > age, "that frame has not been rendered");
  need(age == 0 || ((c->pipeline || c->two_outputs) && F.outBGR[F.out_cur ^ 1].p),
       "age 1 needs two output buffers (s360_set_frame_pipelining or s360_set_output_double_buffer)");
  const int b = age == 0 ? F.out_cur : F.out_cur ^ 1;
  if (F.cubeFrame[b] != F.frames_done - 1 - age || !F.cubeBGR[b].p)
    throw Error(S360_ERR_STATE, "that frame was rendered without s360_set_cubemap_output");
  return b;
}
static int download_cubemap_impl(s360_ctx* c, int slot, int age, uint8_t* out_bgr) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(out_bgr && (age == 0 || age == 1), "bad argument (age is 0 = latest enqueued frame or 1 = the one before)");
    FrameState& F = slot_state(c, slot);
    const int b = cube_buffer(c, F, age);
    // as download_equirect_impl: wait for THAT frame only, copy on the download stream, the context free meanwhile
    ensure_download_stream(c);
    if (!F.downRead[b]) S360_HIP(hipEventCreateWithFlags(&F.downRead[b], hipEventDisableTiming));
    S360_HIP(hipStreamWaitEvent(c->stDown, F.outDone[b], 0));
    S360_HIP(hipMemcpyAsync(out_bgr, F.cubeBGR[b].p, (size_t)F.cubeOutW[b] * F.cubeOutH[b] * 3, hipMemcpyDeviceToHost, c->stDown));
    if (F.outErrDev[b].p) S360_HIP(hipMemcpyAsync(c->downErr, F.outErrDev[b].p, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stDown));
    S360_HIP(hipEventRecord(F.downRead[b], c->stDown));
    S360_HIP(hipEventRecord(c->evDown, c->stDown));
    const hipEvent_t ev = c->evDown;
    const unsigned* errw = F.outErrDev[b].p ? c->downErr : nullptr;
    lk.unlock();
    const hipError_t rc = hipEventSynchronize(ev);
    lk.lock();
    S360_HIP(rc);
    if (errw && (errw[0] | errw[1] | errw[2])) {
      for (FlowEngine* e : {c->flow.get(), c->flow_pole.get(), c->flow_pr.get()})
        if (e) (void)e->take_error(c->st);
      throw Error(S360_ERR_HIP, "banded sweep timed out waiting for a neighbour band (results invalid)");
    }
  });
}
int s360_frame_download_cubemap(s360_ctx* c, int age, uint8_t* out_bgr) { return download_cubemap_impl(c, -1, age, out_bgr); }
int s360_frame_download_cubemap_slot(s360_ctx* c, int slot, int age, uint8_t* out_bgr) {
  if (slot < 0) return S360_ERR_INVALID_ARG;
  return download_cubemap_impl(c, slot, age, out_bgr);
}
size_t s360_frame_cubemap_png_bound(s360_ctx* c) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] {
    if (c->cube_fw > 0 && c->cube_fh > 0)
      n = PngPlan::make(c->cube_video ? 3 * c->cube_fw : c->cube_fw, c->cube_video ? 4 * c->cube_fh : 12 * c->cube_fh).file_bound;
  });
  return n;
}
static int download_cubemap_png_impl(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(out && n_out && (age == 0 || age == 1), "bad argument (age is 0 = latest enqueued frame or 1 = the one before)");
    FrameState& F = slot_state(c, slot);
    const int b = cube_buffer(c, F, age);
    if (F.cubePngFrame[b] != F.frames_done - 1 - age || !F.cubePngFile[b].p)
      throw Error(S360_ERR_STATE, "that frame was rendered without s360_set_png_encode");
    if (!F.downRead[b]) S360_HIP(hipEventCreateWithFlags(&F.downRead[b], hipEventDisableTiming));
    png_fetch(c, lk, F.cubePngPlan[b], F.cubePngMeta[b], F.cubePngFile[b], F.outDone[b], F.downRead[b], F.outErrDev[b].p, out, cap, n_out);
  });
}
int s360_frame_download_cubemap_png(s360_ctx* c, int age, uint8_t* out, size_t cap, size_t* n_out) {
  return download_cubemap_png_impl(c, -1, age, out, cap, n_out);
}
int s360_frame_download_cubemap_png_slot(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  if (slot < 0) return S360_ERR_INVALID_ARG;
  return download_cubemap_png_impl(c, slot, age, out, cap, n_out);
}

int s360_frame_cubemap(s360_ctx* c, int face_w, int face_h, const char* format, int whc[3], uint8_t* out_bgr) {
  return frame_guard(c, [&] {
    need(c && format && whc, "bad argument");
    const std::string f(format);
    if (f != "video" && f != "photo")  // CvUtil.cpp:134-137
      throw Error(S360_ERR_INVALID_ARG, "unexpected cubemap format: " + f + ". valid formats are: video,photo");
    need(face_w > 0 && face_h > 0 && face_w <= 16384 && face_h <= 16384, "cubemap face size must be in 1..16384");
    whc[0] = f == "video" ? 3 * face_w : face_w;
    whc[1] = f == "video" ? 4 * face_h : 12 * face_h;
    whc[2] = 3;
    if (!out_bgr) return;
    int ow = 0, oh = 0;
    wait_finish_stream(c);  // the cubemap kernel reads the composited panoramas
    frame_cubemap(c, face_w, face_h, f == "video", &ow, &oh);
    d2h(c, out_bgr, frame_state(c).cubeOut.p, (size_t)ow * oh * 3);
  });
}
// Where the named 8-bit intermediate of the selected slot's latest frame lies on the device (the names of s360_frame_get_u8).
// `pack_eye`: eye_l / eye_r are packed to B,G,R into op_f (the caller wants their pixels, not only their size).
static const void* frame_u8_source(s360_ctx* c, FrameState& F, const std::string& n, int idx, bool pack_eye, int& w, int& h, int& ch) {
  const s360_geometry& g = c->g;
  const int W = c->P.eqr_width, H = c->P.eqr_height, P = F.P;
  const void* src = nullptr;
  w = 0; h = 0; ch = 4;
  const int nloc = F.side_p1 - F.side_p0;
  if (n == "projection") {
    need(idx >= 0 && idx < P && F.sc->proj.p, "projection not available");
    w = g.cam_image_width; h = g.cam_image_height;
    src = F.sc->proj.as<uchar4>() + (size_t)w * h * idx;
  } else if (n == "overlap_l" || n == "overlap_r") {
    need(idx >= F.side_p0 && idx < F.side_p1 && F.overlaps[F.last_side].p, "overlap not available");
    w = g.overlap_image_width; h = g.cam_image_height;
    const int j = idx - F.side_p0 + (n == "overlap_r" ? nloc : 0);
    src = F.overlaps[F.last_side].as<uchar4>() + (size_t)w * h * j;
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
    const int slot = n == "extended_side" ? idx : (idx < 2 ? 4 : 5);
    src = F.extImgs[F.last_pole].as<uchar4>() + F.extStride * slot;
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
int s360_frame_get_u8(s360_ctx* c, const char* name, int idx, int whc[3], uint8_t* dst) {
  return frame_guard(c, [&] {
    need(c && name && whc, "bad argument");
    int w = 0, h = 0, ch = 4;
    const void* src = frame_u8_source(c, frame_state(c), name, idx, dst != nullptr, w, h, ch);
    whc[0] = w; whc[1] = h; whc[2] = ch;
    if (dst) d2h(c, dst, src, (size_t)w * h * ch);
  });
}
/* ---- PNG files of B,G,R and B,G,R,A images, one or many per launch sequence (include/s360_state_png.h) ---- */
size_t s360_png_bound_c(int w, int h, int channels) {
  size_t n = 0;
  (void)guard(nullptr, [&] { n = PngPlan::make(w, h, channels).file_bound; });
  return n;
}
int s360_encode_png_c(s360_ctx* c, const uint8_t* px, int w, int h, int channels, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(px && out && n_out && w > 0 && h > 0, "bad argument");
    const PngPlan plan = PngPlan::make(w, h, channels);
    const size_t nb = (size_t)w * h * channels;
    c->op_a.ensure((nb + 3) & ~(size_t)3);
    c->op_b.ensure(plan.file_bound);
    S360_HIP(hipMemcpyAsync(c->op_a.p, px, nb, hipMemcpyHostToDevice, c->st));
    png_encode_enqueue(c->st, c->op_a.as<uint8_t>(), plan, c->op_c, c->op_d, c->op_b.as<uint8_t>());
    S360_HIP(hipStreamSynchronize(c->st));
    png_fetch(c, lk, plan, c->op_d, c->op_b, nullptr, nullptr, nullptr, out, cap, n_out, false);  // (the operator scratch stays locked)
  }, false);
}
// A batch's plan and its page-locked areas. The table's host copy is rewritten here: the upload of the batch before (a whole encode
// ago) has left it in any real use; if it has not, this is the one place that waits for it.
static void png_batch_prepare(s360_ctx* c, s360_ctx::PngBatch& B, const std::vector<PngPlan>& plans) {
  if (!B.events) {
    S360_HIP(hipEventCreateWithFlags(&B.evEnc, hipEventDisableTiming));
    S360_HIP(hipEventCreateWithFlags(&B.evRead, hipEventDisableTiming));
    S360_HIP(hipEventCreateWithFlags(&B.evAfter, hipEventDisableTiming));
    B.events = true;
  }
  if (B.haveEnc && hipEventQuery(B.evEnc) != hipSuccess) {
    (void)hipGetLastError();
    S360_HIP(hipEventSynchronize(B.evEnc));
  }
  B.haveEnc = false;
  B.plan = PngBatchPlan::make(plans);
  auto grow = [](void*& p, size_t& have, size_t want) {
    if (have >= want) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    have = 0;
    S360_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    have = want;
  };
  grow(B.tabHost, B.tabHostBytes, PngBatchPlan::table_bytes(plans.size(), (size_t)B.plan.nbands));
  grow(B.metaHost, B.metaHostBytes, B.plan.meta_records * sizeof(PngBandMeta));
}
// ... and its launch sequence on the context's stream, the band tables' copy to the host behind it. Nothing waits.
static void png_batch_run(s360_ctx* c, s360_ctx::PngBatch& B, const uint8_t* const* px) {
  if (B.haveRead) S360_HIP(hipStreamWaitEvent(c->st, B.evRead, 0));  // (a fetch of the batch before may still read its file images)
  png_batch_enqueue(c->st, px, B.plan, B.table, B.tabHost, B.scratch, B.meta, B.files);
  S360_HIP(hipMemcpyAsync(B.metaHost, B.meta.p, B.plan.meta_records * sizeof(PngBandMeta), hipMemcpyDeviceToHost, c->st));
  S360_HIP(hipEventRecord(B.evEnc, c->st));
  B.haveEnc = true;
  ++B.gen;
}
// File i of the batch into the caller's buffer. Everything the transfer needs is enqueued, and the read-done event recorded, BEFORE
// the lock is first released; plan, pointers and the batch's generation are taken by value. The file's size is known up front when
// the band tables have already arrived (the usual case from the second file on); otherwise as much as the caller's buffer or the
// file's bound allows is copied, and the size is checked afterwards — a buffer that turns out too small is refused, never overrun.
static void png_batch_fetch(s360_ctx* c, std::unique_lock<std::recursive_mutex>& lk, s360_ctx::PngBatch& B, int i, uint8_t* out, size_t cap,
                            size_t* n_out, bool release) {
  if (!B.haveEnc) throw Error(S360_ERR_STATE, "no PNG batch has been encoded");
  need(i >= 0 && (size_t)i < B.plan.img.size(), "PNG index out of range");
  need(out && n_out, "bad argument");
  const PngPlan plan = B.plan.img[(size_t)i];
  const uint8_t* file = B.files.as<uint8_t>() + B.plan.file_off[(size_t)i];
  const PngBandMeta* mh = static_cast<const PngBandMeta*>(B.metaHost) + B.plan.meta0[(size_t)i];
  const unsigned long long gen = B.gen;
  const char* too_small = "png: output buffer too small (s360_frame_state_png_bound / s360_png_bound_c give the size to allocate)";
  if (!c->stDown) S360_HIP(hipStreamCreateWithFlags(&c->stDown, hipStreamNonBlocking));
  std::vector<PngBandMeta> m((size_t)plan.nbands + 1);
  const bool known = hipEventQuery(B.evEnc) == hipSuccess;
  if (!known) (void)hipGetLastError();
  size_t nbytes = std::min(cap, plan.file_bound);
  if (known) {
    std::memcpy(m.data(), mh, m.size() * sizeof(PngBandMeta));
    nbytes = (size_t)m[(size_t)plan.nbands].file_off;
    if (nbytes > plan.file_bound || nbytes + 28 > cap) throw Error(S360_ERR_INVALID_ARG, too_small);
  }
  hipEvent_t ev = nullptr;  // (an event per call: fetches of different files may wait at the same time)
  S360_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventBlockingSync));
  struct Drop { hipEvent_t e; ~Drop() { (void)hipEventDestroy(e); } } drop{ev};
  S360_HIP(hipStreamWaitEvent(c->stDown, B.evEnc, 0));
  S360_HIP(hipMemcpyAsync(out, file, nbytes, hipMemcpyDeviceToHost, c->stDown));
  S360_HIP(hipEventRecord(B.evRead, c->stDown));
  B.haveRead = true;
  S360_HIP(hipEventRecord(ev, c->stDown));
  if (release) lk.unlock();
  const hipError_t rc = hipEventSynchronize(ev);
  if (release) lk.lock();
  S360_HIP(rc);
  if (B.gen != gen) throw Error(S360_ERR_STATE, "the PNG batch was replaced by a later encode while this file was being fetched");
  if (!known) {
    std::memcpy(m.data(), mh, m.size() * sizeof(PngBandMeta));
    const size_t end = (size_t)m[(size_t)plan.nbands].file_off;
    if (end > plan.file_bound || end + 28 > cap) throw Error(S360_ERR_INVALID_ARG, too_small);
  }
  // the file's frame around the bands and the chunks' CRCs: host work on the caller's buffer and on copies, the context stays free
  if (release) lk.unlock();
  const size_t n = png_finish_host(out, cap, plan, m.data(), png_crc_threads());
  if (release) lk.lock();
  *n_out = n;
}
int s360_encode_png_batch(s360_ctx* c, int n, const uint8_t* const* px, const int* w, const int* h, const int* channels, uint8_t* const* out,
                          const size_t* cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(n > 0 && n <= 4096 && px && w && h && channels && out && cap && n_out, "bad argument");
    std::vector<PngPlan> plans;
    std::vector<size_t> at;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
      need(px[i] && out[i], "bad argument");
      plans.push_back(PngPlan::make(w[i], h[i], channels[i]));
      at.push_back(total);
      total += ((size_t)w[i] * h[i] * channels[i] + 15) & ~(size_t)15;
    }
    c->op_a.ensure(total);
    std::vector<const uint8_t*> dev;
    for (int i = 0; i < n; ++i) {
      dev.push_back(c->op_a.as<uint8_t>() + at[(size_t)i]);
      S360_HIP(hipMemcpyAsync(c->op_a.as<uint8_t>() + at[(size_t)i], px[i], (size_t)w[i] * h[i] * channels[i], hipMemcpyHostToDevice, c->st));
    }
    png_batch_prepare(c, c->opPng, plans);
    png_batch_run(c, c->opPng, dev.data());
    S360_HIP(hipStreamSynchronize(c->st));
    for (int i = 0; i < n; ++i) png_batch_fetch(c, lk, c->opPng, i, out[i], cap[i], &n_out[i], false);  // (the operator scratch stays locked)
  }, false);
}
int s360_frame_encode_state_pngs(s360_ctx* c, int n, const char* const* names, const int* idx) {
  return frame_guard(c, [&] {
    need(c && n > 0 && n <= 4096 && names && idx, "bad argument");
    FrameState& F = frame_state(c);
    std::vector<PngPlan> plans;
    std::vector<const uint8_t*> px;
    for (int i = 0; i < n; ++i) {
      need(names[i] != nullptr, "bad argument");
      int w = 0, h = 0, ch = 0;
      const void* src = frame_u8_source(c, F, names[i], idx[i], false, w, h, ch);
      need(ch == 4 && src, "only the 4-channel intermediates are encoded as state images");
      plans.push_back(PngPlan::make(w, h, 4));
      px.push_back(static_cast<const uint8_t*>(src));
    }
    s360_ctx::PngBatch& B = c->statePng;
    png_batch_prepare(c, B, plans);
    if (c->st2) {  // frame pipelining: the pole stage's images come from the finish stream — ordered on the device, not by the host
      S360_HIP(hipEventRecord(B.evAfter, c->st2));
      S360_HIP(hipStreamWaitEvent(c->st, B.evAfter, 0));
    }
    png_batch_run(c, B, px.data());
  });
}
size_t s360_frame_state_png_bound(s360_ctx* c, int i) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] {
    const s360_ctx::PngBatch& B = c->statePng;
    if (!B.haveEnc) throw Error(S360_ERR_STATE, "no PNG batch has been encoded");
    need(i >= 0 && (size_t)i < B.plan.img.size(), "PNG index out of range");
    n = B.plan.img[(size_t)i].file_bound;
  });
  return n;
}
int s360_frame_download_state_png(s360_ctx* c, int i, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) { png_batch_fetch(c, lk, c->statePng, i, out, cap, n_out, true); });
}
/* ---- banded PNG files decoded on the device (include/s360_png_decode.h, png_decode.hip) ---- */
static const char* const kNotDecodable = "not a banded PNG file of this decoder";
int s360_png_decodable(const uint8_t* file, size_t n, int whc[3], int* band_rows) {
  return guard(nullptr, [&] {
    need(whc && band_rows, "bad argument");
    PngBandedInfo I;
    if (!png_parse_banded(file, n, I)) throw Error(S360_ERR_INVALID_ARG, kNotDecodable);
    whc[0] = I.w; whc[1] = I.h; whc[2] = I.channels;
    *band_rows = I.band_rows;
  });
}
// the files of a call parsed; throws naming the first image that is not this decoder's
// a decode call fails because of file `image`: remembered for s360_png_decode_failure
[[noreturn]] static void png_fail(s360_ctx* c, int image, int reason, const std::string& msg) {
  c->pngDecFailImage = image;
  c->pngDecFailReason = reason;
  throw Error(S360_ERR_INVALID_ARG, msg);
}
static std::vector<PngBandedInfo> png_parse_all(s360_ctx* c, int n, const uint8_t* const* files, const size_t* bytes) {
  c->pngDecFailImage = -1;
  c->pngDecFailReason = S360_PNG_DECODE_FAILURE_NONE;
  std::vector<PngBandedInfo> info((size_t)n);
  for (int i = 0; i < n; ++i) {
    need(files[i] != nullptr, "bad argument");
    if (!png_parse_banded(files[i], bytes[i], info[(size_t)i]))
      png_fail(c, i, S360_PNG_DECODE_FAILURE_NOT_DECODABLE, "png decode: image " + std::to_string(i) + ": " + kNotDecodable);
  }
  return info;
}
// the launch sequence; a damaged file is remembered for s360_png_decode_failure
static void png_decode_checked(s360_ctx* c, int n, const uint8_t* const* files, const std::vector<PngBandedInfo>& info, const std::vector<uint8_t*>& dst) {
  try {
    png_decode_run(c->st, c->pngDec, std::vector<const uint8_t*>(files, files + n), info, dst, c->pngDecStats, &c->prof);
  } catch (const PngDecodeError& e) {
    c->pngDecFailImage = e.image;
    c->pngDecFailReason = S360_PNG_DECODE_FAILURE_DAMAGED;
    throw;
  }
}
int s360_png_decode_failure(s360_ctx* c, int* image, int* reason) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(image && reason, "bad argument");
    *image = c->pngDecFailImage;
    *reason = c->pngDecFailReason;
  });
}
int s360_decode_png_batch(s360_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, uint8_t* const* out, const size_t* cap,
                          int* whc_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>&) {
    need(n > 0 && n <= 4096 && files && bytes && out && cap, "bad argument");
    const std::vector<PngBandedInfo> info = png_parse_all(c, n, files, bytes);
    std::vector<size_t> at;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
      const PngBandedInfo& I = info[(size_t)i];
      const size_t nb = (size_t)I.w * I.h * I.channels;
      need(out[i] != nullptr, "bad argument");
      if (cap[i] < nb) png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + ": output buffer too small");
      at.push_back(total);
      total += (nb + 15) & ~(size_t)15;
    }
    c->op_a.ensure(total);
    std::vector<uint8_t*> dst;
    for (int i = 0; i < n; ++i) dst.push_back(c->op_a.as<uint8_t>() + at[(size_t)i]);
    png_decode_checked(c, n, files, info, dst);
    for (int i = 0; i < n; ++i) {
      const PngBandedInfo& I = info[(size_t)i];
      S360_HIP(hipMemcpyAsync(out[i], dst[(size_t)i], (size_t)I.w * I.h * I.channels, hipMemcpyDeviceToHost, c->st));
      if (whc_out) { whc_out[3 * i] = I.w; whc_out[3 * i + 1] = I.h; whc_out[3 * i + 2] = I.channels; }
    }
    S360_HIP(hipStreamSynchronize(c->st));
  }, false);
}
int s360_png_decode_stats(s360_ctx* c, uint64_t out[4]) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(out != nullptr, "bad argument");
    for (int k = 0; k < 4; ++k) out[k] = c->pngDecStats[k];
  });
}
int s360_png_decode_round_histogram(s360_ctx* c, uint64_t hist[66]) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(hist != nullptr, "bad argument");
    for (int k = 0; k < 66; ++k) hist[k] = c->pngDecStats[4 + k];
  });
}
// A set of previous-state halves is complete: mark the state as handed in, exactly as s360_frame_set_prev_side / _pole /
// _pole_removal leave it.
static void prev_side_arrived(FrameState& F, int pair, unsigned bits) {
  if (F.prevSideGot.size() < (size_t)F.P) F.prevSideGot.resize((size_t)F.P, 0);
  unsigned char& g = F.prevSideGot[(size_t)pair];
  g |= (unsigned char)bits;
  if (g == 15) { g = 0; F.have_prev_side = true; }
}
static void prev_pole_arrived(s360_ctx* c, FrameState& F, int unit, unsigned bits) {
  unsigned char& g = F.prevPoleGot[unit];
  g |= (unsigned char)bits;
  if (g == 7) {
    g = 0;
    F.extW = int(float(c->P.eqr_width) * 1.2f);
    F.extStride = (size_t)F.extW * std::max(c->g.top_rows, c->g.bottom_rows);
    F.poleRowsT = c->g.top_rows;
    F.poleRowsB = c->g.bottom_rows;
    F.have_prev_pole = true;
  }
}
static void prev_pr_arrived(FrameState& F, unsigned bits) {
  F.prevPrGot |= (unsigned char)bits;
  if (F.prevPrGot == 7) { F.prevPrGot = 0; F.have_prev_pr = true; }
}
// the block of pairs the previous side state is laid out for (as s360_frame_set_prev_side)
static void prev_side_block(FrameState& F, int pair, int& j, int& n) {
  need(pair >= 0 && pair < F.P, "pair_idx out of range");
  if (!F.partition_declared) { F.side_p0 = 0; F.side_p1 = F.P; }
  need(pair >= F.side_p0 && pair < F.side_p1, "pair_idx outside the block declared with s360_frame_set_partition");
  j = pair - F.side_p0;
  n = F.side_p1 - F.side_p0;
}
int s360_frame_set_prev_images_png(s360_ctx* c, int n, const char* const* names, const int* idx, const uint8_t* const* files,
                                   const size_t* bytes) {
  return frame_guard(c, [&] {
    need(c && n > 0 && n <= 4096 && names && idx && files && bytes, "bad argument");
    FrameState& F = frame_state(c);
    const std::vector<PngBandedInfo> info = png_parse_all(c, n, files, bytes);
    const size_t on = (size_t)c->g.overlap_image_width * c->g.cam_image_height;
    const int extW = int(float(c->P.eqr_width) * 1.2f);
    const size_t xs = (size_t)extW * std::max(c->g.top_rows, c->g.bottom_rows);
    // where every image goes, and what it must look like; the buffers are sized as the raw-pixel calls size them
    struct Arrival { int kind, k; unsigned bits; };  // kind 0 pair, 1 pole unit, 2 pole removal
    std::vector<uint8_t*> dst;
    std::vector<Arrival> arr;
    int prW = 0, prH = 0;
    for (int i = 0; i < n; ++i) {
      need(names[i] != nullptr, "bad argument");
      const std::string nm(names[i]);
      const PngBandedInfo& I = info[(size_t)i];
      int w = 0, h = 0;
      uchar4* p = nullptr;
      if (nm == "overlap_l" || nm == "overlap_r") {
        int j = 0, nloc = 0;
        prev_side_block(F, idx[i], j, nloc);
        F.overlaps[F.last_side].ensure(2 * nloc * on * sizeof(uchar4));
        w = c->g.overlap_image_width; h = c->g.cam_image_height;
        p = F.overlaps[F.last_side].as<uchar4>() + on * (size_t)(nm == "overlap_r" ? nloc + j : j);
        arr.push_back({0, idx[i], nm == "overlap_r" ? 2u : 1u});
      } else if (nm == "extended_side" || nm == "extended_fisheye") {
        need(idx[i] >= 0 && idx[i] < 4, "pole unit out of range");
        F.extImgs[F.last_pole].ensure(6 * xs * sizeof(uchar4));
        w = extW; h = idx[i] < 2 ? c->g.top_rows : c->g.bottom_rows;
        p = F.extImgs[F.last_pole].as<uchar4>() + xs * (size_t)(nm == "extended_side" ? idx[i] : (idx[i] < 2 ? 4 : 5));
        arr.push_back({1, idx[i], nm == "extended_side" ? 1u : 2u});
      } else if (nm == "bottom_image" || nm == "bottom_image2") {
        need(c->P.enable_pole_removal != 0, "this context does not run pole removal");
        if (!prW) { prW = I.w; prH = I.h; }
        const size_t pn = (size_t)prW * prH;
        F.prImgs[F.last_pr].ensure(2 * pn * sizeof(uchar4));
        w = prW; h = prH;
        if (F.poleW > 0 && (F.poleW != prW || F.poleH != prH))
          png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + " (" + nm + "): not the size of the bottom camera's image");
        p = F.prImgs[F.last_pr].as<uchar4>() + (nm == "bottom_image2" ? pn : 0);
        arr.push_back({2, 0, nm == "bottom_image2" ? 2u : 1u});
      } else {
        throw Error(S360_ERR_INVALID_ARG, "not a previous-state image name: " + nm);
      }
      if (I.channels != 4 || I.w != w || I.h != h)
        png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + " (" + nm + "): wrong size/channels for the previous state");
      dst.push_back(reinterpret_cast<uint8_t*>(p));
    }
    // (a later ensure() of a buffer an earlier image of this call points into would move it: sizes per buffer are the same for
    // every image of a kind, except pole removal, whose size the first such image fixes)
    png_decode_checked(c, n, files, info, dst);
    for (const Arrival& a : arr) {
      if (a.kind == 0) prev_side_arrived(F, a.k, a.bits);
      else if (a.kind == 1) {
        // the fisheye image is shared by the two units of a pole
        if (a.bits == 2u) { prev_pole_arrived(c, F, a.k, 2u); prev_pole_arrived(c, F, a.k ^ 1, 2u); }
        else prev_pole_arrived(c, F, a.k, 1u);
      } else {
        F.prevPrW = prW; F.prevPrH = prH;
        prev_pr_arrived(F, a.bits);
      }
    }
  });
}
int s360_frame_set_prev_flow(s360_ctx* c, const char* name, int idx, const float* flow) {
  return frame_guard(c, [&] {
    need(c && name && flow, "bad argument");
    FrameState& F = frame_state(c);
    const std::string nm(name);
    if (nm == "flow_l_to_r" || nm == "flow_r_to_l") {
      int j = 0, nloc = 0;
      prev_side_block(F, idx, j, nloc);
      const size_t on = (size_t)c->g.overlap_image_width * c->g.cam_image_height;
      F.sideFlows.ensure(2 * nloc * on * sizeof(float2));
      h2d(c, F.sideFlows.as<float2>() + on * (size_t)(nm == "flow_r_to_l" ? nloc + j : j), flow, on * sizeof(float2));
      S360_HIP(hipStreamSynchronize(c->st));
      prev_side_arrived(F, idx, nm == "flow_r_to_l" ? 8u : 4u);
    } else if (nm == "flow_pole") {
      need(idx >= 0 && idx < 4, "pole unit out of range");
      const int extW = int(float(c->P.eqr_width) * 1.2f);
      const size_t xs = (size_t)extW * std::max(c->g.top_rows, c->g.bottom_rows);
      const size_t xn = (size_t)extW * (idx < 2 ? c->g.top_rows : c->g.bottom_rows);
      F.poleFlows.ensure(4 * xs * sizeof(float2));
      h2d(c, F.poleFlows.as<float2>() + xs * (size_t)idx, flow, xn * sizeof(float2));
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
    const int nloc = F.side_p1 - F.side_p0;
    if (n == "flow_l_to_r" || n == "flow_r_to_l") {
      need(idx >= F.side_p0 && idx < F.side_p1 && F.sideFlows.p, "flow not available");
      w = g.overlap_image_width; h = g.cam_image_height;
      const int j = idx - F.side_p0 + (n == "flow_r_to_l" ? nloc : 0);
      src = F.sideFlows.as<float2>() + (size_t)w * h * j;
    } else if (n == "flow_bottom_secondary") {
      need(F.prFlow[F.last_pr].p && F.have_prev_pr, "not available (pole removal not run)");
      w = F.poleW; h = F.poleH;
      src = F.prFlow[F.last_pr].p;
    } else if (n == "flow_pole") {
      need(idx >= 0 && idx < 4 && F.poleFlows.p, "flow not available");
      w = F.extW; h = idx < 2 ? F.poleRowsT : F.poleRowsB;
      src = F.poleFlows.as<float2>() + F.extStride * idx;
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
  return guard(nullptr, [&] {
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
  return guard(nullptr, [&] {
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


// ---- soft ISP (isp.cpp / isp_kernels.hip; Raw2Rgb's non-accelerated path, CameraIsp.h) ------------------------------
void s360_isp_config_defaults(s360_isp_config* cfg) {
  if (cfg) isp_config_defaults(cfg);
}
int s360_isp_config_from_json(const char* json_text, s360_isp_config* cfg) {
  return guard(nullptr, [&] {
    need(json_text && cfg, "null argument");
    isp_config_from_json(json_text, cfg);
  });
}
int s360_isp_create(s360_isp** out, int device, const s360_isp_config* cfg) {
  if (!out) return S360_ERR_INVALID_ARG;
  *out = nullptr;
  s360_isp* o = nullptr;
  const int rc = guard(nullptr, [&] {
    need(cfg != nullptr, "null argument");
    o = new s360_isp;
    isp_init(o, device, *cfg);
  });
  if (rc != S360_OK) {
    if (o) isp_release(o);
    delete o;
    return rc;
  }
  *out = o;
  return S360_OK;
}
void s360_isp_destroy(s360_isp* isp) {
  if (!isp) return;
  isp_release(isp);
  delete isp;
}
int s360_isp_process(s360_isp* isp, const uint16_t* raw16, int w, int h, void* out_bgr) {
  return guard(nullptr, [&] {
    need(isp && raw16 && out_bgr && w > 0 && h > 0, "bad argument");
    isp_process(isp, raw16, w, h, out_bgr);
  });
}
int s360_isp_process_packed(s360_isp* isp, const uint8_t* frame, int bits, int w, int h, void* out_bgr) {
  return guard(nullptr, [&] {
    need(isp && frame && out_bgr && w > 0 && h > 0, "bad argument");
    isp_process_packed(isp, frame, bits, w, h, out_bgr);
  });
}
// test tap (include/s360_debug_isp.h): the ISP's intermediates where the product's own launch sequence leaves them
int s360_debug_isp_stages(s360_isp* isp, const uint16_t* raw16, int w, int h, int stop_after, float* plane, uint8_t* flag, float* gv,
                          float* gh, float* green, float* tone, float* low, void* out_bgr) {
  return guard(nullptr, [&] {
    need(isp && raw16 && w > 0 && h > 0, "bad argument");
    IspStageOut s;
    s.plane = plane; s.gv = gv; s.gh = gh; s.green = green; s.tone = tone; s.low = low; s.flag = flag; s.out = out_bgr;
    isp_debug_stages(isp, raw16, w, h, stop_after, s);
  });
}
/* ---- 16-bit PNG files, and the ISP's result as a finished PNG file (include/s360_isp_png.h) ---- */
size_t s360_png_bound_16(int w, int h) {
  size_t n = 0;
  (void)guard(nullptr, [&] { n = PngPlan::make(w, h, 3, 16).file_bound; });
  return n;
}
int s360_encode_png16(s360_ctx* c, const uint16_t* bgr16, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(bgr16 && out && n_out && w > 0 && h > 0, "bad argument");
    const PngPlan plan = PngPlan::make(w, h, 3, 16);
    need(cap >= plan.file_bound, "png: output buffer too small (s360_png_bound_16 gives the size to allocate)");
    const size_t nb = (size_t)w * h * 6;
    c->op_a.ensure((nb + 3) & ~(size_t)3);
    c->op_b.ensure(plan.file_bound);
    S360_HIP(hipMemcpyAsync(c->op_a.p, bgr16, nb, hipMemcpyHostToDevice, c->st));
    png_encode_enqueue(c->st, c->op_a.as<uint8_t>(), plan, c->op_c, c->op_d, c->op_b.as<uint8_t>());
    S360_HIP(hipStreamSynchronize(c->st));
    png_fetch(c, lk, plan, c->op_d, c->op_b, nullptr, nullptr, nullptr, out, cap, n_out, false);  // (the operator scratch stays locked)
  }, false);
}
static PngPlan isp_png_plan(const s360_isp* o, int w, int h) {
  const int r = o->cfg.resize > 0 ? o->cfg.resize : 1;
  return PngPlan::make(w / r, h / r, 3, o->cfg.output_bpp == 16 ? 16 : 8);
}
size_t s360_isp_png_bound(const s360_isp* isp, int w, int h) {
  size_t n = 0;
  if (!isp) return 0;
  (void)guard(nullptr, [&] { n = isp_png_plan(isp, w, h).file_bound; });
  return n;
}
// The encoder behind the ISP's kernels on the object's stream over `px` (the result on the device), the band table to its page-locked
// place: first wait. Then the file's bytes: second wait. Then the host's share on the caller's buffer.
static void isp_png_encode(s360_isp* o, const void* px, const PngPlan& plan, uint8_t* out, size_t cap, size_t* n_out) {
  const size_t mbytes = ((size_t)plan.nbands + 1) * sizeof(PngBandMeta);
  if (o->hPngMetaBytes < mbytes) {
    if (o->hPngMeta) (void)hipHostFree(o->hPngMeta);
    o->hPngMeta = nullptr;
    o->hPngMetaBytes = 0;
    S360_HIP(hipHostMalloc(&o->hPngMeta, mbytes, hipHostMallocDefault));
    o->hPngMetaBytes = mbytes;
  }
  o->dPngFile.ensure(plan.file_bound);
  png_encode_enqueue(o->st, static_cast<const uint8_t*>(px), plan, o->dPngScratch, o->dPngMeta, o->dPngFile.as<uint8_t>());
  isp_time_end(o);
  S360_HIP(hipMemcpyAsync(o->hPngMeta, o->dPngMeta.p, mbytes, hipMemcpyDeviceToHost, o->st));
  S360_HIP(hipStreamSynchronize(o->st));
  isp_time_take(o);
  const PngBandMeta* m = static_cast<const PngBandMeta*>(o->hPngMeta);
  const size_t end_bands = (size_t)m[plan.nbands].file_off;
  if (end_bands > plan.file_bound || end_bands + 28 > cap) throw Error(S360_ERR_STATE, "png: the band table names more bytes than the file's bound");
  S360_HIP(hipMemcpyAsync(out, o->dPngFile.p, end_bands, hipMemcpyDeviceToHost, o->st));
  S360_HIP(hipStreamSynchronize(o->st));
  *n_out = png_finish_host(out, cap, plan, m, png_crc_threads());
}
int s360_isp_process_png(s360_isp* isp, const uint16_t* raw16, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  return guard(nullptr, [&] {
    need(isp && raw16 && out && n_out && w > 0 && h > 0, "bad argument");
    const PngPlan plan = isp_png_plan(isp, w, h);
    need(cap >= plan.file_bound, "png: output buffer too small (s360_isp_png_bound gives the size to allocate)");
    isp_png_encode(isp, isp_develop(isp, "s360_isp_process_png", raw16, w, h), plan, out, cap, n_out);
  });
}
int s360_isp_process_packed_png(s360_isp* isp, const uint8_t* frame, int bits, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  return guard(nullptr, [&] {
    need(isp && frame && out && n_out && w > 0 && h > 0, "bad argument");
    const PngPlan plan = isp_png_plan(isp, w, h);
    need(cap >= plan.file_bound, "png: output buffer too small (s360_isp_png_bound gives the size to allocate)");
    isp_png_encode(isp, isp_develop_packed(isp, "s360_isp_process_packed_png", frame, bits, w, h), plan, out, cap, n_out);
  });
}
int s360_isp_pipe_generated(s360_isp* isp, const s360_camera_isp_gen_args* args) {
  return guard(nullptr, [&] {
    need(isp && args, "null argument");
    isp_pipe_generated(isp, *args);
  });
}
int s360_isp_config_tables(const s360_isp_config* cfg, float* ccm9, float* lut, int w, int h, float* curve_h,
                           float* curve_v) {
  return guard(nullptr, [&] {
    need(cfg != nullptr, "null argument");
    IspDev d;
    std::vector<float> l, ch, cv;
    isp_derive(*cfg, d, l);
    if (ccm9) std::memcpy(ccm9, d.ccm, 9 * sizeof(float));
    if (lut) std::memcpy(lut, l.data(), l.size() * sizeof(float));
    if (curve_h || curve_v) {
      need(w > 0 && h > 0, "bad frame size");
      isp_vignette_curves(*cfg, w, h, ch, cv);
      if (curve_h) std::memcpy(curve_h, ch.data(), ch.size() * sizeof(float));
      if (curve_v) std::memcpy(curve_v, cv.data(), cv.size() * sizeof(float));
    }
  });
}

}  // extern "C"
