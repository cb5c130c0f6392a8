// api_debug_images.hip — the reference's debug images through the C ABI (include/s360_debug_images.h): the switch, the list of a
// frame's images and their pixels, their PNG files as one device batch, pole removal as an operator; and the test tap of
// k_debug_views (include/s360_debug_views.h). The images themselves are kept by the frame's finish stage (render.hip
// debug_images_collect).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/s360.h"
#include "../../include/s360_debug_views.h"
#include "api_internal.hpp"
#include "debug_views.hpp"

using namespace s360;

namespace {

// the list of the selected slot's latest frame; S360_ERR_STATE when no frame was rendered with the switch on
const std::vector<FrameState::DebugImages::Img>& debug_list(s360_ctx* c) {
  FrameState& F = frame_state(c);
  if (!c->debug_images || F.dbg.frame < 0 || F.dbg.frame != F.frames_done - 1)
    throw Error(S360_ERR_STATE, "no debug images: render a frame after s360_set_debug_images(ctx, 1)");
  return F.dbg.list;
}

}  // namespace

extern "C" {

int s360_set_debug_images(s360_ctx* c, int on) {
  return frame_guard(c, [&] { need(c, "null ctx"); set_debug_images(c, on != 0); });
}
int s360_frame_debug_image_count(s360_ctx* c) {
  int n = 0;
  const int rc = frame_guard(c, [&] { need(c, "null ctx"); n = (int)debug_list(c).size(); });
  return rc < 0 ? rc : n;
}
int s360_frame_debug_image_info(s360_ctx* c, int i, char name[96], int whc[3]) {
  return frame_guard(c, [&] {
    need(c && name && whc, "bad argument");
    const auto& list = debug_list(c);
    need(i >= 0 && (size_t)i < list.size(), "debug image index out of range");
    std::memcpy(name, list[(size_t)i].name, 96);
    whc[0] = list[(size_t)i].w; whc[1] = list[(size_t)i].h; whc[2] = list[(size_t)i].ch;
  });
}
int s360_frame_get_debug_image(s360_ctx* c, int i, uint8_t* dst) {
  return frame_guard(c, [&] {
    need(c && dst, "bad argument");
    const auto& list = debug_list(c);
    need(i >= 0 && (size_t)i < list.size(), "debug image index out of range");
    const auto& m = list[(size_t)i];
    d2h(c, dst, m.px, (size_t)m.w * m.h * m.ch);
  });
}
int s360_frame_encode_debug_pngs(s360_ctx* c) {
  return frame_guard(c, [&] {
    need(c, "null ctx");
    const auto& list = debug_list(c);
    std::vector<PngPlan> plans;
    std::vector<const uint8_t*> px;
    for (const auto& m : list) {
      plans.push_back(PngPlan::make(m.w, m.h, m.ch));
      px.push_back(m.px);
    }
    // (frames with debug images are complete on the device when their render call returns: nothing to order behind)
    png_batch_prepare(c, c->debugPng, plans);
    png_batch_run(c, c->debugPng, px.data());
  });
}
size_t s360_frame_debug_png_bound(s360_ctx* c, int i) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] {
    const s360_ctx::PngBatch& B = c->debugPng;
    if (!B.haveEnc) throw Error(S360_ERR_STATE, "no PNG batch has been encoded");
    need(i >= 0 && (size_t)i < B.plan.img.size(), "PNG index out of range");
    n = B.plan.img[(size_t)i].file_bound;
  });
  return n;
}
int s360_frame_download_debug_png(s360_ctx* c, int i, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) { png_batch_fetch(c, lk, c->debugPng, i, out, cap, n_out, true); });
}

// combineBottomImagesWithPoleRemoval (PoleRemoval.cpp:32-188), prevFrameDataDir = "NONE": the launch sequence of render.hip
// dev_pole_removal on the operator scratch, with the call's own feather size and radii.
int s360_pole_removal_combine(s360_ctx* c, const uint8_t* bottom, const uint8_t* bottom2, const uint8_t* mask, const uint8_t* mask2, int w,
                              int h, float radius, float radius2, int flip180, int feather_size, const char* flow_alg,
                              uint8_t* bottom_image, uint8_t* bottom_image2, uint8_t* bottom_warp2, uint8_t* bottom_combined, float* flow) {
  return guard(c, [&] {
    need(c && bottom && bottom2 && mask && mask2 && flow_alg, "null argument");
    need(w >= 4 && h >= 4 && (size_t)w * h <= ((size_t)1 << 28), "image too small: the reference's bilinear taps need a 2x2 image after the x0.5 entry downscale (PixFlow.h:457-475)");
    need(feather_size >= 1 && feather_size <= 31 && feather_size % 2 == 1, "feather_size must be odd and in 1..31 (it is the GaussianBlur kernel size, CvUtil.cpp:151)");
    const PixFlowConsts pc = pixflow_consts_by_name(flow_alg);
    FrameState& F = frame_state(c);
    hipStream_t st = c->st;
    const size_t n = (size_t)w * h;
    // op_a: staging of a B,G,R upload; op_b: the two red-mask planes; op_c: bottomImage, bottomImage2 (the flow's inputs, adjacent);
    // op_d: the flow; op_e: the secondary image before its flip, then bottomWarp2; op_f: _bottomCombined
    c->op_a.ensure(n * 3); c->op_b.ensure(2 * n); c->op_c.ensure(2 * n * sizeof(uchar4)); c->op_d.ensure(n * sizeof(float2));
    c->op_e.ensure(n * sizeof(uchar4)); c->op_f.ensure(n * sizeof(uchar4));
    const int* taps = nullptr;
    DevBuf tapBuf;
    const bool std_size = feather_size == c->P.std_alpha_feather_size;
    if (!std_size) {
      const std::vector<int> t = feather_gauss_taps(feather_size);
      tapBuf.ensure(t.size() * sizeof(int));
      h2d(c, tapBuf.p, t.data(), t.size() * sizeof(int));
      S360_HIP(hipStreamSynchronize(st));  // (t leaves scope)
      taps = tapBuf.as<int>();
    }
    auto feather = [&](uchar4* img) {  // featherAlphaChannel, in place (extW == cols: every thread rewrites its own pixel)
      if (std_size) dev_feather_alpha_to_ext(c, img, w, h, img, w);
      else dev_feather_alpha_to_ext(c, img, w, h, img, w, feather_size, taps);
    };
    uchar4* img1 = c->op_c.as<uchar4>();
    uchar4* img2 = img1 + n;
    uchar4* tmp = c->op_e.as<uchar4>();
    const uint8_t* masks[2] = {mask, mask2};
    const uint8_t* srcs[2] = {bottom, bottom2};
    for (int k = 0; k < 2; ++k) {
      h2d(c, c->op_a.p, masks[k], n * 3);
      launch_red_mask(st, c->op_a.as<uint8_t>(), c->op_b.as<uint8_t>() + n * k, n);
      S360_HIP(hipStreamSynchronize(st));  // (the staging buffer takes the next upload)
    }
    for (int k = 0; k < 2; ++k) {
      uchar4* dst = k == 0 ? img1 : (flip180 ? tmp : img2);
      h2d(c, c->op_a.p, srcs[k], n * 3);
      launch_bgr_to_bgra(st, c->op_a.as<uint8_t>(), 3, dst, n);
      S360_HIP(hipStreamSynchronize(st));
      launch_circle_alpha(st, dst, c->op_b.as<uint8_t>() + n * k, dst, w, h, k == 0 ? radius : radius2);
      feather(dst);
    }
    if (flip180) launch_flip_both(st, tmp, img2, w, h, h);
    {
      FlowEngine& fe = flow_engine(c, 0);
      FlowBatch fb;
      fb.add_images(img1, 2, n);
      fb.add_flow(0, 1, c->op_d.as<float2>(), nullptr);
      fe.compute(st, pc, fb, w, h, S360_HINT_DOWN);
    }
    uchar4* warp = tmp;  // (the unflipped secondary image is dead)
    uchar4* merged = c->op_f.as<uchar4>();
    launch_remap_by_flow(st, img2, w, h, c->op_d.as<float2>(), warp, F.tab.dev);
    S360_HIP(hipMemcpyAsync(merged, img1, n * sizeof(uchar4), hipMemcpyDeviceToDevice, st));
    launch_pole_removal_combine(st, merged, warp, n);
    launch_circle_alpha(st, merged, nullptr, merged, w, h, radius);
    feather(merged);
    if (bottom_image) d2h(c, bottom_image, img1, n * sizeof(uchar4));
    if (bottom_image2) d2h(c, bottom_image2, img2, n * sizeof(uchar4));
    if (bottom_warp2) d2h(c, bottom_warp2, warp, n * sizeof(uchar4));
    if (bottom_combined) d2h(c, bottom_combined, merged, n * sizeof(uchar4));
    if (flow) d2h(c, flow, c->op_d.p, n * sizeof(float2));
    S360_HIP(hipStreamSynchronize(st));
    check_sweep_error(c);
  });
}

// test tap: k_debug_views on caller-made images and descriptors
int s360_debug_views(s360_ctx* c, int n, const s360_debug_view* views, const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t dst_bytes) {
  return guard(c, [&] {
    need(c && views && src && dst && src_bytes > 0 && dst_bytes > 0, "null argument");
    need(n >= 1 && n <= 65535, "1 .. 65535 views per launch");
    c->op_a.ensure(src_bytes);
    c->op_b.ensure(dst_bytes);
    std::vector<DebugViewDesc> tab((size_t)n);
    for (int i = 0; i < n; ++i) {
      const s360_debug_view& v = views[i];
      DebugViewDesc& d = tab[(size_t)i];
      need(v.src_pitch > 0 && v.src_rows > 0 && v.w > 0 && v.h > 0 && v.pad_rows >= 0 && (v.channels_out == 3 || v.channels_out == 4) &&
           v.w <= (1 << 24) && v.h <= (1 << 24) && v.pad_rows <= (1 << 24), "debug view: bad size or channel count");
      need(v.src_off <= src_bytes && (size_t)v.src_pitch * v.src_rows * 4 <= src_bytes - v.src_off, "debug view: the source lies outside the source area");
      need(v.dst_off <= dst_bytes && (size_t)v.w * ((size_t)v.h + v.pad_rows) * v.channels_out <= dst_bytes - v.dst_off,
           "debug view: the destination lies outside the destination area");
      d.src = c->op_a.as<uint8_t>() + v.src_off;
      d.dst = c->op_b.as<uint8_t>() + v.dst_off;
      d.src_pitch = v.src_pitch; d.src_rows = v.src_rows;
      d.x0 = v.x0; d.y0 = v.y0; d.w = v.w; d.h = v.h;
      d.shift = v.shift; d.pad_rows = v.pad_rows; d.channels_in = v.channels_in; d.channels_out = v.channels_out;
      debug_view_check(d);
    }
    c->op_c.ensure(tab.size() * sizeof(DebugViewDesc));
    h2d(c, c->op_a.p, src, src_bytes);
    h2d(c, c->op_b.p, dst, dst_bytes);
    h2d(c, c->op_c.p, tab.data(), tab.size() * sizeof(DebugViewDesc));
    launch_debug_views(c->st, c->op_c.as<DebugViewDesc>(), tab.data(), n);
    d2h(c, dst, c->op_b.p, dst_bytes);
  });
}

}  // extern "C"
