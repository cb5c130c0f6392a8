// api_taps.hip — the test taps of the C ABI (include/s360_debug*.h): single launchers and stages of the library on caller-made
// inputs, for the tests that compare them with the oracle. Not part of the product's interface.
#include <cstring>
#include <vector>

#include "../../include/s360.h"
#include "../../include/s360_debug.h"
#include "../../include/s360_debug_final_flow.h"
#include "../../include/s360_debug_flow_level.h"
#include "../../include/s360_debug_flow_pyramid.h"
#include "../../include/s360_debug_isp.h"
#include "../../include/s360_debug_cubemap.h"
#include "../../include/s360_debug_remap.h"
#include "api_internal.hpp"
#include "isp.hpp"

using namespace s360;

extern "C" {

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
// test tap (include/s360_debug_isp.h): the ISP's intermediates where the product's own launch sequence leaves them
int s360_debug_isp_stages(s360_isp* isp, const uint16_t* raw16, int w, int h, int stop_after, float* plane, uint8_t* flag, float* gv,
                          float* gh, float* green, float* tone, float* low, void* out_bgr) {
  return guard([&] {
    need(isp && raw16 && w > 0 && h > 0, "bad argument");
    IspStageOut s;
    s.plane = plane; s.gv = gv; s.gh = gh; s.green = green; s.tone = tone; s.low = low; s.flag = flag; s.out = out_bgr;
    isp_debug_stages(isp, raw16, w, h, stop_after, s);
  });
}

}  // extern "C"
