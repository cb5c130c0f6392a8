// api_ops.hip — the operator level of the C ABI (include/s360.h): one reference operator per call on the caller's images,
// through the context's operator scratch. Argument checks, host <-> device copies, the launchers of the frame.
#include <cstdlib>
#include <cstring>

#include "../../include/s360.h"
#include "api_internal.hpp"

using namespace s360;

extern "C" {

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
    const int extW = extended_width(W);
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

}  // extern "C"
