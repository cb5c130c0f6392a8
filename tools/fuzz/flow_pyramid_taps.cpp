// runs the flow-pyramid test taps (include/s360_debug_flow_pyramid.h) of the emulated, sanitised library at the smallest and the
// boundary shapes of tests/flow_pyramid_cases.py: the engine's preparation at 2 x 2 .. 5 x 5 after the entry downscale, on the tile's
// edges, with one and two levels, every planes-per-thread class, with and without previous state, a smaller call after a larger one; the
// linear resize on both sides of its dispatch rule, with boxes that fill the 76 x 20 floats of LDS, tiny sources and destinations,
// unaligned rows, 63 .. 66 workgroups; the cubic flow resize with windows that fill 72 x 24, sources of 1 .. 3 pixels, through the
// pointer table. Device buffers are heap blocks with red zones there, so a kernel's out-of-bounds access is a report with file and
// line; host buffers are heap blocks of exactly the sizes the header states. Prints one checksum line per call. argv: rig.json
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/s360.h"
#include "../../include/s360_debug_flow_pyramid.h"

static unsigned g_seed = 2468;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) / 16777216.0f; }
static unsigned sum(const void* p, size_t n) {
  unsigned s = 2166136261u;
  for (size_t i = 0; i < n; ++i) s = (s ^ static_cast<const uint8_t*>(p)[i]) * 16777619u;
  return s;
}
static const float kOdd[] = {0.f, -0.f, 40.f, -40.f, 1e-16f, 1e-40f, -1e-40f, 1.f};

static int prepare(s360_ctx* c, int w, int h, int N, int B, bool prev, int fill) {
  // the sizes of the levels, as the header states them: finest first, x0.9 rounded while both stay above 24
  int lw[64], lh[64], L = 0;
  size_t P = 0;
  for (int cw = w / 2, ch = h / 2;;) {
    lw[L] = cw; lh[L] = ch; ++L;
    P += (size_t)cw * ch;
    const int nw = int(cw * 0.9f + 0.5f), nh = int(ch * 0.9f + 0.5f);
    if (nw <= 24 || nh <= 24 || L >= 64) break;
    cw = nw; ch = nh;
  }
  const size_t n = (size_t)w * h;
  uint8_t* img = new uint8_t[N * n * 4];
  uint8_t* pimg = prev ? new uint8_t[N * n * 4] : nullptr;
  float* pflow = prev ? new float[B * n * 2] : nullptr;
  for (size_t i = 0; i < N * n * 4; ++i) img[i] = (uint8_t)(rnd() * 256);
  if (prev) {
    for (size_t i = 0; i < N * n * 4; ++i) pimg[i] = rnd() < 0.5f ? img[i] : (uint8_t)(rnd() * 256);
    for (size_t i = 0; i < B * n * 2; ++i) pflow[i] = rnd() < 0.2f ? kOdd[(int)(rnd() * 8)] : (rnd() * 2 - 1) * 9.f;
  }
  int* i0 = new int[B];
  int* i1 = new int[B];
  for (int b = 0; b < B; ++b) { i0[b] = b % N; i1[b] = (b + 1) % N; }
  int* gw = new int[L];
  int* gh = new int[L];
  float* fac = new float[L];
  float* pyr = new float[2 * N * P];
  float* ppyr = prev ? new float[B * P * 2] : nullptr;
  float* mpyr = prev ? new float[N * P] : nullptr;
  int nl = -1;
  s360_flow_prepare_out o;
  std::memset(&o, 0, sizeof o);
  o.cap_levels = L; o.cap_pixels = P;
  o.level_w = gw; o.level_h = gh; o.n_levels = &nl; o.factors = fac; o.pyr_images = pyr; o.prev_pyr = ppyr; o.motion_pyr = mpyr;
  const int rc = s360_debug_flow_prepare(c, img, N, w, h, i0, i1, B, pimg, pflow, "pixflow_low", fill, &o);
  bool sizes = rc == S360_OK && nl == L;
  for (int l = 0; sizes && l < L; ++l) sizes = gw[l] == lw[l] && gh[l] == lh[l];
  std::printf("prepare %dx%d N %d B %d prev %d fill %d: rc %d levels %d sizes %s images %08x prev %08x motion %08x\n", w, h, N, B, (int)prev, fill, rc, nl,
              sizes ? "ok" : "WRONG", rc ? 0 : sum(pyr, 2 * N * P * 4), (rc || !prev) ? 0 : sum(ppyr, B * P * 8), (rc || !prev) ? 0 : sum(mpyr, N * P * 4));
  delete[] img; delete[] pimg; delete[] pflow; delete[] i0; delete[] i1; delete[] gw; delete[] gh; delete[] fac; delete[] pyr; delete[] ppyr; delete[] mpyr;
  return rc || !sizes;
}
static int linear(s360_ctx* c, int sw, int sh, int dw, int dh, int cn, int B, int want_tiled) {
  const size_t ns = (size_t)sw * sh * cn, nd = (size_t)dw * dh * cn;
  float* src = new float[B * ns];
  float* dst = new float[B * nd];
  for (size_t i = 0; i < B * ns; ++i) src[i] = rnd() < 0.1f ? kOdd[(int)(rnd() * 8)] : rnd() * 2 - 1;
  std::memset(dst, 0xFF, B * nd * 4);
  int tiled = -1, asked = -1;
  const int rc0 = s360_debug_resize_linear_f32(nullptr, nullptr, sw, sh, cn, B, dw, dh, 1.f, 0, nullptr, &asked);  // report only
  const int rc = s360_debug_resize_linear_f32(c, src, sw, sh, cn, B, dw, dh, 1.0f / 0.9f, B & 1, dst, &tiled);
  size_t unwritten = 0;
  for (size_t i = 0; i < B * nd; ++i) { uint32_t v; std::memcpy(&v, dst + i, 4); unwritten += v == 0xFFFFFFFFu; }
  const bool ok = rc == S360_OK && rc0 == S360_OK && tiled == asked && (want_tiled < 0 || tiled == want_tiled) && unwritten == 0;
  std::printf("linear %dx%d -> %dx%d cn %d x%d: rc %d tiled %d unwritten %zu result %08x%s\n", sw, sh, dw, dh, cn, B, rc, tiled, unwritten, sum(dst, B * nd * 4),
              ok ? "" : " WRONG");
  delete[] src; delete[] dst;
  return !ok;
}
static int cubic(s360_ctx* c, int sw, int sh, int dw, int dh, int B, int table, int want_tiled) {
  const size_t ns = (size_t)sw * sh * 2, nd = (size_t)dw * dh * 2;
  float* src = new float[B * ns];
  float* dst = new float[B * nd];
  for (size_t i = 0; i < B * ns; ++i) src[i] = rnd() < 0.1f ? kOdd[(int)(rnd() * 8)] : (rnd() * 2 - 1) * 5.f;
  std::memset(dst, 0xFF, B * nd * 4);
  int tiled = -1;
  const int rc = s360_debug_resize_cubic_flow(c, src, sw, sh, B, dw, dh, 1.0f / 0.9f, table, dst, &tiled);
  size_t unwritten = 0;
  for (size_t i = 0; i < B * nd; ++i) { uint32_t v; std::memcpy(&v, dst + i, 4); unwritten += v == 0xFFFFFFFFu; }
  const bool ok = rc == S360_OK && tiled == want_tiled && unwritten == 0;
  std::printf("cubic %dx%d -> %dx%d x%d table %d: rc %d tiled %d unwritten %zu result %08x%s\n", sw, sh, dw, dh, B, table, rc, tiled, unwritten,
              sum(dst, B * nd * 4), ok ? "" : " WRONG");
  delete[] src; delete[] dst;
  return !ok;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<s360_camera> cams(24);
  const int n = s360_rig_load_json(argv[1], cams.data(), 24);
  if (n < 0) { std::fprintf(stderr, "rig: %s\n", s360_last_error(nullptr)); return 2; }
  s360_params P;
  std::memset(&P, 0, sizeof P);
  P.interpupilary_dist = 6.4; P.zero_parallax_dist = 10000; P.side_alpha_feather_size = 100; P.std_alpha_feather_size = 31;
  P.eqr_width = 252; P.eqr_height = 126; P.final_eqr_width = 240; P.final_eqr_height = 240;
  std::strcpy(P.side_flow_alg, "pixflow_low"); std::strcpy(P.polar_flow_alg, "pixflow_low");
  s360_ctx* c = nullptr;
  if (s360_create(&c, 0, cams.data(), n, &P) != S360_OK) { std::fprintf(stderr, "create: %s\n", s360_last_error(nullptr)); return 2; }
  int bad = 0;
  // the preparation: larger first, so that the later calls run in buffers that are larger than they need
  bad |= prepare(c, 142, 142, 3, 2, true, -1);     // 11 levels down to 25 x 25
  bad |= prepare(c, 140, 70, 4, 4, true, 0xFF);    // a 63 x 32 level; 4 planes per thread everywhere
  bad |= prepare(c, 131, 35, 3, 3, true, 0xFF);    // 65 x 17, one level, 1 / 2 planes per thread
  const int small[][2] = {{4, 4}, {5, 4}, {4, 7}, {6, 5}, {9, 8}, {10, 11}, {128, 32}, {126, 30}, {54, 55}, {56, 56}, {57, 54}};
  for (const auto& s : small)
    for (int prev = 0; prev <= 1; ++prev) bad |= prepare(c, s[0], s[1], 2, 1, prev != 0, prev ? -1 : 0xFF);
  for (int N = 1; N <= 4; ++N) bad |= prepare(c, 66, 58, N, 5 - N, true, 0xFF);
  // the linear resize: both sides of the rule, the full box, tiny shapes, unaligned rows, the grid classes
  const int lin[][5] = {{144, 18, 128, 16, 1}, {145, 18, 128, 16, 0}, {73, 18, 64, 16, 1}, {72, 38, 64, 32, 1}, {72, 39, 64, 32, 0}, {200, 18, 177, 16, 0},
                        {2, 2, 64, 16, 1}, {2, 2, 70, 20, 1}, {9, 7, 8, 6, 1}, {1, 1, 5, 4, 1}, {2, 1, 3, 1, 1}, {1, 2, 1, 5, 1}, {40, 40, 1, 1, 1},
                        {143, 37, 129, 33, 1}, {71, 17, 64, 16, 1}, {37, 21, 33, 19, 1}, {300, 30, 133, 27, 0}, {31, 300, 28, 100, 0}, {64, 16, 64, 16, 1}};
  for (const auto& l : lin)
    for (int B = 1; B <= 4; ++B) {
      bad |= linear(c, l[0], l[1], l[2], l[3], 1, B, l[4]);
      bad |= linear(c, l[0], l[1], l[2], l[3], 2, B, 0);
    }
  bad |= linear(c, 213, 124, 192, 112, 1, 3, 1);   // 63 workgroups
  bad |= linear(c, 284, 284, 256, 256, 1, 1, 1);   // 64
  bad |= linear(c, 71, 231, 64, 208, 1, 5, 1);     // 65
  bad |= linear(c, 111, 44, 100, 40, 1, 11, 1);    // 66, partial last tiles
  // the cubic flow resize: tiled upscales with the largest windows (ratio 1), tiny sources, generic downscales, the table
  const int cub[][5] = {{25, 25, 28, 28, 1}, {65, 44, 72, 49, 1}, {70, 20, 70, 20, 1}, {130, 40, 130, 40, 1}, {69, 23, 70, 24, 1}, {10, 5, 70, 35, 1},
                        {1, 1, 5, 4, 1}, {2, 1, 64, 3, 1}, {1, 3, 2, 17, 1}, {3, 2, 65, 16, 1}, {59, 16, 65, 17, 1}, {75, 60, 37, 30, 0}, {80, 20, 40, 40, 0},
                        {20, 80, 40, 40, 0}, {5, 4, 1, 1, 0}, {75, 75, 37, 37, 0}};
  for (const auto& q : cub)
    for (int B = 1; B <= 3; B += 2) {
      bad |= cubic(c, q[0], q[1], q[2], q[3], B, 0, q[4]);
      bad |= cubic(c, q[0], q[1], q[2], q[3], B, 1, 0);
    }
  bad |= cubic(c, 120, 230, 128, 256, 3, 0, 1);    // 96 workgroups
  s360_destroy(c);
  std::printf(bad ? "FAILED\n" : "all calls returned S360_OK\n");
  return bad ? 1 : 0;
}
