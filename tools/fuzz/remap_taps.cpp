// runs the remap test taps (include/s360_debug_remap.h) of the emulated, sanitised library at the edge shapes of
// tests/remap_packed_cases.py: sources of 1 .. 5 pixels, boxes at the LDS limit (64 x 64, 65 x 64, 4 x 1020, 4 x 1024), tiles without a
// live pixel, NaN / infinite / overflowing coordinates, every grid class of the tile re-deal, a feather longer than the image, the
// pole warp with a zero divisor in its ramp, gathered tiles. Device buffers are heap blocks with red zones there, so a kernel's
// out-of-bounds access is a report with file and line. Prints one checksum line per call. argv: rig.json
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/s360.h"
#include "../../include/s360_debug_remap.h"

static unsigned g_seed = 12345;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) / 16777216.0f; }
static unsigned sum(const void* p, size_t n) {
  unsigned s = 2166136261u;
  for (size_t i = 0; i < n; ++i) s = (s ^ static_cast<const uint8_t*>(p)[i]) * 16777619u;
  return s;
}
enum Kind { AROUND, NANS, FAR, BOX, TALL };
static const float kFar[] = {1e9f, -1e9f, 7e7f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                             std::numeric_limits<float>::quiet_NaN(), 40000.f, -40000.f, -0.0f};

static int remap(s360_ctx* c, int sw, int sh, int dw, int dh, int batch, int mode, int feather, int weights, Kind kind, int p0 = 0, int p1 = 0) {
  const size_t sn = (size_t)sw * sh, dn = (size_t)dw * dh, nt = (size_t)((dw + 63) / 64) * ((dh + 15) / 16);
  // (heap blocks of exactly the sizes the header states: the library reading or writing past them is a report too)
  uint8_t* src = new uint8_t[batch * sn * 4];
  float* map = new float[batch * dn * 2];
  uint8_t* dst = new uint8_t[batch * dn * 4];
  uint32_t* packed = new uint32_t[batch * dn];
  int32_t* tiles = new int32_t[batch * nt * 4];
  for (size_t i = 0; i < batch * sn * 4; ++i) src[i] = (uint8_t)(rnd() * 256);
  for (size_t i = 0; i < batch * dn; ++i) {
    float x = -3.4f + rnd() * (sw + 4.3f), y = -3.4f + rnd() * (sh + 4.3f);
    if (kind == NANS) x = y = kFar[5];
    if (kind == FAR && rnd() < 0.3f) (rnd() < 0.5f ? x : y) = kFar[(int)(rnd() * 9)];
    if (kind == BOX) { x = 11.f + rnd() * (p0 - 11.f); y = 6.f + rnd() * (p1 - 6.f); if (i % 64 == 0) { x = 11.f; y = 6.f; } if (i % 64 == 1) { x = (float)p0 + 1; y = (float)p1 + 1; } }
    if (kind == TALL) { x = 3.f; y = 11.f + rnd() * (p0 - 11.f); if (i % 64 == 0) y = 11.f; if (i % 64 == 1) y = (float)p0 + 1; }
    map[2 * i] = x; map[2 * i + 1] = y;
  }
  std::memset(dst, 0xA5, batch * dn * 4); std::memset(packed, 0xA5, batch * dn * 4); std::memset(tiles, 0xA5, batch * nt * 16);
  const int rc = s360_debug_remap_packed(c, src, sw, sh, map, dw, dh, batch, mode, dh - 1 - feather, feather, weights, dst, packed, tiles);
  std::printf("remap %dx%d -> %dx%d x%d mode %d feather %d weights %d kind %d: rc %d pixels %08x packed %08x tiles %08x\n", sw, sh, dw, dh, batch, mode,
              feather, weights, (int)kind, rc, sum(dst, batch * dn * 4), sum(packed, batch * dn * 4), sum(tiles, batch * nt * 16));
  delete[] src; delete[] map; delete[] dst; delete[] packed; delete[] tiles;
  return rc;
}
static int pole(s360_ctx* c, int w, int h, float amp, float start, float mid, bool nans) {
  const size_t n = (size_t)w * h, nt = (size_t)((w + 63) / 64) * ((h + 15) / 16);
  uint8_t* src = new uint8_t[n * 4];
  float* flow = new float[n * 2];
  uint8_t* dst = new uint8_t[n * 4];
  uint32_t* packed = new uint32_t[n];
  int32_t* tiles = new int32_t[nt * 4];
  for (size_t i = 0; i < n * 4; ++i) src[i] = (uint8_t)(rnd() * 256);
  for (size_t i = 0; i < n * 2; ++i) flow[i] = (nans && rnd() < 0.1f) ? kFar[(int)(rnd() * 9)] : (rnd() * 2 - 1) * amp;
  const int rc = s360_debug_pole_warp_packed(c, src, w, h, flow, 90.f, start, mid, 75.f, dst, packed, tiles);
  uint8_t* dst2 = new uint8_t[n * 4];
  const int rc2 = s360_debug_remap_by_flow(c, src, w, h, flow, dst2);
  std::printf("pole warp %dx%d amp %g ramp %g..%g nans %d: rc %d %d pixels %08x packed %08x tiles %08x by flow %08x\n", w, h, amp, start, mid, (int)nans, rc,
              rc2, sum(dst, n * 4), sum(packed, n * 4), sum(tiles, nt * 16), sum(dst2, n * 4));
  delete[] src; delete[] flow; delete[] dst; delete[] packed; delete[] tiles; delete[] dst2;
  return rc | rc2;
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
  const int tiny[][2] = {{1, 1}, {2, 3}, {3, 2}, {5, 1}, {1, 5}, {5, 5}};
  for (const auto& t : tiny)
    for (int w = 1; w <= 2; ++w) bad |= remap(c, t[0], t[1], 70, 20, 2, w - 1, 3, w, AROUND);
  const int grids[][3] = {{5, 3, 1}, {530, 100, 1}, {490, 120, 1}, {317, 203, 1}, {4485, 3, 1}, {330, 50, 3}};
  for (const auto& g : grids) bad |= remap(c, 37, 29, g[0], g[1], g[2], 0, 1, 0, AROUND);
  for (int mode = 0; mode <= 2; ++mode) {
    bad |= remap(c, 37, 29, 130, 40, 1, mode, 50, 2, FAR);   // a feather longer than the image; far dead pixels beside live ones
    bad |= remap(c, 37, 29, 130, 40, 1, mode, 1, 1, NANS);   // no live pixel anywhere
  }
  bad |= remap(c, 101, 90, 128, 32, 1, 0, 1, 2, BOX, 70, 65);  // 64 x 64: the whole LDS tile
  bad |= remap(c, 101, 90, 128, 32, 1, 0, 1, 2, BOX, 71, 65);  // 65 x 64: gathered
  bad |= remap(c, 101, 90, 128, 32, 1, 0, 1, 1, BOX, 69, 66);  // 63 x 65
  bad |= remap(c, 8, 1100, 128, 16, 1, 0, 1, 2, TALL, 1026);   // 4 x 1020
  bad |= remap(c, 8, 1100, 128, 16, 1, 0, 1, 2, TALL, 1029);   // 4 x 1023
  bad |= remap(c, 8, 1100, 128, 16, 1, 0, 1, 2, TALL, 1030);   // 4 x 1024: gathered through the field limit
  bad |= pole(c, 150, 37, 0.f, 30.f, 60.f, false);
  bad |= pole(c, 150, 37, 6.f, 30.f, 60.f, true);
  bad |= pole(c, 150, 37, 90.f, 30.f, 60.f, false);
  bad |= pole(c, 150, 37, 6.f, 45.f, 45.f, true);  // phiRampStart == phiMid: 0 / 0 on row 18
  bad |= pole(c, 70, 9, 1000.f, 30.f, 60.f, true);
  s360_destroy(c);
  std::printf(bad ? "FAILED\n" : "all calls returned S360_OK\n");
  return bad ? 1 : 0;
}
