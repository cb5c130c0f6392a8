// runs the cubemap test taps (include/s360_debug_cubemap.h) of the emulated, sanitised library at the edge shapes of
// tests/cubemap_tiles_cases.py: eyes of 1 .. 12 pixels whose tile boxes wrap once down and twice up in x and once each way in y,
// sh = 1 (every tile gathers by the limits), faces of one pixel, odd eyes and faces (scalar stores), both LDS box sizes, every tile
// gathering by its area, 17 slots (two launches). Device buffers are heap blocks with red zones there, so a kernel's out-of-bounds
// access is a report with file and line. Prints one checksum line per call. argv: rig.json
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/s360.h"
#include "../../include/s360_debug_cubemap.h"

static unsigned g_seed = 24680;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 24; }
static unsigned sum(const void* p, size_t n) {
  unsigned s = 2166136261u;
  for (size_t i = 0; i < n; ++i) s = (s ^ static_cast<const uint8_t*>(p)[i]) * 16777619u;
  return s;
}

static int cube(s360_ctx* c, int slots, int sw, int sh, int fw, int fh, int video, int lds) {
  const size_t en = (size_t)2 * slots * sw * sh * 4, px = (size_t)6 * fw * fh, on = (size_t)slots * 2 * px * 3;
  const size_t nt = (size_t)6 * ((fw + 15) / 16) * ((fh + 15) / 16);
  // (heap blocks of exactly the sizes the header states: the library reading or writing past them is a report too)
  uint8_t* eyes = new uint8_t[en];
  uint8_t* out = new uint8_t[on];
  uint8_t* out2 = new uint8_t[on];
  float* maps = new float[px * 2];
  float* maps2 = new float[px * 2];
  uint32_t* packed = new uint32_t[px];
  int32_t* tiles = new int32_t[nt * 4];
  for (size_t i = 0; i < en; ++i) eyes[i] = (uint8_t)rnd();
  std::memset(out, 0xA5, on); std::memset(out2, 0x5A, on); std::memset(maps, 0xA5, px * 8); std::memset(maps2, 0x5A, px * 8);
  std::memset(packed, 0xA5, px * 4); std::memset(tiles, 0xA5, nt * 16);
  const int rc = s360_debug_cubemap_tiles(c, eyes, slots, sw, sh, fw, fh, video, lds, out, maps, packed, tiles);
  const int rc2 = s360_debug_cubemap(c, eyes, slots, sw, sh, fw, fh, video, out2, maps2);
  const bool same = std::memcmp(out, out2, on) == 0 && std::memcmp(maps, maps2, px * 8) == 0;
  std::printf("cubemap %dx%d -> %dx%d x%d %s box %d: rc %d %d pixels %08x maps %08x packed %08x tiles %08x %s\n", sw, sh, fw, fh, slots,
              video ? "video" : "photo", lds, rc, rc2, sum(out, on), sum(maps, px * 8), sum(packed, px * 4), sum(tiles, nt * 16),
              same ? "both kernels equal" : "THE KERNELS DIFFER");
  delete[] eyes; delete[] out; delete[] out2; delete[] maps; delete[] maps2; delete[] packed; delete[] tiles;
  return rc | rc2 | (same ? 0 : 1);
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
  // {sw, sh, fw, fh}: the limits of the box load's wrap, all-gather by the limits, faces of one pixel, odd sizes
  const int edge[][4] = {{1, 1, 16, 16}, {1, 2, 33, 17}, {1, 3, 16, 16}, {1, 5, 17, 16}, {2, 1, 5, 3}, {2, 2, 16, 16}, {2, 2, 17, 16},
                         {3, 3, 20, 12}, {3, 3, 18, 12}, {7, 2, 16, 16}, {5, 1, 16, 16}, {5, 1, 18, 16}, {12, 6, 20, 20}, {28, 14, 16, 16},
                         {28, 14, 33, 17}, {28, 14, 1, 17}, {28, 14, 20, 1}, {28, 14, 1, 1}, {64, 32, 96, 96}, {301, 77, 37, 53}};
  for (const auto& e : edge)
    for (int video = 0; video <= 1; ++video)
      for (int lds = 2560; lds <= 4096; lds += 1536) bad |= cube(c, 2, e[0], e[1], e[2], e[3], video, lds);
  for (int lds = 2560; lds <= 4096; lds += 1536) {
    bad |= cube(c, 1, 700, 350, 40, 40, 1, lds);   // boxes on both sides of either limit
    bad |= cube(c, 1, 700, 350, 42, 40, 0, lds);
    bad |= cube(c, 1, 2048, 1024, 30, 32, 1, lds);  // every tile gathers by its area
  }
  bad |= cube(c, 17, 28, 14, 33, 17, 1, 4096);  // two launches, the second with base 16
  bad |= cube(c, 17, 12, 6, 20, 12, 0, 2560);
  bad |= cube(c, 33, 3, 3, 4, 4, 1, 4096);      // three launches
  s360_destroy(c);
  std::printf(bad ? "FAILED\n" : "all calls returned S360_OK\n");
  return bad ? 1 : 0;
}
