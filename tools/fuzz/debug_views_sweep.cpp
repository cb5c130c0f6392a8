// runs the test tap of k_debug_views (include/s360_debug_views.h) on the emulated, sanitised library over the sizes of
// tests/debug_views_cases.py — widths 1, 3, 5, 63, 64, 65, 127, 130, 1100 x heights 1, 2, 17 x shifts 0, 1, w / 3, w - 1 x 0 / 7 rows
// of padding x 4 -> 4 / 4 -> 3 channels x destinations 0 / 4 bytes behind a 16-byte boundary, with and without a crop — one call per
// view on heap blocks of EXACTLY the view's bytes (device buffers are heap blocks with red zones there too, so a work item reading
// or writing past its view is a report with file and line), then all of them in one call. Every result is compared with a
// restatement in plain C++ (crop, rotate, pad, drop alpha). argv: rig.json
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/s360.h"
#include "../../include/s360_debug_views.h"

static unsigned g_seed = 97531;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 24; }

struct View { int w, h, shift, pad, cout, base, crop; };

static void restate(const View& v, const uint8_t* src, int pitch, int x0, int y0, uint8_t* dst) {
  for (int y = 0; y < v.h + v.pad; ++y)
    for (int x = 0; x < v.w; ++x)
      for (int k = 0; k < v.cout; ++k) {
        const int sx = ((x - v.shift) % v.w + v.w) % v.w;
        dst[((size_t)y * v.w + x) * v.cout + k] = y < v.h ? src[((size_t)(y0 + y) * pitch + x0 + sx) * 4 + k] : 0;
      }
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

  const int widths[] = {1, 3, 5, 63, 64, 65, 127, 130, 1100}, heights[] = {1, 2, 17};
  std::vector<View> views;
  for (int w : widths)
    for (int h : heights) {
      if (w == 1100 && h != 2) continue;
      const int shifts[] = {0, 1 % w, w / 3, w - 1};
      for (int si = 0; si < 4; ++si) {
        bool seen = false;
        for (int sj = 0; sj < si; ++sj) seen |= shifts[sj] == shifts[si];
        if (seen) continue;
        for (int pad = 0; pad <= 7; pad += 7)
          for (int cout = 4; cout >= 3; --cout)
            for (int base = 0; base <= 4; base += 4) views.push_back({w, h, shifts[si], pad, cout, base, (int)(views.size() & 1)});
      }
    }
  int bad = 0;
  // all views of one call: their sources and destinations in two areas, a gap of canary bytes behind every destination
  std::vector<s360_debug_view> all;
  std::vector<uint8_t> allSrc, allDst, allWant;
  for (const View& v : views) {
    const int pitch = v.w + (v.crop ? 5 : 0), rows = v.h + (v.crop ? 3 : 0), x0 = v.crop ? 3 : 0, y0 = v.crop ? 2 : 0;
    const size_t sn = (size_t)pitch * rows * 4, dn = (size_t)v.w * (v.h + v.pad) * v.cout;
    uint8_t* src = new uint8_t[sn];
    for (size_t i = 0; i < sn; ++i) src[i] = (uint8_t)rnd();
    // alone: the destination area is `base` bytes and the view, nothing behind it
    uint8_t* dst = new uint8_t[v.base + dn];
    uint8_t* want = new uint8_t[v.base + dn];
    std::memset(dst, 0xA5, v.base + dn);
    std::memset(want, 0xA5, v.base + dn);
    restate(v, src, pitch, x0, y0, want + v.base);
    s360_debug_view d;
    std::memset(&d, 0, sizeof d);
    d.src_off = 0; d.dst_off = (uint64_t)v.base; d.src_pitch = pitch; d.src_rows = rows; d.x0 = x0; d.y0 = y0; d.w = v.w; d.h = v.h;
    d.shift = v.shift; d.pad_rows = v.pad; d.channels_in = 4; d.channels_out = v.cout;
    const int rc = s360_debug_views(c, 1, &d, src, sn, dst, v.base + dn);
    const bool same = rc == S360_OK && std::memcmp(dst, want, v.base + dn) == 0;
    if (!same) {
      std::printf("view %dx%d shift %d pad %d channels %d base %d crop %d: rc %d %s\n", v.w, v.h, v.shift, v.pad, v.cout, v.base, v.crop, rc,
                  rc == S360_OK ? "WRONG BYTES" : s360_last_error(c));
      bad = 1;
    }
    d.src_off = allSrc.size();
    d.dst_off = allDst.size() + (size_t)v.base;
    allSrc.insert(allSrc.end(), src, src + sn);
    allSrc.resize((allSrc.size() + 15) / 16 * 16, 0);
    allDst.resize(allDst.size() + v.base + dn + 48, 0xA5);
    allWant.resize(allDst.size(), 0xA5);
    std::memcpy(allWant.data() + d.dst_off, want + v.base, dn);
    allDst.resize((allDst.size() + 15) / 16 * 16, 0xA5);
    allWant.resize(allDst.size(), 0xA5);
    all.push_back(d);
    delete[] src; delete[] dst; delete[] want;
  }
  {
    uint8_t* src = new uint8_t[allSrc.size()];
    uint8_t* dst = new uint8_t[allDst.size()];
    std::memcpy(src, allSrc.data(), allSrc.size());
    std::memcpy(dst, allDst.data(), allDst.size());
    const int rc = s360_debug_views(c, (int)all.size(), all.data(), src, allSrc.size(), dst, allDst.size());
    const bool same = rc == S360_OK && std::memcmp(dst, allWant.data(), allDst.size()) == 0;
    std::printf("%zu views alone, then in one call of %zu source and %zu destination bytes: rc %d %s\n", views.size(), allSrc.size(),
                allDst.size(), rc, same ? "equal to the restatement, canaries intact" : "WRONG BYTES");
    if (!same) bad = 1;
    delete[] src; delete[] dst;
  }
  s360_destroy(c);
  std::printf(bad ? "FAILED\n" : "all calls returned S360_OK\n");
  return bad ? 1 : 0;
}
