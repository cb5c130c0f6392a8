// runs the device JPEG encoder (include/s360_jpeg.h) of the emulated, sanitised library size by size and compares every file with
// host/jpeg_io.hpp's jpegio::encode, byte for byte: every (w, h) of 1..34 x 1..34 (every residue modulo 16 of both, whole and
// partial MCUs, dummy columns and rows) with ramps, and the larger sizes of tests/jpeg_cases.py with noise and two checkers. Heap
// blocks of exactly the sizes the header states: device buffers have red zones there, so a kernel's out-of-bounds access is a
// report with file and line. One encoder object serves every size. Prints one line at the end; exit status 1 on a mismatch.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../host/jpeg_io.hpp"
#include "../../include/s360_jpeg.h"

static unsigned g_seed = 12345;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 24; }
enum Kind { RAMPS, NOISE, CHECKER1, CHECKER3 };

static int one(s360_jpeg* e, int w, int h, Kind kind, int quality) {
  uint8_t* bgr = new uint8_t[(size_t)w * h * 3];
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      uint8_t* p = bgr + ((size_t)y * w + x) * 3;
      if (kind == RAMPS) { p[0] = (uint8_t)(x * 255 / (w > 1 ? w - 1 : 1)); p[1] = (uint8_t)(y * 255 / (h > 1 ? h - 1 : 1)); p[2] = (uint8_t)((x + y) * 255 / (w + h > 2 ? w + h - 2 : 1)); }
      else if (kind == NOISE) { p[0] = (uint8_t)rnd(); p[1] = (uint8_t)rnd(); p[2] = (uint8_t)rnd(); }
      else p[0] = p[1] = p[2] = (uint8_t)((kind == CHECKER1 ? (x + y) & 1 : (x / 3 + y / 3) & 1) * 255);
    }
  const std::vector<uint8_t> want = jpegio::encode(bgr, w, h, quality);
  const size_t cap = s360_jpeg_bound(w, h);
  uint8_t* out = new uint8_t[cap];
  size_t n = 0;
  int bad = 0;
  if (s360_jpeg_encode(e, bgr, w, h, out, cap, &n) < 0) {
    std::printf("%d x %d kind %d: %s\n", w, h, (int)kind, s360_last_error(nullptr));
    bad = 1;
  } else if (n != want.size() || std::memcmp(out, want.data(), n) != 0) {
    size_t i = 0;
    while (i < n && i < want.size() && out[i] == want[i]) ++i;
    std::printf("%d x %d kind %d: %zu bytes, the host writer's file has %zu; first difference at byte %zu\n", w, h, (int)kind, n, want.size(), i);
    bad = 1;
  } else {  // ... and a buffer of exactly the file's size is enough
    uint8_t* tight = new uint8_t[n];
    size_t n2 = 0;
    if (s360_jpeg_encode(e, bgr, w, h, tight, n, &n2) < 0 || n2 != n || std::memcmp(tight, out, n) != 0) {
      std::printf("%d x %d kind %d: the second encode into a buffer of the file's size differs\n", w, h, (int)kind);
      bad = 1;
    }
    delete[] tight;
  }
  delete[] out;
  delete[] bgr;
  return bad;
}

int main() {
  s360_jpeg* e = nullptr;
  if (s360_jpeg_create(&e, 0, 1030, 304, 95) < 0) {
    std::printf("create: %s\n", s360_last_error(nullptr));
    return 1;
  }
  int files = 0, bad = 0;
  const int big[][2] = {{1030, 70}, {400, 304}, {70, 37}, {257, 3}, {3, 257}, {640, 33}, {64, 64}};
  for (const auto& s : big)  // (the large ones first: the small ones then run on their scratch)
    for (Kind k : {NOISE, CHECKER1, CHECKER3}) { bad += one(e, s[0], s[1], k, 95); ++files; }
  for (int h = 1; h <= 34; ++h)
    for (int w = 1; w <= 34; ++w) { bad += one(e, w, h, RAMPS, 95); ++files; }
  s360_jpeg_destroy(e);
  std::printf("%d files, %d mismatches\n", files, bad);
  return bad ? 1 : 0;
}
