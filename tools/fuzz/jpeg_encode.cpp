// jpeg_encode — the JPEG writer of host/jpeg_io.hpp (jpegio::encode) as a stand-alone program for the sanitizer build
// (tools/Makefile: fuzz/jpeg_encode, AddressSanitizer + UndefinedBehaviorSanitizer):
//   jpeg_encode <in.bgr> <w> <h> <out.jpg>    encodes one headerless B,G,R image (tests/test_cpu_preview.py compares the
//                                             file with PIL's own encoding of the same pixels)
//   jpeg_encode --sweep                       every size from 1 x 1 to 40 x 40 and a few larger ones, three contents each,
//                                             encoded and decoded again by the reader of the same header: sizes must match
//                                             and the decoded pixels must stay within 48 levels of the source at quality 95
//                                             (a coarse bound: the point of the sweep is the edge handling under the
//                                             sanitizers — padding to whole blocks, dummy blocks, odd sizes)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_io.hpp"

static std::vector<uint8_t> image(int w, int h, int kind) {
  std::vector<uint8_t> px((size_t)w * h * 3);
  uint32_t s = 12345u + (uint32_t)(w * 131 + h * 7 + kind);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) {
        s = s * 1664525u + 1013904223u;
        uint8_t v;
        if (kind == 0) v = (uint8_t)((x * 5 + y * 3 + c * 40) & 255);  // ramps
        else if (kind == 1) v = (uint8_t)(c * 100 + 20);                // constant colour
        else v = (uint8_t)(128 + (int)((s >> 24) & 31) - 16);           // mild noise
        px[((size_t)y * w + x) * 3 + c] = v;
      }
  return px;
}

int main(int argc, char** argv) {
  try {
    if (argc == 2 && std::string(argv[1]) == "--sweep") {
      std::vector<std::pair<int, int>> sizes;
      for (int h = 1; h <= 40; ++h)
        for (int w = 1; w <= 40; ++w) sizes.push_back({w, h});
      for (auto s : {std::pair<int, int>{70, 37}, {96, 48}, {257, 3}, {3, 257}, {640, 33}}) sizes.push_back(s);
      long files = 0;
      for (auto [w, h] : sizes)
        for (int kind = 0; kind < 3; ++kind) {
          const std::vector<uint8_t> px = image(w, h, kind);
          const std::vector<uint8_t> file = jpegio::encode(px.data(), w, h);
          const pngio::Image im = jpegio::decode_any(file, "sweep", false);
          if (im.w != w || im.h != h || im.c != 3) { std::fprintf(stderr, "%d x %d: decoded as %d x %d x %d\n", w, h, im.w, im.h, im.c); return 1; }
          if (kind != 0) {  // (ramps wrap around: steps of 255 levels are not kept by any JPEG)
            for (size_t i = 0; i < px.size(); ++i)
              if (std::abs((int)px[i] - (int)im.px[i]) > 48) { std::fprintf(stderr, "%d x %d kind %d: byte %zu is %d, was %d\n", w, h, kind, i, im.px[i], px[i]); return 1; }
          }
          ++files;
        }
      std::printf("%ld files encoded and decoded\n", files);
      return 0;
    }
    if (argc != 5) { std::fprintf(stderr, "usage: jpeg_encode <in.bgr> <w> <h> <out.jpg> | --sweep\n"); return 2; }
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> px((size_t)w * h * 3);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(px.data(), 1, px.size(), f) != px.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
    jpegio::write(argv[4], px.data(), w, h);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
