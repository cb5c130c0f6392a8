// DEVELOPER TOOL — what one host thread takes for host/jpeg_io.hpp's jpegio::encode of an image (tools/frame_jpeg_time.py):
//   jpeg_host_time <in.bgr> <w> <h> [reps] [quality]
// prints one line per encode: "<milliseconds> <file bytes>"; the image is read once, before the clock starts.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../host/jpeg_io.hpp"

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: jpeg_host_time <in.bgr> <w> <h> [reps] [quality]\n");
    return 2;
  }
  const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), reps = argc > 4 ? std::atoi(argv[4]) : 3, quality = argc > 5 ? std::atoi(argv[5]) : 95;
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || reps < 1) return 2;
  std::vector<uint8_t> bgr((size_t)w * h * 3);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) {
    std::fprintf(stderr, "jpeg_host_time: cannot read %zu bytes from %s\n", bgr.size(), argv[1]);
    return 1;
  }
  std::fclose(f);
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<uint8_t> file = jpegio::encode(bgr.data(), w, h, quality);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%.3f %zu\n", ms, file.size());
  }
  return 0;
}
