// DEVELOPER / TEST TOOL — host/jpeg_io.hpp's JPEG writer behind a main() of its own, plainly optimised and without a sanitizer,
// so that the GPU tests may run it too: the byte oracle of the device encoder (include/s360_jpeg.h).
//   jpeg_host_encode <in.bgr> <w> <h> <out.jpg> [quality] [--blocks <out.bin>]
// writes jpegio::encode's file. --blocks: also what include/s360_debug_jpeg.h's tap returns, from the two halves of the writer
// (enc_detail::make_blocks / emit_blocks): n x 64 int16 coefficients, then n uint32 bit lengths, n = 6 * ceil(w/16) * ceil(h/16).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../host/jpeg_io.hpp"

int main(int argc, char** argv) {
  std::vector<std::string> pos;
  std::string blocksPath;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--blocks") && i + 1 < argc) blocksPath = argv[++i];
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 4 || pos.size() > 5) {
    std::fprintf(stderr, "usage: jpeg_host_encode <in.bgr> <w> <h> <out.jpg> [quality] [--blocks <out.bin>]\n");
    return 2;
  }
  const int w = std::atoi(pos[1].c_str()), h = std::atoi(pos[2].c_str()), quality = pos.size() == 5 ? std::atoi(pos[4].c_str()) : 95;
  if (w < 1 || h < 1 || w > 65535 || h > 65535) {
    std::fprintf(stderr, "jpeg_host_encode: size outside 1..65535\n");
    return 2;
  }
  std::vector<uint8_t> bgr((size_t)w * h * 3);
  FILE* f = std::fopen(pos[0].c_str(), "rb");
  if (!f || std::fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) {
    std::fprintf(stderr, "jpeg_host_encode: cannot read %zu bytes from %s\n", bgr.size(), pos[0].c_str());
    return 1;
  }
  std::fclose(f);
  try {
    const std::vector<uint8_t> file = jpegio::encode(bgr.data(), w, h, quality);
    f = std::fopen(pos[3].c_str(), "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f)) throw std::runtime_error("cannot write " + pos[3]);
    if (!blocksPath.empty()) {
      int q[2][64];
      jpegio::enc_detail::quant_tables(quality, q);
      const std::vector<int16_t> blocks = jpegio::enc_detail::make_blocks(bgr.data(), w, h, q);
      std::vector<uint8_t> scan;
      std::vector<uint32_t> bits;
      jpegio::enc_detail::emit_blocks(blocks, scan, &bits);
      f = std::fopen(blocksPath.c_str(), "wb");
      if (!f || std::fwrite(blocks.data(), 2, blocks.size(), f) != blocks.size() || std::fwrite(bits.data(), 4, bits.size(), f) != bits.size() ||
          std::fclose(f))
        throw std::runtime_error("cannot write " + blocksPath);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "jpeg_host_encode: %s\n", e.what());
    return 1;
  }
  return 0;
}
