// feeds the files of a directory to the device PNG decoder of the emulated, sanitised library (s360_png_decodable,
// s360_decode_png_batch), every file on a fresh context and with output buffers of exactly the image's size; writes <file>.out (the pixels) where the library reports
// success, and one line per file: "<name> <return code>". A 16-bit file (s360_input_png_decodable takes it, s360_png_decodable does
// not) goes through s360_decode_input_png_batch twice, to uint16 samples (<file>.out) and to high bytes (<file>.out8), again with
// buffers of exactly those sizes. argv: rig.json dir
#include <dirent.h>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include <algorithm>
#include "../../include/s360.h"
static std::vector<uint8_t> slurp(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::vector<s360_camera> cams(24);
  const int n = s360_rig_load_json(argv[1], cams.data(), 24);
  if (n < 0) { std::fprintf(stderr, "rig: %s\n", s360_last_error(nullptr)); return 2; }
  s360_params P;
  std::memset(&P, 0, sizeof P);
  P.interpupilary_dist = 6.4; P.zero_parallax_dist = 10000; P.side_alpha_feather_size = 100; P.std_alpha_feather_size = 31;
  P.eqr_width = 252; P.eqr_height = 126; P.final_eqr_width = 240; P.final_eqr_height = 240;
  std::strcpy(P.side_flow_alg, "pixflow_low"); std::strcpy(P.polar_flow_alg, "pixflow_low");
  std::vector<std::string> names;
  if (DIR* d = opendir(argv[2])) {
    while (dirent* e = readdir(d)) {
      const std::string s = e->d_name;
      if (s.size() > 4 && s.substr(s.size() - 4) == ".png") names.push_back(s);
    }
    closedir(d);
  }
  std::sort(names.begin(), names.end());
  for (const std::string& nm : names) {
    const std::string path = std::string(argv[2]) + "/" + nm;
    // (a heap block of exactly the file's size: a read past the file's end is a sanitizer report)
    const std::vector<uint8_t> src = slurp(path);
    uint8_t* file = new uint8_t[src.size() ? src.size() : 1];
    std::memcpy(file, src.data(), src.size());
    int whc[3] = {0, 0, 0}, rows = 0, rc = s360_png_decodable(file, src.size(), whc, &rows);
    if (rc == S360_OK) {
      // a context of its own per file: the decoder's device buffers only grow, so on a context that has seen a larger file the red
      // zones would sit behind that file's sizes, not behind this one's
      s360_ctx* c = nullptr;
      if (s360_create(&c, 0, cams.data(), n, &P) != S360_OK) { std::fprintf(stderr, "create: %s\n", s360_last_error(nullptr)); return 2; }
      const size_t bytes = (size_t)whc[0] * whc[1] * whc[2];
      uint8_t* out = new uint8_t[bytes];
      const uint8_t* files[1] = {file};
      const size_t len[1] = {src.size()}, cap[1] = {bytes};
      uint8_t* outs[1] = {out};
      rc = s360_decode_png_batch(c, 1, files, len, outs, cap, nullptr);
      if (rc == S360_OK) { std::ofstream o(path + ".out", std::ios::binary); o.write((const char*)out, (std::streamsize)bytes); }
      delete[] out;
      s360_destroy(c);
    }
    int info[5] = {0, 0, 0, 0, 0};
    if (rc != S360_OK && s360_input_png_decodable(file, src.size(), info) == S360_OK && info[3] == 16) {
      for (int keep16 = 1; keep16 >= 0; --keep16) {
        s360_ctx* c = nullptr;
        if (s360_create(&c, 0, cams.data(), n, &P) != S360_OK) { std::fprintf(stderr, "create: %s\n", s360_last_error(nullptr)); return 2; }
        const size_t bytes = (size_t)info[0] * info[1] * info[2] * (keep16 ? 2 : 1);
        uint8_t* out = new uint8_t[bytes];  // (operator new: aligned for uint16)
        const uint8_t* files[1] = {file};
        const size_t len[1] = {src.size()}, cap[1] = {bytes};
        void* outs[1] = {out};
        rc = s360_decode_input_png_batch(c, 1, files, len, outs, cap, keep16, nullptr);
        if (rc == S360_OK) { std::ofstream o(path + (keep16 ? ".out" : ".out8"), std::ios::binary); o.write((const char*)out, (std::streamsize)bytes); }
        delete[] out;
        s360_destroy(c);
        if (rc != S360_OK) break;
      }
    }
    delete[] file;
    std::printf("%s %d\n", nm.c_str(), rc);
  }
  return 0;
}
