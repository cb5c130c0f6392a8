// runs the device JPEG decoder (include/s360_input_jpeg.h) of the emulated, sanitised library over the .jpg files of a directory and
// over damaged copies of some of them, and compares every accepted file with host/jpeg_io.hpp's jpegio::decode_any, byte for byte.
// tests/test_cpu_input_jpeg.py fills the directory: sizes 1..40 x 1..40 and the case sizes at the three samplings ("base_*.jpg",
// which must all decode), and a few small files to damage ("mut_*.jpg"). The damage is made here, deterministically: single bytes of
// the scan replaced or a bit flipped, the scan cut at EVERY byte of the smallest file, bytes of the DHT segments changed. Files
// and output buffers are heap blocks of exactly their sizes, and damaged files run on a context of their own (the decoder's
// device buffers only grow: on a fresh context the red zones sit right behind this file's sizes), so an out-of-bounds access of a
// kernel is a report with file and line. Every call must return success with the host decoder's pixels, or fail with an error
// that names the image. Prints one line at the end; exit status 1 on a violation. argv: rig.json dir
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../host/jpeg_io.hpp"
#include "../../include/s360.h"

static std::vector<uint8_t> slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static unsigned g_seed = 2468;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static std::vector<s360_camera> g_cams(24);
static int g_ncams = 0;
static s360_params g_P;
static s360_ctx* make_ctx() {
  s360_ctx* c = nullptr;
  if (s360_create(&c, 0, g_cams.data(), g_ncams, &g_P) != S360_OK) {
    std::fprintf(stderr, "create: %s\n", s360_last_error(nullptr));
    std::exit(2);
  }
  return c;
}

struct Tally { int files = 0, accepted = 0, refused = 0, bad = 0; };

// one file through the decoder on context c; must_decode: a refusal is a violation too
static void one(s360_ctx* c, const std::string& name, const std::vector<uint8_t>& src, bool must_decode, Tally& T) {
  ++T.files;
  uint8_t* file = new uint8_t[src.size() ? src.size() : 1];  // (a heap block of exactly the file's size)
  std::memcpy(file, src.data(), src.size());
  int info[6] = {0, 0, 0, 0, 0, 0};
  const bool ours = s360_input_jpeg_decodable(file, src.size(), info) == S360_OK;
  const size_t bytes = ours ? (size_t)info[0] * info[1] * 3 : 1;
  uint8_t* out = new uint8_t[bytes];
  const uint8_t* files[1] = {file};
  const size_t len[1] = {src.size()}, cap[1] = {bytes};
  void* outs[1] = {out};
  const int rc = s360_decode_input_jpeg_batch(c, 1, files, len, outs, cap, nullptr);
  if (rc == S360_OK) {
    ++T.accepted;
    try {
      const pngio::Image im = jpegio::decode_any(src, name, false);
      if (!ours || im.px.size() != bytes || std::memcmp(im.px.data(), out, bytes) != 0) {
        std::printf("%s: accepted, but the pixels are not the host decoder's\n", name.c_str());
        ++T.bad;
      }
    } catch (const std::exception& e) {
      std::printf("%s: accepted, but the host decoder refuses it: %s\n", name.c_str(), e.what());
      ++T.bad;
    }
  } else {
    ++T.refused;
    const char* msg = s360_last_error(c);
    if (!msg || !std::strstr(msg, "image 0") || must_decode) {
      std::printf("%s: refused%s: %s\n", name.c_str(), must_decode ? " (an undamaged file)" : " without naming the image", msg ? msg : "(null)");
      ++T.bad;
    }
  }
  delete[] out;
  delete[] file;
}

// [begin, end) of the entropy-coded segment and of every DHT segment's payload
static bool layout(const std::vector<uint8_t>& f, size_t& scan0, size_t& scan1, std::vector<std::pair<size_t, size_t>>& dht) {
  size_t p = 2;
  while (p + 4 <= f.size() && f[p] == 0xFF) {
    const int m = f[p + 1];
    const size_t n = ((size_t)f[p + 2] << 8) | f[p + 3];
    if (m == 0xC4) dht.emplace_back(p + 4, p + 2 + n);
    if (m == 0xDA) {
      scan0 = p + 2 + n;
      scan1 = f.size() - 2;
      return scan1 > scan0;
    }
    p += 2 + n;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  g_ncams = s360_rig_load_json(argv[1], g_cams.data(), 24);
  if (g_ncams < 0) { std::fprintf(stderr, "rig: %s\n", s360_last_error(nullptr)); return 2; }
  std::memset(&g_P, 0, sizeof g_P);
  g_P.interpupilary_dist = 6.4; g_P.zero_parallax_dist = 10000; g_P.side_alpha_feather_size = 100; g_P.std_alpha_feather_size = 31;
  g_P.eqr_width = 252; g_P.eqr_height = 126; g_P.final_eqr_width = 240; g_P.final_eqr_height = 240;
  std::strcpy(g_P.side_flow_alg, "pixflow_low"); std::strcpy(g_P.polar_flow_alg, "pixflow_low");
  std::vector<std::string> names;
  if (DIR* d = opendir(argv[2])) {
    while (dirent* e = readdir(d)) {
      const std::string s = e->d_name;
      if (s.size() > 4 && s.substr(s.size() - 4) == ".jpg") names.push_back(s);
    }
    closedir(d);
  }
  std::sort(names.begin(), names.end());
  Tally base, mut;
  // the undamaged files: one context per 64 files, so that the buffers' red zones stay near the sizes in use
  s360_ctx* c = nullptr;
  int on_ctx = 0;
  for (const std::string& nm : names) {
    if (nm.compare(0, 5, "base_") != 0) continue;
    if (!c || on_ctx == 64) {
      if (c) s360_destroy(c);
      c = make_ctx();
      on_ctx = 0;
    }
    one(c, nm, slurp(std::string(argv[2]) + "/" + nm), true, base);
    ++on_ctx;
  }
  if (c) s360_destroy(c);
  // the damaged ones, each on a context of its own
  size_t smallest = (size_t)-1;
  std::string smallest_name;
  for (const std::string& nm : names) {
    if (nm.compare(0, 4, "mut_") != 0) continue;
    const std::vector<uint8_t> src = slurp(std::string(argv[2]) + "/" + nm);
    size_t s0 = 0, s1 = 0;
    std::vector<std::pair<size_t, size_t>> dht;
    if (!layout(src, s0, s1, dht) || dht.empty()) { std::printf("%s: no scan / DHT found\n", nm.c_str()); ++mut.bad; continue; }
    if (s1 - s0 < smallest) { smallest = s1 - s0; smallest_name = nm; }
    auto run = [&](const std::vector<uint8_t>& f, const char* what, int k) {
      s360_ctx* cc = make_ctx();
      one(cc, nm + ":" + what + std::to_string(k), f, false, mut);
      s360_destroy(cc);
    };
    for (int k = 0; k < 40; ++k) {  // a byte of the scan replaced, or one of its bits flipped
      std::vector<uint8_t> f = src;
      const size_t at = s0 + rnd() % (s1 - s0);
      if (k & 1) f[at] ^= (uint8_t)(1u << (rnd() & 7)); else f[at] = (uint8_t)rnd();
      run(f, "scan", k);
    }
    for (int k = 0; k < 24; ++k) {  // a byte of a DHT segment changed: the counts (the first 17 bytes of a table) or the values
      std::vector<uint8_t> f = src;
      const auto& seg = dht[rnd() % dht.size()];
      const size_t at = (k & 1) ? seg.first + rnd() % std::min<size_t>(17, seg.second - seg.first) : seg.first + rnd() % (seg.second - seg.first);
      f[at] = (k & 2) ? (uint8_t)rnd() : (uint8_t)(f[at] + 1 + rnd() % 3);
      run(f, "dht", k);
    }
  }
  if (!smallest_name.empty()) {  // the scan cut at every byte, with and without the EOI marker behind it
    const std::vector<uint8_t> src = slurp(std::string(argv[2]) + "/" + smallest_name);
    size_t s0 = 0, s1 = 0;
    std::vector<std::pair<size_t, size_t>> dht;
    layout(src, s0, s1, dht);
    for (size_t cut = s0; cut < s1; ++cut) {
      std::vector<uint8_t> f(src.begin(), src.begin() + (long)cut);
      if (cut & 1) { f.push_back(0xFF); f.push_back(0xD9); }
      s360_ctx* cc = make_ctx();
      one(cc, smallest_name + ":cut" + std::to_string(cut - s0), f, false, mut);
      s360_destroy(cc);
    }
  }
  std::printf("%d undamaged files, %d accepted; %d damaged files, %d accepted, %d refused; %d violations\n", base.files, base.accepted, mut.files,
              mut.accepted, mut.refused, base.bad + mut.bad);
  return base.bad + mut.bad ? 1 : 0;
}
