// DEVELOPER / TEST TOOL — host/jpeg_io.hpp's reader behind a main() of its own, plainly optimised and without a sanitizer, so that
// the GPU tests may run it too: the byte oracle of the device JPEG decoder (include/s360_input_jpeg.h).
//   jpeg_host_decode <list.txt>
// list.txt: one "<in file> <out file>" pair per line. Every input goes through jpegio::decode_any; its B,G,R bytes are written to
// the output file and "ok <w> <h>" is printed, or "fail <message>" and nothing is written. Exit code 0 if every line was read.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../host/jpeg_io.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: jpeg_host_decode <list.txt>\n");
    return 2;
  }
  std::ifstream list(argv[1]);
  std::string line;
  while (std::getline(list, line)) {
    std::istringstream ls(line);
    std::string in, out;
    if (!(ls >> in >> out)) continue;
    try {
      std::ifstream f(in, std::ios::binary);
      if (!f) throw std::runtime_error("cannot read " + in);
      const std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
      const pngio::Image im = jpegio::decode_any(file, in, false);
      std::ofstream o(out, std::ios::binary);
      o.write(reinterpret_cast<const char*>(im.px.data()), (std::streamsize)im.px.size());
      if (!o) throw std::runtime_error("cannot write " + out);
      std::printf("ok %d %d\n", im.w, im.h);
    } catch (const std::exception& e) {
      std::string m = e.what();
      for (char& c : m)
        if (c == '\n') c = ' ';
      std::printf("fail %s\n", m.c_str());
    }
  }
  return 0;
}
