// jpeg_decode.hpp — baseline JPEG camera files decoded on the device (jpeg_decode.hip, include/s360_input_jpeg.h): the pixels
// host/jpeg_io.hpp's jpegio::decode_any gives, byte for byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "core.hpp"

namespace s360 {

// One Huffman table as the kernels read it: the first 10 bits of a code looked up directly, longer codes by the length loop of
// jpegio::Reader::decode_sym (the same two comparisons, so that a damaged table decodes as it does there).
struct JpegHuffDev {
  uint16_t lut[1024];  // length << 8 | symbol of the code that starts these 10 bits; 0: no code of at most 10 bits
  int mincode[17], maxcode[17], valptr[17];
  uint8_t vals[256];
};
// What the device gets per file: tables [2 c] DC and [2 c + 1] AC of component c, the components' quantisation tables (natural order).
struct JpegTabDev {
  JpegHuffDev h[6];
  uint16_t q[3][64];
};

// What the host reads out of the container of a file this decoder takes (jpeg_in_parse).
struct JpegInInfo {
  int w = 0, h = 0, hs = 1, vs = 1;      // luma sampling factors: 2x2 (4:2:0), 2x1 (4:2:2), 1x1 (4:4:4); chroma is 1x1
  size_t scan_off = 0, scan_len = 0;     // the entropy-coded segment in the file, byte stuffing included
  size_t nstuff = 0;                     // its stuffing bytes (0x00 behind 0xFF)
  std::vector<uint32_t> seg_stuff;       // stuffing bytes in front of every kJpegUnstuffSeg bytes of the segment
  JpegTabDev tab;
};
constexpr size_t kJpegUnstuffSeg = 16384;  // stuffed bytes one workgroup of k_jpeg_unstuff takes
constexpr unsigned kJpegSubBits = 4096;    // S: bits of a subsequence (jpeg_decode.hip's header says why)
unsigned jpeg_sub_bits();                  // ... or what the developer switch S360_JPEG_SUB_BITS asks for (64 .. 2^24)
constexpr int kJpegSyncThreads = 256;      // subsequences per workgroup of k_jpeg_sync / k_jpeg_coef

// true: SOF0, 8-bit, three components coded as Y, Cb, Cr with luma sampling 2x2, 2x1 or 1x1 and chroma 1x1, one interleaved scan
// (Ss 0, Se 63, Ah = Al = 0), 8-bit quantisation tables, no restart interval, EXIF orientation absent or 1, not Adobe transform 0,
// the scan shorter than 2^32 bits. false: not this decoder's file (the host decoder's business); `info` is unspecified.
bool jpeg_in_parse(const uint8_t* file, size_t n, JpegInInfo& info);

// Where k_jpeg_pixels leaves an image (the stores of png_decode.hpp's PngStore that an 8-bit colour image has).
enum JpegStore : int {
  kJpegStoreBytes = 0,  // packed B,G,R
  kJpegStoreSide = 2,   // a side camera's source slot: uchar4 B,G,R,A with side_src_alpha's row ramp
  kJpegStorePole = 3    // a pole camera's source slot: uchar4 B,G,R,255
};
struct JpegDecodeDst {
  uint8_t* p = nullptr;  // device memory (4-byte aligned for the slot stores)
  int store = kJpegStoreBytes;
  int feather = 0;       // kJpegStoreSide: side_alpha_feather_size
};

// Per-file status words (include/s360_input_jpeg.h names them): what jpeg_decode_run throws with.
enum JpegStatus : unsigned {
  kJpegOk = 0, kJpegBadCode = 1, kJpegBadRun = 2, kJpegShort = 3, kJpegBlocksMissing = 4, kJpegLeftOver = 5, kJpegMarker = 6
};
struct JpegDecodeError : Error {
  int image;
  unsigned status;
  JpegDecodeError(int img, unsigned s, const std::string& m) : Error(-1, m), image(img), status(s) {}
};

// Device buffers of the decoder: grow only, owned by the context.
struct JpegDecodeBufs {
  DevBuf in, unst, files, tabs, segs, subs, wgs, counters, coef, dc, chunks, planes;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  JpegDecodeBufs() {}
  ~JpegDecodeBufs() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
struct JpegDecodeStats {
  unsigned long long files = 0, subsequences = 0, rounds = 0, most_file_rounds = 0;  // rounds: synchronisation launches of the call
  double ms_entropy = 0, ms_pixels = 0;
  std::vector<uint32_t> file_rounds;  // per file: the most decode passes one of its workgroups made over all launches
};

// One launch sequence for all files: the scans are uploaded once, unstuffed, synchronised to the serial decoder's states at every
// subsequence boundary (launches driven by a downloaded "changed" counter), decoded into quantised coefficients, and turned into
// pixels at dst[i]. The stream waits for the events of `before` (null entries are skipped) in front of the pixel kernel, the only
// one that writes the destinations. Synchronous. Throws JpegDecodeError naming the first damaged image. `coef_tap` (may be null):
// host memory for image `tap_image`'s coefficients in emission order, 64 int16 a block, absolute DC.
void jpeg_decode_run(hipStream_t st, JpegDecodeBufs& D, const std::vector<const uint8_t*>& files, const std::vector<JpegInInfo>& info,
                     const std::vector<JpegDecodeDst>& dst, const std::vector<hipEvent_t>& before, JpegDecodeStats& stats,
                     int16_t* coef_tap = nullptr, int tap_image = 0);
inline size_t jpeg_in_blocks(const JpegInInfo& I) {
  return (size_t)((I.w + 8 * I.hs - 1) / (8 * I.hs)) * (size_t)((I.h + 8 * I.vs - 1) / (8 * I.vs)) * (size_t)(I.hs * I.vs + 2);
}

}  // namespace s360
