// png_decode.hpp — banded PNG files ("sbNd": one raw-deflate segment per band of rows) inflated and unfiltered on the device
// (png_decode.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "core.hpp"

namespace s360 {

// What the host reads out of the container of a file this decoder takes (png_parse_banded).
struct PngBandedInfo {
  int w = 0, h = 0, channels = 0, band_rows = 0, nbands = 0;
  std::vector<std::pair<size_t, size_t>> bands;  // (offset, length) of every band's IDAT data in the file
  uint32_t adler = 0;                            // the file's trailing Adler-32 (of all filtered scanlines)
};
// true: the file is a PNG, 8-bit, colour type 2 or 6, not interlaced, with an "sbNd" chunk, a first IDAT of the 2-byte zlib header,
// exactly ceil(h / band_rows) band IDATs and a 4-byte last IDAT (the conditions of the parallel reader of host/png_io.hpp, which,
// like this function, does not check the chunks' CRCs), and every band is small enough for 32-bit bit positions (rows x line <=
// 2^30 bytes, segment < 2^28 bytes). false: not this decoder's file; `info` is untouched.
bool png_parse_banded(const uint8_t* file, size_t n, PngBandedInfo& info);

// What png_decode_run throws: the first image whose bands failed (include/s360_png_decode.h: S360_PNG_DECODE_FAILURE_DAMAGED).
struct PngDecodeError : Error {
  int image;
  PngDecodeError(int img, const std::string& m) : Error(-1, m), image(img) {}
};
// Device buffers of the decoder: grow only, owned by the context.
struct PngDecodeBufs {
  DevBuf in, filt, table, outs;  // the files' bytes; the bands' filtered scanlines; band + image tables; per-band results + counters
};
constexpr int kPngDecodeStatWords = 4 + 66;  // fast, general, stored-only, most rounds; histogram of a fast band's most rounds (0..65)
// One launch sequence for all bands of all images: the files' bytes are uploaded once, k_png_inflate (a wave per band) leaves
// filtered scanlines in `filt`, k_png_unfilter (a workgroup per band) writes B,G,R(,A) pixels to dst[i] (device memory, 4-byte aligned
// for 4 channels, w x h x channels bytes) and the bands' Adler-32 pieces. Synchronous: returns when every band's status and every
// file's Adler-32 are known. Throws PngDecodeError (S360_ERR_INVALID_ARG) naming the first image whose bands failed. `stats` receives the
// kPngDecodeStatWords counters of this call; `prof` (may be null) the two kernels' times as "png_inflate" and "png_unfilter".
void png_decode_run(hipStream_t st, PngDecodeBufs& D, const std::vector<const uint8_t*>& files, const std::vector<PngBandedInfo>& info,
                    const std::vector<uint8_t*>& dst, unsigned long long* stats, Profiler* prof);

}  // namespace s360
