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
  int depth = 8;                                 // bits per sample: 8, or (png_parse_banded_input only) 16 with 3 channels
  std::vector<std::pair<size_t, size_t>> bands;  // (offset, length) of every band's IDAT data in the file
  uint32_t adler = 0;                            // the file's trailing Adler-32 (of all filtered scanlines)
};
// true: the file is a PNG, 8-bit, colour type 2 or 6, not interlaced, with an "sbNd" chunk, a first IDAT of the 2-byte zlib header,
// exactly ceil(h / band_rows) band IDATs and a 4-byte last IDAT (the conditions of the parallel reader of host/png_io.hpp, which,
// like this function, does not check the chunks' CRCs), and every band is small enough for 32-bit bit positions (rows x line <=
// 2^30 bytes, segment < 2^28 bytes). false: not this decoder's file; `info` is untouched.
bool png_parse_banded(const uint8_t* file, size_t n, PngBandedInfo& info);
// ... and the camera-image form (include/s360_input_png.h): the same, plus depth 16 with colour type 2 — what png.hip's k_png_band<6>
// writes: 6 bytes per pixel, R,G,B with the high byte first, line = 1 + 6 w, the same two bounds.
bool png_parse_banded_input(const uint8_t* file, size_t n, PngBandedInfo& info);

// Where k_png_unfilter leaves an image's pixels.
enum PngStore : int {
  kPngStoreBytes = 0,  // packed 8-bit B,G,R(,A); a 16-bit file keeps its samples' high bytes (png_set_strip_16)
  kPngStoreU16 = 1,    // packed little-endian uint16 B,G,R: 16-bit files only, 2-byte aligned
  kPngStoreSide = 2,   // a side camera's source slot: uchar4 B,G,R,A with side_src_alpha's row ramp (3-channel files)
  kPngStorePole = 3    // a pole camera's source slot: uchar4 B,G,R,255 (3-channel files)
};
struct PngDecodeDst {
  uint8_t* p = nullptr;  // device memory
  int store = kPngStoreBytes;
  int feather = 0;       // kPngStoreSide: side_alpha_feather_size
};

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
// The same with a store per image (8- and 16-bit files); the stream waits for the events of `before` (null entries are skipped) in
// front of the unfilter launch, the first kernel that writes the destinations.
void png_decode_run(hipStream_t st, PngDecodeBufs& D, const std::vector<const uint8_t*>& files, const std::vector<PngBandedInfo>& info,
                    const std::vector<PngDecodeDst>& dst, const std::vector<hipEvent_t>& before, unsigned long long* stats, Profiler* prof);

}  // namespace s360
