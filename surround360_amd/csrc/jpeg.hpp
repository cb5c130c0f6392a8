// jpeg.hpp — baseline JPEG encoded on the device (jpeg.hip): the encoder object behind include/s360_jpeg.h and behind the
// preview object's .jpg output (preview.hip). The file is the one host/jpeg_io.hpp's jpegio::encode writes, byte for byte.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "core.hpp"

namespace s360 {

constexpr int JPEG_HEADER_BYTES = 623;     // SOI, APP0, DQT x 2, SOF0, DHT x 4, SOS
constexpr int JPEG_MAX_BLOCK_BITS = 1660;  // chroma: DC 11 + 11, 63 x (AC 16 + 10); luma: 1658
constexpr int JPEG_SCAN_ITEMS = 1024;      // items (blocks, stream tiles) one workgroup of a scan kernel takes
constexpr int JPEG_STUFF_TILE = 4096;      // stream bytes one workgroup of the stuffing kernels takes
// Offset types: bit and byte offsets into the scan are 32-bit. With 6 blocks of at most JPEG_MAX_BLOCK_BITS bits per MCU that
// holds for up to JPEG_MAX_MCUS MCUs of 16 x 16 pixels (every size up to 8192 x 8192 has at most 262 144); larger images are
// refused with S360_ERR_INVALID_ARG.
constexpr long long JPEG_MAX_MCUS = 0xFFFFFFFFll / (6 * JPEG_MAX_BLOCK_BITS) - 1;  // 431 220

inline long long jpeg_mcus(int w, int h) { return (long long)((w + 15) / 16) * ((h + 15) / 16); }
// bytes of the scan before stuffing, rounded up to whole words; stuffing at most doubles it
inline size_t jpeg_raw_cap_mcus(long long mcus) { return (((size_t)mcus * 6 * JPEG_MAX_BLOCK_BITS + 7) / 8 + 3) / 4 * 4; }
inline size_t jpeg_raw_cap(int w, int h) { return jpeg_raw_cap_mcus(jpeg_mcus(w, h)); }
inline size_t jpeg_scan_cap(int w, int h) { return 2 * jpeg_raw_cap(w, h); }
inline size_t jpeg_file_bound(int w, int h) { return JPEG_HEADER_BYTES + jpeg_scan_cap(w, h) + 2; }
// The scan buffers a frame slot keeps (s360_set_jpeg_encode, include/s360_frame_jpeg.h) are not the worst case: 768 bytes per MCU,
// the size of the MCU's own 16 x 16 B,G,R pixels (the worst case is 2490). A scan that needs more is refused, never cut short.
constexpr size_t JPEG_FRAME_MCU_BYTES = 16 * 16 * 3;
inline size_t jpeg_frame_scan_cap(int w, int h) { return (size_t)jpeg_mcus(w, h) * JPEG_FRAME_MCU_BYTES; }
inline bool jpeg_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 65535 && h <= 65535 && jpeg_mcus(w, h) <= JPEG_MAX_MCUS; }

struct JpegEncoder {
  int maxW = 0, maxH = 0, quality = 95;
  long long maxMcus = 0;  // what the buffers hold: jpeg_mcus(maxW, maxH), or what init_mcus was given
  int q[2][64];  // quantisation tables, natural order
  DevBuf dTab, dCoef, dBlkBits, dBlkOff, dGrpTot, dGrpOff, dWords, dTileCnt, dTileOff, dTotals;
  // allocates for images up to max_w x max_h and uploads the tables on `st` (which is synchronised before returning)
  void init(int max_w, int max_h, int quality_, hipStream_t st);
  // ... for images of any shape with up to max_mcus MCUs of 16 x 16 pixels (1..JPEG_MAX_MCUS): an encoder that serves images of
  // several shapes (a frame's equirect and its cubemap) is sized by the largest of them, not by the box around them
  void init_mcus(long long max_mcus, int quality_, hipStream_t st);
  // Enqueues the whole encoder on `st`; nothing synchronises. bgr: device memory, h rows of w x 3 bytes. scan: device memory of
  // scan_cap bytes, receives the entropy-coded segment (stuffed, padded); count[0] its byte count. scan_cap >= jpeg_scan_cap(w, h)
  // holds every scan, and a smaller one is refused here unless `capped`: then a scan of more than scan_cap bytes is not stored at
  // all — not one byte of it — and count[0] > scan_cap is how the caller learns of it, and of the size it needed.
  void encode(const uint8_t* bgr, int w, int h, uint8_t* scan, size_t scan_cap, uint32_t* count, hipStream_t st, bool capped = false);
  // the JPEG_HEADER_BYTES bytes in front of the scan
  void header(uint8_t* out, int w, int h) const;
  // test tap: after encode() has run, the coefficient blocks and their bit lengths (device pointers)
  const int16_t* coef() const { return dCoef.as<int16_t>(); }
  const uint32_t* block_bits() const { return dBlkBits.as<uint32_t>(); }
};

}  // namespace s360
