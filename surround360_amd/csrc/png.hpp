// png.hpp — the finished equirect as a PNG file, encoded on the device (png.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "core.hpp"

namespace s360 {

// Geometry of one encode: an 8-bit B,G,R (channels = 3) or B,G,R,A (channels = 4) image of w x h pixels (rows contiguous) becomes
// an 8-bit RGB (colour type 2) or RGBA (colour type 6, alpha kept) PNG — or a 16-bit B,G,R image (depth = 16: the ISP's output_bpp 16
// result, 6 bytes per pixel) a 16-bit RGB PNG, Sub at a distance of 6 bytes — whose scanlines are deflated in bands of `rows_per_band`
// rows, one workgroup and one IDAT chunk per band. The band rule is one on bytes: ~192 KB of scanlines, at least ~64 bands.
struct PngPlan {
  int w = 0, h = 0, rows_per_band = 0, nbands = 0, channels = 3;
  int depth = 8;           // bits per sample: 8, or 16 with channels = 3 (little-endian uint16 B,G,R in, big-endian R,G,B samples out)
  size_t pixel_bytes() const { return (size_t)channels * (size_t)(depth / 8); }
  size_t line = 0;         // bytes of a filtered scanline: 1 + pixel_bytes x w
  size_t band_stride = 0;  // bytes reserved per band in the scratch (a band coded as stored blocks always fits)
  size_t file_bound = 0;   // upper bound of the file's size
  static PngPlan make(int w, int h, int channels = 3, int depth = 8);
};
// n images of differing size and channel count encoded by ONE launch sequence (png_batch_enqueue): where every image's bands,
// band table (nbands + 1 records) and file image (file_bound bytes, 16-byte aligned) lie in the batch's buffers.
struct PngBatchPlan {
  std::vector<PngPlan> img;
  std::vector<int> band0;                            // index of the image's first band among all bands of the batch
  std::vector<size_t> scratch_off, meta0, file_off;  // bytes, records, bytes
  int nbands = 0;
  size_t scratch_bytes = 0, meta_records = 0, file_bytes = 0;
  static PngBatchPlan make(const std::vector<PngPlan>& plans);
  static size_t table_bytes(size_t n, size_t nbands);  // the device table: per-image descriptors + the per-band image index
};
// What the device leaves per band (device layout; the host reads it back before the bytes).
struct PngBandMeta {
  unsigned bytes;    // deflate bytes of the band's segment (byte aligned: sync-flushed, the last band final)
  unsigned s1, s2;   // Adler-32 pieces of the band's filtered scanlines: sum of bytes, sum of (n - i) * byte[i], both mod 65521
  unsigned stored;   // 1: the band went out as stored blocks (Huffman coding would not have made it smaller)
  unsigned long long file_off;  // where the band's IDAT chunk starts in the file image (filled by the layout kernel)
};
// Enqueues filter + deflate + layout of `bgr` on `st`: afterwards `file` (>= plan.file_bound bytes) holds the IDAT chunks of
// the bands at their final offsets — length and type fields written, the 4 CRC bytes of every chunk left for the host — and
// `meta` (plan.nbands + 1 records; the last one's file_off = the offset behind the last band chunk) the band table. `scratch`
// (nbands x band_stride) is dead once the call's kernels have run: images encoded one after the other on one stream share it.
// Nothing waits.
void png_encode_enqueue(hipStream_t st, const uint8_t* bgr, const PngPlan& plan, DevBuf& scratch, DevBuf& meta, uint8_t* file);
// Host side, after `file[0 .. meta[nbands].file_off)` and the band table have been copied to host memory: writes signature,
// IHDR, sbNd, the zlib header chunk, every band chunk's CRC, the Adler-32 chunk and IEND. Returns the file's size.
size_t png_finish_host(uint8_t* file, size_t cap, const PngPlan& plan, const PngBandMeta* meta, int crc_threads);
// The batch: px[i] is image i's device pointer (4-byte aligned). One upload of the table (built in `table_host`, table_bytes of
// page-locked memory the caller keeps untouched until the copy has run), one k_png_band launch over all bands of all images, one
// layout launch (a workgroup per image: the prefix sum is segmented) and one gather launch. Afterwards files[file_off[i] ..] and
// meta[meta0[i] ..] hold for image i what png_encode_enqueue leaves for one image. Nothing waits on the host between images.
void png_batch_enqueue(hipStream_t st, const uint8_t* const* px, const PngBatchPlan& plan, DevBuf& table, void* table_host, DevBuf& scratch,
                       DevBuf& meta, DevBuf& files);
// offset of the first band chunk in the file (signature + IHDR + sbNd + zlib-header IDAT)
constexpr size_t kPngPreamble = 8 + 25 + 16 + 14;
uint32_t crc32_update(uint32_t crc, const uint8_t* p, size_t n);  // PNG / zlib CRC-32 (own tables, slicing by 8)

}  // namespace s360
