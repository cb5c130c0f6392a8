// debug_views.hip — k_debug_views: the images of --save_debug_images that no buffer of a frame holds in the written form, all of a
// frame's in ONE table-driven launch (debug_views.hpp): the crop of the feathered side image (TRSP:396-397), the pole layer padded
// to full rows (TRSP:538-546), the offset-wrapped panoramas (TRSP:795-796), the eyes without their alpha (TRSP:890-894).
//
// Work item: one 16-byte-ALIGNED chunk of one destination row. grid.x walks (row, segment of 256 chunks), grid.y the descriptors;
// a workgroup past its view's last row segment returns (the grid is sized for the largest view). A destination row starts at any
// byte — 3-channel rows of an odd width, a base 4 bytes into a line — so the chunk grid is laid over ADDRESSES, not over the row:
// the chunks inside the row are stored with one 16-byte store, the row's head and tail chunks byte by byte (they share their 16
// bytes with the neighbouring rows, which other work items write). 4 -> 4 channels reads its four pixels with one 16-byte load where
// they are contiguous in the source (no wrap inside the chunk) and that address is 16-byte aligned, else pixel by pixel; 4 -> 3
// reads the six pixels its 16 bytes touch pixel by pixel (4-byte loads). Every source index is checked against the descriptor's
// extents and every destination byte against the row before it addresses memory; what fails the check reads as 0 / is not stored.
//
// gfx950, VGPRs / SGPRs / LDS bytes (no scratch, no spills): k_debug_views 14/46/0, 8 waves per SIMD
#include "debug_views.hpp"

#include <algorithm>
#include <string>

#include "../../include/s360.h"
#include "core.hpp"

namespace s360 {

namespace {

constexpr int DV_THREADS = 256;
constexpr int DV_CHUNK = 16;

__host__ __device__ inline unsigned dv_row_bytes(const DebugViewDesc& D) { return (unsigned)D.w * (unsigned)D.channels_out; }
// chunks a row can touch: its bytes and up to 15 bytes of its head chunk that lie in front of it
__host__ __device__ inline unsigned dv_segments(const DebugViewDesc& D) {
  const unsigned chunks = (dv_row_bytes(D) + DV_CHUNK - 1) / DV_CHUNK + 1;
  return (chunks + DV_THREADS - 1) / DV_THREADS;
}

// destination pixel px of row y as the source holds it (B | G << 8 | R << 16 | A << 24); 0 in the padding and outside the extents
__device__ __forceinline__ unsigned dv_pixel(const DebugViewDesc& D, int y, int px) {
  if (y >= D.h || px < 0 || px >= D.w) return 0u;
  int sx = px - D.shift;
  if (sx < 0) sx += D.w;
  const int X = D.x0 + sx, Y = D.y0 + y;
  if (sx < 0 || sx >= D.w || X < 0 || X >= D.src_pitch || Y < 0 || Y >= D.src_rows) return 0u;
  return reinterpret_cast<const unsigned*>(D.src)[(size_t)Y * D.src_pitch + X];
}

}  // namespace

__global__ __launch_bounds__(DV_THREADS) void k_debug_views(const DebugViewDesc* __restrict__ table, int n) {
  const int d = blockIdx.y;
  if (d >= n) return;
  const DebugViewDesc D = table[d];
  const int rows = D.h + D.pad_rows;
  const unsigned rowBytes = dv_row_bytes(D), segs = dv_segments(D);
  if (blockIdx.x >= (unsigned long long)rows * segs) return;  // (a smaller view than the one the grid was sized for)
  const int y = (int)(blockIdx.x / segs);
  const unsigned seg = blockIdx.x % segs;
  uint8_t* row = D.dst + (size_t)y * rowBytes;
  const int head = (int)(reinterpret_cast<uintptr_t>(row) & (DV_CHUNK - 1));  // bytes of the first chunk in front of the row
  const int b0 = (int)((seg * DV_THREADS + threadIdx.x) * DV_CHUNK) - head;   // the chunk's first byte, relative to the row
  if (b0 >= (int)rowBytes) return;
  unsigned v[4];
  if (D.channels_out == 4) {
    const int p0 = b0 >> 2;  // (b0 is a multiple of 4: the destination is 4-byte aligned; arithmetic shift for the head chunk)
    bool wide = false;
    if (y < D.h && p0 >= 0 && p0 + 3 < D.w && (p0 >= D.shift || p0 + 3 < D.shift)) {  // four pixels of the row, no wrap between them
      int sx = p0 - D.shift;
      if (sx < 0) sx += D.w;
      const int X = D.x0 + sx, Y = D.y0 + y;
      if (sx >= 0 && sx + 3 < D.w && X >= 0 && X + 3 < D.src_pitch && Y >= 0 && Y < D.src_rows) {
        const unsigned* s = reinterpret_cast<const unsigned*>(D.src) + (size_t)Y * D.src_pitch + X;
        if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
          const uint4 q = *reinterpret_cast<const uint4*>(s);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
          wide = true;
        }
      }
    }
    if (!wide) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = dv_pixel(D, y, p0 + k);
    }
  } else {
    // 16 bytes of B,G,R triples begin `rem` bytes into pixel pf and end inside pixel pf + 5
    const int pf = (b0 + 18) / 3 - 6;  // floor(b0 / 3) for b0 >= -18
    const int rem = b0 - 3 * pf;
    unsigned q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = dv_pixel(D, y, pf + k) & 0xffffffu;
    // the 18 bytes of the six pixels as dwords, then shifted down by rem bytes
    const unsigned s0 = q[0] | (q[1] << 24), s1 = (q[1] >> 8) | (q[2] << 16), s2 = (q[2] >> 16) | (q[3] << 8);
    const unsigned s3 = q[4] | (q[5] << 24), s4 = q[5] >> 8;
    const unsigned sh = 8u * (unsigned)rem;
    v[0] = (unsigned)((((unsigned long long)s1 << 32) | s0) >> sh);
    v[1] = (unsigned)((((unsigned long long)s2 << 32) | s1) >> sh);
    v[2] = (unsigned)((((unsigned long long)s3 << 32) | s2) >> sh);
    v[3] = (unsigned)((((unsigned long long)s4 << 32) | s3) >> sh);
  }
  const int left = (int)rowBytes - b0;
  const int lo = b0 < 0 ? -b0 : 0, hi = left < DV_CHUNK ? left : DV_CHUNK;  // bytes [lo, hi) of the chunk are the row's
  if (lo == 0 && hi == DV_CHUNK) {
    *reinterpret_cast<uint4*>(row + b0) = make_uint4(v[0], v[1], v[2], v[3]);  // (row + b0 is 16-byte aligned by construction)
  } else {
#pragma unroll
    for (int j = 0; j < DV_CHUNK; ++j)
      if (j >= lo && j < hi) row[b0 + j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
  }
}

void debug_view_check(const DebugViewDesc& d) {
  auto bad = [](const char* what) { throw Error(S360_ERR_INVALID_ARG, std::string("debug view: ") + what); };
  if (!d.src || !d.dst) bad("null image");
  if (d.channels_in != 4 || (d.channels_out != 3 && d.channels_out != 4)) bad("channels must be 4 -> 4 or 4 -> 3");
  if (d.w <= 0 || d.h <= 0 || d.pad_rows < 0 || d.src_pitch <= 0 || d.src_rows <= 0) bad("empty image");
  if (d.w > (1 << 24) || d.h > (1 << 24) || d.pad_rows > (1 << 24)) bad("image too large");
  if (d.x0 < 0 || d.y0 < 0 || d.x0 > d.src_pitch - d.w || d.y0 > d.src_rows - d.h) bad("the rectangle does not lie inside its source");
  if (d.shift < 0 || d.shift >= d.w) bad("the shift must lie in [0, w)");
  if (reinterpret_cast<uintptr_t>(d.src) & 3) bad("the source must be 4-byte aligned");
  if (d.channels_out == 4 && (reinterpret_cast<uintptr_t>(d.dst) & 3)) bad("a 4-channel destination must be 4-byte aligned");
}

void launch_debug_views(hipStream_t st, const DebugViewDesc* table_dev, const DebugViewDesc* table_host, int n) {
  if (n < 1 || n > 65535 || !table_dev || !table_host) throw Error(S360_ERR_INVALID_ARG, "debug views: 1 .. 65535 descriptors per launch");
  unsigned long long tiles = 0;
  for (int i = 0; i < n; ++i) {
    debug_view_check(table_host[i]);
    tiles = std::max(tiles, (unsigned long long)(table_host[i].h + table_host[i].pad_rows) * dv_segments(table_host[i]));
  }
  if (tiles > 0x7fffffffull) throw Error(S360_ERR_INVALID_ARG, "debug views: image too large");
  hipLaunchKernelGGL(k_debug_views, dim3((unsigned)tiles, (unsigned)n), dim3(DV_THREADS), 0, st, table_dev, n);
}

}  // namespace s360
