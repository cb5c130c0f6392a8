// debug_views.hpp — the views of --save_debug_images that no buffer of a frame holds in the written form (debug_views.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace s360 {

// One view: a rectangle of a B,G,R,A image, rotated horizontally inside itself, written with or without its alpha, with
// transparent rows below. The destination's rows are contiguous (w x channels_out bytes, no pitch):
//   dst(x, y) = src(x0 + (x - shift) mod w, y0 + y)   for y < h            (np.roll(rect, shift, axis = 1); offsetHorizontalWrap)
//   dst(x, y) = 0                                      for h <= y < h + pad_rows   (copyMakeBorder below, TRSP:538-546)
// Device layout (the table k_debug_views reads) and host layout are the same.
struct DebugViewDesc {
  const uint8_t* src;  // B,G,R,A, 4-byte aligned
  uint8_t* dst;        // 4-byte aligned with channels_out 4, any alignment with 3
  int src_pitch;       // pixels per source row
  int src_rows;        // rows of the source image (with src_pitch: the extents every source index is checked against)
  int x0, y0, w, h;    // the rectangle
  int shift;           // 0 <= shift < w
  int pad_rows;
  int channels_in;     // 4
  int channels_out;    // 4, or 3: alpha dropped (cvtColor BGRA2BGR, TRSP:890-894)
};

// Throws Error(S360_ERR_INVALID_ARG) for a descriptor the kernel would refuse to index (a rectangle outside its source, a shift
// outside the rectangle, unsupported channel counts, misaligned pointers).
void debug_view_check(const DebugViewDesc& d);
// ONE launch for all `n` views (1 .. 65535): grid = (row segments of the largest view, n). table_dev: the n descriptors on the
// device; table_host: the same on the host (grid sizing and debug_view_check only — not read after the call returns).
void launch_debug_views(hipStream_t st, const DebugViewDesc* table_dev, const DebugViewDesc* table_host, int n);

}  // namespace s360
