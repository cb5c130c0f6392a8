/* s360_debug_views.h — test tap of libs360 like those of s360_debug_remap.h (not part of the API of include/s360.h): k_debug_views,
 * the kernel behind the views of s360_set_debug_images (s360_debug_images.h), on caller-made images and descriptors. */
#ifndef S360_DEBUG_VIEWS_H
#define S360_DEBUG_VIEWS_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One view: dst(x, y) = src(x0 + (x - shift) mod w, y0 + y) for y < h, 0 for h <= y < h + pad_rows; the destination's rows are
 * contiguous, w x channels_out bytes. src_off / dst_off: where the source image (src_pitch x src_rows B,G,R,A pixels, 4-byte
 * aligned) and the destination (4-byte aligned with channels_out 4) begin in the call's two areas, in bytes. */
typedef struct s360_debug_view {
  uint64_t src_off, dst_off;
  int32_t src_pitch, src_rows;
  int32_t x0, y0, w, h;
  int32_t shift;        /* 0 <= shift < w */
  int32_t pad_rows;
  int32_t channels_in;  /* 4 */
  int32_t channels_out; /* 4 or 3 */
} s360_debug_view;

/* ONE k_debug_views launch over all n views (1 .. 65535; they may differ in size, the grid is the largest one's). src: src_bytes
 * of source images; dst: dst_bytes, IN / OUT — what the caller's array holds is uploaded before the launch, so a byte no work item
 * stores comes back as the caller left it. Both areas begin 256-byte aligned on the device. A view that does not lie inside the
 * areas, or that the kernel's own checks refuse, is S360_ERR_INVALID_ARG and nothing is launched. Works on any context. */
int s360_debug_views(s360_ctx* ctx, int n, const s360_debug_view* views, const uint8_t* src, size_t src_bytes, uint8_t* dst,
                     size_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif
