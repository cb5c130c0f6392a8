/* s360_debug_frame_jpeg.h — test tap of the frame JPEG encoder (include/s360_frame_jpeg.h); not part of the API. It reaches the
 * capacity rule of a slot's scan buffer, and sizes no test can afford to render, without rendering anything. */
#ifndef S360_DEBUG_FRAME_JPEG_H_
#define S360_DEBUG_FRAME_JPEG_H_
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Encodes bgr (host memory, h rows of w B,G,R pixels) through the context's frame encoder — the object and the quality of
 * s360_set_jpeg_encode, grown to the image if need be — into a device buffer of scan_cap bytes (0 .. the worst case of the size)
 * followed by a guard region of 4096 bytes; the whole buffer is filled with a pattern first. Synchronous.
 *   The scan fits: `out` receives the complete file and *n_out its size, as s360_frame_download_jpeg returns them; *stored = the
 *   scan's bytes. cap smaller than the file: S360_ERR_INVALID_ARG, *n_out = the size needed.
 *   It does not fit: the error of s360_frame_download_jpeg for such a frame (S360_ERR_STATE, the message names the bytes the scan
 *   needed, *n_out = the size the file would have had); *stored = the bytes of the scan buffer that no longer hold the pattern —
 *   0 when the rule is kept.
 * *guard_touched: the bytes of the guard region that no longer hold the pattern, in either case. ms (nullable): device time of
 * the encode's kernels (hipEvents around them, the upload and the pattern fill not included). */
int s360_debug_frame_jpeg(s360_ctx* ctx, const uint8_t* bgr, int w, int h, size_t scan_cap, uint8_t* out, size_t cap, size_t* n_out,
                          size_t* stored, size_t* guard_touched, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* S360_DEBUG_FRAME_JPEG_H_ */
