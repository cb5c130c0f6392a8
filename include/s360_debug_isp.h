/* s360_debug_isp.h — a test tap of libs360 like those of s360_debug.h (not part of the API of include/s360.h): the ISP's
 * intermediates where its kernels leave them. */
#ifndef S360_DEBUG_ISP_H
#define S360_DEBUG_ISP_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test tap: one image through the object's own launch sequence — what s360_isp_process enqueues: the same kernels, grids and
 * buffers — and then copies of the device buffers that survive it. Every output pointer may be NULL; one that names a buffer the
 * configuration does not have is refused (S360_ERR_INVALID_ARG). W x H is the output's size (w / resize x h / resize).
 *   soft ISP (pipe = 0): plane W x H floats (the normalised Bayer plane after clamp-and-stretch and stuck-pixel removal);
 *     flag W x H bytes (dH <= dV), gv, gh, green W x H floats — demosaic_filter 2 only; tone H x W x 3 floats (r, g, b: the
 *     tone-mapped image before sharpening); low H x W x 3 floats (the low pass; with sharpening only).
 *   pipeline (pipe = 1 / 2): plane (W + 16) x (H + 16) floats (the site plane on the image extended by 8); flag (W + 12) x
 *     (H + 12) bytes; green (W + 4) x (H + 4) floats; tone, low H x W x 3 floats; gv / gh never. pipe = 2 has plane and tone only.
 * stop_after: 0 = the whole sequence. 1 = the sequence ends after the low pass's first direction (rows for the soft ISP, y for
 * the pipeline), which the second direction overwrites: `low` then holds that, and out_bgr (not produced) must be NULL. Nothing
 * is launched that s360_isp_process does not launch. out_bgr: as s360_isp_process. */
int s360_debug_isp_stages(s360_isp* isp, const uint16_t* raw16, int w, int h, int stop_after, float* plane, uint8_t* flag, float* gv,
                          float* gh, float* green, float* tone, float* low, void* out_bgr);

#ifdef __cplusplus
}
#endif
#endif
