/* s360_debug.h — test taps of libs360 that are not part of the API of include/s360.h: entry points the parity tests use to run
 * one stage of the path on caller-made inputs. (s360_debug_flow_levels, the older tap, is declared in s360.h.) */
#ifndef S360_DEBUG_H
#define S360_DEBUG_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test tap: PixFlow's entry on `batch` caller-made BGRA images of sw x sh: the INTER_CUBIC resize to dw x dh and the grey
 * and alpha planes of the resized images (batch x dh x dw floats each). generic == 0: the launch as the flow engine makes
 * it (the tiled kernel where a tile's source box fits, *tiled = 1; the generic kernels otherwise, *tiled = 0); down_out may
 * then be NULL, and the image is not stored. generic != 0: the one-thread-per-pixel resize and the grey / alpha kernel
 * whatever the shape. */
int s360_debug_entry_downscale(s360_ctx* ctx, const uint8_t* src_bgra, int sw, int sh, int batch, int dw, int dh, int generic,
                               uint8_t* down_out, float* gray_out, float* alpha_out, int* tiled);

#ifdef __cplusplus
}
#endif
#endif
