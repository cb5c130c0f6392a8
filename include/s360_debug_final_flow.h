/* s360_debug_final_flow.h — a test tap of libs360 like those of s360_debug.h (not part of the API of include/s360.h): PixFlow's
 * final step on caller-made flows. */
#ifndef S360_DEBUG_FINAL_FLOW_H
#define S360_DEBUG_FINAL_FLOW_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test tap: PixFlow's final step (PixFlow.h:175-182) on `batch` caller-made flows of sw x sh (2 floats per pixel): the
 * INTER_LINEAR resize to dw x dh, the multiplication by post_scale and the 3x3 Gaussian blur (sigma 1), written through a table
 * of `batch` destination pointers into allocations of their own, as the flow engine writes its flows; out: batch x dh x dw x 2
 * floats. generic == 0: the launch as the flow engine makes it (the tiled kernel where a tile's source box fits, *tiled = 1;
 * the blur kernel that resizes while it loads its tile otherwise, *tiled = 0). generic != 0: the latter whatever the shape. */
int s360_debug_upscale_blur(s360_ctx* ctx, const float* src_flow, int sw, int sh, int batch, int dw, int dh, float post_scale,
                            int generic, float* out, int* tiled);

#ifdef __cplusplus
}
#endif
#endif
