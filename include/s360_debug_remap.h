/* s360_debug_remap.h — test taps of libs360 like those of s360_debug.h (not part of the API of include/s360.h): the bicubic remap
 * kernels of the frame on caller-made sources, maps and flows, through the frame's own launchers, on buffers of the call's own (the
 * context's cache of packed maps is neither read nor written). */
#ifndef S360_DEBUG_REMAP_H
#define S360_DEBUG_REMAP_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Every output below is IN / OUT: what the caller's array holds is uploaded before the launches, so a word that no workgroup
 * stores comes back as the caller left it. */

/* Test tap: launch_remap_pack_map then launch_remap_cubic_u8c4_packed (the side cameras', the poles' projection) on `batch` BGRA
 * sources of sw x sh and `batch` maps of dw x dh (2 floats per pixel: x, y). alpha_mode 0: the interpolated alpha is kept; 1: the
 * pole rule of a 3-channel source (255, the feather rows 255 * ramp); 2: the pole rule of a 4-channel source (the minimum of the
 * interpolated alpha and the ramp). weights 0: as the library is configured (S360_REMAP_REBUILD_WEIGHTS), 1: the 1024 x 16 table,
 * 2: the weights rebuilt in the kernel — S360_ERR_INVALID_ARG where the host's rebuild of the table had failed.
 * dst: batch x dh x dw x 4 bytes; packed: batch x dh x dw dwords {live << 31 | row in the box << 21 | column in the box << 10 |
 * fraction index}; tiles: batch x ceil(dh / 16) x ceil(dw / 64) records of 4 ints {box x0, box y0, box width, box height; height
 * -1 = the box does not fit, the tile gathers through the map; no live pixel: INT_MAX, INT_MAX, 0, 0}. */
int s360_debug_remap_packed(s360_ctx* ctx, const uint8_t* src, int sw, int sh, const float* map, int dw, int dh, int batch,
                            int alpha_mode, int y_feather_start, int feather_size, int weights, uint8_t* dst, uint32_t* packed,
                            int32_t* tiles);

/* Test tap: launch_pole_warp_packed (poleToSideFlow's ramped warp of the extended fisheye image) on a caller-made BGRA image of
 * ext_w x rows and a caller-made flow (2 floats per pixel). warped, packed, tiles: as above, one image. */
int s360_debug_pole_warp_packed(s360_ctx* ctx, const uint8_t* ext_fisheye, int ext_w, int rows, const float* flow,
                                float pole_camera_radius, float phi_ramp_start, float phi_mid, float phi_ramp_end, uint8_t* warped,
                                uint32_t* packed, int32_t* tiles);

/* Test tap: launch_remap_by_flow (pole removal: the BGRA image sampled at (x, y) + flow) on a caller-made image and flow of w x h. */
int s360_debug_remap_by_flow(s360_ctx* ctx, const uint8_t* src, int w, int h, const float* flow, uint8_t* dst);

#ifdef __cplusplus
}
#endif
#endif
