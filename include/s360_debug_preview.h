/* s360_debug_preview.h — test taps of the preview object (include/s360_preview.h), like those of s360_debug.h: not part of the
 * API. layer: 0 top, 1 bottom, 2 secondary bottom. All pointers are host memory. */
#ifndef S360_DEBUG_PREVIEW_H
#define S360_DEBUG_PREVIEW_H
#include "s360_preview.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The layer's rescaled camera (Camera::createRescaledCamera of the chosen camera). */
int s360_debug_preview_camera(const s360_preview* p, int layer, s360_camera* out);
/* The layer's warp map: eqr_h x eqr_w x 2 floats (x, y; (-1, -1) where the camera does not see the point). */
int s360_debug_preview_map(s360_preview* p, int layer, float* map_out);
/* Caller-made maps in place of the built ones, for every render that follows; a NULL pointer leaves that layer's map. */
int s360_debug_preview_set_maps(s360_preview* p, const float* map_top, const float* map_bottom, const float* map_bottom2);
/* The layer's developed image as the last render left it: (raw_h / 2) x (raw_w / 2) x 4 floats, B,G,R,alpha. */
int s360_debug_preview_developed(s360_preview* p, int layer, float* out);
/* The layer's developed image through its map (k_preview_compose's sample of that layer, before the softmax): eqr_h x eqr_w x 4
 * floats. */
int s360_debug_preview_remapped(s360_preview* p, int layer, float* out);

#ifdef __cplusplus
}
#endif
#endif
