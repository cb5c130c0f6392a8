/* s360_debug_cubemap.h — test taps of libs360 like those of s360_debug_remap.h (not part of the API of include/s360.h): the stereo
 * cubemap kernels of the frame on caller-made eyes, through the frame's own map construction and launchers, on buffers of the
 * call's own (the context's cache of face maps and prepared maps is neither read nor written). */
#ifndef S360_DEBUG_CUBEMAP_H
#define S360_DEBUG_CUBEMAP_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Every output below is IN / OUT: what the caller's array holds is uploaded before the launches, so a word that no workgroup
 * stores comes back as the caller left it. */

/* Test tap: the face maps of (sw, sh, fw, fh) as s360_set_cubemap_output builds them, then launch_cubemap_pack and
 * launch_cubemap_tiles (the cubemap of every frame of a stream or a batch) on `n_slots` pairs of BGRA eyes of sw x sh:
 * eyes[2 k], eyes[2 k + 1] = left, right eye of slot k, 2 * n_slots x sh x sw x 4 bytes. video 1: the "video" layout (3 x 2 faces
 * per eye, flipped horizontally), 0: "photo" (six faces stacked). lds_pixels: 4096 or 2560, the source box a tile may hold.
 * n_slots: 1 .. 64 (a launch covers 16 slots).
 * out: n_slots stacked B,G,R cubemaps (video: 4 fh x 3 fw x 3 bytes each, photo: 12 fh x fw x 3); maps: 6 x fh x fw x 2 floats
 * (faces RIGHT, LEFT, TOP, BOTTOM, BACK, FRONT; x, y); packed: ONE eye's half of the stacked layout, one dword per pixel {1 << 31 |
 * row in the box << 21 | column in the box << 10 | fraction index}, 0 in a tile that gathers; tiles: 6 x ceil(fh / 16) x
 * ceil(fw / 16) records of 4 ints, face slots in the layout's order {box x0, box y0, box width, box height; height -1 = no compact
 * box, the tile gathers through the float map}. */
int s360_debug_cubemap_tiles(s360_ctx* ctx, const uint8_t* eyes, int n_slots, int sw, int sh, int fw, int fh, int video,
                             int lds_pixels, uint8_t* out, float* maps, uint32_t* packed, int32_t* tiles);

/* Test tap: launch_cubemap (s360_frame_cubemap's kernel, one thread per pixel) on the same eyes and the same maps, slot by slot.
 * out, maps: as above. */
int s360_debug_cubemap(s360_ctx* ctx, const uint8_t* eyes, int n_slots, int sw, int sh, int fw, int fh, int video, uint8_t* out,
                       float* maps);

#ifdef __cplusplus
}
#endif
#endif
