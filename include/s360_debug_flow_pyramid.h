/* s360_debug_flow_pyramid.h — test taps of libs360 like those of s360_debug.h (not part of the API of include/s360.h): what
 * PixFlow::computeOpticalFlow (PixFlow.h:81-153) does in front of its level loop — pre-blur, the image pyramids, the previous
 * images, the motion map, the previous flow and their pyramids — as FlowEngine::prepare runs it, and the two resizes between the
 * pyramid's levels (INTER_LINEAR of float planes, INTER_CUBIC of flows) on caller-made data of any size. */
#ifndef S360_DEBUG_FLOW_PYRAMID_H
#define S360_DEBUG_FLOW_PYRAMID_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What s360_debug_flow_prepare hands out; every pointer may be null. N images, B flows; a plane's pyramid is its levels one after
 * the other, finest first, P pixels in all. */
typedef struct s360_flow_prepare_out {
  int cap_levels;     /* entries of level_w, level_h and factors */
  size_t cap_pixels;  /* the P that pyr_images, prev_pyr and motion_pyr have room for; a larger pyramid is an error */
  int* level_w;       /* the sizes of the levels ... */
  int* level_h;
  int* n_levels;      /* ... and their number */
  float* factors;     /* per level: what the level multiplies the previous flow by as it reads it (level 0: 1) */
  float* pyr_images;  /* 2N x P: per level N grey planes (pre-blurred at level 0), then N alpha planes */
  float* prev_pyr;    /* B x P x 2: per level the B previous flows, downscaled and x rows_down / rows_full, NOT yet x factors[l] */
  float* motion_pyr;  /* N x P: per level the N motion planes. Both only with previous state */
} s360_flow_prepare_out;

/* Test tap: FlowEngine::prepare as FlowEngine::compute calls it, on n_images BGRA images of w x h (images: n_images x h x w x 4)
 * and the flows i0[b] -> i1[b]. prev_images (n_images x h x w x 4) and prev_flows (n_flows x h x w x 2): both or neither; they
 * are uploaded as one allocation per image / flow and reach the kernels through the batch's pointer tables. fill in 0..255: every
 * engine buffer the preparation writes holds that byte before it runs; -1: the buffers stay as the last call left them.
 * w, h >= 4 (2 x 2 after the entry downscale); 1 <= n_flows <= 2048; 0 <= i0[b], i1[b] < n_images. */
int s360_debug_flow_prepare(s360_ctx* ctx, const uint8_t* images, int n_images, int w, int h, const int* i0, const int* i1, int n_flows,
                            const uint8_t* prev_images, const float* prev_flows, const char* alg, int fill,
                            const s360_flow_prepare_out* out);

/* Test tap: launch_resize_linear_f32 (the pyramids' INTER_LINEAR resize) of `planes` planes of cn (1 or 2) interleaved channels,
 * sw x sh -> dw x dh, times post_scale where do_scale is not 0. dst (planes x dh x dw x cn) is uploaded first: a word no thread
 * stores comes back as the caller left it. *tiled (may be null): 1 if the launcher takes the tiled one-channel kernel for the shape.
 * dst == null: nothing is launched, only *tiled is reported (src and ctx may be null too). */
int s360_debug_resize_linear_f32(s360_ctx* ctx, const float* src, int sw, int sh, int cn, int planes, int dw, int dh, float post_scale,
                                 int do_scale, float* dst, int* tiled);

/* Test tap: launch_resize_cubic_f32c2 (INTER_CUBIC of flows, then x post_scale) of n_flows flows, sw x sh -> dw x dh.
 * through_table != 0: every source is an allocation of its own and reaches the kernel through a device pointer table, as the
 * previous flows do. dst and *tiled as above. */
int s360_debug_resize_cubic_flow(s360_ctx* ctx, const float* src, int sw, int sh, int n_flows, int dw, int dh, float post_scale,
                                 int through_table, float* dst, int* tiled);

#ifdef __cplusplus
}
#endif
#endif
