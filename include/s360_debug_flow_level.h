/* s360_debug_flow_level.h — a test tap of libs360 like those of s360_debug.h (not part of the API of include/s360.h): ONE pyramid
 * level of PixFlow (patchMatchPropagationAndSearch, PixFlow.h:344-413, and adjustFlowTowardPrevious, :185-193) on caller-made
 * planes, with what the level's launches leave between them. */
#ifndef S360_DEBUG_FLOW_LEVEL_H
#define S360_DEBUG_FLOW_LEVEL_H
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What the tap hands out; every pointer may be null. N images, B flows of w x h. */
typedef struct s360_flow_level_out {
  float* gradients;    /* N x h x w x 2: {Ix, Iy} of every image (Sobel + 3x3 Gaussian) */
  float* initial_flow; /* B x h x w x 2: the flow the record blur reads (the caller's, or zeros + the search's result) */
  float* blurred_flow; /* B x h x w x 2: the 15x15 blur decoded from the sweeps' records; defined only where `updated` is 1 */
  uint8_t* updated;    /* B x h x w: 1 where the record does not carry the not-updated mark (alpha0 > 0.9f && alpha1 > 0.9f) */
  uint32_t* row_flags; /* B x h words: 0 = the row has an updated pixel, all-ones = it has none */
  float* sweep_forward;  /* B x h x w x 2 each: the flow after the forward sweep, ... */
  float* median_first;   /* ... the first median, */
  float* sweep_backward; /* ... the backward sweep, */
  float* median_second;  /* ... the second median */
  float* diffused;       /* ... and lowAlphaFlowDiffusion; without previous state only (with it the diffusion and the adjustment
                            are one launch, and asking for this is an error) */
  float* final_flow;     /* what the level hands to the upscale: the diffused flow, adjusted toward the previous one if given */
} s360_flow_level_out;

/* info[] of s360_debug_flow_level: what was launched */
enum {
  S360_FLI_LANES_PER_PIXEL = 0, /* of the sweep: 3 or 4 (throughput kernel), 0 = the lockstep kernel */
  S360_FLI_BANDS = 1,           /* bands per flow of a sweep launch */
  S360_FLI_WAVES = 2,           /* waves of a sweep launch (throughput kernel: persistent ones, each takes band tickets) */
  S360_FLI_FAST_DIVISION = 3,   /* 1: the verified fast division / square root, 0: the IEEE expansions */
  S360_FLI_MEDIAN_TILE = 4,     /* threads per tile row of the row-8 median: 32 / 16 / 8 / 4, 0 = the narrow kernel */
  S360_FLI_SWEEP_ERROR = 5,     /* the sweep error word after the level (0 = no band timed out); reading it resets it */
  S360_FLI_COUNT = 8
};

/* Test tap: the body of the flow engine's level loop, once, as FlowEngine::compute runs it, in the context's sweep mode
 * (s360_set_sweep_mode). gray, alpha: n_images planes of w x h floats each. Flow b matches plane i0[b] (I0) against i1[b] (I1).
 * initial_flow (n_flows x h x w x 2) or null: null takes the coarsest level's path (zeros, and with pixflow_search_20 and a hint
 * the search). prev_flow (n_flows x h x w x 2) and motion (n_images x h x w; flow b reads plane i1[b]) are both given or both
 * null; the previous flow is multiplied by prev_scale as it is read. info: S360_FLI_COUNT ints, may be null.
 * w, h >= 2; 1 <= n_flows <= 2048; 0 <= i0[b], i1[b] < n_images. */
int s360_debug_flow_level(s360_ctx* ctx, const float* gray, const float* alpha, int n_images, int w, int h, const int* i0,
                          const int* i1, int n_flows, const float* initial_flow, const char* alg, int hint, const float* prev_flow,
                          const float* motion, float prev_scale, const s360_flow_level_out* out, int* info);

#ifdef __cplusplus
}
#endif
#endif
