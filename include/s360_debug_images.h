/*
 * s360_debug_images.h — the reference's debug images (TestRenderStereoPanorama --save_debug_images, TestPoleRemoval) from a frame
 * that was rendered on the device, and pole removal as an operator (extension of the C ABI of s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. They are kept in a header of their own
 * because they are one optional path: the pictures a user looks at to judge a rig's calibration and pole masks
 * (debug/<frame>/projections/crop_<camera>.png, sphericalImg_offsetwrap{L,R}.png, warpedSpherical_<eye>.png, _bottomCombined.png
 * ...), kept on the device when a frame is rendered, fetched raw or as finished PNG files.
 */
#ifndef S360_DEBUG_IMAGES_H_
#define S360_DEBUG_IMAGES_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Switches the debug images of the frames rendered from now on on or off (default off). While on, a render keeps every image of
 * the list below for the selected slot's latest frame — a superset of s360_set_keep_intermediates, which stays as it is — until the
 * next render call of the context: the copies of what later kernels of the frame overwrite (the panoramas before the pole
 * composite, the eyes before the sharpen), and the views no buffer holds (one k_debug_views launch behind the frame's last kernel).
 * While on, the context renders frames ONE AT A TIME: switching on ends frame pipelining (s360_set_frame_pipelining(ctx, 1) is
 * then refused with S360_ERR_STATE), a context with more than one frame slot is refused (and s360_set_frame_slots above 1 while
 * on), and a render call returns only when its frame is complete on the device, so that no later frame can overwrite a kept image
 * before it is fetched. While off nothing is allocated, nothing is launched and no byte of any output differs. The pixels of a
 * frame's equirect, cubemap, flows and state images do not depend on the switch. Waits for the context's streams. */
int s360_set_debug_images(s360_ctx* ctx, int on);

/* The images of the selected slot's latest frame, in this fixed order; only those the reference writes for the context's flags and
 * whose buffers this context holds appear (no top_* without enable_top, no _sharpened at sharpening 0, no pole-removal images
 * without enable_pole_removal):
 *   projections/crop_<camera id>.png          one per side camera, rig order        B,G,R,A   TRSP:177-184
 *   sphericalImgL.png, sphericalImgR.png      the side panoramas before padding     B,G,R,A   TRSP:797-798
 *   sphericalImg_offsetwrapL.png, ...R.png    offsetHorizontalWrap(pano, cols / 3)  B,G,R,A   TRSP:795-800
 *   _topSpherical.png                         (enable_top)                          B,G,R,A   TRSP:680-684
 *   bottomImage.png, bottomImage2.png, bottomWarp2.png, _bottomCombined.png   (enable_pole_removal)   B,G,R,A   PoleRemoval.cpp:148-187
 *   _bottomSpherical.png                      (enable_bottom)                       B,G,R,A   TRSP:639-643
 *   croppedSideSpherical_<eye>.png, warpedSpherical_<eye>.png, extendedSideSpherical_<eye>.png
 *                                             per enabled pole unit: top_left, top_right, bottom_left, bottom_right   B,G,R,A   TRSP:548-560
 *   eqr_sideL.png, eqr_sideR.png              the eyes after the pole composite     B,G,R     TRSP:896-899
 *   _eqr_sideL_sharpened.png, ...R...         (sharpening > 0)                      B,G,R     TRSP:908-911
 * `name` is the reference's path relative to <output_data_dir>/debug/<frame>/. s360_frame_debug_image_count returns the number of
 * images, or an error code (< 0): S360_ERR_STATE when no frame has been rendered with the switch on. */
int s360_frame_debug_image_count(s360_ctx* ctx);
int s360_frame_debug_image_info(s360_ctx* ctx, int i, char name[96], int whc[3]);
/* Image i as raw pixels, whc[0] x whc[1] x whc[2] bytes, rows contiguous: for tests and for callers that encode themselves. */
int s360_frame_get_debug_image(s360_ctx* ctx, int i, uint8_t* dst);

/* All images of the list as finished PNG files, encoded where they lie: the two-phase contract of s360_frame_encode_state_pngs /
 * s360_frame_state_png_bound / s360_frame_download_state_png (s360_state_png.h), on a batch of its own. The encode is ONE launch
 * sequence over all images of the frame, 3- and 4-channel ones mixed, and returns without waiting; file i of the last encode call
 * is fetched with s360_frame_download_debug_png (cap >= s360_frame_debug_png_bound(ctx, i); a smaller buffer is refused with
 * S360_ERR_INVALID_ARG, not overrun; S360_ERR_STATE before any encode, _bound answers 0 then). Nothing travels to the host but
 * the files. The files have the banded layout of s360_encode_png_c. */
int s360_frame_encode_debug_pngs(s360_ctx* ctx);
size_t s360_frame_debug_png_bound(s360_ctx* ctx, int i);
int s360_frame_download_debug_png(s360_ctx* ctx, int i, uint8_t* out, size_t cap, size_t* n_out);

/* combineBottomImagesWithPoleRemoval (SR/render/PoleRemoval.cpp:32-188) without previous-frame state, as TestPoleRemoval calls it:
 * the two bottom cameras' images merged through the flow between them, with the masked pole cut out. bottom, bottom2, mask, mask2:
 * B,G,R images of w x h (a mask pixel counts as pole where it is red, CvUtil.cpp cutRedMaskOutOfAlphaChannel); radius, radius2:
 * the usable-pixel radii of the two cameras (s360_camera_usable_pixels_radius); flip180: the secondary image is rotated by 180
 * degrees (the up vectors of the two cameras point apart); feather_size: odd, 1 .. 31 (alpha_feather_size); flow_alg: a PixFlow
 * name. Outputs (each may be NULL): the four B,G,R,A images the reference writes as bottomImage.png, bottomImage2.png,
 * bottomWarp2.png and _bottomCombined.png, and the flow (w x h x 2 floats). Built from the kernels the frame runs with
 * enable_pole_removal. Synchronous; works on any context, also one whose flags describe no renderable frame. */
int s360_pole_removal_combine(s360_ctx* ctx, const uint8_t* bottom, const uint8_t* bottom2, const uint8_t* mask, const uint8_t* mask2,
                              int w, int h, float radius, float radius2, int flip180, int feather_size, const char* flow_alg,
                              uint8_t* bottom_image, uint8_t* bottom_image2, uint8_t* bottom_warp2, uint8_t* bottom_combined,
                              float* flow);

#ifdef __cplusplus
}
#endif
#endif /* S360_DEBUG_IMAGES_H_ */
