/*
 * s360_pole_inputs.h — pole removal's inputs on the device input paths, and the pole masks as state of the context (extension of
 * the C ABI of s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. --enable_pole_removal
 * (combineBottomImagesWithPoleRemoval, SR/render/PoleRemoval.cpp:32-188) needs the secondary bottom camera's image for every frame
 * and the two red pole masks, which are properties of the rig. s360_frame_upload_pole_removal hands all three in as pixels with
 * every frame. Here the masks are handed in once (s360_set_pole_masks) and the secondary camera is a camera like the others:
 * S360_CAMERA_BOTTOM2 in s360_frame_upload_raw / _packed / _png / _jpeg, or its pixels through s360_frame_upload_bottom2.
 *
 * Every alpha plane pole removal computes is a function of the masks, the two cameras' usable radii, the image size and
 * std_alpha_feather_size alone (circleAlphaCut overwrites alpha from geometry, cutRedMaskOutOfAlphaChannel reads only the mask,
 * featherAlphaChannel reads only alpha: SR/util/CvUtil.cpp:140-157, 201-222). s360_set_pole_masks computes the three planes once;
 * a frame then costs one pass that writes both flow inputs and one pass that writes the merged image. The frames are byte for byte
 * those of s360_frame_upload_pole_removal.
 */
#ifndef S360_POLE_INPUTS_H_
#define S360_POLE_INPUTS_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The secondary bottom camera (s360_rig_find_bottom2) as `camera` of s360_frame_upload_raw / s360_frame_upload_packed and as
 * cameras[i] of s360_frame_upload_png / s360_frame_upload_jpeg — on a context created with enable_pole_removal only; every other
 * context refuses it as it refuses any index below S360_CAMERA_BOTTOM ("camera index out of range"). The image lands in the selected
 * slot's secondary bottom source, B,G,R,A with alpha 255 like the bottom camera's, behind the frame before's last reads of the pole
 * sources. It must have the bottom camera's size, whichever of the two arrives first (the rule of s360_frame_upload_pole_removal). */
#define S360_CAMERA_BOTTOM2 (-3)

/* The secondary bottom camera's image as host pixels (BGR, w x h), as s360_frame_upload_bottom hands in the bottom camera's. */
int s360_frame_upload_bottom2(s360_ctx* ctx, const uint8_t* bgr, int w, int h);

/* The red masks of both bottom cameras (BGR, w x h; pure red (0,0,255) = pole) as state of the context, shared by all its frame
 * slots. S360_ERR_STATE on a context without enable_pole_removal. Waits for the context's streams, computes the alpha planes, and
 * holds for every frame rendered after it returns. May be called again with other masks (the planes are rebuilt);
 * (NULL, NULL, 0, 0) clears the masks. While masks are resident
 *  - s360_frame_upload_pole_removal is refused with S360_ERR_STATE (the two ways are never mixed within a context),
 *  - a bottom or secondary bottom image of another size than the masks is refused with S360_ERR_INVALID_ARG,
 *  - a slot's pole-removal inputs are complete when it holds a secondary image of the masks' size, handed in through
 *    s360_frame_upload_bottom2 or as S360_CAMERA_BOTTOM2 — before or after the masks; like every source image it persists from
 *    frame to frame until it is replaced. A render of a slot that never got one fails as a render without
 *    s360_frame_upload_pole_removal does. */
int s360_set_pole_masks(s360_ctx* ctx, const uint8_t* mask_bgr, const uint8_t* mask2_bgr, int w, int h);

#ifdef __cplusplus
}
#endif
#endif /* S360_POLE_INPUTS_H_ */
