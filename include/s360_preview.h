/* s360_preview.h — pole-camera previews straight from a capture's packed frames: the per-frame work of the reference's
 * TestHyperPreview (SR/test/TestHyperPreview.cpp; scripts/preview.py drives it) on the device. The top camera and the two
 * bottom cameras of a rig are demosaiced crudely at half resolution (simpleDemosaic, :163-184), faded (topDownAlphaFade for
 * the bottom layers, radialAlphaFade for all three: SR/util/CvUtil.cpp:312-334), projected to an equirect with a float bicubic
 * remap through maps built once (precomputeProjectionWarp, :117-129; projectEquirectToCam, SR/render/ImageWarper.cpp:179-196) and
 * blended by flattenLayersAlphaSoftmax (CvUtil.cpp:336-360); the result, scaled by 255 / 65535 and converted like imwrite converts
 * a float image (saturate_cast<uchar>), is the B,G,R image the reference hands to its JPEG encoder.
 *
 * Independent of s360_ctx. Errors as everywhere in include/s360.h: a negative code, the message in s360_last_error(NULL).
 * One object serves one host thread at a time. */
#ifndef S360_PREVIEW_H_
#define S360_PREVIEW_H_
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct s360_preview s360_preview;

/* PreviewRenderer() (TestHyperPreview.cpp:83-96). cams: the whole rig; the three cameras are chosen by s360_rig_find_top,
 * s360_rig_find_bottom and s360_rig_find_bottom2, each rescaled by 0.5 as Camera::createRescaledCamera does (Camera.cpp:273-289)
 * and the three warp maps (eqr_w x eqr_h) built on the device. raw_w x raw_h: the size of a camera's raw image (the layers are
 * raw_w / 2 x raw_h / 2). gamma, softmax_coef: the flags of those names (1.0, 30.0). The three raw images start as zeros
 * (initRaws, :98-103). */
int s360_preview_create(s360_preview** out, const s360_camera* cams, int n_cams, int device, int raw_w, int raw_h, int eqr_w,
                        int eqr_h, double gamma, double softmax_coef);
void s360_preview_destroy(s360_preview* p);
/* Indices into `cams` of the top, bottom and secondary bottom camera the object chose. */
int s360_preview_cameras(const s360_preview* p, int idx_out[3]);

/* addTopImage / addBottomImage / addBottomImage2 + render (:105-161) of one frame. top, bottom, bottom2: the cameras' packed
 * frames as a .bin container holds them (bits 8: raw_w * raw_h bytes; 12: 3 * raw_w / 2 bytes per row, even raw_w; widened to 16
 * bits by replication as s360_isp_process_packed does). A NULL pointer keeps that layer's previous raw image. out_bgr: eqr_h x
 * eqr_w x 3 bytes, B,G,R. */
int s360_preview_render_packed(s360_preview* p, const uint8_t* top, const uint8_t* bottom, const uint8_t* bottom2, int bits,
                               uint8_t* out_bgr);
/* The same in two halves, for a host that overlaps its stages. submit enqueues uploads and kernels and returns; with frame
 * buffers from s360_host_alloc nothing in it waits, and the buffers must stay untouched until the matching fetch has returned.
 * fetch copies the OLDEST submitted frame that was not fetched yet into out_bgr (page-locked memory makes it one direct
 * transfer, on a stream of its own) and waits for it. Up to two frames may be submitted and unfetched: frame k + 1 is then
 * uploaded and rendered while frame k travels to the host. A third submit, and a fetch with nothing submitted: S360_ERR_STATE. */
int s360_preview_submit_packed(s360_preview* p, const uint8_t* top, const uint8_t* bottom, const uint8_t* bottom2, int bits);
int s360_preview_fetch(s360_preview* p, uint8_t* out_bgr);
/* Device time of the two kernels of the last submitted frame, in ms (hipEvents on the object's stream; waits for that frame). */
int s360_preview_last_times(s360_preview* p, float* develop_ms, float* compose_ms);

/* The frame as a .jpg file made on the device (include/s360_jpeg.h: the file jpegio::encode / cv::imwrite writes from the same
 * pixels, byte for byte). on != 0: frames SUBMITTED from now on are also encoded behind the compose kernel, on the same stream,
 * into a buffer of their slot; quality as libjpeg's, clamped to 1..100 (the reference's files: 95). Changing the quality waits
 * for the frames in flight; frames already submitted keep the quality they were submitted with, header and scan. on == 0: frames submitted from now on are not encoded. An equirect beyond the encoder's limits:
 * S360_ERR_INVALID_ARG. s360_preview_fetch keeps working on encoded frames (it takes the pixels). */
int s360_preview_set_jpeg(s360_preview* p, int on, int quality);
/* A size no .jpg of the object's equirect exceeds: the buffer s360_preview_fetch_jpeg wants (0 beyond the encoder's limits). */
size_t s360_preview_jpeg_bound(const s360_preview* p);
/* As s360_preview_fetch, but takes the OLDEST unfetched frame as its file: the byte count travels first, then exactly that many
 * bytes (out in page-locked memory makes that one direct transfer). *n_out: the file's size. S360_ERR_STATE when that frame was
 * submitted with the encoder off — it stays queued for s360_preview_fetch; S360_ERR_INVALID_ARG when cap is smaller than the file
 * (*n_out = the size needed; the frame stays queued). */
int s360_preview_fetch_jpeg(s360_preview* p, uint8_t* out, size_t cap, size_t* n_out);
/* Device time of the encoder's kernels for the last frame submitted with the encoder on, in ms (waits for that frame). */
int s360_preview_last_jpeg_time(s360_preview* p, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* S360_PREVIEW_H_ */
