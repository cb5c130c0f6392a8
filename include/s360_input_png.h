/*
 * s360_input_png.h — a frame's camera images handed in as banded PNG files, 8- or 16-bit, and decoded on the device (extension of
 * the C ABI of s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. They are one optional path, the read
 * side of s360_isp_png.h: the 17 camera images a frame starts from, as Unpacker --device_png and Raw2Rgb --device_png write them
 * (16-bit by default), are not inflated on host threads and uploaded as pixels; the files' bytes go to the device as they are and
 * the pixels are written straight into the frame's source slots.
 *
 * The files are those of s360_png_decode.h (chunk "sbNd", one IDAT per band, each a complete raw-deflate segment; scanline
 * filters 0 and 1) with one more format: 16 bits per sample with colour type 2 — 6 bytes per pixel, R,G,B with the high byte first,
 * Sub at a distance of 6 bytes. What s360_png_decodable, s360_decode_png_batch and s360_frame_set_prev_images_png accept is
 * unchanged: they keep refusing 16-bit files.
 */
#ifndef S360_INPUT_PNG_H_
#define S360_INPUT_PNG_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device needed. 0: the n bytes at `file` are a file these entry points take: what s360_png_decodable takes, or the
 * same container with depth 16 and colour type 2; info = {width, height, channels (3 or 4), bits per sample (8 or 16), rows per
 * band}. Otherwise S360_ERR_INVALID_ARG with the message "not a banded PNG file of this decoder" and nothing is touched. */
int s360_input_png_decodable(const uint8_t* file, size_t n, int info[5]);

/* Operator form: n files in host memory in, n host images out, through ONE launch sequence over all bands of all files. 8-bit files
 * give w x h x channels bytes, B,G,R(,A). 16-bit files give w x h x 3 little-endian uint16 samples, B,G,R, if keep16 is not 0 (out[i]
 * 2-byte aligned), else w x h x 3 bytes: every sample's high byte, what png_set_strip_16 and an 8-bit imread make of such a file.
 * cap_bytes[i] smaller than that is refused, not overrun. info_out (5 n ints, may be NULL) receives every file's info as
 * s360_input_png_decodable gives it. Refusals and failures as s360_decode_png_batch reports them: a file that is not decodable, or
 * whose bands fail, makes the call fail with S360_ERR_INVALID_ARG and "image <i>" in s360_last_error; nothing is written to any
 * out[] in the first case. s360_png_decode_stats, _round_histogram and _failure report on this call too: it is a decode call on
 * this context. Synchronous; works on any context, also one whose flags describe no renderable frame. */
int s360_decode_input_png_batch(s360_ctx* ctx, int n, const uint8_t* const* files, const size_t* bytes, void* const* out,
                                const size_t* cap_bytes, int keep16, int* info_out);

/* n camera images of the selected slot's frame from their files: cameras[i] is a side index, S360_CAMERA_TOP,
 * S360_CAMERA_BOTTOM or, on a context with enable_pole_removal, S360_CAMERA_BOTTOM2 (s360_pole_inputs.h; every camera at most once), files[i] / bytes[i] its file. Every file must be decodable with colour type 2,
 * depth 8 or 16 (a 16-bit file gives its high bytes, as s360_frame_upload_raw does). The side images of a call must all have the
 * same size, and the size of the side images handed in before (the rule of s360_frame_upload_side). The files' bytes are copied
 * and decoded on the context's upload stream by one inflate launch and one unfilter launch that writes the source slots directly —
 * a side slot with the alpha ramp s360_frame_upload_side gives a 3-channel image, a pole slot with alpha 255 — behind the frame
 * before's last reads of those slots.
 * SYNCHRONOUS, unlike the pixel uploads: the call holds the context until every band's status and every file's Adler-32 are
 * known (the locking of s360_frame_set_prev_images_png), so files[] may be reused as soon as it returns. On success the images
 * count as uploaded exactly as after s360_frame_upload_side / _top / _bottom. On failure (S360_ERR_INVALID_ARG, "image <i>" in
 * the message, s360_png_decode_failure says which and why) NOTHING is marked as uploaded, and what the slots of this call's
 * cameras hold is unspecified until they are uploaded again. Pole removal's masks come through s360_set_pole_masks or
 * s360_frame_upload_pole_removal. */
int s360_frame_upload_png(s360_ctx* ctx, int n, const int* cameras, const uint8_t* const* files, const size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* S360_INPUT_PNG_H_ */
