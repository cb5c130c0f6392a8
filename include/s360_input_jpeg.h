/*
 * s360_input_jpeg.h — a frame's camera images handed in as baseline JPEG files and decoded on the device (extension of the C ABI of
 * s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. They are one optional path beside
 * s360_input_png.h: camera images that are .jpg files — what the reference's imgs_dir may hold, and the only camera file from
 * outside this project the device can take — are not decoded on host threads and uploaded as pixels; the files' bytes go to the
 * device as they are and the pixels are written straight into the frame's source slots. The pixels are those of libjpeg at its
 * defaults (islow IDCT, fancy upsampling, 16-bit colour tables), i.e. of cv::imread and of PIL, byte for byte.
 *
 * A file is decodable here when it is SOF0 (baseline), 8-bit, three components coded as Y, Cb, Cr with luma sampling 2x2, 2x1 or 1x1
 * and chroma 1x1 (4:2:0, 4:2:2, 4:4:4), one interleaved scan (Ss 0, Se 63, Ah = Al = 0), 8-bit quantisation tables, any Huffman
 * tables, no restart interval, EXIF orientation absent or 1, not Adobe transform 0, and its scan is shorter than 2^32 bits.
 * Everything else (greyscale, progressive, restart markers, ...) is "not decodable": the host decoder's business.
 */
#ifndef S360_INPUT_JPEG_H_
#define S360_INPUT_JPEG_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device needed. 0: the n bytes at `file` are a file these entry points take; info = {width, height, 3, luma
 * horizontal sampling, luma vertical sampling, bytes of the entropy-coded segment}. Otherwise S360_ERR_INVALID_ARG with the message
 * "not a JPEG file of this decoder" and nothing is touched. */
int s360_input_jpeg_decodable(const uint8_t* file, size_t n, int info[6]);

/* Operator form: n files in host memory in, n host images out (w x h x 3 bytes, B,G,R), through ONE launch sequence over all files.
 * cap_bytes[i] smaller than that is refused, not overrun. info_out (6 n ints, may be NULL) receives every file's info as
 * s360_input_jpeg_decodable gives it. A file that is not decodable, or damaged (the reasons below), makes the call fail with
 * S360_ERR_INVALID_ARG and "image <i>" in s360_last_error; nothing is written to any out[] in the first case.
 * Synchronous; works on any context, also one whose flags describe no renderable frame. */
int s360_decode_input_jpeg_batch(s360_ctx* ctx, int n, const uint8_t* const* files, const size_t* bytes, void* const* out,
                                 const size_t* cap_bytes, int* info_out);

/* n camera images of the selected slot's frame from their files — the contract of s360_frame_upload_png: cameras[i] is a side
 * index, S360_CAMERA_TOP, S360_CAMERA_BOTTOM or (enable_pole_removal) S360_CAMERA_BOTTOM2 (every camera at most once), files[i] / bytes[i] its file, which must be decodable.
 * The side images of a call must all have the same size, and the size of the side images handed in before (the rule of
 * s360_frame_upload_side). The files' scans are copied and decoded on the context's upload stream; the last kernel writes the
 * source slots directly — a side slot with the alpha ramp s360_frame_upload_side gives a 3-channel image, a pole slot with alpha
 * 255 — behind the frame before's last reads of those slots.
 * SYNCHRONOUS, unlike the pixel uploads: the call holds the context until every file's status is known, so files[] may be reused as
 * soon as it returns. On success the images count as uploaded exactly as after s360_frame_upload_side / _top / _bottom. On failure
 * (S360_ERR_INVALID_ARG, "image <i>" in the message, s360_jpeg_decode_failure says which and why) NOTHING is marked as uploaded, and
 * what the slots of this call's cameras hold is unspecified until they are uploaded again. Pole removal's masks come through
 * s360_set_pole_masks or s360_frame_upload_pole_removal. */
int s360_frame_upload_jpeg(s360_ctx* ctx, int n, const int* cameras, const uint8_t* const* files, const size_t* bytes);

/* The last decode call on this context (either entry point above): counts = {files, subsequences (of 4096 scan bits), synchronisation
 * launches, the most decode passes any file needed}; ms = {device time of the entropy stage: unstuffing, synchronisation with the
 * host's round trips between its launches, coefficients, DC; device time of the pixel stage: IDCT, upsampling, colour, store};
 * file_rounds (may be NULL; cap entries) receives per file the most decode passes one of its workgroups made (1: every guessed
 * start was right or nothing depended on it). */
int s360_jpeg_decode_stats(s360_ctx* ctx, uint64_t counts[4], double ms[2], uint32_t* file_rounds, int cap);

/* Why the last decode call on this context failed: *image = index of the file in that call (-1: it did not fail because of a file),
 * *reason = one of the values below. A call that succeeded leaves S360_JPEG_DECODE_FAILURE_NONE. */
#define S360_JPEG_DECODE_FAILURE_NONE 0
#define S360_JPEG_DECODE_FAILURE_NOT_DECODABLE 1 /* not a JPEG file of this decoder */
#define S360_JPEG_DECODE_FAILURE_MISMATCH 2      /* size not what the destination takes, or the output buffer too small */
#define S360_JPEG_DECODE_FAILURE_BAD_CODE 3      /* an invalid Huffman code */
#define S360_JPEG_DECODE_FAILURE_BAD_RUN 4       /* a run past coefficient 63 */
#define S360_JPEG_DECODE_FAILURE_SHORT 5         /* the scan ends inside a block */
#define S360_JPEG_DECODE_FAILURE_BLOCKS 6        /* blocks missing at the end */
#define S360_JPEG_DECODE_FAILURE_LEFT_OVER 7     /* bits left over beyond the padding */
#define S360_JPEG_DECODE_FAILURE_MARKER 8        /* a marker inside the scan */
int s360_jpeg_decode_failure(s360_ctx* ctx, int* image, int* reason);

#ifdef __cplusplus
}
#endif
#endif /* S360_INPUT_JPEG_H_ */
