/*
 * s360_state_png.h — PNG files of B,G,R,A images and of many images at once, encoded on the device (extension of the C ABI of
 * s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. They are kept in a header of their
 * own because they are one optional path: the temporal state a per-frame caller leaves on disk for the next frame (36 B,G,R,A
 * images per 8K frame) as finished PNG files instead of raw pixels for host threads to deflate.
 */
#ifndef S360_STATE_PNG_H_
#define S360_STATE_PNG_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Operator form of the encoder behind s360_encode_png for 3 or 4 channels. channels = 3: `px` is B,G,R, the file 8-bit RGB, byte for
 * byte what s360_encode_png writes. channels = 4: `px` is B,G,R,A, the file 8-bit RGBA (colour type 6): bytes 0 and 2 of every pixel
 * swapped, alpha kept, Sub filter at a distance of 4 bytes. Any other channel count is S360_ERR_INVALID_ARG (s360_png_bound_c: 0).
 * The file has the banded layout of s360_encode_png (chunk "sbNd"), which host/png_io.hpp reads back band-parallel. cap >=
 * s360_png_bound_c(w, h, channels); a smaller buffer is refused, not overrun. Synchronous; works on any context, also one whose
 * flags describe no renderable frame. */
size_t s360_png_bound_c(int w, int h, int channels);
int s360_encode_png_c(s360_ctx* ctx, const uint8_t* px, int w, int h, int channels, uint8_t* out, size_t cap, size_t* n_out);

/* n host images of differing size and channel count in, n complete files out: out[i] (cap[i] >= s360_png_bound_c(w[i], h[i],
 * channels[i]) bytes) receives n_out[i] bytes, byte for byte the file s360_encode_png_c writes for image i alone. ONE launch sequence
 * on the device for all of them: one deflate launch over all bands of all images, one layout launch, one gather launch. Synchronous. */
int s360_encode_png_batch(s360_ctx* ctx, int n, const uint8_t* const* px, const int* w, const int* h, const int* channels,
                          uint8_t* const* out, const size_t* cap, size_t* n_out);

/* The same batch over device-resident intermediates of the selected slot's latest frame, in two phases.
 * s360_frame_encode_state_pngs enqueues the encode of n images named like s360_frame_get_u8 names them — overlap_l, overlap_r
 * (idx = pair), extended_side, extended_fisheye (idx 0..3), bottom_image, bottom_image2, or any other of its 4-channel names —
 * behind that frame's kernels and returns; it waits for nothing. Errors (S360_ERR_INVALID_ARG): an unknown name, a 3-channel
 * name, a name whose buffer this context does not hold (another rank's pair or pole unit, pole removal not run). A failed call
 * leaves the batch of the call before it fetchable.
 * s360_frame_state_png_bound(ctx, i) / s360_frame_download_state_png(ctx, i, out, cap, n_out) fetch file i of the LAST encode call
 * (S360_ERR_STATE before any; S360_ERR_INVALID_ARG for i out of range or cap too small — refused, not overrun; _bound answers 0).
 * Like the other *_download_* calls the fetch runs on a stream of its own and releases the context while it waits for the device
 * and while it computes the chunk CRCs and the file's frame on the caller's thread: different i may be fetched from different
 * host threads, they are served one after the other. An encode call that replaces the batch while a fetch of it waits makes that
 * fetch fail with S360_ERR_STATE; the new batch's kernels wait on the device for every fetch that was already enqueued.
 * The batch's file images, band tables and scratch are allocated on first use, grow only, and belong to the context. */
int s360_frame_encode_state_pngs(s360_ctx* ctx, int n, const char* const* names, const int* idx);
size_t s360_frame_state_png_bound(s360_ctx* ctx, int i);
int s360_frame_download_state_png(s360_ctx* ctx, int i, uint8_t* out, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* S360_STATE_PNG_H_ */
