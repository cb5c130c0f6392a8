/* s360_frame_jpeg.h — a finished frame's equirect and cubemap as baseline JPEG FILES, encoded on the device. Included from s360.h.
 *
 * Replaces imwriteExceptionOnFail (TRSP:938-961, 917-935) for an --output_equirect_path / --output_cubemap_path that ends in
 * .jpg, .jpeg or .jpe: cv::imwrite chooses its codec by the extension, and its JpegEncoder at OpenCV's defaults (quality 95,
 * 4:2:0) writes the file host/jpeg_io.hpp's jpegio::encode writes. The entry points mirror the PNG ones of s360.h and
 * s360_cubemap.h one for one; the encoder is the one of s360_jpeg.h (surround360_amd/csrc/jpeg.hip).
 *
 * The specification: the file is jpegio::encode(pixels, w, h, quality) of the pixels that s360_frame_download_equirect_of /
 * s360_frame_download_cubemap return for that frame, byte for byte — header, scan, EOI.
 *
 * s360_set_jpeg_encode(ctx, on, quality): frames enqueued after it are also encoded as JPEG behind the final stage, on the
 * stream that renders it. quality 1..100, clamped as s360_jpeg_create clamps it; it is kept with each frame, so a later change
 * never mixes tables. Independent of s360_set_png_encode: both may be on, neither changes the other's bytes. While it has never
 * been on, nothing is allocated and nothing is launched. One encoder serves all frame slots of a context; its scratch is the
 * format's worst case for the larger of the equirect and the cubemap (2.1 KB per MCU of 16 x 16 pixels: 0.56 GB for 8192 x 8192).
 *
 * Capacity. Each slot keeps, per output buffer (two with s360_set_frame_pipelining or s360_set_output_double_buffer), a scan
 * buffer of 768 bytes per MCU — the size of the MCU's own B,G,R pixels, 201 MB for 8192 x 8192 — not the format's worst case of
 * 2490 (which would be 650 MB each). s360_frame_jpeg_bound(ctx) / s360_frame_cubemap_jpeg_bound(ctx) are exactly 623 + that
 * capacity + 2: a host buffer of the bound holds every file a fetch can return. Measured with the host writer: uniform
 * white noise takes 300 bytes per MCU at quality 95 and 506 at 100, full-amplitude binary noise 364 and 588; an 8K frame of the
 * measurement's synthetic footage at quality 95 takes 23. Only an image constructed for it — every coefficient of every block in the
 * highest size categories at a quality near 100 — comes near the 768. A frame whose scan needs more leaves NO file: nothing of the
 * scan is stored, and the fetch fails with S360_ERR_STATE, a message that names the size the scan needed, and *n_out = the size the
 * file would have had. Its pixels remain available through s360_frame_download_equirect_of.
 *
 * s360_frame_download_jpeg(ctx, age, out, cap, n_out) and its _slot / cubemap forms: age 0 / 1, slot and threading contract
 * exactly as s360_frame_download_png[_slot] (one fetching thread per context; the context is released while the fetch waits for
 * the frame; once the fetch of frame k has been called, frame k+2 waits on the device for k's transfer — the event that makes it
 * wait is recorded before the context is first released). A frame rendered without the switch: S360_ERR_STATE. cap smaller than
 * the file: S360_ERR_INVALID_ARG with *n_out = the size needed and nothing written (the rule of s360_jpeg_encode); a cap below
 * the bound makes the call wait for the frame with the context held, because only the finished frame tells the file's size.
 * With cap >= the bound and a frame that is still rendering, the whole scan buffer is transferred instead of the scan alone;
 * page-locked memory (s360_host_alloc) makes the copy a direct transfer. A timed-out banded sweep fails the fetch of its frame
 * as it fails s360_frame_download_png. */
#ifndef S360_FRAME_JPEG_H_
#define S360_FRAME_JPEG_H_
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

int s360_set_jpeg_encode(s360_ctx* ctx, int on, int quality);
size_t s360_frame_jpeg_bound(s360_ctx* ctx);
size_t s360_frame_cubemap_jpeg_bound(s360_ctx* ctx); /* 0 without s360_set_cubemap_output */
int s360_frame_download_jpeg(s360_ctx* ctx, int age, uint8_t* out, size_t cap, size_t* n_out);
int s360_frame_download_jpeg_slot(s360_ctx* ctx, int slot, int age, uint8_t* out, size_t cap, size_t* n_out);
int s360_frame_download_cubemap_jpeg(s360_ctx* ctx, int age, uint8_t* out, size_t cap, size_t* n_out);
int s360_frame_download_cubemap_jpeg_slot(s360_ctx* ctx, int slot, int age, uint8_t* out, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* S360_FRAME_JPEG_H_ */
