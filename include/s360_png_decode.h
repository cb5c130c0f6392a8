/*
 * s360_png_decode.h — banded PNG files decoded on the device, and previous-frame state handed in as such files (extension of the
 * C ABI of s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. They are one optional path, the read
 * side of s360_state_png.h: a per-frame caller reads back the 36 B,G,R,A state images the frame before left on disk; instead of
 * inflating them on host threads and uploading 919 MB of pixels (8K), the files' 123 MB go to the device as they are.
 *
 * The decoder takes the files s360_encode_png* and host/png_io.hpp write: 8-bit, colour type 2 or 6, not interlaced, a private
 * chunk "sbNd" (rows per band), a first IDAT of the 2-byte zlib header, exactly ceil(h / band_rows) IDAT chunks each of which is a
 * complete byte-aligned raw-deflate segment of its band's scanlines, a last IDAT of the 4-byte Adler-32. Within that layout it is a
 * full inflate (stored, fixed and dynamic blocks, any number per band, any distance inside the band's own output); scanline
 * filters 0 (None) and 1 (Sub) are undone, any other filter type is reported as unsupported. Chunk CRCs are not checked (neither
 * does host/png_io.hpp); the Adler-32 of the scanlines is.
 */
#ifndef S360_PNG_DECODE_H_
#define S360_PNG_DECODE_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device needed. 0: the n bytes at `file` are a file this decoder takes; whc = {width, height, channels (3 or 4)} and
 * *band_rows are filled. Otherwise S360_ERR_INVALID_ARG with the message "not a banded PNG file of this decoder" and nothing is
 * touched — not an error of the file: such a file is read by a general PNG reader. */
int s360_png_decodable(const uint8_t* file, size_t n, int whc[3], int* band_rows);

/* Operator form: n files in host memory in, n host images out, through ONE launch sequence (one inflate launch over all bands of all
 * files, one unfilter launch). out[i] receives w x h x channels bytes: B,G,R for colour type 2, B,G,R,A for type 6; whc_out (3 n
 * ints, may be NULL) the sizes. cap[i] smaller than that is refused, not overrun. A file that is not decodable, or whose bands fail
 * (a band's status word, the Adler-32), makes the call fail with S360_ERR_INVALID_ARG and "image <i>" in s360_last_error; nothing is
 * written to any out[] in the first case. Synchronous; works on any context, also one whose flags describe no renderable frame. */
int s360_decode_png_batch(s360_ctx* ctx, int n, const uint8_t* const* files, const size_t* bytes, uint8_t* const* out, const size_t* cap,
                          int* whc_out);

/* The counters of the last decode call on this context (s360_decode_png_batch or s360_frame_set_prev_images_png): out[0] bands
 * decoded on the fast path (a wave per band, speculative parallel decode), out[1] on the general path (serial), out[2] bands of
 * stored blocks only, out[3] the largest number of speculation rounds any window of any band took: the rounds up to the last one in which a lane decoded
 * its span again, plus the one that found no start changed (2 = every lane was in step after one correction). */
int s360_png_decode_stats(s360_ctx* ctx, uint64_t out[4]);
/* ... and the histogram behind out[3]: hist[r] = fast-path bands whose slowest window took r rounds, r = 0..65 (66 entries). */
int s360_png_decode_round_histogram(s360_ctx* ctx, uint64_t hist[66]);

/* Why the last decode call on this context (s360_decode_png_batch or s360_frame_set_prev_images_png) failed, for a caller that
 * reacts to it rather than prints it: *image = index of the first failing file in that call (-1: none, or not about one file),
 * *reason = one of the values below. A call that succeeded leaves S360_PNG_DECODE_FAILURE_NONE. */
#define S360_PNG_DECODE_FAILURE_NONE 0
#define S360_PNG_DECODE_FAILURE_NOT_DECODABLE 1 /* not a banded PNG file of this decoder */
#define S360_PNG_DECODE_FAILURE_MISMATCH 2      /* size or channels not what the destination takes, or the output buffer too small */
#define S360_PNG_DECODE_FAILURE_DAMAGED 3       /* a band's status word, or the Adler-32 */
int s360_png_decode_failure(s360_ctx* ctx, int* image, int* reason);

/* Decodes n files straight into the selected slot's previous-state image buffers: no host pixels in between. names[i] / idx[i] as
 * s360_frame_encode_state_pngs takes them: overlap_l, overlap_r (idx = pair), extended_side, extended_fisheye (idx 0..3),
 * bottom_image, bottom_image2. Every file must be decodable, 4 channels, and of the size the context expects for that name.
 * Refused like s360_frame_set_prev_side: a pair outside the context's partition; bottom_image / bottom_image2 on a context without
 * pole removal. Synchronous: returns once every band's status and every Adler-32 are known; on failure nothing is marked as handed
 * in. A pair, pole unit or pole-removal state counts as handed in — s360_frame_render(ctx, 1) then uses it exactly as after
 * s360_frame_set_prev_side / _pole / _pole_removal — once its images (this call) and its flows (s360_frame_set_prev_flow) have both
 * arrived, in either order. Halves that have arrived and wait for the rest are forgotten when the stage they belong to is rendered
 * (side pairs, pole units, pole removal) and when the same pair / unit / pole removal is handed in through s360_frame_set_prev_side /
 * _pole / _pole_removal: a half never completes a set across a rendered frame. */
int s360_frame_set_prev_images_png(s360_ctx* ctx, int n, const char* const* names, const int* idx, const uint8_t* const* files,
                                   const size_t* bytes);

/* The flow half of s360_frame_set_prev_side / _pole / _pole_removal. Names of s360_frame_get_f32: flow_l_to_r, flow_r_to_l (idx =
 * pair), flow_pole (idx = unit 0..3), flow_bottom_secondary (idx ignored). The context knows the sizes; flow_bottom_secondary has
 * the size of the bottom images, which must be known by then: bottom_image / bottom_image2 handed in, or the bottom camera's image
 * uploaded (S360_ERR_STATE otherwise). */
int s360_frame_set_prev_flow(s360_ctx* ctx, const char* name, int idx, const float* flow);

#ifdef __cplusplus
}
#endif
#endif /* S360_PNG_DECODE_H_ */
