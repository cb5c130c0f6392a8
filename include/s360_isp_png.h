/*
 * s360_isp_png.h — 16-bit PNG files encoded on the device, and the ISP's result leaving as a finished PNG file (extension of the
 * C ABI of s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. They are kept in a header of their
 * own because they are one optional path: the unpack step (host/Unpacker, host/Raw2Rgb) writes every camera image as a PNG — 16-bit
 * B,G,R by default — and without these calls downloads the ISP's pixels and deflates them on host threads.
 */
#ifndef S360_ISP_PNG_H_
#define S360_ISP_PNG_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Operator form of the encoder for 16-bit images. `bgr16`: h x w x 3 little-endian uint16, B,G,R interleaved (host) — what
 * s360_isp_process returns with output_bpp 16. The file is a 16-bit RGB PNG (IHDR depth 16, colour type 2): samples in R,G,B order,
 * high byte first, the Sub filter at a distance of 6 bytes on every scanline, in the banded layout of s360_encode_png (chunk
 * "sbNd", one IDAT chunk and one Huffman block per band). Any PNG reader decodes it; host/png_io.hpp reads it on its sequential
 * path. cap >= s360_png_bound_16(w, h); a smaller buffer is refused with S360_ERR_INVALID_ARG before anything runs, not overrun.
 * s360_png_bound_16 answers 0 for a size the encoder does not take. Synchronous; works on any context, also one whose flags
 * describe no renderable frame. */
size_t s360_png_bound_16(int w, int h);
int s360_encode_png16(s360_ctx* ctx, const uint16_t* bgr16, int w, int h, uint8_t* out, size_t cap, size_t* n_out);

/* The bound of the file s360_isp_process_png / _packed_png write for an INPUT of w x h through this object: it follows the object's
 * `resize` (the image is (w / resize) x (h / resize)) and `output_bpp` (16: as s360_png_bound_16; 8: as s360_png_bound). 0 for a
 * null object or a size the encoder does not take. */
size_t s360_isp_png_bound(const s360_isp* isp, int w, int h);
/* What s360_isp_process / s360_isp_process_packed run, then the encoder on the object's own stream over the result where it lies on
 * the device: the pixels are never copied to the host. output_bpp 16 gives the 16-bit file of s360_encode_png16, output_bpp 8 the
 * 8-bit file of s360_encode_png — byte for byte the file those calls write for the pixels s360_isp_process* returns.
 * `out` receives n_out bytes; cap >= s360_isp_png_bound(isp, w, h), a smaller buffer is refused with S360_ERR_INVALID_ARG before
 * anything runs. The upload, the ISP's kernels, the encoder's kernels and the copy of the band table are enqueued before the first
 * wait; the second wait is for the file's bytes, whose count the band table gives. The chunk CRCs and the file's frame are host work
 * on `out`. The encoder's scratch, band table and file image belong to the object, are allocated on first use and grow only;
 * nothing of the object is touched from another thread, so one object serves one thread at a time (host/Unpacker: one per camera
 * thread). An object that feeds a context (s360_frame_upload_raw) refuses these calls as it refuses s360_isp_process. */
int s360_isp_process_png(s360_isp* isp, const uint16_t* raw16, int w, int h, uint8_t* out, size_t cap, size_t* n_out);
int s360_isp_process_packed_png(s360_isp* isp, const uint8_t* frame, int bits, int w, int h, uint8_t* out, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* S360_ISP_PNG_H_ */
