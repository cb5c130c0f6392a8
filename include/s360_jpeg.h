/* s360_jpeg.h — baseline JPEG files encoded on the device: colour conversion, 4:2:0 downsampling, the integer DCT, quantisation,
 * Huffman coding and byte stuffing all run as kernels (surround360_amd/csrc/jpeg.hip); only the 623 header bytes in front of the
 * scan (SOI, APP0, DQT x 2, SOF0, DHT x 4, SOS) and the EOI marker behind it are written on the host. The file is the one
 * host/jpeg_io.hpp's jpegio::encode writes — what cv::imwrite writes through libjpeg — byte for byte: baseline sequential, one
 * interleaved scan, 2 x 2 luma sampling, the Annex K tables scaled by jpeg_quality_scaling with force_baseline.
 *
 * Independent of s360_ctx. Errors as everywhere in include/s360.h: a negative code, the message in s360_last_error(NULL).
 * One object serves one host thread at a time.
 *
 * Limits. Width and height 1..65535 each. Bit and byte offsets into the scan are 32-bit on the device, which holds for images of
 * up to 431 220 MCUs of 16 x 16 pixels (ceil(w / 16) * ceil(h / 16); every size up to 8192 x 8192 has at most 262 144); beyond
 * that: S360_ERR_INVALID_ARG. Device buffers are sized for the worst case of the format (1660 bits per 8 x 8 block, doubled by
 * byte stuffing: about 5 KB per MCU of max_w x max_h with the uploaded image), so no image can overflow them. */
#ifndef S360_JPEG_H_
#define S360_JPEG_H_
#include "s360.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct s360_jpeg s360_jpeg;

/* An encoder for images of up to max_w x max_h pixels (both the width and the height of every image must fit). quality: 1..100
 * as libjpeg's; values outside are clamped to that range, as jpegio::encode clamps them. */
int s360_jpeg_create(s360_jpeg** out, int device, int max_w, int max_h, int quality);
void s360_jpeg_destroy(s360_jpeg* e);
/* A size no file of w x h exceeds (0 for a size outside the limits above). */
size_t s360_jpeg_bound(int w, int h);
/* bgr: any 8-bit B,G,R image in host memory, h rows of w pixels, rows contiguous. out receives the complete file
 * jpegio::encode(bgr, w, h, quality) returns, byte for byte, *n_out its size; synchronous. cap smaller than the file:
 * S360_ERR_INVALID_ARG with *n_out = the size needed and nothing written. An image larger than max_w x max_h: S360_ERR_INVALID_ARG. */
int s360_jpeg_encode(s360_jpeg* e, const uint8_t* bgr, int w, int h, uint8_t* out, size_t cap, size_t* n_out);
/* Device time of the last encode's kernels in ms (hipEvents on the object's stream, the upload not included). */
int s360_jpeg_last_time(s360_jpeg* e, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* S360_JPEG_H_ */
