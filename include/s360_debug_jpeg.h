/* s360_debug_jpeg.h — test tap of the device JPEG encoder (include/s360_jpeg.h); not part of the API. It places a byte
 * mismatch in the block stage (colour conversion, downsampling, DCT, quantisation, dummy blocks) or in the bitstream stage. */
#ifndef S360_DEBUG_JPEG_H_
#define S360_DEBUG_JPEG_H_
#include "s360_jpeg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Encodes bgr (as s360_jpeg_encode takes it) and copies out what the kernels left behind. With n = 6 * ceil(w / 16) * ceil(h / 16)
 * blocks: coef_out receives n x 64 quantised coefficients, the blocks in emission order (Y00 Y01 Y10 Y11 Cb Cr per MCU, dummy
 * blocks included), natural order inside a block; bits_out receives n bit lengths, each block's Huffman codes and extra bits
 * before byte stuffing. */
int s360_debug_jpeg_blocks(s360_jpeg* e, const uint8_t* bgr, int w, int h, int16_t* coef_out, uint32_t* bits_out);

#ifdef __cplusplus
}
#endif
#endif /* S360_DEBUG_JPEG_H_ */
