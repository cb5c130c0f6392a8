/* s360_debug_input_jpeg.h — test tap of the device JPEG decoder (include/s360_input_jpeg.h); not part of the API. It places a pixel
 * mismatch in the entropy stage (unstuffing, synchronisation, coefficients, DC) or in the pixel stage (IDCT, upsampling, colour). */
#ifndef S360_DEBUG_INPUT_JPEG_H_
#define S360_DEBUG_INPUT_JPEG_H_
#include "s360_input_jpeg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Decodes one file (as s360_decode_input_jpeg_batch takes it) and copies out what the entropy stage left behind. With n = blocks per
 * MCU x MCUs (6, 4 or 3 blocks for 4:2:0, 4:2:2, 4:4:4; MCUs of 16 x 16, 16 x 8 or 8 x 8 pixels): coef_out (cap_blocks >= n) receives
 * n x 64 quantised coefficients, the blocks in emission order (the Y blocks of an MCU, then Cb, Cr; dummy blocks included), natural
 * order inside a block, the DC as a value, not as a difference. *n_out = n. */
int s360_debug_input_jpeg_blocks(s360_ctx* ctx, const uint8_t* file, size_t bytes, int16_t* coef_out, size_t cap_blocks, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* S360_DEBUG_INPUT_JPEG_H_ */
