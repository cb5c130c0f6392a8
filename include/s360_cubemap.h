/*
 * s360_cubemap.h — the stereo cubemap as an output of every frame (extension of the C ABI of s360.h, libs360.so).
 *
 * s360.h includes this header: a program that includes s360.h has these entry points too. They are kept in a header of
 * their own because they are one optional output with its own switch, size query and fetch calls, mirroring the equirect's.
 */
#ifndef S360_CUBEMAP_H_
#define S360_CUBEMAP_H_

#include "s360.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cubemap of s360_frame_cubemap as an output of EVERY frame, for the hosts that stream or batch (the reference's per-frame caller asks for one
 * beside every equirect: scripts/batch_process_video.py:40-47, --cubemap_format video). After s360_set_cubemap_output(ctx, fw, fh,
 * "video" | "photo") the finish stage of every frame rendered from then on — s360_frame_render / _finish / _composite, every slot of
 * s360_frame_render_batch / _slots — also renders its stereo cubemap from the sharpened eyes (TRSP:901-935), all slots of a batch in one
 * launch, into a per-slot buffer that alternates with the equirect's: the age 0 / age 1 contract of
 * s360_frame_download_equirect_of, s360_set_output_double_buffer and s360_set_frame_pipelining holds for it unchanged, and the
 * fetches below behave like s360_frame_download_equirect_slot / s360_frame_download_png_slot (own stream, wait for that frame only,
 * context released while waiting). face_width or face_height 0 turns the output off; any other format is S360_ERR_INVALID_ARG. The
 * size or format may change between frames: s360_frame_cubemap_size / _png_bound answer for the CURRENT setting (S360_ERR_STATE /
 * 0 while off), each stored frame keeps the size it was rendered with. The face maps and their prepared form are built by this call
 * (a host wait; once per size and format and context, shared by all slots). Fetching a frame that was rendered with the output off
 * — or its PNG with s360_set_png_encode off — is S360_ERR_STATE. On a sharded frame the output appears on the compositing rank.
 * Bytes equal s360_frame_cubemap's. */
int s360_set_cubemap_output(s360_ctx* ctx, int face_width, int face_height, const char* format);
int s360_frame_cubemap_size(s360_ctx* ctx, int whc[3]);
int s360_frame_download_cubemap(s360_ctx* ctx, int age, uint8_t* out_bgr);
int s360_frame_download_cubemap_slot(s360_ctx* ctx, int slot, int age, uint8_t* out_bgr);
size_t s360_frame_cubemap_png_bound(s360_ctx* ctx);
int s360_frame_download_cubemap_png(s360_ctx* ctx, int age, uint8_t* out, size_t cap, size_t* n_out);
int s360_frame_download_cubemap_png_slot(s360_ctx* ctx, int slot, int age, uint8_t* out, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* S360_CUBEMAP_H_ */
