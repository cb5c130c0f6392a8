// api_internal.hpp — the few helpers that the files of the C ABI share (api.hip, api_ops.hip, api_png.hip, api_taps.hip,
// api_isp.hip), besides the guard (api_guard.hpp).
#pragma once
#include <mutex>
#include <string>
#include <vector>

#include "api_guard.hpp"
#include "ctx.hpp"
#include "render.hpp"

namespace s360 {

// api.hip: throws S360_ERR_HIP when a banded sweep of one of the context's flow engines timed out (and resets their error words).
// `frame_words` (a fetch of a finished frame): the three sweep error words that frame snapshotted in front of its outDone event
// (render.hpp); only a non-zero snapshot looks at the engines.
void check_sweep_error(s360_ctx* c, const unsigned* frame_words = nullptr);
// api.hip: where the named 8-bit intermediate of a slot's latest frame lies on the device (the names of s360_frame_get_u8)
const void* frame_u8_source(s360_ctx* c, FrameState& F, const std::string& n, int idx, bool pack_eye, int& w, int& h, int& ch);
// api.hip: previous state handed in for one pair: its place j in the block the state is laid out for (render.hpp PrevLayout) ...
PrevLayout prev_side_block(s360_ctx* c, FrameState& F, int pair, int& j);
// ... and the book-keeping of state that arrives in halves (s360_frame_set_prev_images_png / s360_frame_set_prev_flow)
void prev_side_arrived(FrameState& F, int pair, unsigned bits);
void prev_pole_arrived(s360_ctx* c, FrameState& F, int unit, unsigned bits);
void prev_pr_arrived(FrameState& F, unsigned bits);
// api_png.hip: host threads for a PNG file's CRCs (developer switch S360_PNG_CRC_THREADS)
int png_crc_threads();
// api_png.hip: what the fetches of a finished frame share. A refused slot number; the state of frame slot `slot` (-1: the selected
// one); the download stream with its event and the error words' landing area; the output buffer that holds the frame `age` frames
// back, and that frame's cubemap
constexpr int kNoSlot = -2;
FrameState& slot_state(s360_ctx* c, int slot);
void ensure_download_stream(s360_ctx* c);
int frame_buffer(s360_ctx* c, FrameState& F, int age);
int cube_buffer(s360_ctx* c, FrameState& F, int age);

// api_png.hip: a batch of PNG files encoded by one launch sequence (ctx.hpp PngBatch): its plan and page-locked areas; its launch
// sequence over the device images px[i] on the context's stream, the band tables' copy behind it (nothing waits); file i of the
// batch into the caller's buffer (`release`: the context is given back while the call waits and while it computes the CRCs)
void png_batch_prepare(s360_ctx* c, s360_ctx::PngBatch& B, const std::vector<PngPlan>& plans);
void png_batch_run(s360_ctx* c, s360_ctx::PngBatch& B, const uint8_t* const* px);
void png_batch_fetch(s360_ctx* c, std::unique_lock<std::recursive_mutex>& lk, s360_ctx::PngBatch& B, int i, uint8_t* out, size_t cap,
                     size_t* n_out, bool release);

inline void h2d(s360_ctx* c, void* d, const void* h, size_t n) {
  S360_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->st));
}
// Frame pipelining: frame_finish runs on st2. Anything enqueued on st that READS what frame_finish writes (panoramas,
// warped poles, extended pole images, the stacked equirect) must be ordered after it: the host waits for st2 first.
inline void wait_finish_stream(s360_ctx* c) {
  if (c->st2) S360_HIP(hipStreamSynchronize(c->st2));
}
inline void d2h(s360_ctx* c, void* h, const void* d, size_t n) {
  if (c->st2) S360_HIP(hipStreamSynchronize(c->st2));  // frame pipelining: the data may come from the finish stream
  S360_HIP(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->st));
  S360_HIP(hipStreamSynchronize(c->st));
  check_sweep_error(c);
}

}  // namespace s360
