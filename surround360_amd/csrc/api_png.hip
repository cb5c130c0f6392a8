// api_png.hip — fetching what a finished frame left on the device, and the PNG family of the C ABI (include/s360.h,
// s360_cubemap.h, s360_state_png.h, s360_png_decode.h, s360_isp_png.h, s360_input_png.h): downloads by age and slot, frames / cubemaps / state images
// as PNG files encoded on the device (png.hip), banded PNG files decoded on the device (png_decode.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../../include/s360.h"
#include "api_internal.hpp"

using namespace s360;

namespace s360 {
int png_crc_threads() {
  const char* e = std::getenv("S360_PNG_CRC_THREADS");
  const int n = e ? std::atoi(e) : 4;
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}
// ---- what the fetches of a finished frame share (api_internal.hpp; api_frame_jpeg.hip uses them too) ----
// the state of frame slot `slot` (-1: the selected one) without touching the selection: a fetching thread names its slot, so that
// the thread that feeds the context can go on selecting slots for its uploads
FrameState& slot_state(s360_ctx* c, int slot) {
  if (slot < 0) return frame_state(c);
  need(slot < (int)std::max<size_t>(c->slots.size(), 1), "frame slot out of range");
  const int saved = c->slot;
  c->slot = slot;
  struct Restore { s360_ctx* c; int s; ~Restore() { c->slot = s; } } restore{c, saved};
  return frame_state(c);
}
// the download stream, the event its host thread sleeps on, the error words' landing area
void ensure_download_stream(s360_ctx* c) {
  if (!c->stDown) S360_HIP(hipStreamCreateWithFlags(&c->stDown, hipStreamNonBlocking));
  if (!c->evDown) S360_HIP(hipEventCreateWithFlags(&c->evDown, hipEventDisableTiming | hipEventBlockingSync));
  if (!c->downErr.p) {
    c->downErr.ensure(4 * sizeof(unsigned));
    std::memset(c->downErr.p, 0, 4 * sizeof(unsigned));
  }
}
// the output buffer that holds the frame `age` frames back (0 = latest enqueued frame, 1 = the one before)
int frame_buffer(s360_ctx* c, FrameState& F, int age) {
  need(F.frames_done > age, "that frame has not been rendered");
  need(age == 0 || ((c->pipeline || c->two_outputs) && F.outBGR[F.out_cur ^ 1].p),
       "age 1 needs two output buffers (s360_set_frame_pipelining or s360_set_output_double_buffer)");
  return age == 0 ? F.out_cur : F.out_cur ^ 1;
}
// ... and that frame's cubemap (s360_set_cubemap_output)
int cube_buffer(s360_ctx* c, FrameState& F, int age) {
  const int b = frame_buffer(c, F, age);
  if (F.cubeFrame[b] != F.frames_done - 1 - age || !F.cubeBGR[b].p)
    throw Error(S360_ERR_STATE, "that frame was rendered without s360_set_cubemap_output");
  return b;
}
}  // namespace s360

extern "C" {

// `bytes` bytes at `src`, which belong to output buffer b of slot F (the stacked equirect, the cubemap), into the caller's buffer
static void fetch_frame_bytes(s360_ctx* c, std::unique_lock<std::recursive_mutex>& lk, FrameState& F, int b, const void* src, size_t bytes,
                              uint8_t* out) {
  // wait for THAT frame only (its event sits behind its last kernel), then copy on a stream of its own so that the
  // transfer does not queue behind the kernels of the frame enqueued after it
  ensure_download_stream(c);
  if (!F.downRead[b]) S360_HIP(hipEventCreateWithFlags(&F.downRead[b], hipEventDisableTiming));
  S360_HIP(hipStreamWaitEvent(c->stDown, F.outDone[b], 0));
  S360_HIP(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stDown));
  // the frame's error words travel with it (a later frame's finish stage rewrites them as soon as downRead[b] has fired): a device
  // -> page-locked host copy on the download's own stream (a host -> host "async" copy would block this thread with the lock held)
  if (F.outErrDev[b].p) S360_HIP(hipMemcpyAsync(c->downErr.p, F.outErrDev[b].p, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stDown));
  S360_HIP(hipEventRecord(F.downRead[b], c->stDown));
  S360_HIP(hipEventRecord(c->evDown, c->stDown));
  const hipEvent_t ev = c->evDown;
  const unsigned* errw = F.outErrDev[b].p ? c->downErr.as<unsigned>() : nullptr;  // (nothing of the slot is touched after the lock is back: it may be gone)
  // The wait is most of a frame long: the context is free meanwhile (the next frame's uploads and enqueue need it).
  // One fetching thread per context: evDown is re-recorded by the next call.
  lk.unlock();
  const hipError_t rc = hipEventSynchronize(ev);
  lk.lock();
  S360_HIP(rc);
  // the frame's sweep error words were snapshotted in front of outDone[b] (render.hpp): a timed-out banded sweep
  // fails THIS frame's download, before the host hands the pixels to an encoder
  if (errw) check_sweep_error(c, errw);
}
// the stacked equirect, or (`cube`) the stacked cubemap, of the frame `age` frames back of a slot (-1: the selected one; the
// _slot entry points, which name their slot, pass a negative one on as kNoSlot)
static int download_impl(s360_ctx* c, int slot, int age, bool cube, uint8_t* out_bgr) {
  if (!c || slot < -1) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(out_bgr && (age == 0 || age == 1), "bad argument (age is 0 = latest enqueued frame or 1 = the one before)");
    FrameState& F = slot_state(c, slot);
    const int b = cube ? cube_buffer(c, F, age) : frame_buffer(c, F, age);
    if (cube) fetch_frame_bytes(c, lk, F, b, F.cubeBGR[b].p, (size_t)F.cubeOutW[b] * F.cubeOutH[b] * 3, out_bgr);
    else fetch_frame_bytes(c, lk, F, b, F.outBGR[b].p, (size_t)c->g.out_width * c->g.out_height * 3, out_bgr);
  });
}
int s360_frame_download_equirect_of(s360_ctx* c, int age, uint8_t* out_bgr) { return download_impl(c, -1, age, false, out_bgr); }
int s360_frame_download_equirect_slot(s360_ctx* c, int slot, int age, uint8_t* out_bgr) {
  return download_impl(c, slot < 0 ? kNoSlot : slot, age, false, out_bgr);
}
/* ---- the equirect as a PNG file, encoded on the device (png.hip; replaces imwriteExceptionOnFail, TRSP:938-961) ---- */
int s360_set_png_encode(s360_ctx* c, int on) {
  return guard(c, [&] { need(c, "null ctx"); c->png_encode = on != 0; });
}
// the bound of one file, 0 for a size or format the encoder refuses (the message is the thread's error)
static size_t png_file_bound(int w, int h, int channels = 3, int bits = 8) {
  size_t n = 0;
  (void)guard([&] { n = PngPlan::make(w, h, channels, bits).file_bound; });
  return n;
}
size_t s360_png_bound(int w, int h) { return png_file_bound(w, h); }
size_t s360_frame_png_bound(s360_ctx* c) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] { n = PngPlan::make(c->g.out_width, c->g.out_height).file_bound; });
  return n;
}
// band table to the host (event wait with the context released), then the file image's bytes, then the CRCs off the lock
// (plan, pointers and events by value: the slot they come from may be gone once the lock has been released)
static void png_fetch(s360_ctx* c, std::unique_lock<std::recursive_mutex>& lk, const PngPlan plan, const void* meta, const void* file,
                      hipEvent_t after /* nullable: what the copy waits for */, hipEvent_t readDone /* nullable: recorded behind the copies */,
                      const void* errDev, uint8_t* out, size_t cap, size_t* n_out, bool release = true) {
  ensure_download_stream(c);
  const size_t mbytes = ((size_t)plan.nbands + 1) * sizeof(PngBandMeta);
  c->pngMetaHost.ensure(mbytes);
  if (after) S360_HIP(hipStreamWaitEvent(c->stDown, after, 0));
  S360_HIP(hipMemcpyAsync(c->pngMetaHost.p, meta, mbytes, hipMemcpyDeviceToHost, c->stDown));
  if (errDev) S360_HIP(hipMemcpyAsync(c->downErr.p, errDev, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stDown));
  S360_HIP(hipEventRecord(c->evDown, c->stDown));
  hipEvent_t ev = c->evDown;
  if (release) lk.unlock();
  hipError_t rc = hipEventSynchronize(ev);
  if (release) lk.lock();
  S360_HIP(rc);
  std::vector<PngBandMeta> m((size_t)plan.nbands + 1);
  std::memcpy(m.data(), c->pngMetaHost.p, mbytes);
  unsigned errw[3] = {0u, 0u, 0u};  // (a copy: the landing area is rewritten by the next fetch)
  if (errDev) std::memcpy(errw, c->downErr.p, sizeof(errw));
  const size_t end_bands = (size_t)m[plan.nbands].file_off;
  if (end_bands > plan.file_bound || end_bands + 28 > cap) {
    if (readDone) S360_HIP(hipEventRecord(readDone, c->stDown));
    throw Error(S360_ERR_INVALID_ARG, "png: output buffer too small (s360_frame_png_bound / s360_png_bound give the size to allocate)");
  }
  S360_HIP(hipMemcpyAsync(out, file, end_bands, hipMemcpyDeviceToHost, c->stDown));
  if (readDone) S360_HIP(hipEventRecord(readDone, c->stDown));
  S360_HIP(hipEventRecord(c->evDown, c->stDown));
  ev = c->evDown;
  if (release) lk.unlock();
  rc = hipEventSynchronize(ev);
  if (rc != hipSuccess) { if (release) lk.lock(); S360_HIP(rc); }
  if (errw[0] | errw[1] | errw[2]) {
    if (release) lk.lock();
    check_sweep_error(c, errw);
  }
  // the file's frame around the bands and the chunks' CRCs: host work on the caller's buffer, the context stays free meanwhile
  const size_t n = png_finish_host(out, cap, plan, m.data(), png_crc_threads());
  if (release) lk.lock();
  *n_out = n;
}
// the file image of the equirect, or (`cube`) of the cubemap, of that frame
static int download_png_impl(s360_ctx* c, int slot, int age, bool cube, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c || slot < -1) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(out && n_out && (age == 0 || age == 1), "bad argument (age is 0 = latest enqueued frame or 1 = the one before)");
    FrameState& F = slot_state(c, slot);
    const int b = cube ? cube_buffer(c, F, age) : frame_buffer(c, F, age);
    const DevBuf& file = cube ? F.cubePngFile[b] : F.pngFile[b];
    if ((cube ? F.cubePngFrame[b] : F.pngFrame[b]) != F.frames_done - 1 - age || !file.p)
      throw Error(S360_ERR_STATE, "that frame was rendered without s360_set_png_encode");
    if (!F.downRead[b]) S360_HIP(hipEventCreateWithFlags(&F.downRead[b], hipEventDisableTiming));
    png_fetch(c, lk, cube ? F.cubePngPlan[b] : F.pngPlan[b], (cube ? F.cubePngMeta[b] : F.pngMeta[b]).p, file.p, F.outDone[b], F.downRead[b],
              F.outErrDev[b].p, out, cap, n_out);
  });
}
int s360_frame_download_png(s360_ctx* c, int age, uint8_t* out, size_t cap, size_t* n_out) { return download_png_impl(c, -1, age, false, out, cap, n_out); }
int s360_frame_download_png_slot(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  return download_png_impl(c, slot < 0 ? kNoSlot : slot, age, false, out, cap, n_out);
}
// The operator encoders: one image of `channels` samples of `bits` bits per pixel from the caller's memory. The plan is made
// inside the guard (a refused size or format is the call's error); `bound_msg` (nullable): the buffer must hold the file's bound.
static int encode_png_op(s360_ctx* c, const void* px, int w, int h, int channels, int bits, const char* bound_msg, bool needs_frame,
                         uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(px && out && n_out && w > 0 && h > 0, "bad argument");
    const PngPlan plan = PngPlan::make(w, h, channels, bits);
    if (bound_msg) need(cap >= plan.file_bound, bound_msg);
    const size_t nb = (size_t)w * h * channels * (bits / 8);
    c->op_a.ensure((nb + 3) & ~(size_t)3);
    c->op_b.ensure(plan.file_bound);
    S360_HIP(hipMemcpyAsync(c->op_a.p, px, nb, hipMemcpyHostToDevice, c->st));
    png_encode_enqueue(c->st, c->op_a.as<uint8_t>(), plan, c->op_c, c->op_d, c->op_b.as<uint8_t>());
    S360_HIP(hipStreamSynchronize(c->st));
    png_fetch(c, lk, plan, c->op_d.p, c->op_b.p, nullptr, nullptr, nullptr, out, cap, n_out, false);  // (the operator scratch stays locked)
  }, needs_frame);
}
int s360_encode_png(s360_ctx* c, const uint8_t* bgr, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  return encode_png_op(c, bgr, w, h, 3, 8, nullptr, true, out, cap, n_out);
}
int s360_frame_download_cubemap(s360_ctx* c, int age, uint8_t* out_bgr) { return download_impl(c, -1, age, true, out_bgr); }
int s360_frame_download_cubemap_slot(s360_ctx* c, int slot, int age, uint8_t* out_bgr) {
  return download_impl(c, slot < 0 ? kNoSlot : slot, age, true, out_bgr);
}
size_t s360_frame_cubemap_png_bound(s360_ctx* c) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] {
    if (c->cube_fw > 0 && c->cube_fh > 0)
      n = PngPlan::make(c->cube_video ? 3 * c->cube_fw : c->cube_fw, c->cube_video ? 4 * c->cube_fh : 12 * c->cube_fh).file_bound;
  });
  return n;
}
int s360_frame_download_cubemap_png(s360_ctx* c, int age, uint8_t* out, size_t cap, size_t* n_out) {
  return download_png_impl(c, -1, age, true, out, cap, n_out);
}
int s360_frame_download_cubemap_png_slot(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  return download_png_impl(c, slot < 0 ? kNoSlot : slot, age, true, out, cap, n_out);
}
/* ---- PNG files of B,G,R and B,G,R,A images, one or many per launch sequence (include/s360_state_png.h) ---- */
size_t s360_png_bound_c(int w, int h, int channels) { return png_file_bound(w, h, channels); }
int s360_encode_png_c(s360_ctx* c, const uint8_t* px, int w, int h, int channels, uint8_t* out, size_t cap, size_t* n_out) {
  return encode_png_op(c, px, w, h, channels, 8, nullptr, false, out, cap, n_out);
}
}  // extern "C"
namespace s360 {
// A batch's plan and its page-locked areas. The table's host copy is rewritten here: the upload of the batch before (a whole encode
// ago) has left it in any real use; if it has not, this is the one place that waits for it.
void png_batch_prepare(s360_ctx* c, s360_ctx::PngBatch& B, const std::vector<PngPlan>& plans) {
  if (!B.events) {
    S360_HIP(hipEventCreateWithFlags(&B.evEnc, hipEventDisableTiming));
    S360_HIP(hipEventCreateWithFlags(&B.evRead, hipEventDisableTiming));
    S360_HIP(hipEventCreateWithFlags(&B.evAfter, hipEventDisableTiming));
    B.events = true;
  }
  if (B.haveEnc && hipEventQuery(B.evEnc) != hipSuccess) {
    (void)hipGetLastError();
    S360_HIP(hipEventSynchronize(B.evEnc));
  }
  B.haveEnc = false;
  B.plan = PngBatchPlan::make(plans);
  B.tabHost.ensure(PngBatchPlan::table_bytes(plans.size(), (size_t)B.plan.nbands));
  B.metaHost.ensure(B.plan.meta_records * sizeof(PngBandMeta));
}
// ... and its launch sequence on the context's stream, the band tables' copy to the host behind it. Nothing waits.
void png_batch_run(s360_ctx* c, s360_ctx::PngBatch& B, const uint8_t* const* px) {
  if (B.haveRead) S360_HIP(hipStreamWaitEvent(c->st, B.evRead, 0));  // (a fetch of the batch before may still read its file images)
  png_batch_enqueue(c->st, px, B.plan, B.table, B.tabHost.p, B.scratch, B.meta, B.files);
  S360_HIP(hipMemcpyAsync(B.metaHost.p, B.meta.p, B.plan.meta_records * sizeof(PngBandMeta), hipMemcpyDeviceToHost, c->st));
  S360_HIP(hipEventRecord(B.evEnc, c->st));
  B.haveEnc = true;
  ++B.gen;
}
// File i of the batch into the caller's buffer. Everything the transfer needs is enqueued, and the read-done event recorded, BEFORE
// the lock is first released; plan, pointers and the batch's generation are taken by value. The file's size is known up front when
// the band tables have already arrived (the usual case from the second file on); otherwise as much as the caller's buffer or the
// file's bound allows is copied, and the size is checked afterwards — a buffer that turns out too small is refused, never overrun.
void png_batch_fetch(s360_ctx* c, std::unique_lock<std::recursive_mutex>& lk, s360_ctx::PngBatch& B, int i, uint8_t* out, size_t cap,
                            size_t* n_out, bool release) {
  if (!B.haveEnc) throw Error(S360_ERR_STATE, "no PNG batch has been encoded");
  need(i >= 0 && (size_t)i < B.plan.img.size(), "PNG index out of range");
  need(out && n_out, "bad argument");
  const PngPlan plan = B.plan.img[(size_t)i];
  const uint8_t* file = B.files.as<uint8_t>() + B.plan.file_off[(size_t)i];
  const PngBandMeta* mh = B.metaHost.as<const PngBandMeta>() + B.plan.meta0[(size_t)i];
  const unsigned long long gen = B.gen;
  const char* too_small = "png: output buffer too small (s360_frame_state_png_bound / s360_png_bound_c give the size to allocate)";
  ensure_download_stream(c);
  std::vector<PngBandMeta> m((size_t)plan.nbands + 1);
  const bool known = hipEventQuery(B.evEnc) == hipSuccess;
  if (!known) (void)hipGetLastError();
  size_t nbytes = std::min(cap, plan.file_bound);
  if (known) {
    std::memcpy(m.data(), mh, m.size() * sizeof(PngBandMeta));
    nbytes = (size_t)m[(size_t)plan.nbands].file_off;
    if (nbytes > plan.file_bound || nbytes + 28 > cap) throw Error(S360_ERR_INVALID_ARG, too_small);
  }
  hipEvent_t ev = nullptr;  // (an event per call: fetches of different files may wait at the same time)
  S360_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventBlockingSync));
  struct Drop { hipEvent_t e; ~Drop() { (void)hipEventDestroy(e); } } drop{ev};
  S360_HIP(hipStreamWaitEvent(c->stDown, B.evEnc, 0));
  S360_HIP(hipMemcpyAsync(out, file, nbytes, hipMemcpyDeviceToHost, c->stDown));
  S360_HIP(hipEventRecord(B.evRead, c->stDown));
  B.haveRead = true;
  S360_HIP(hipEventRecord(ev, c->stDown));
  if (release) lk.unlock();
  const hipError_t rc = hipEventSynchronize(ev);
  if (release) lk.lock();
  S360_HIP(rc);
  if (B.gen != gen) throw Error(S360_ERR_STATE, "the PNG batch was replaced by a later encode while this file was being fetched");
  if (!known) {
    std::memcpy(m.data(), mh, m.size() * sizeof(PngBandMeta));
    const size_t end = (size_t)m[(size_t)plan.nbands].file_off;
    if (end > plan.file_bound || end + 28 > cap) throw Error(S360_ERR_INVALID_ARG, too_small);
  }
  // the file's frame around the bands and the chunks' CRCs: host work on the caller's buffer and on copies, the context stays free
  if (release) lk.unlock();
  const size_t n = png_finish_host(out, cap, plan, m.data(), png_crc_threads());
  if (release) lk.lock();
  *n_out = n;
}
}  // namespace s360
extern "C" {
int s360_encode_png_batch(s360_ctx* c, int n, const uint8_t* const* px, const int* w, const int* h, const int* channels, uint8_t* const* out,
                          const size_t* cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(n > 0 && n <= 4096 && px && w && h && channels && out && cap && n_out, "bad argument");
    std::vector<PngPlan> plans;
    std::vector<size_t> at;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
      need(px[i] && out[i], "bad argument");
      plans.push_back(PngPlan::make(w[i], h[i], channels[i]));
      at.push_back(total);
      total += ((size_t)w[i] * h[i] * channels[i] + 15) & ~(size_t)15;
    }
    c->op_a.ensure(total);
    std::vector<const uint8_t*> dev;
    for (int i = 0; i < n; ++i) {
      dev.push_back(c->op_a.as<uint8_t>() + at[(size_t)i]);
      S360_HIP(hipMemcpyAsync(c->op_a.as<uint8_t>() + at[(size_t)i], px[i], (size_t)w[i] * h[i] * channels[i], hipMemcpyHostToDevice, c->st));
    }
    png_batch_prepare(c, c->opPng, plans);
    png_batch_run(c, c->opPng, dev.data());
    S360_HIP(hipStreamSynchronize(c->st));
    for (int i = 0; i < n; ++i) png_batch_fetch(c, lk, c->opPng, i, out[i], cap[i], &n_out[i], false);  // (the operator scratch stays locked)
  }, false);
}
int s360_frame_encode_state_pngs(s360_ctx* c, int n, const char* const* names, const int* idx) {
  return frame_guard(c, [&] {
    need(c && n > 0 && n <= 4096 && names && idx, "bad argument");
    FrameState& F = frame_state(c);
    std::vector<PngPlan> plans;
    std::vector<const uint8_t*> px;
    for (int i = 0; i < n; ++i) {
      need(names[i] != nullptr, "bad argument");
      int w = 0, h = 0, ch = 0;
      const void* src = frame_u8_source(c, F, names[i], idx[i], false, w, h, ch);
      need(ch == 4 && src, "only the 4-channel intermediates are encoded as state images");
      plans.push_back(PngPlan::make(w, h, 4));
      px.push_back(static_cast<const uint8_t*>(src));
    }
    s360_ctx::PngBatch& B = c->statePng;
    png_batch_prepare(c, B, plans);
    if (c->st2) {  // frame pipelining: the pole stage's images come from the finish stream — ordered on the device, not by the host
      S360_HIP(hipEventRecord(B.evAfter, c->st2));
      S360_HIP(hipStreamWaitEvent(c->st, B.evAfter, 0));
    }
    png_batch_run(c, B, px.data());
  });
}
size_t s360_frame_state_png_bound(s360_ctx* c, int i) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] {
    const s360_ctx::PngBatch& B = c->statePng;
    if (!B.haveEnc) throw Error(S360_ERR_STATE, "no PNG batch has been encoded");
    need(i >= 0 && (size_t)i < B.plan.img.size(), "PNG index out of range");
    n = B.plan.img[(size_t)i].file_bound;
  });
  return n;
}
int s360_frame_download_state_png(s360_ctx* c, int i, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) { png_batch_fetch(c, lk, c->statePng, i, out, cap, n_out, true); });
}
/* ---- banded PNG files decoded on the device (include/s360_png_decode.h, png_decode.hip) ---- */
static const char* const kNotDecodable = "not a banded PNG file of this decoder";
int s360_png_decodable(const uint8_t* file, size_t n, int whc[3], int* band_rows) {
  return guard([&] {
    need(whc && band_rows, "bad argument");
    PngBandedInfo I;
    if (!png_parse_banded(file, n, I)) throw Error(S360_ERR_INVALID_ARG, kNotDecodable);
    whc[0] = I.w; whc[1] = I.h; whc[2] = I.channels;
    *band_rows = I.band_rows;
  });
}
// the files of a call parsed; throws naming the first image that is not this decoder's
// a decode call fails because of file `image`: remembered for s360_png_decode_failure
[[noreturn]] static void png_fail(s360_ctx* c, int image, int reason, const std::string& msg) {
  c->pngDecFailImage = image;
  c->pngDecFailReason = reason;
  throw Error(S360_ERR_INVALID_ARG, msg);
}
static std::vector<PngBandedInfo> png_parse_all(s360_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, bool input = false) {
  c->pngDecFailImage = -1;
  c->pngDecFailReason = S360_PNG_DECODE_FAILURE_NONE;
  std::vector<PngBandedInfo> info((size_t)n);
  for (int i = 0; i < n; ++i) {
    need(files[i] != nullptr, "bad argument");
    if (!(input ? png_parse_banded_input : png_parse_banded)(files[i], bytes[i], info[(size_t)i]))
      png_fail(c, i, S360_PNG_DECODE_FAILURE_NOT_DECODABLE, "png decode: image " + std::to_string(i) + ": " + kNotDecodable);
  }
  return info;
}
// the launch sequence; a damaged file is remembered for s360_png_decode_failure
static void png_decode_checked(s360_ctx* c, int n, const uint8_t* const* files, const std::vector<PngBandedInfo>& info, const std::vector<uint8_t*>& dst) {
  try {
    png_decode_run(c->st, c->pngDec, std::vector<const uint8_t*>(files, files + n), info, dst, c->pngDecStats, &c->prof);
  } catch (const PngDecodeError& e) {
    c->pngDecFailImage = e.image;
    c->pngDecFailReason = S360_PNG_DECODE_FAILURE_DAMAGED;
    throw;
  }
}
int s360_png_decode_failure(s360_ctx* c, int* image, int* reason) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(image && reason, "bad argument");
    *image = c->pngDecFailImage;
    *reason = c->pngDecFailReason;
  });
}
int s360_decode_png_batch(s360_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, uint8_t* const* out, const size_t* cap,
                          int* whc_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>&) {
    need(n > 0 && n <= 4096 && files && bytes && out && cap, "bad argument");
    const std::vector<PngBandedInfo> info = png_parse_all(c, n, files, bytes);
    std::vector<size_t> at;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
      const PngBandedInfo& I = info[(size_t)i];
      const size_t nb = (size_t)I.w * I.h * I.channels;
      need(out[i] != nullptr, "bad argument");
      if (cap[i] < nb) png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + ": output buffer too small");
      at.push_back(total);
      total += (nb + 15) & ~(size_t)15;
    }
    c->op_a.ensure(total);
    std::vector<uint8_t*> dst;
    for (int i = 0; i < n; ++i) dst.push_back(c->op_a.as<uint8_t>() + at[(size_t)i]);
    png_decode_checked(c, n, files, info, dst);
    for (int i = 0; i < n; ++i) {
      const PngBandedInfo& I = info[(size_t)i];
      S360_HIP(hipMemcpyAsync(out[i], dst[(size_t)i], (size_t)I.w * I.h * I.channels, hipMemcpyDeviceToHost, c->st));
      if (whc_out) { whc_out[3 * i] = I.w; whc_out[3 * i + 1] = I.h; whc_out[3 * i + 2] = I.channels; }
    }
    S360_HIP(hipStreamSynchronize(c->st));
  }, false);
}
int s360_png_decode_stats(s360_ctx* c, uint64_t out[4]) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(out != nullptr, "bad argument");
    for (int k = 0; k < 4; ++k) out[k] = c->pngDecStats[k];
  });
}
int s360_png_decode_round_histogram(s360_ctx* c, uint64_t hist[66]) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(hist != nullptr, "bad argument");
    for (int k = 0; k < 66; ++k) hist[k] = c->pngDecStats[4 + k];
  });
}
int s360_frame_set_prev_images_png(s360_ctx* c, int n, const char* const* names, const int* idx, const uint8_t* const* files,
                                   const size_t* bytes) {
  return frame_guard(c, [&] {
    need(c && n > 0 && n <= 4096 && names && idx && files && bytes, "bad argument");
    FrameState& F = frame_state(c);
    const std::vector<PngBandedInfo> info = png_parse_all(c, n, files, bytes);
    // where every image goes, and what it must look like; the buffers are sized as the raw-pixel calls size them
    struct Arrival { int kind, k; unsigned bits; };  // kind 0 pair, 1 pole unit, 2 pole removal
    std::vector<uint8_t*> dst;
    std::vector<Arrival> arr;
    int prW = 0, prH = 0;
    for (int i = 0; i < n; ++i) {
      need(names[i] != nullptr, "bad argument");
      const std::string nm(names[i]);
      const PngBandedInfo& I = info[(size_t)i];
      int w = 0, h = 0;
      uchar4* p = nullptr;
      if (nm == "overlap_l" || nm == "overlap_r") {
        int j = 0;
        const PrevLayout L = prev_side_block(c, F, idx[i], j);
        F.overlaps[F.last_side].ensure(L.overlaps_bytes());
        w = c->g.overlap_image_width; h = c->g.cam_image_height;
        p = F.overlaps[F.last_side].as<uchar4>() + (nm == "overlap_r" ? L.right(j) : L.left(j));
        arr.push_back({0, idx[i], nm == "overlap_r" ? 2u : 1u});
      } else if (nm == "extended_side" || nm == "extended_fisheye") {
        need(idx[i] >= 0 && idx[i] < 4, "pole unit out of range");
        const PrevLayout L(c);
        F.extImgs[F.last_pole].ensure(L.ext_bytes());
        w = L.extW; h = L.rows(idx[i]);
        p = F.extImgs[F.last_pole].as<uchar4>() + (nm == "extended_side" ? L.side(idx[i]) : L.fisheye(idx[i]));
        arr.push_back({1, idx[i], nm == "extended_side" ? 1u : 2u});
      } else if (nm == "bottom_image" || nm == "bottom_image2") {
        need(c->P.enable_pole_removal != 0, "this context does not run pole removal");
        if (!prW) { prW = I.w; prH = I.h; }
        const size_t pn = (size_t)prW * prH;
        F.prImgs[F.last_pr].ensure(2 * pn * sizeof(uchar4));
        w = prW; h = prH;
        if (F.poleW > 0 && (F.poleW != prW || F.poleH != prH))
          png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + " (" + nm + "): not the size of the bottom camera's image");
        p = F.prImgs[F.last_pr].as<uchar4>() + (nm == "bottom_image2" ? pn : 0);
        arr.push_back({2, 0, nm == "bottom_image2" ? 2u : 1u});
      } else {
        throw Error(S360_ERR_INVALID_ARG, "not a previous-state image name: " + nm);
      }
      if (I.channels != 4 || I.w != w || I.h != h)
        png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + " (" + nm + "): wrong size/channels for the previous state");
      dst.push_back(reinterpret_cast<uint8_t*>(p));
    }
    // (a later ensure() of a buffer an earlier image of this call points into would move it: sizes per buffer are the same for
    // every image of a kind, except pole removal, whose size the first such image fixes)
    png_decode_checked(c, n, files, info, dst);
    for (const Arrival& a : arr) {
      if (a.kind == 0) prev_side_arrived(F, a.k, a.bits);
      else if (a.kind == 1) {
        // the fisheye image is shared by the two units of a pole
        if (a.bits == 2u) { prev_pole_arrived(c, F, a.k, 2u); prev_pole_arrived(c, F, a.k ^ 1, 2u); }
        else prev_pole_arrived(c, F, a.k, 1u);
      } else {
        F.prevPrW = prW; F.prevPrH = prH;
        prev_pr_arrived(F, a.bits);
      }
    }
  });
}
/* ---- camera images as banded PNG files, 8- or 16-bit, decoded on the device (include/s360_input_png.h) ---- */
static void input_png_info(const PngBandedInfo& I, int* info) {
  info[0] = I.w; info[1] = I.h; info[2] = I.channels; info[3] = I.depth; info[4] = I.band_rows;
}
int s360_input_png_decodable(const uint8_t* file, size_t n, int info[5]) {
  return guard([&] {
    need(info != nullptr, "bad argument");
    PngBandedInfo I;
    if (!png_parse_banded_input(file, n, I)) throw Error(S360_ERR_INVALID_ARG, kNotDecodable);
    input_png_info(I, info);
  });
}
int s360_decode_input_png_batch(s360_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, void* const* out, const size_t* cap_bytes,
                                int keep16, int* info_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>&) {
    need(n > 0 && n <= 4096 && files && bytes && out && cap_bytes, "bad argument");
    const std::vector<PngBandedInfo> info = png_parse_all(c, n, files, bytes, true);
    std::vector<size_t> at, nbytes;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
      const PngBandedInfo& I = info[(size_t)i];
      const bool u16 = I.depth == 16 && keep16;
      const size_t nb = (size_t)I.w * I.h * I.channels * (u16 ? 2 : 1);
      need(out[i] != nullptr, "bad argument");
      if (cap_bytes[i] < nb) png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + ": output buffer too small");
      if (u16 && (reinterpret_cast<uintptr_t>(out[i]) & 1))
        png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + ": 16-bit output not 2-byte aligned");
      at.push_back(total);
      nbytes.push_back(nb);
      total += (nb + 15) & ~(size_t)15;
    }
    c->op_a.ensure(total);
    std::vector<PngDecodeDst> dst((size_t)n);
    for (int i = 0; i < n; ++i) {
      dst[(size_t)i].p = c->op_a.as<uint8_t>() + at[(size_t)i];
      dst[(size_t)i].store = info[(size_t)i].depth == 16 && keep16 ? kPngStoreU16 : kPngStoreBytes;
    }
    try {
      png_decode_run(c->st, c->pngDec, std::vector<const uint8_t*>(files, files + n), info, dst, {}, c->pngDecStats, &c->prof);
    } catch (const PngDecodeError& e) {
      c->pngDecFailImage = e.image;
      c->pngDecFailReason = S360_PNG_DECODE_FAILURE_DAMAGED;
      throw;
    }
    for (int i = 0; i < n; ++i) {
      S360_HIP(hipMemcpyAsync(out[i], dst[(size_t)i].p, nbytes[(size_t)i], hipMemcpyDeviceToHost, c->st));
      if (info_out) input_png_info(info[(size_t)i], info_out + 5 * i);
    }
    S360_HIP(hipStreamSynchronize(c->st));
  }, false);
}
int s360_frame_upload_png(s360_ctx* c, int n, const int* cameras, const uint8_t* const* files, const size_t* bytes) {
  return frame_guard(c, [&] {
    need(c && n > 0 && n <= 66 && cameras && files && bytes, "bad argument");
    FrameState& F = frame_state(c);
    need(F.P <= 64, "more than 64 side cameras");
    for (int i = 0; i < n; ++i) {
      need(upload_camera_valid(c, cameras[i], F.P), "camera index out of range");
      for (int j = 0; j < i; ++j) need(cameras[j] != cameras[i], "a camera is named twice");
    }
    const std::vector<PngBandedInfo> info = png_parse_all(c, n, files, bytes, true);
    int sw = F.have_side ? F.srcW : 0, sh = F.have_side ? F.srcH : 0;
    for (int i = 0; i < n; ++i) {
      const PngBandedInfo& I = info[(size_t)i];
      if (I.channels != 3)
        png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + ": a camera image must have colour type 2 (3 channels)");
      if (cameras[i] < 0) continue;
      if (!sw) { sw = I.w; sh = I.h; }
      if (I.w != sw || I.h != sh) png_fail(c, i, S360_PNG_DECODE_FAILURE_MISMATCH, "png decode: image " + std::to_string(i) + ": side image size changed");
    }
    try {
      frame_upload_png(c, std::vector<int>(cameras, cameras + n), std::vector<const uint8_t*>(files, files + n), info);
    } catch (const PngDecodeError& e) {
      c->pngDecFailImage = e.image;
      c->pngDecFailReason = S360_PNG_DECODE_FAILURE_DAMAGED;
      throw;
    }
  });
}
/* ---- 16-bit PNG files, and the ISP's result as a finished PNG file (include/s360_isp_png.h) ---- */
size_t s360_png_bound_16(int w, int h) { return png_file_bound(w, h, 3, 16); }
int s360_encode_png16(s360_ctx* c, const uint16_t* bgr16, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  return encode_png_op(c, bgr16, w, h, 3, 16, "png: output buffer too small (s360_png_bound_16 gives the size to allocate)", false, out, cap, n_out);
}

}  // extern "C"
