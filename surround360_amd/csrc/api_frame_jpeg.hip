// api_frame_jpeg.hip — C ABI (libs360.so), part 7: a finished frame's equirect and cubemap as baseline JPEG files encoded on the
// device (include/s360_frame_jpeg.h, s360_debug_frame_jpeg.h; jpeg.hip; the finish stage of render.hip enqueues the encodes). The
// entry points mirror the PNG ones of api_png.hip one for one.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/s360.h"
#include "../../include/s360_debug_frame_jpeg.h"
#include "api_internal.hpp"

using namespace s360;

namespace {

// a scan that did not fit the buffer it was given: nothing of it was stored (jpeg.hip), the error names what it needed
[[noreturn]] void scan_refused(size_t n, size_t cap, size_t* n_out) {
  *n_out = JPEG_HEADER_BYTES + n + 2;
  throw Error(S360_ERR_STATE, "jpeg: the frame's scan needs " + std::to_string(n) + " bytes, its buffer on the device holds " + std::to_string(cap) +
                                  " (768 per MCU of 16 x 16 pixels, include/s360_frame_jpeg.h): no file for this frame");
}
[[noreturn]] void cap_refused(size_t n, size_t* n_out) {
  *n_out = JPEG_HEADER_BYTES + n + 2;
  throw Error(S360_ERR_INVALID_ARG, "jpeg: cap is smaller than the file, which has " + std::to_string(*n_out) +
                                        " bytes (its size is in *n_out; s360_frame_jpeg_bound / s360_frame_cubemap_jpeg_bound give the size to allocate)");
}

// The file of one image of a finished frame into the caller's buffer. Everything the transfer needs is enqueued, and the slot's
// read-done event recorded, BEFORE the lock is first released: a feeder that enqueues the frame after next in that window finds the
// event and waits for this copy on the device. Header, pointers, events and sizes are taken by value: the slot they come from may
// be gone once the lock has been released. The scan's size is known up front when the frame has already finished (its page-locked
// copy was written in front of `after`): then exactly the scan is copied. Otherwise the whole slot buffer is copied and the size,
// which travels with it, is read afterwards; a caller whose buffer cannot take that is made to wait for the frame with the
// context held — the price of a buffer below the bound, never a write past it.
void jpeg_fetch(s360_ctx* c, std::unique_lock<std::recursive_mutex>& lk, const std::vector<uint8_t> hdr, const uint8_t* scan, size_t slot_cap,
                const uint32_t* count_dev, const uint32_t* count_pin, hipEvent_t after, hipEvent_t readDone, const void* errDev, uint8_t* out,
                size_t cap, size_t* n_out) {
  *n_out = 0;
  ensure_download_stream(c);
  c->jpegDown.ensure(sizeof(uint32_t));
  bool known = hipEventQuery(after) == hipSuccess;
  if (!known) (void)hipGetLastError();
  if (!known && cap < JPEG_HEADER_BYTES + slot_cap + 2) {
    S360_HIP(hipEventSynchronize(after));
    known = true;
  }
  size_t n = slot_cap;
  if (known) {
    n = *count_pin;
    if (n > slot_cap) scan_refused(n, slot_cap, n_out);
    if (JPEG_HEADER_BYTES + n + 2 > cap) cap_refused(n, n_out);
  }
  hipEvent_t ev = nullptr;  // (an event per call: evDown belongs to the PNG and pixel fetches)
  S360_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventBlockingSync));
  struct Drop { hipEvent_t e; ~Drop() { (void)hipEventDestroy(e); } } drop{ev};
  uint32_t* landed = c->jpegDown.as<uint32_t>();
  const unsigned* errLanded = errDev ? c->downErr.as<unsigned>() : nullptr;
  S360_HIP(hipStreamWaitEvent(c->stDown, after, 0));
  if (!known) S360_HIP(hipMemcpyAsync(landed, count_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stDown));
  if (errDev) S360_HIP(hipMemcpyAsync(c->downErr.p, errDev, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stDown));
  if (n) S360_HIP(hipMemcpyAsync(out + JPEG_HEADER_BYTES, scan, n, hipMemcpyDeviceToHost, c->stDown));
  S360_HIP(hipEventRecord(readDone, c->stDown));
  S360_HIP(hipEventRecord(ev, c->stDown));
  // The wait is most of a frame long: the context is free meanwhile. One fetching thread per context: the landing areas are
  // rewritten by the next fetch.
  lk.unlock();
  const hipError_t rc = hipEventSynchronize(ev);
  unsigned errw[3] = {0u, 0u, 0u};
  if (rc == hipSuccess && errLanded) std::memcpy(errw, errLanded, sizeof errw);
  if (rc == hipSuccess && !known) n = *landed;
  lk.lock();
  S360_HIP(rc);
  if (errw[0] | errw[1] | errw[2]) check_sweep_error(c, errw);
  if (n > slot_cap) scan_refused(n, slot_cap, n_out);
  std::memcpy(out, hdr.data(), JPEG_HEADER_BYTES);
  out[JPEG_HEADER_BYTES + n] = 0xFF;
  out[JPEG_HEADER_BYTES + n + 1] = 0xD9;
  *n_out = JPEG_HEADER_BYTES + n + 2;
}

// the file of the equirect, or (`cube`) of the cubemap, of that frame
int download_jpeg_impl(s360_ctx* c, int slot, int age, bool cube, uint8_t* out, size_t cap, size_t* n_out) {
  if (!c || slot < -1) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>& lk) {
    need(out && n_out && (age == 0 || age == 1), "bad argument (age is 0 = latest enqueued frame or 1 = the one before)");
    FrameState& F = slot_state(c, slot);
    const int b = cube ? cube_buffer(c, F, age) : frame_buffer(c, F, age);
    const int k = cube ? 1 : 0;
    const FrameState::JpegOut& J = F.jpeg[k];
    if (J.frame[b] != F.frames_done - 1 - age || !J.scan[b].p) throw Error(S360_ERR_STATE, "that frame was rendered without s360_set_jpeg_encode");
    if (!F.downRead[b]) S360_HIP(hipEventCreateWithFlags(&F.downRead[b], hipEventDisableTiming));
    jpeg_fetch(c, lk, J.hdr[b], J.scan[b].as<uint8_t>(), J.cap[b], F.jpegCount[b].as<uint32_t>() + k, F.jpegCountPin[b].as<uint32_t>() + k,
               F.outDone[b], F.downRead[b], F.outErrDev[b].p, out, cap, n_out);
  });
}
size_t bound_of(int w, int h) { return jpeg_size_ok(w, h) ? JPEG_HEADER_BYTES + jpeg_frame_scan_cap(w, h) + 2 : 0; }

}  // namespace

extern "C" {

int s360_set_jpeg_encode(s360_ctx* c, int on, int quality) {
  return guard(c, [&] {
    need(c, "null ctx");
    if (on && c->frame_invalid.empty())
      need(jpeg_size_ok(c->g.out_width, c->g.out_height), "s360_set_jpeg_encode: a JPEG file holds at most 65535 x 65535 pixels and this encoder 431 220 MCUs of 16 x 16");
    c->jpeg_encode = on != 0;
    if (on) c->jpeg_quality = quality < 1 ? 1 : quality > 100 ? 100 : quality;  // as s360_jpeg_create clamps
  });
}
size_t s360_frame_jpeg_bound(s360_ctx* c) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] {
    if (c->frame_invalid.empty()) n = bound_of(c->g.out_width, c->g.out_height);
  });
  return n;
}
size_t s360_frame_cubemap_jpeg_bound(s360_ctx* c) {
  size_t n = 0;
  if (!c) return 0;
  (void)guard(c, [&] {
    if (c->cube_fw > 0 && c->cube_fh > 0) n = bound_of(c->cube_video ? 3 * c->cube_fw : c->cube_fw, c->cube_video ? 4 * c->cube_fh : 12 * c->cube_fh);
  });
  return n;
}
int s360_frame_download_jpeg(s360_ctx* c, int age, uint8_t* out, size_t cap, size_t* n_out) { return download_jpeg_impl(c, -1, age, false, out, cap, n_out); }
int s360_frame_download_jpeg_slot(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  return download_jpeg_impl(c, slot < 0 ? kNoSlot : slot, age, false, out, cap, n_out);
}
int s360_frame_download_cubemap_jpeg(s360_ctx* c, int age, uint8_t* out, size_t cap, size_t* n_out) {
  return download_jpeg_impl(c, -1, age, true, out, cap, n_out);
}
int s360_frame_download_cubemap_jpeg_slot(s360_ctx* c, int slot, int age, uint8_t* out, size_t cap, size_t* n_out) {
  return download_jpeg_impl(c, slot < 0 ? kNoSlot : slot, age, true, out, cap, n_out);
}

/* ---- the test tap (include/s360_debug_frame_jpeg.h) ---- */
int s360_debug_frame_jpeg(s360_ctx* c, const uint8_t* bgr, int w, int h, size_t scan_cap, uint8_t* out, size_t cap, size_t* n_out,
                          size_t* stored, size_t* guard_touched, float* ms) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>&) {
    need(bgr && out && n_out && stored && guard_touched && jpeg_size_ok(w, h), "bad argument");
    need(scan_cap <= jpeg_scan_cap(w, h), "scan_cap above the worst case of the size");
    *n_out = 0;
    constexpr size_t kGuard = 4096;
    constexpr int kFill = 0xA5;
    const size_t npx = (size_t)w * h * 3, nbuf = scan_cap + kGuard;
    wait_finish_stream(c);  // (the frame path's encodes run on the finish stream: the encoder's scratch is shared)
    S360_HIP(hipStreamSynchronize(c->st));
    JpegEncoder& E = frame_jpeg_encoder(c, jpeg_mcus(w, h), c->st);
    c->op_a.ensure((npx + 3) & ~(size_t)3);
    c->op_b.ensure(nbuf);
    c->op_c.ensure(sizeof(uint32_t));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Drop { hipEvent_t* e; ~Drop() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } drop{ev};
    for (hipEvent_t& e : ev) S360_HIP(hipEventCreate(&e));
    S360_HIP(hipMemcpyAsync(c->op_a.p, bgr, npx, hipMemcpyHostToDevice, c->st));
    S360_HIP(hipMemsetAsync(c->op_b.p, kFill, nbuf, c->st));
    S360_HIP(hipEventRecord(ev[0], c->st));
    E.encode(c->op_a.as<uint8_t>(), w, h, c->op_b.as<uint8_t>(), scan_cap, c->op_c.as<uint32_t>(), c->st, true);
    S360_HIP(hipEventRecord(ev[1], c->st));
    uint32_t count = 0;
    std::vector<uint8_t> host(nbuf);
    S360_HIP(hipMemcpyAsync(&count, c->op_c.p, sizeof count, hipMemcpyDeviceToHost, c->st));
    S360_HIP(hipMemcpyAsync(host.data(), c->op_b.p, nbuf, hipMemcpyDeviceToHost, c->st));
    S360_HIP(hipStreamSynchronize(c->st));
    if (ms) S360_HIP(hipEventElapsedTime(ms, ev[0], ev[1]));
    *guard_touched = 0;
    for (size_t i = scan_cap; i < nbuf; ++i) *guard_touched += host[i] != kFill;
    const size_t n = count;
    if (n > scan_cap) {
      *stored = 0;
      for (size_t i = 0; i < scan_cap; ++i) *stored += host[i] != kFill;
      scan_refused(n, scan_cap, n_out);
    }
    *stored = n;
    if (JPEG_HEADER_BYTES + n + 2 > cap) cap_refused(n, n_out);
    E.header(out, w, h);
    std::memcpy(out + JPEG_HEADER_BYTES, host.data(), n);
    out[JPEG_HEADER_BYTES + n] = 0xFF;
    out[JPEG_HEADER_BYTES + n + 1] = 0xD9;
    *n_out = JPEG_HEADER_BYTES + n + 2;
  }, false);
}

}  // extern "C"
