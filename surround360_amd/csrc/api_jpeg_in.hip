// api_jpeg_in.hip — C ABI (libs360.so), part 6: camera images as baseline JPEG files decoded on the device (include/s360_input_jpeg.h,
// s360_debug_input_jpeg.h; jpeg_decode.hip). The shapes are those of api_png.hip's input-PNG entry points.
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/s360.h"
#include "../../include/s360_debug_input_jpeg.h"
#include "api_internal.hpp"

using namespace s360;

namespace {
const char* const kNotDecodable = "not a JPEG file of this decoder";

// a decode call fails because of file `image`: remembered for s360_jpeg_decode_failure
[[noreturn]] void jpeg_fail(s360_ctx* c, int image, int reason, const std::string& msg) {
  c->jpegDecFailImage = image;
  c->jpegDecFailReason = reason;
  throw Error(S360_ERR_INVALID_ARG, msg);
}
// the files of a call parsed; throws naming the first image that is not this decoder's
std::vector<JpegInInfo> jpeg_parse_all(s360_ctx* c, int n, const uint8_t* const* files, const size_t* bytes) {
  c->jpegDecFailImage = -1;
  c->jpegDecFailReason = S360_JPEG_DECODE_FAILURE_NONE;
  std::vector<JpegInInfo> info((size_t)n);
  for (int i = 0; i < n; ++i) {
    need(files[i] != nullptr, "bad argument");
    if (!jpeg_in_parse(files[i], bytes[i], info[(size_t)i]))
      jpeg_fail(c, i, S360_JPEG_DECODE_FAILURE_NOT_DECODABLE, "jpeg decode: image " + std::to_string(i) + ": " + kNotDecodable);
  }
  return info;
}
void jpeg_info(const JpegInInfo& I, int* info) {
  info[0] = I.w; info[1] = I.h; info[2] = 3; info[3] = I.hs; info[4] = I.vs; info[5] = (int)I.scan_len;
}
// a damaged file is remembered for s360_jpeg_decode_failure (the status words of jpeg_decode.hpp follow the header's reasons by 2)
template <typename F>
void jpeg_run_checked(s360_ctx* c, F&& f) {
  try {
    f();
  } catch (const JpegDecodeError& e) {
    c->jpegDecFailImage = e.image;
    c->jpegDecFailReason = (int)e.status + 2;
    throw;
  }
}
static_assert(kJpegBadCode + 2 == S360_JPEG_DECODE_FAILURE_BAD_CODE && kJpegMarker + 2 == S360_JPEG_DECODE_FAILURE_MARKER, "reasons follow the status words");
}  // namespace

extern "C" {

int s360_input_jpeg_decodable(const uint8_t* file, size_t n, int info[6]) {
  return guard([&] {
    need(info != nullptr, "bad argument");
    JpegInInfo I;
    if (!jpeg_in_parse(file, n, I)) throw Error(S360_ERR_INVALID_ARG, kNotDecodable);
    jpeg_info(I, info);
  });
}
int s360_decode_input_jpeg_batch(s360_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, void* const* out, const size_t* cap_bytes,
                                 int* info_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>&) {
    need(n > 0 && n <= 4096 && files && bytes && out && cap_bytes, "bad argument");
    const std::vector<JpegInInfo> info = jpeg_parse_all(c, n, files, bytes);
    std::vector<size_t> at, nbytes;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
      const JpegInInfo& I = info[(size_t)i];
      const size_t nb = (size_t)I.w * I.h * 3;
      need(out[i] != nullptr, "bad argument");
      if (cap_bytes[i] < nb) jpeg_fail(c, i, S360_JPEG_DECODE_FAILURE_MISMATCH, "jpeg decode: image " + std::to_string(i) + ": output buffer too small");
      at.push_back(total);
      nbytes.push_back(nb);
      total += (nb + 15) & ~(size_t)15;
    }
    c->op_a.ensure(total);
    std::vector<JpegDecodeDst> dst((size_t)n);
    for (int i = 0; i < n; ++i) dst[(size_t)i].p = c->op_a.as<uint8_t>() + at[(size_t)i];
    jpeg_run_checked(c, [&] { jpeg_decode_run(c->st, c->jpegDec, std::vector<const uint8_t*>(files, files + n), info, dst, {}, c->jpegDecStats); });
    for (int i = 0; i < n; ++i) {
      S360_HIP(hipMemcpyAsync(out[i], dst[(size_t)i].p, nbytes[(size_t)i], hipMemcpyDeviceToHost, c->st));
      if (info_out) jpeg_info(info[(size_t)i], info_out + 6 * i);
    }
    S360_HIP(hipStreamSynchronize(c->st));
  }, false);
}
int s360_frame_upload_jpeg(s360_ctx* c, int n, const int* cameras, const uint8_t* const* files, const size_t* bytes) {
  return frame_guard(c, [&] {
    need(c && n > 0 && n <= 66 && cameras && files && bytes, "bad argument");
    FrameState& F = frame_state(c);
    need(F.P <= 64, "more than 64 side cameras");
    for (int i = 0; i < n; ++i) {
      need(upload_camera_valid(c, cameras[i], F.P), "camera index out of range");
      for (int j = 0; j < i; ++j) need(cameras[j] != cameras[i], "a camera is named twice");
    }
    const std::vector<JpegInInfo> info = jpeg_parse_all(c, n, files, bytes);
    int sw = F.have_side ? F.srcW : 0, sh = F.have_side ? F.srcH : 0;
    for (int i = 0; i < n; ++i) {
      const JpegInInfo& I = info[(size_t)i];
      if (cameras[i] < 0) continue;
      if (!sw) { sw = I.w; sh = I.h; }
      if (I.w != sw || I.h != sh) jpeg_fail(c, i, S360_JPEG_DECODE_FAILURE_MISMATCH, "jpeg decode: image " + std::to_string(i) + ": side image size changed");
    }
    jpeg_run_checked(c, [&] { frame_upload_jpeg(c, std::vector<int>(cameras, cameras + n), std::vector<const uint8_t*>(files, files + n), info); });
  });
}
int s360_jpeg_decode_stats(s360_ctx* c, uint64_t counts[4], double ms[2], uint32_t* file_rounds, int cap) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(counts && ms && cap >= 0 && (file_rounds || !cap), "bad argument");
    const JpegDecodeStats& S = c->jpegDecStats;
    counts[0] = S.files; counts[1] = S.subsequences; counts[2] = S.rounds; counts[3] = S.most_file_rounds;
    ms[0] = S.ms_entropy; ms[1] = S.ms_pixels;
    for (size_t i = 0; i < (size_t)cap; ++i) file_rounds[i] = i < S.file_rounds.size() ? S.file_rounds[i] : 0u;
  });
}
int s360_jpeg_decode_failure(s360_ctx* c, int* image, int* reason) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard(c, [&] {
    need(image && reason, "bad argument");
    *image = c->jpegDecFailImage;
    *reason = c->jpegDecFailReason;
  });
}
/* ---- the test tap (include/s360_debug_input_jpeg.h) ---- */
int s360_debug_input_jpeg_blocks(s360_ctx* c, const uint8_t* file, size_t bytes, int16_t* coef_out, size_t cap_blocks, size_t* n_out) {
  if (!c) return S360_ERR_INVALID_ARG;
  return guard_l(c, [&](std::unique_lock<std::recursive_mutex>&) {
    need(file && coef_out && n_out, "bad argument");
    const uint8_t* const files[1] = {file};
    const std::vector<JpegInInfo> info = jpeg_parse_all(c, 1, files, &bytes);
    const size_t nb = jpeg_in_blocks(info[0]);
    if (cap_blocks < nb) jpeg_fail(c, 0, S360_JPEG_DECODE_FAILURE_MISMATCH, "jpeg decode: image 0: output buffer too small");
    c->op_a.ensure((size_t)info[0].w * info[0].h * 3);
    std::vector<JpegDecodeDst> dst(1);
    dst[0].p = c->op_a.as<uint8_t>();
    jpeg_run_checked(c, [&] { jpeg_decode_run(c->st, c->jpegDec, {file}, info, dst, {}, c->jpegDecStats, coef_out, 0); });
    *n_out = nb;
  }, false);
}

}  // extern "C"
