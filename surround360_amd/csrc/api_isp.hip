// api_isp.hip — the soft ISP's entry points (include/s360.h, s360_isp_png.h; isp.cpp / isp_kernels.hip: Raw2Rgb's
// non-accelerated path, CameraIsp.h). The objects are not locked.
#include <cstring>
#include <vector>

#include "../../include/s360.h"
#include "api_internal.hpp"
#include "isp.hpp"

using namespace s360;

/* ---- the ISP's result as a finished PNG file (include/s360_isp_png.h) ---- */
static PngPlan isp_png_plan(const s360_isp* o, int w, int h) {
  const int r = o->cfg.resize > 0 ? o->cfg.resize : 1;
  return PngPlan::make(w / r, h / r, 3, o->cfg.output_bpp == 16 ? 16 : 8);
}
// The encoder behind the ISP's kernels on the object's stream over `px` (the result on the device), the band table to its page-locked
// place: first wait. Then the file's bytes: second wait. Then the host's share on the caller's buffer.
static void isp_png_encode(s360_isp* o, const void* px, const PngPlan& plan, uint8_t* out, size_t cap, size_t* n_out) {
  const size_t mbytes = ((size_t)plan.nbands + 1) * sizeof(PngBandMeta);
  o->hPngMeta.ensure(mbytes);
  o->dPngFile.ensure(plan.file_bound);
  png_encode_enqueue(o->st, static_cast<const uint8_t*>(px), plan, o->dPngScratch, o->dPngMeta, o->dPngFile.as<uint8_t>());
  isp_time_end(o);
  S360_HIP(hipMemcpyAsync(o->hPngMeta.p, o->dPngMeta.p, mbytes, hipMemcpyDeviceToHost, o->st));
  S360_HIP(hipStreamSynchronize(o->st));
  isp_time_take(o);
  const PngBandMeta* m = o->hPngMeta.as<const PngBandMeta>();
  const size_t end_bands = (size_t)m[plan.nbands].file_off;
  if (end_bands > plan.file_bound || end_bands + 28 > cap) throw Error(S360_ERR_STATE, "png: the band table names more bytes than the file's bound");
  S360_HIP(hipMemcpyAsync(out, o->dPngFile.p, end_bands, hipMemcpyDeviceToHost, o->st));
  S360_HIP(hipStreamSynchronize(o->st));
  *n_out = png_finish_host(out, cap, plan, m, png_crc_threads());
}
// the two entry points: `develop` enqueues the upload and the ISP's kernels and returns the result on the device
template <typename Develop>
static int isp_process_png(s360_isp* isp, const void* in, int w, int h, uint8_t* out, size_t cap, size_t* n_out, Develop&& develop) {
  return guard([&] {
    need(isp && in && out && n_out && w > 0 && h > 0, "bad argument");
    const PngPlan plan = isp_png_plan(isp, w, h);
    need(cap >= plan.file_bound, "png: output buffer too small (s360_isp_png_bound gives the size to allocate)");
    isp_png_encode(isp, develop(), plan, out, cap, n_out);
  });
}

extern "C" {

void s360_isp_config_defaults(s360_isp_config* cfg) {
  if (cfg) isp_config_defaults(cfg);
}
int s360_isp_config_from_json(const char* json_text, s360_isp_config* cfg) {
  return guard([&] {
    need(json_text && cfg, "null argument");
    isp_config_from_json(json_text, cfg);
  });
}
int s360_isp_create(s360_isp** out, int device, const s360_isp_config* cfg) {
  if (!out) return S360_ERR_INVALID_ARG;
  *out = nullptr;
  s360_isp* o = nullptr;
  const int rc = guard([&] {
    need(cfg != nullptr, "null argument");
    o = new s360_isp;
    isp_init(o, device, *cfg);
  });
  if (rc != S360_OK) {
    if (o) isp_release(o);
    delete o;
    return rc;
  }
  *out = o;
  return S360_OK;
}
void s360_isp_destroy(s360_isp* isp) {
  if (!isp) return;
  isp_release(isp);
  delete isp;
}
int s360_isp_process(s360_isp* isp, const uint16_t* raw16, int w, int h, void* out_bgr) {
  return guard([&] {
    need(isp && raw16 && out_bgr && w > 0 && h > 0, "bad argument");
    isp_process(isp, raw16, w, h, out_bgr);
  });
}
int s360_isp_process_packed(s360_isp* isp, const uint8_t* frame, int bits, int w, int h, void* out_bgr) {
  return guard([&] {
    need(isp && frame && out_bgr && w > 0 && h > 0, "bad argument");
    isp_process_packed(isp, frame, bits, w, h, out_bgr);
  });
}
size_t s360_isp_png_bound(const s360_isp* isp, int w, int h) {
  size_t n = 0;
  if (!isp) return 0;
  (void)guard([&] { n = isp_png_plan(isp, w, h).file_bound; });
  return n;
}
int s360_isp_process_png(s360_isp* isp, const uint16_t* raw16, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  return isp_process_png(isp, raw16, w, h, out, cap, n_out, [&] { return isp_develop(isp, "s360_isp_process_png", raw16, w, h); });
}
int s360_isp_process_packed_png(s360_isp* isp, const uint8_t* frame, int bits, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  return isp_process_png(isp, frame, w, h, out, cap, n_out, [&] { return isp_develop_packed(isp, "s360_isp_process_packed_png", frame, bits, w, h); });
}
int s360_isp_pipe_generated(s360_isp* isp, const s360_camera_isp_gen_args* args) {
  return guard([&] {
    need(isp && args, "null argument");
    isp_pipe_generated(isp, *args);
  });
}
int s360_isp_config_tables(const s360_isp_config* cfg, float* ccm9, float* lut, int w, int h, float* curve_h,
                           float* curve_v) {
  return guard([&] {
    need(cfg != nullptr, "null argument");
    IspDev d;
    std::vector<float> l, ch, cv;
    isp_derive(*cfg, d, l);
    if (ccm9) std::memcpy(ccm9, d.ccm, 9 * sizeof(float));
    if (lut) std::memcpy(lut, l.data(), l.size() * sizeof(float));
    if (curve_h || curve_v) {
      need(w > 0 && h > 0, "bad frame size");
      isp_vignette_curves(*cfg, w, h, ch, cv);
      if (curve_h) std::memcpy(curve_h, ch.data(), ch.size() * sizeof(float));
      if (curve_v) std::memcpy(curve_v, cv.data(), cv.size() * sizeof(float));
    }
  });
}

}  // extern "C"
