// DEVELOPER / TEST TOOL — not part of the product: the library's whole PixFlow path (FlowEngine: flow.hip,
// flow_kernels.hip, median.hip, sweep_lock.hip, sweep_quad.hip) compiled for the CPU over tools/hip_wave_shim and run
// kernel by kernel with the GPU's execution model (see the shim's header). tests/test_cpu_flow_emulation.py compares its
// flows with the oracle's computeOpticalFlow bit for bit, so that the HIP sources' indexing, batching, pyramid schedule
// and hand-offs are checked where no GPU is attached. Build: make -C tools libflow_emu.so.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../surround360_amd/csrc/flow.hpp"

using namespace s360;

// A batch like the library's: n_images images of h x w BGRA, n_flows flows, flow b matching image i0[b] against i1[b]
// (all with one direction hint, as FlowEngine::compute takes it); optional previous images / flows for the temporal
// regularisation; out: n_flows x h x w x 2. sweep_mode 2 = latency kernel, 3 = throughput kernel.
extern "C" int emu_flow_batch(const uint8_t* images, int n_images, int w, int h, const char* alg, int hint, int n_flows,
                              const int* i0, const int* i1, const uint8_t* prev_images, const float* prev_flows,
                              int sweep_mode, float* out_flows, char* err, int cap) {
  try {
    const PixFlowConsts pc = pixflow_consts_by_name(alg);
    const size_t n = (size_t)w * h;
    DevBuf img, pimg, out, pflow;
    img.ensure((size_t)n_images * n * 4);
    std::memcpy(img.p, images, (size_t)n_images * n * 4);
    out.ensure((size_t)n_flows * n * sizeof(float2));
    FlowBatch fb;
    fb.add_images(img.as<uchar4>(), n_images, n);
    if (prev_flows) {
      pimg.ensure((size_t)n_images * n * 4);
      std::memcpy(pimg.p, prev_images, (size_t)n_images * n * 4);
      pflow.ensure((size_t)n_flows * n * sizeof(float2));
      std::memcpy(pflow.p, prev_flows, (size_t)n_flows * n * sizeof(float2));
      fb.add_prev_images(pimg.as<uchar4>(), n_images, n);
    }
    for (int b = 0; b < n_flows; ++b)
      fb.add_flow(i0[b], i1[b], out.as<float2>() + n * b, prev_flows ? pflow.as<float2>() + n * b : nullptr);
    Profiler prof;
    FlowEngine eng(&prof);
    eng.set_sweep_mode(sweep_mode);
    eng.compute(nullptr, pc, fb, w, h, hint);
    if (eng.take_error(nullptr)) throw Error(-3, "a sweep band timed out waiting for its neighbour");
    std::memcpy(out_flows, out.p, (size_t)n_flows * n * sizeof(float2));
    return 0;
  } catch (const std::exception& e) {
    if (err && cap > 0) { std::strncpy(err, e.what(), cap - 1); err[cap - 1] = 0; }
    return -1;
  }
}

// The pyramid's resize on its own (B one-channel planes sw x sh -> dw x dh): sizes with many tiles per plane and enough
// workgroups for the XCD-aware tile order to permute them — the frames the emulated tests can afford never get there.
extern "C" int emu_resize_linear_planes(const float* src, int sw, int sh, int B, int dw, int dh, float* dst) {
  try {
    launch_resize_linear_f32(nullptr, src, sw, sh, (size_t)sw * sh, dst, dw, dh, (size_t)dw * dh, 1, B, 1.f, 0);
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}

// The INTER_CUBIC resize of BGRA images (B images sw x sh -> dw x dh): with sh == dh the horizontal-only kernel.
extern "C" int emu_resize_cubic_u8c4(const uint8_t* src, int sw, int sh, int B, int dw, int dh, uint8_t* dst) {
  try {
    launch_resize_cubic_u8c4(nullptr, (const uchar4*)src, sw, sh, (size_t)sw * sh, (uchar4*)dst, dw, dh, (size_t)dw * dh, B);
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}

// The same resize by the one-thread-per-pixel kernel whatever the shape (the tiled kernels' second opinion).
extern "C" int emu_resize_cubic_u8c4_generic(const uint8_t* src, int sw, int sh, int B, int dw, int dh, uint8_t* dst) {
  try {
    launch_resize_cubic_u8c4_generic(nullptr, (const uchar4*)src, sw, sh, (size_t)sw * sh, (uchar4*)dst, dw, dh, (size_t)dw * dh, B);
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}
// PixFlow's entry downscale with the grey and alpha planes (B x dh x dw floats each) from the same launch; down == nullptr: the
// resized image is not stored. by_table: the sources are passed as a table of B pointers, as FlowEngine does. Returns 1 when the
// tiled kernel took the shape, 0 when the generic resize and k_gray_alpha did.
extern "C" int emu_entry_downscale(const uint8_t* src, int sw, int sh, int B, int dw, int dh, uint8_t* down, float* gray,
                                   float* alpha, int by_table) {
  try {
    const size_t ns = (size_t)sw * sh, nd = (size_t)dw * dh;
    std::vector<const uchar4*> tab(B);
    for (int b = 0; b < B; ++b) tab[b] = (const uchar4*)src + ns * b;
    DevBuf scratch;
    scratch.ensure(B * nd * sizeof(uchar4));
    launch_entry_downscale(nullptr, by_table ? nullptr : (const uchar4*)src, sw, sh, by_table ? 0 : ns, (uchar4*)down,
                           scratch.as<uchar4>(), dw, dh, nd, B, by_table ? tab.data() : nullptr, gray, alpha, nd);
    return resize_cubic_u8c4_tiled_fits(sw, sh, dw, dh) ? 1 : 0;
  } catch (const std::exception&) {
    return -1;
  }
}
// The final flow (INTER_LINEAR resize of B flows sw x sh to dw x dh, * post_scale, 3x3 Gaussian blur), written through a table of
// B destination pointers as FlowEngine does. Returns 1 when the tiled kernel took the shape, 0 when k_sepblur<1, 2, 0, 2> did.
static int emu_upscale_blur_impl(const float* src, int sw, int sh, int B, int dw, int dh, float post_scale, float* out, bool generic) {
  try {
    const size_t ns = (size_t)sw * sh, nd = (size_t)dw * dh;
    std::vector<float*> tab(B);
    for (int b = 0; b < B; ++b) tab[b] = out + 2 * nd * b;
    launch_upscale_blur(nullptr, (const float2*)src, sw, sh, ns, nullptr, dw, dh, nd, B, post_scale, gaussian_taps(3, 1.0f), tab.data(),
                        generic);
    return !generic && upscale_blur_tiled_fits(sw, sh, dw, dh) ? 1 : 0;
  } catch (const std::exception&) {
    return -1;
  }
}
extern "C" int emu_upscale_blur(const float* src, int sw, int sh, int B, int dw, int dh, float post_scale, float* out) {
  return emu_upscale_blur_impl(src, sw, sh, B, dw, dh, post_scale, out, false);
}
extern "C" int emu_upscale_blur_generic(const float* src, int sw, int sh, int B, int dw, int dh, float post_scale, float* out) {
  return emu_upscale_blur_impl(src, sw, sh, B, dw, dh, post_scale, out, true);
}
// k_gray_alpha on B images of n pixels.
extern "C" int emu_gray_alpha(const uint8_t* src, size_t n, int B, float* gray, float* alpha) {
  try {
    launch_gray_alpha(nullptr, (const uchar4*)src, n, n, gray, alpha, n, B);
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}

// The 15x15 blur launchers with an epilogue on the alphas (flow_kernels.hip: k_sepblur EPI 1 - 4) on caller-made planes, one level of B flows:
// flow / out B x h x w x 2, alpha n_images x h x w, flow b uses the alphas i0[b] and i1[b]. prev (B x h x w x 2) and motion
// (n_images x h x w) given: launch_diffusion_adjust with prev_scale.
extern "C" int emu_diffusion(const float* flow, const float* alpha, int w, int h, int B, const int* i0, const int* i1,
                             const float* prev, const float* motion, float prev_scale, float* out) {
  try {
    const BlurTaps t = gaussian_taps(15, 8.0f);
    const FlowIdx idx = {i0, i1};
    const size_t n = (size_t)w * h;
    if (prev) launch_diffusion_adjust(nullptr, (const float2*)flow, (float2*)out, w, h, n, B, t, alpha, idx, (const float2*)prev, motion, prev_scale);
    else launch_diffusion(nullptr, (const float2*)flow, (float2*)out, w, h, n, B, t, alpha, idx);
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}
// grad == nullptr: half-records (rec B x h x w x 2); grad (n_images x h x w x 2) given: full records (B x h x w x 4).
// rowflags: B x h, as the caller initialised them.
extern "C" int emu_blur_to_records(const float* flow, const float* alpha, const float* grad, int w, int h, int B, const int* i0,
                                   const int* i1, float* rec, unsigned* rowflags) {
  try {
    const FlowIdx idx = {i0, i1};
    launch_blur_to_records(nullptr, (const float2*)flow, rec, w, h, (size_t)w * h, B, gaussian_taps(15, 8.0f), (const float2*)grad, alpha,
                           idx, rowflags);
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}
// tiles of the blur into records by the way they went since the last reset: exit taken, full. Returns 0 when
// S360_KNOWN_RESULT=0 is set.
extern "C" int emu_known_result_stats(unsigned long long* out2, int reset) {
  for (int i = 0; i < 2; ++i) {
    if (out2) out2[i] = __atomic_load_n(&g_known_stats[i], __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(&g_known_stats[i], 0ull, __ATOMIC_RELAXED);
  }
  return known_result_enabled() ? 1 : 0;
}
