// preview.hip — pole-camera previews from packed capture frames on gfx950 (include/s360_preview.h): the per-frame work of
// the reference's TestHyperPreview (SR/test/TestHyperPreview.cpp) as three kernels.
//
//   k_preview_map      once per object and layer: precomputeProjectionWarp + projectEquirectToCam (:117-129,
//                      SR/render/ImageWarper.cpp:179-196) — float direction from host-built sinf / cosf tables, then
//                      Camera::sees and Camera::pixel (SR/render/Camera.h:133-180) in double
//   k_preview_develop  one launch for the layers whose raw image changed: unpack (as k_isp_unpack), simpleDemosaic at half
//                      resolution (:163-184), BGR2BGRA, topDownAlphaFade / radialAlphaFade (SR/util/CvUtil.cpp:312-334) -> float4
//   k_preview_compose  per output pixel: cv::remap INTER_CUBIC / BORDER_CONSTANT(0) of the three 32FC4 layers,
//                      flattenLayersAlphaSoftmax (CvUtil.cpp:336-360), * kNorm16to8, saturate_cast<uchar> -> B,G,R
//
// All three are per-pixel stream / gather kernels bound by memory traffic; the float4 intermediate between develop and compose
// (16 bytes per half-resolution pixel and layer) stays in HBM. float arithmetic in the reference's operation order (the library
// is built with -ffp-contract=off).
//
// s360_preview_set_jpeg: the frame is also encoded as a baseline JPEG file behind k_preview_compose, on the same stream
// (jpeg.hip; the per-slot scan buffer travels to the host instead of the pixels).
#include "../../include/s360_debug_preview.h"
#include "../../include/s360_preview.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "api_guard.hpp"
#include "core.hpp"
#include "devmath.hpp"
#include "expf_glibc.hpp"
#include "jpeg.hpp"
#include "render_kernels.hpp"

namespace s360 {
namespace {

struct PreviewCam {
  DevCamera c;
  double resolution[2], fovThreshold;
};

// ---- the warp map --------------------------------------------------------------------------------------------------
// theta depends on x only, phi on y only: cosf / sinf of both come from the host's libm as tables (as k_spherical_map's do).
__global__ __launch_bounds__(256) void k_preview_map(float2* __restrict__ map, int W, int H, PreviewCam cam,
                                                     const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                     const float* __restrict__ sinP, const float* __restrict__ cosP) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= W || y >= H) return;
  const float ux = sinP[y] * cosT[x];
  const float uy = sinP[y] * sinT[x];
  const float uz = cosP[y];
  const double depth = 1000000.0;  // Camera::kNearInfinity through the `const float depth` parameter: exact
  const double vx = depth * (double)ux - cam.c.pos[0], vy = depth * (double)uy - cam.c.pos[1],
               vz = depth * (double)uz - cam.c.pos[2];
  const double* R = cam.c.R;
  // Camera::isOutsideFov (Camera.h:161-173); backward() is the rotation's third row
  bool outside = false;
  if (cam.fovThreshold != -1) {
    const double behind = R[6] * vx + R[7] * vy + R[8] * vz;
    if (cam.fovThreshold == 0) {
      outside = behind >= 0;
    } else {
      const double dot = -behind;
      outside = dot * fabs(dot) <= cam.fovThreshold * (vx * vx + vy * vy + vz * vz);
    }
  }
  float2 o = make_float2(-1.f, -1.f);  // "this will sample 0-alpha when cv::remap'd"
  if (!outside) {
    const double cx = R[0] * vx + R[1] * vy + R[2] * vz;
    const double cy = R[3] * vx + R[4] * vy + R[5] * vz;
    const double cz = R[6] * vx + R[7] * vy + R[8] * vz;
    double sx, sy;
    if (cam.c.type == 0) {  // FTHETA
      const double norm = sqrt(cx * cx + cy * cy);
      const double r = atan2(norm, -cz);
      const double r2 = r * r;
      const double f = ((1 + r2 * (cam.c.distortion[0] + r2 * cam.c.distortion[1])) * r) / norm;
      sx = f * cx;
      sy = f * cy;
    } else {  // RECTILINEAR
      const double px = cx / -cz, py = cy / -cz;
      const double r2 = px * px + py * py;
      const double f = 1 + r2 * (cam.c.distortion[0] + r2 * cam.c.distortion[1]);
      sx = f * px;
      sy = f * py;
    }
    const double px = cam.c.focal[0] * sx + cam.c.principal[0];
    const double py = cam.c.focal[1] * sy + cam.c.principal[1];
    if (0 <= px && px < cam.resolution[0] && 0 <= py && py < cam.resolution[1]) o = make_float2((float)px, (float)py);  // (no - 0.5 here)
  }
  map[(size_t)y * W + x] = o;
}

// ---- develop -------------------------------------------------------------------------------------------------------
struct DevelopArgs {
  const unsigned char* packed[3];
  float4* dev[3];
  int layer[3];  // grid z -> layer
};
__device__ __forceinline__ float widen12(unsigned u) { return (float)(int)((u << 4 | u >> 8) & 0xFFFFu); }

__global__ __launch_bounds__(256) void k_preview_develop(DevelopArgs a, int bits, int rawW, int hw, int hh, float gamma,
                                                         int gammaIsOne) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= hw) return;
  const int layer = a.layer[blockIdx.z];
  const unsigned char* __restrict__ p = a.packed[layer];
  // simpleDemosaic's taps: g1 (2y, 2x), b (2y, 2x + 1), r (2y + 1, 2x), g2 (2y + 1, 2x + 1)
  float g1, g2, b, r;
  if (bits == 8) {
    const unsigned char* r0 = p + (size_t)(2 * y) * rawW + 2 * x;
    const unsigned char* r1 = r0 + rawW;
    g1 = (float)(int)(r0[0] * 0x101u);
    b = (float)(int)(r0[1] * 0x101u);
    r = (float)(int)(r1[0] * 0x101u);
    g2 = (float)(int)(r1[1] * 0x101u);
  } else {  // three bytes hold the pixels 2x and 2x + 1 of a row (RawConverter::convert12Frame; see k_isp_unpack)
    const size_t rowBytes = 3 * (size_t)rawW / 2;
    const unsigned char* r0 = p + (size_t)(2 * y) * rowBytes + (size_t)x * 3;
    const unsigned char* r1 = r0 + rowBytes;
    const unsigned a0 = r0[0], a1 = r0[1], a2 = r0[2], c0 = r1[0], c1 = r1[1], c2 = r1[2];
    g1 = widen12(a0 << 4 | (a1 & 0xFu));
    b = widen12(a2 << 4 | a1 >> 4);
    r = widen12(c0 << 4 | (c1 & 0xFu));
    g2 = widen12(c2 << 4 | c1 >> 4);
  }
  // `2^16-1` and `2^32-1` in simpleDemosaic are C++ XOR expressions: 2 ^ 15 = 13 and 2 ^ 31 = 29
  const float kMaxValue16 = 13.0f, kMaxValue32 = 29.0f;
  g1 = g1 / kMaxValue16;
  g2 = g2 / kMaxValue16;
  b = b / kMaxValue16;
  r = r / kMaxValue16;
  float g = (g1 + g2) / 2.0f;
  if (!gammaIsOne) {  // powf(x, 1) returns x; otherwise pow in double, rounded once more (not glibc's powf to the last bit)
    r = (float)pow((double)r, (double)gamma);
    g = (float)pow((double)g, (double)gamma);
    b = (float)pow((double)b, (double)gamma);
  }
  float alpha = 1.0f;                                    // cvtColor BGR2BGRA of a float image
  if (layer > 0) alpha *= (float)y / (float)hh;          // topDownAlphaFade, the bottom layers only
  const float dx = (float)x - (float)hw / 2.0f;          // radialAlphaFade
  const float dy = (float)y - (float)hh / 2.0f;
  const float rad = sqrtf(dx * dx + dy * dy) / (float)((float)(hh < hw ? hh : hw) / 2.0f);
  const float fade = 1.0f - rad;
  alpha *= (0.0f < fade) ? fade : 0.0f;                  // std::max(0.0f, 1.0f - r)
  a.dev[layer][(size_t)y * hw + x] = make_float4(b * kMaxValue32, g * kMaxValue32, r * kMaxValue32, alpha);
}

// ---- compose -------------------------------------------------------------------------------------------------------
// cv::remap INTER_CUBIC, BORDER_CONSTANT(0), 32FC4: float weights; interior sums row by row (4 terms left-associated, then
// sum += row), border taps are added one by one — remap_cubic_f32c2_at's order (render_kernels.hip) on four channels.
__device__ __forceinline__ float4 remap_cubic_f32c4_at(const float4* __restrict__ src, int sw, int sh, float mx, float my,
                                                       const float* __restrict__ tab) {
  int sx, sy, fxy;
  remap_coord(mx, my, &sx, &sy, &fxy);
  const float* w = tab + fxy * 16;
  const unsigned width1 = sw - 3 > 0 ? sw - 3 : 0, height1 = sh - 3 > 0 ? sh - 3 : 0;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((unsigned)sx < width1 && (unsigned)sy < height1) {
    const float4* S = src + (size_t)sy * sw + sx;
    float4 px[4][4], wr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // all loads are requested before the first is used
      wr[r] = *reinterpret_cast<const float4*>(w + 4 * r);
#pragma unroll
      for (int q = 0; q < 4; ++q) px[r][q] = S[(size_t)r * sw + q];
    }
    o.x = px[0][0].x * wr[0].x + px[0][1].x * wr[0].y + px[0][2].x * wr[0].z + px[0][3].x * wr[0].w;
    o.y = px[0][0].y * wr[0].x + px[0][1].y * wr[0].y + px[0][2].y * wr[0].z + px[0][3].y * wr[0].w;
    o.z = px[0][0].z * wr[0].x + px[0][1].z * wr[0].y + px[0][2].z * wr[0].z + px[0][3].z * wr[0].w;
    o.w = px[0][0].w * wr[0].x + px[0][1].w * wr[0].y + px[0][2].w * wr[0].z + px[0][3].w * wr[0].w;
#pragma unroll
    for (int r = 1; r < 4; ++r) {
      o.x += px[r][0].x * wr[r].x + px[r][1].x * wr[r].y + px[r][2].x * wr[r].z + px[r][3].x * wr[r].w;
      o.y += px[r][0].y * wr[r].x + px[r][1].y * wr[r].y + px[r][2].y * wr[r].z + px[r][3].y * wr[r].w;
      o.z += px[r][0].z * wr[r].x + px[r][1].z * wr[r].y + px[r][2].z * wr[r].z + px[r][3].z * wr[r].w;
      o.w += px[r][0].w * wr[r].x + px[r][1].w * wr[r].y + px[r][2].w * wr[r].z + px[r][3].w * wr[r].w;
    }
  } else if (!(sx >= sw || sx + 4 <= 0 || sy >= sh || sy + 4 <= 0)) {
    for (int r = 0; r < 4; ++r) {
      const int yi = sy + r;
      if (yi < 0 || yi >= sh) continue;
      for (int q = 0; q < 4; ++q) {
        const int xi = sx + q;
        if (xi < 0 || xi >= sw) continue;
        const float4 p = src[(size_t)yi * sw + xi];
        const float ww = w[r * 4 + q];
        o.x += p.x * ww;
        o.y += p.y * ww;
        o.z += p.z * ww;
        o.w += p.w * ww;
      }
    }
  }
  return o;
}

struct ComposeArgs {
  const float2* map[3];
  const float4* dev[3];
};
constexpr int PC_W = 64, PC_H = 4;

// remapped (test tap, nullable): layer tapLayer's sample per output pixel
__global__ __launch_bounds__(PC_W* PC_H) void k_preview_compose(ComposeArgs a, int hw, int hh, int W, int H,
                                                                const float* __restrict__ tab,
                                                                const unsigned long long* __restrict__ exptab, float coef,
                                                                unsigned char* __restrict__ out, float4* __restrict__ remapped,
                                                                int tapLayer) {
  const TileId t = xcd_tile();
  const int x = t.x * PC_W + threadIdx.x, y = t.y * PC_H + threadIdx.y;
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * W + x;
  float sumAlpha = 0.0f, sb = 0.0f, sg = 0.0f, sr = 0.0f;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const float2 m = a.map[l][i];
    // (-1, -1), "the camera does not see this point": the four taps inside the image all carry the weight 0 and the layers hold
    // finite non-negative values, so the sample is exactly +0 in every channel — the loads are skipped
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(m.x == -1.0f && m.y == -1.0f)) s = remap_cubic_f32c4_at(a.dev[l], hw, hh, m.x, m.y, tab);
    if (remapped && l == tapLayer) remapped[i] = s;
    const float alpha = expf_glibc(coef * s.w, exptab) - 1.0f;
    sb += alpha * s.x;
    sg += alpha * s.y;
    sr += alpha * s.z;
    sumAlpha += alpha;
  }
  // Vec3f / float multiplies by 1.f / sumAlpha; 0 * inf = NaN where no layer has alpha: cvRound gives INT_MIN, saturated to 0
  const float inv = 1.f / sumAlpha;
  const float kNorm16to8 = 255.0f / 65535.0f;
  unsigned char* o = out + i * 3;
  o[0] = (unsigned char)sat_u8(cv_round((sb * inv) * kNorm16to8));
  o[1] = (unsigned char)sat_u8(cv_round((sg * inv) * kNorm16to8));
  o[2] = (unsigned char)sat_u8(cv_round((sr * inv) * kNorm16to8));
}

inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// Camera::createRescaledCamera (Camera.cpp:273-289): int() of the scaled resolution, FLOAT scale factors applied to the double
// principal point and focal length
s360_camera rescaled_camera(const s360_camera& cam, float scale) {
  s360_camera s = cam;
  s.resolution[0] = (double)(int)(cam.resolution[0] * scale);
  s.resolution[1] = (double)(int)(cam.resolution[1] * scale);
  const float scaleX = (float)(s.resolution[0] / cam.resolution[0]);
  const float scaleY = (float)(s.resolution[1] / cam.resolution[1]);
  s.principal[0] *= scaleX;
  s.principal[1] *= scaleY;
  s.focal[0] *= scaleX;
  s.focal[1] *= scaleY;
  return s;
}

PreviewCam preview_cam(const s360_camera& c) {
  PreviewCam d;
  d.c.type = c.type;
  for (int i = 0; i < 3; ++i) d.c.pos[i] = c.position[i];
  for (int i = 0; i < 9; ++i) d.c.R[i] = c.rotation[i];
  for (int i = 0; i < 2; ++i) {
    d.c.principal[i] = c.principal[i];
    d.c.focal[i] = c.focal[i];
    d.c.distortion[i] = c.distortion[i];
    d.resolution[i] = c.resolution[i];
  }
  d.fovThreshold = c.fov_threshold;
  return d;
}

}  // namespace
}  // namespace s360

using namespace s360;

struct s360_preview {
  int device = 0;
  hipStream_t st = nullptr, stCopy = nullptr;
  int rawW = 0, rawH = 0, hw = 0, hh = 0, W = 0, H = 0;
  float gamma = 1.0f, coef = 30.0f;
  int camIdx[3] = {-1, -1, -1};
  s360_camera cam[3];
  DevBuf dMap[3], dPacked[3], dDev[3], dOut[2], dTab, dExp, dTapOut, dTapRemap;
  hipEvent_t evDone[2] = {nullptr, nullptr}, evT[3] = {nullptr, nullptr, nullptr};
  unsigned long long submitted = 0, fetched = 0;
  // .jpg output (s360_preview_set_jpeg): the encoder, the scan and its byte count per slot
  std::unique_ptr<JpegEncoder> jenc;
  bool jpegOn = false, slotJpeg[2] = {false, false}, jpegTimed = false;
  DevBuf dScan[2], dCount[2];
  hipEvent_t evJ[2] = {nullptr, nullptr};
  uint32_t* hCount = nullptr;
  uint8_t slotHeader[2][JPEG_HEADER_BYTES];  // written at submit: the tables of the encoder that made the slot's scan
  size_t packed_bytes(int bits) const { return bits == 8 ? (size_t)rawW * rawH : (size_t)rawH * (3 * (size_t)rawW / 2); }
  ~s360_preview() {
    if (st) (void)hipStreamSynchronize(st);
    if (stCopy) (void)hipStreamSynchronize(stCopy);
    for (hipEvent_t e : evDone)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : evT)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : evJ)
      if (e) (void)hipEventDestroy(e);
    if (hCount) (void)hipHostFree(hCount);
    if (st) (void)hipStreamDestroy(st);
    if (stCopy) (void)hipStreamDestroy(stCopy);
  }
};

namespace {

void develop(s360_preview* p, const bool changed[3], int bits) {
  DevelopArgs a;
  int n = 0;
  for (int l = 0; l < 3; ++l) {
    a.packed[l] = p->dPacked[l].as<unsigned char>();
    a.dev[l] = p->dDev[l].as<float4>();
    a.layer[l] = 0;
    if (changed[l]) a.layer[n++] = l;
  }
  if (n)
    hipLaunchKernelGGL(k_preview_develop, dim3(cdiv(p->hw, 256), p->hh, n), dim3(256), 0, p->st, a, bits, p->rawW, p->hw, p->hh,
                       p->gamma, p->gamma == 1.0f ? 1 : 0);
}
void compose(s360_preview* p, unsigned char* out, float4* remapped, int tapLayer) {
  ComposeArgs a;
  for (int l = 0; l < 3; ++l) {
    a.map[l] = p->dMap[l].as<float2>();
    a.dev[l] = p->dDev[l].as<float4>();
  }
  hipLaunchKernelGGL(k_preview_compose, dim3(cdiv(p->W, PC_W), cdiv(p->H, PC_H)), dim3(PC_W, PC_H), 0, p->st, a, p->hw, p->hh, p->W,
                     p->H, p->dTab.as<float>(), p->dExp.as<unsigned long long>(), p->coef, out, remapped, tapLayer);
}

void preview_init(s360_preview* p, const s360_camera* cams, int n, int device, int rawW, int rawH, int W, int H, double gamma,
                  double coef) {
  need(cams && n > 0, "s360_preview_create: no cameras");
  need(rawW >= 2 && rawH >= 2 && rawW <= 65536 && rawH <= 65536, "s360_preview_create: raw image size outside 2..65536");
  need(W >= 1 && H >= 1 && W <= 65536 && H <= 65536, "s360_preview_create: equirect size outside 1..65536");
  p->camIdx[0] = s360_rig_find_top(cams, n);
  p->camIdx[1] = s360_rig_find_bottom(cams, n);
  p->camIdx[2] = s360_rig_find_bottom2(cams, n);
  for (int l = 0; l < 3; ++l) {
    need(p->camIdx[l] >= 0 && p->camIdx[l] < n, "s360_preview_create: the rig has no top / bottom / secondary bottom camera");
    p->cam[l] = rescaled_camera(cams[p->camIdx[l]], 0.5f);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw Error(S360_ERR_NO_DEVICE, "no HIP device available (libs360 has no CPU path)");
  need(device >= 0 && device < ndev, "device index out of range");
  p->device = device;
  p->rawW = rawW; p->rawH = rawH; p->hw = rawW / 2; p->hh = rawH / 2; p->W = W; p->H = H;  // Size / int
  p->gamma = (float)gamma;  // powf(x, FLAGS_gamma), flattenLayersAlphaSoftmax(layers, FLAGS_softmax_coef): both narrow to float
  p->coef = (float)coef;
  S360_HIP(hipSetDevice(device));
  S360_HIP(hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
  S360_HIP(hipStreamCreateWithFlags(&p->stCopy, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k) S360_HIP(hipEventCreateWithFlags(&p->evDone[k], hipEventDisableTiming));
  for (int k = 0; k < 3; ++k) S360_HIP(hipEventCreate(&p->evT[k]));
  // tables: the 1024 x 16 float weights of remap's INTER_CUBIC (initInterTab2D), expf's 2^(i/32)
  std::vector<float> tf(1024 * 16);
  float t1[32][4];
  for (int k = 0; k < 32; ++k) cubic_coeffs(k * (1.f / 32), t1[k]);
  for (int iy = 0; iy < 32; ++iy)
    for (int ix = 0; ix < 32; ++ix)
      for (int k1 = 0; k1 < 4; ++k1)
        for (int k2 = 0; k2 < 4; ++k2) tf[(iy * 32 + ix) * 16 + k1 * 4 + k2] = t1[iy][k1] * t1[ix][k2];
  unsigned long long et[32];
  expf_glibc_table(et);
  p->dTab.ensure(tf.size() * sizeof(float));
  p->dExp.ensure(sizeof et);
  S360_HIP(hipMemcpyAsync(p->dTab.p, tf.data(), tf.size() * sizeof(float), hipMemcpyHostToDevice, p->st));
  S360_HIP(hipMemcpyAsync(p->dExp.p, et, sizeof et, hipMemcpyHostToDevice, p->st));
  // trig tables (TestHyperPreview.cpp:121-122): the expressions as written there — 2.0f * M_PI and 1.0 - ... are double,
  // (x + 0.5f) / float(width) is float; M_PI * (y + 0.5f) / float(height) is double throughout; both rounded to float once
  std::vector<float> trig(2 * (size_t)W + 2 * (size_t)H);
  float *cosT = trig.data(), *sinT = cosT + W, *sinP = sinT + W, *cosP = sinP + H;
  for (int x = 0; x < W; ++x) {
    const float theta = 2.0f * M_PI * (1.0 - (x + 0.5f) / float(W));
    cosT[x] = cosf(theta);
    sinT[x] = sinf(theta);
  }
  for (int y = 0; y < H; ++y) {
    const float phi = M_PI * (y + 0.5f) / float(H);
    sinP[y] = sinf(phi);
    cosP[y] = cosf(phi);
  }
  DevBuf dTrig;
  dTrig.ensure(trig.size() * sizeof(float));
  S360_HIP(hipMemcpyAsync(dTrig.p, trig.data(), trig.size() * sizeof(float), hipMemcpyHostToDevice, p->st));
  const float* dp = dTrig.as<float>();
  const size_t maxPacked = p->packed_bytes(12) > p->packed_bytes(8) ? p->packed_bytes(12) : p->packed_bytes(8);
  for (int l = 0; l < 3; ++l) {
    p->dMap[l].ensure((size_t)W * H * sizeof(float2));
    hipLaunchKernelGGL(k_preview_map, dim3(cdiv(W, 64), cdiv(H, 4)), dim3(64, 4), 0, p->st, p->dMap[l].as<float2>(), W, H,
                       preview_cam(p->cam[l]), dp, dp + W, dp + 2 * (size_t)W, dp + 2 * (size_t)W + H);
    p->dPacked[l].ensure(maxPacked);
    p->dDev[l].ensure((size_t)p->hw * p->hh * sizeof(float4));
    S360_HIP(hipMemsetAsync(p->dPacked[l].p, 0, maxPacked, p->st));  // initRaws: zeros
  }
  for (int k = 0; k < 2; ++k) p->dOut[k].ensure((size_t)W * H * 3);
  const bool all[3] = {true, true, true};
  develop(p, all, 8);  // the layers of three raw images of zeros
  S360_HIP(hipGetLastError());
  S360_HIP(hipStreamSynchronize(p->st));  // (the host tables go out of scope)
}

void submit(s360_preview* p, const uint8_t* const frames[3], int bits) {
  need(bits == 8 || bits == 12, "packed frames are 8 or 12 bits per pixel");
  need(bits == 8 || !(p->rawW & 1), "12-bit packed frames need an even width");
  if (p->submitted - p->fetched >= 2) throw Error(S360_ERR_STATE, "s360_preview_submit_packed: two frames are waiting to be fetched");
  S360_HIP(hipSetDevice(p->device));
  bool changed[3];
  for (int l = 0; l < 3; ++l) {
    changed[l] = frames[l] != nullptr;
    if (changed[l]) S360_HIP(hipMemcpyAsync(p->dPacked[l].p, frames[l], p->packed_bytes(bits), hipMemcpyHostToDevice, p->st));
  }
  const int slot = (int)(p->submitted & 1);
  S360_HIP(hipEventRecord(p->evT[0], p->st));
  develop(p, changed, bits);
  S360_HIP(hipEventRecord(p->evT[1], p->st));
  compose(p, p->dOut[slot].as<unsigned char>(), nullptr, -1);
  S360_HIP(hipEventRecord(p->evT[2], p->st));
  S360_HIP(hipGetLastError());
  p->slotJpeg[slot] = p->jpegOn;
  if (p->jpegOn) {
    S360_HIP(hipEventRecord(p->evJ[0], p->st));
    p->jenc->encode(p->dOut[slot].as<uint8_t>(), p->W, p->H, p->dScan[slot].as<uint8_t>(), p->dScan[slot].cap, p->dCount[slot].as<uint32_t>(),
                    p->st);
    S360_HIP(hipEventRecord(p->evJ[1], p->st));
    p->jenc->header(p->slotHeader[slot], p->W, p->H);
    p->jpegTimed = true;
  }
  S360_HIP(hipEventRecord(p->evDone[slot], p->st));
  p->submitted += 1;
}
void set_jpeg(s360_preview* p, int on, int quality) {
  if (!on) {
    p->jpegOn = false;
    return;
  }
  need(jpeg_size_ok(p->W, p->H), "s360_preview_set_jpeg: the equirect is larger than the JPEG encoder's limits (include/s360_jpeg.h)");
  S360_HIP(hipSetDevice(p->device));
  const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
  if (!p->jenc || p->jenc->quality != q) {
    S360_HIP(hipStreamSynchronize(p->st));  // (frames in flight may still use the tables of the encoder that goes)
    std::unique_ptr<JpegEncoder> e(new JpegEncoder);
    e->init(p->W, p->H, q, p->st);
    p->jenc = std::move(e);
  }
  for (int k = 0; k < 2; ++k) {
    p->dScan[k].ensure(jpeg_scan_cap(p->W, p->H));
    p->dCount[k].ensure(sizeof(uint32_t));
    if (!p->evJ[k]) S360_HIP(hipEventCreate(&p->evJ[k]));
  }
  if (!p->hCount) S360_HIP(hipHostMalloc((void**)&p->hCount, sizeof(uint32_t), hipHostMallocDefault));
  p->jpegOn = true;
}
void fetch_jpeg(s360_preview* p, uint8_t* out, size_t cap, size_t* n_out) {
  *n_out = 0;
  if (p->fetched == p->submitted) throw Error(S360_ERR_STATE, "s360_preview_fetch_jpeg: no submitted frame is waiting");
  const int slot = (int)(p->fetched & 1);
  if (!p->slotJpeg[slot]) throw Error(S360_ERR_STATE, "s360_preview_fetch_jpeg: the oldest frame was submitted with the encoder off (s360_preview_fetch takes it)");
  S360_HIP(hipSetDevice(p->device));
  // the byte count first, then exactly that many bytes
  S360_HIP(hipStreamWaitEvent(p->stCopy, p->evDone[slot], 0));
  S360_HIP(hipMemcpyAsync(p->hCount, p->dCount[slot].p, sizeof(uint32_t), hipMemcpyDeviceToHost, p->stCopy));
  S360_HIP(hipStreamSynchronize(p->stCopy));
  const size_t n = *p->hCount;
  if (n > p->dScan[slot].cap) throw Error(S360_ERR_STATE, "s360_preview_fetch_jpeg: the scan is longer than its worst case");
  *n_out = JPEG_HEADER_BYTES + n + 2;
  need(out && cap >= *n_out, "s360_preview_fetch_jpeg: cap is smaller than the file (its size is in *n_out; the frame stays queued)");
  p->fetched += 1;  // (a failed transfer does not leave the frame in the queue)
  std::memcpy(out, p->slotHeader[slot], JPEG_HEADER_BYTES);  // (the encoder may have been replaced by another quality since)
  S360_HIP(hipMemcpyAsync(out + JPEG_HEADER_BYTES, p->dScan[slot].p, n, hipMemcpyDeviceToHost, p->stCopy));
  S360_HIP(hipStreamSynchronize(p->stCopy));
  out[JPEG_HEADER_BYTES + n] = 0xFF;
  out[JPEG_HEADER_BYTES + n + 1] = 0xD9;
}
void fetch(s360_preview* p, uint8_t* out) {
  if (p->fetched == p->submitted) throw Error(S360_ERR_STATE, "s360_preview_fetch: no submitted frame is waiting");
  S360_HIP(hipSetDevice(p->device));
  const int slot = (int)(p->fetched & 1);
  p->fetched += 1;  // (a failed transfer does not leave the frame in the queue)
  S360_HIP(hipStreamWaitEvent(p->stCopy, p->evDone[slot], 0));
  S360_HIP(hipMemcpyAsync(out, p->dOut[slot].p, (size_t)p->W * p->H * 3, hipMemcpyDeviceToHost, p->stCopy));
  S360_HIP(hipStreamSynchronize(p->stCopy));
}
void read_back(s360_preview* p, void* dst, const void* src, size_t bytes) {
  S360_HIP(hipSetDevice(p->device));
  S360_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, p->st));
  S360_HIP(hipStreamSynchronize(p->st));
}

}  // namespace

extern "C" {

int s360_preview_create(s360_preview** out, const s360_camera* cams, int n_cams, int device, int raw_w, int raw_h, int eqr_w,
                        int eqr_h, double gamma, double softmax_coef) {
  if (!out) return S360_ERR_INVALID_ARG;
  *out = nullptr;
  s360_preview* p = nullptr;
  const int rc = guard([&] {
    p = new s360_preview;
    preview_init(p, cams, n_cams, device, raw_w, raw_h, eqr_w, eqr_h, gamma, softmax_coef);
  });
  if (rc != S360_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return S360_OK;
}
void s360_preview_destroy(s360_preview* p) { delete p; }
int s360_preview_cameras(const s360_preview* p, int idx_out[3]) {
  return guard([&] {
    need(p && idx_out, "null argument");
    for (int l = 0; l < 3; ++l) idx_out[l] = p->camIdx[l];
  });
}
int s360_preview_submit_packed(s360_preview* p, const uint8_t* top, const uint8_t* bottom, const uint8_t* bottom2, int bits) {
  return guard([&] {
    need(p != nullptr, "null argument");
    const uint8_t* const f[3] = {top, bottom, bottom2};
    submit(p, f, bits);
  });
}
int s360_preview_fetch(s360_preview* p, uint8_t* out_bgr) {
  return guard([&] {
    need(p && out_bgr, "null argument");
    fetch(p, out_bgr);
  });
}
int s360_preview_render_packed(s360_preview* p, const uint8_t* top, const uint8_t* bottom, const uint8_t* bottom2, int bits,
                               uint8_t* out_bgr) {
  return guard([&] {
    need(p && out_bgr, "null argument");
    if (p->submitted != p->fetched) throw Error(S360_ERR_STATE, "s360_preview_render_packed: submitted frames are waiting to be fetched");
    const uint8_t* const f[3] = {top, bottom, bottom2};
    submit(p, f, bits);
    fetch(p, out_bgr);
  });
}
int s360_preview_last_times(s360_preview* p, float* develop_ms, float* compose_ms) {
  return guard([&] {
    need(p && develop_ms && compose_ms, "null argument");
    if (!p->submitted) throw Error(S360_ERR_STATE, "s360_preview_last_times: nothing was submitted");
    S360_HIP(hipEventSynchronize(p->evT[2]));
    S360_HIP(hipEventElapsedTime(develop_ms, p->evT[0], p->evT[1]));
    S360_HIP(hipEventElapsedTime(compose_ms, p->evT[1], p->evT[2]));
  });
}
int s360_preview_set_jpeg(s360_preview* p, int on, int quality) {
  return guard([&] {
    need(p != nullptr, "null argument");
    set_jpeg(p, on, quality);
  });
}
size_t s360_preview_jpeg_bound(const s360_preview* p) { return p && jpeg_size_ok(p->W, p->H) ? jpeg_file_bound(p->W, p->H) : 0; }
int s360_preview_fetch_jpeg(s360_preview* p, uint8_t* out, size_t cap, size_t* n_out) {
  return guard([&] {
    need(p && n_out, "null argument");
    fetch_jpeg(p, out, cap, n_out);
  });
}
int s360_preview_last_jpeg_time(s360_preview* p, float* ms) {
  return guard([&] {
    need(p && ms, "null argument");
    if (!p->jpegTimed) throw Error(S360_ERR_STATE, "s360_preview_last_jpeg_time: no frame was submitted with the encoder on");
    S360_HIP(hipEventSynchronize(p->evJ[1]));
    S360_HIP(hipEventElapsedTime(ms, p->evJ[0], p->evJ[1]));
  });
}

// ---- test taps (include/s360_debug_preview.h) -----------------------------------------------------------------------
int s360_debug_preview_camera(const s360_preview* p, int layer, s360_camera* out) {
  return guard([&] {
    need(p && out && layer >= 0 && layer < 3, "bad argument");
    *out = p->cam[layer];
  });
}
int s360_debug_preview_map(s360_preview* p, int layer, float* map_out) {
  return guard([&] {
    need(p && map_out && layer >= 0 && layer < 3, "bad argument");
    read_back(p, map_out, p->dMap[layer].p, (size_t)p->W * p->H * sizeof(float2));
  });
}
int s360_debug_preview_set_maps(s360_preview* p, const float* map_top, const float* map_bottom, const float* map_bottom2) {
  return guard([&] {
    need(p != nullptr, "null argument");
    S360_HIP(hipSetDevice(p->device));
    const float* const m[3] = {map_top, map_bottom, map_bottom2};
    for (int l = 0; l < 3; ++l)
      if (m[l]) S360_HIP(hipMemcpyAsync(p->dMap[l].p, m[l], (size_t)p->W * p->H * sizeof(float2), hipMemcpyHostToDevice, p->st));
    S360_HIP(hipStreamSynchronize(p->st));
  });
}
int s360_debug_preview_developed(s360_preview* p, int layer, float* out) {
  return guard([&] {
    need(p && out && layer >= 0 && layer < 3, "bad argument");
    read_back(p, out, p->dDev[layer].p, (size_t)p->hw * p->hh * sizeof(float4));
  });
}
int s360_debug_preview_remapped(s360_preview* p, int layer, float* out) {
  return guard([&] {
    need(p && out && layer >= 0 && layer < 3, "bad argument");
    S360_HIP(hipSetDevice(p->device));
    p->dTapOut.ensure((size_t)p->W * p->H * 3);
    p->dTapRemap.ensure((size_t)p->W * p->H * sizeof(float4));
    compose(p, p->dTapOut.as<unsigned char>(), p->dTapRemap.as<float4>(), layer);
    S360_HIP(hipGetLastError());
    read_back(p, out, p->dTapRemap.p, (size_t)p->W * p->H * sizeof(float4));
  });
}

}  // extern "C"
