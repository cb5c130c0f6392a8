// flow.hip — FlowEngine: PixFlow::computeOpticalFlow (PixFlow.h:81-183) as a batched HIP
// launch sequence on one stream. See flow.hpp.
#include "flow.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace s360 {

PixFlowConsts pixflow_consts_by_name(const std::string& name) {
  PixFlowConsts c;
  c.pyrScaleFactor = 0.9f;
  c.smoothnessCoef = 0.001f;
  c.verticalRegularizationCoef = 0.01f;
  c.horizontalRegularizationCoef = 0.01f;
  c.gradientStepSize = 0.5f;
  c.downscaleFactor = 0.5f;
  c.maxPercentage = 0;
  if (name == "pixflow_low") return c;
  if (name == "pixflow_search_20") {
    c.maxPercentage = 20;
    return c;
  }
  throw Error(-4, "unrecognized flow algorithm name: " + name);
}

BlurTaps gaussian_taps(int n, double sigma) {
  // cv::getGaussianKernel(n, sigma, CV_32F): exp in double, taps stored as float, normalised by
  // the double sum of the float taps.
  float k[16];
  const double sigmaX = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
  const double scale2X = -0.5 / (sigmaX * sigmaX);
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    k[i] = (float)std::exp(scale2X * x * x);
    sum += k[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) k[i] = (float)(k[i] * sum);
  BlurTaps t;
  std::memset(&t, 0, sizeof(t));
  t.r = n / 2;
  for (int j = 0; j <= t.r; ++j) t.k[j] = k[t.r + j];
  return t;
}

void FlowLevels::build(int dw, int dh, float pyrScale) {
  w.clear(); h.clear(); off.clear();
  total = 0;
  int cw = dw, ch = dh;
  for (;;) {
    w.push_back(cw); h.push_back(ch); off.push_back(total);
    total += (size_t)cw * ch;
    const int nw = int(cw * pyrScale + 0.5f), nh = int(ch * pyrScale + 0.5f);
    if (nh <= 24 || nw <= 24 || w.size() >= 1000) break;  // kPyrMinImageSize, kPyrMaxLevels
    cw = nw; ch = nh;
  }
}

// Layout of the uploaded table (8-byte words): [N][B][images N][prev_images N][prev_flow B][out B][int i0[B], int i1[B]]
const unsigned long long* FlowEngine::batch_tables(hipStream_t st, const FlowBatch& b) {
  const size_t N = b.images.size(), B = b.out.size();
  std::vector<unsigned long long> key;
  key.reserve(2 * N + 3 * B + 2);
  key.push_back(N);
  key.push_back(B);
  for (size_t k = 0; k < N; ++k) key.push_back((unsigned long long)b.images[k]);
  for (size_t k = 0; k < N; ++k) key.push_back(b.prev_images.empty() ? 0ull : (unsigned long long)b.prev_images[k]);
  for (size_t k = 0; k < B; ++k) key.push_back(b.prev_flow.empty() ? 0ull : (unsigned long long)b.prev_flow[k]);
  for (size_t k = 0; k < B; ++k) key.push_back((unsigned long long)b.out[k]);
  {
    std::vector<int> ints(2 * B);
    for (size_t k = 0; k < B; ++k) { ints[k] = b.i0[k]; ints[B + k] = b.i1[k]; }
    const size_t at = key.size();
    key.resize(at + B);
    std::memcpy(&key[at], ints.data(), 2 * B * sizeof(int));
  }
  for (TabSlot& t : tabs_)
    if (t.key == key) return t.buf.as<unsigned long long>() + 2;
  TabSlot& t = tabs_[tab_next_];
  tab_next_ = (tab_next_ + 1) % 4;
  S360_HIP(hipStreamSynchronize(st));  // earlier launches may still read the slot that is being replaced
  t.key = key;
  t.buf.ensure(key.size() * sizeof(unsigned long long));
  S360_HIP(hipMemcpyAsync(t.buf.p, t.key.data(), key.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
  S360_HIP(hipStreamSynchronize(st));
  return t.buf.as<unsigned long long>() + 2;
}

FlowPrepared FlowEngine::prepare(hipStream_t st, const PixFlowConsts& pc, const FlowBatch& batch, int w, int h) {
  const int N = (int)batch.images.size(), B = (int)batch.out.size();
  if (B < 1 || B > kMaxFlows || (int)batch.i0.size() != B || (int)batch.i1.size() != B)
    throw Error(-1, "FlowEngine: bad batch");
  if (!batch.prev_flow.empty() && ((int)batch.prev_flow.size() != B || (int)batch.prev_images.size() != N))
    throw Error(-1, "FlowEngine: previous-frame state must cover the whole batch");
  for (int b = 0; b < B; ++b)
    if (batch.i0[b] < 0 || batch.i0[b] >= N || batch.i1[b] < 0 || batch.i1[b] >= N) throw Error(-1, "FlowEngine: image index out of range");
  Profiler& P = *prof_;
  FlowBufs& M = *bufs_;
  dw_ = int(w * pc.downscaleFactor);
  dh_ = int(h * pc.downscaleFactor);
  // every caller, not only the operator entry point (the frame stages come here directly): the sweep kernels' tap
  // footprints and window placement assume at least 2 x 2 pixels at every pyramid level
  if (dw_ < 2 || dh_ < 2)
    throw Error(-1, "image too small for PixFlow: the reference's bilinear taps need a 2x2 image after the entry downscale (PixFlow.h:457-475)");
  const size_t n0 = (size_t)dw_ * dh_;
  lv_.build(dw_, dh_, pc.pyrScaleFactor);
  const int L = (int)lv_.w.size();
  const bool usePrev = !batch.prev_flow.empty();
  const unsigned long long* tab = batch_tables(st, batch);
  const uchar4* const* imageTab = reinterpret_cast<const uchar4* const*>(tab);
  const uchar4* const* prevImageTab = reinterpret_cast<const uchar4* const*>(tab + N);
  const float2* const* prevFlowTab = reinterpret_cast<const float2* const*>(tab + 2 * N);
  FlowPrepared p;
  p.N = N; p.B = B; p.L = L;
  p.usePrev = usePrev;
  p.outTab = reinterpret_cast<float* const*>(tab + 2 * N + B);
  p.idx.i0 = reinterpret_cast<const int*>(tab + 2 * N + 2 * B);
  p.idx.i1 = p.idx.i0 + B;

  M.down.ensure(N * n0 * sizeof(uchar4));
  M.gray.ensure(N * n0 * sizeof(float));
  M.pyrI.ensure(2 * N * lv_.total * sizeof(float));  // per level: N grey planes, then N alpha planes
  M.G.ensure(N * n0 * sizeof(float2));
  M.flowA.ensure(B * n0 * sizeof(float2));
  M.flowB.ensure(B * n0 * sizeof(float2));
  std::vector<float> divs;
  divs.push_back(0.001f);
  for (int l = 0; l < L; ++l) {
    divs.push_back((float)lv_.w[l]);
    divs.push_back((float)lv_.h[l]);
  }
  p.fast = sweeps_fast(st, divs);
  M.rec.ensure(B * n0 * (sweep_mode_ == 3 ? sizeof(float2) : sizeof(float4)));  // half-records / full records (flow_kernels.hpp)
  // Band hand-off granules + ticket counters of every sweep launch of this call (2 per level): one arena, reset to
  // all-ones ("not written") by ONE memset instead of one per launch.
  // + per level one word per (flow, row): all-ones = no pixel of the row is updated (written by the record kernel)
  p.hoff.assign(L + 1, 0);
  for (int l = 0; l < L; ++l) p.hoff[l + 1] = p.hoff[l] + 2 * handoff_bytes(lv_.w[l], lv_.h[l], B) + rowflag_bytes(lv_.h[l], B);
  M.handoff.ensure(p.hoff[L]);
  S360_HIP(hipMemsetAsync(M.handoff.p, 0xFF, p.hoff[L], st));
  if (!err_.p) {
    err_.ensure(sizeof(unsigned));
    S360_HIP(hipMemsetAsync(err_.p, 0, sizeof(unsigned), st));
  }
  p.pyrI = M.pyrI.as<float>();
  auto LI = [&](int l) { return level_gray(p, l); };
  auto LA = [&](int l) { return level_alpha(p, l); };

  const BlurTaps tPre = gaussian_taps(5, 0.25f);
  {
    ProfScope ps(P, "flow_entry");
    // the downscaled image itself is read again only by k_motion (temporal state): stored only then
    launch_entry_downscale(st, nullptr, w, h, 0, usePrev ? M.down.as<uchar4>() : nullptr, M.down.as<uchar4>(), dw_, dh_, n0, N,
                           imageTab, M.gray.as<float>(), LA(0), n0);
    launch_sepblur(st, M.gray.as<float>(), LI(0), dw_, dh_, 1, n0, N, tPre);
  }
  {
    ProfScope ps(P, "flow_pyramid");
    for (int l = 1; l < L; ++l) {
      const size_t ns = (size_t)lv_.w[l - 1] * lv_.h[l - 1], nd = (size_t)lv_.w[l] * lv_.h[l];
      // grey and alpha planes of a level are adjacent: one launch resizes all 2N planes
      launch_resize_linear_f32(st, LI(l - 1), lv_.w[l - 1], lv_.h[l - 1], ns, LI(l), lv_.w[l], lv_.h[l], nd, 1, 2 * N, 1.f,
                               0);
    }
  }
  if (usePrev) {
    ProfScope ps(P, "flow_prev");
    M.prevdown.ensure(N * n0 * sizeof(uchar4));
    M.prevPyr.ensure(B * lv_.total * sizeof(float2));
    M.motionPyr.ensure(N * lv_.total * sizeof(float));
    float2* prevPyr = p.prevPyr = M.prevPyr.as<float2>();
    float* motionPyr = p.motionPyr = M.motionPyr.as<float>();
    launch_resize_cubic_u8c4(st, nullptr, w, h, 0, M.prevdown.as<uchar4>(), dw_, dh_, n0, N, prevImageTab);
    launch_motion(st, M.down.as<uchar4>(), M.prevdown.as<uchar4>(), n0, n0, motionPyr, n0, N);
    // prevFlowDownscaled = resize(prevFlow) * (rows_down / rows_full)  (PixFlow.h:103-104)
    launch_resize_cubic_f32c2(st, nullptr, w, h, 0, prevPyr, dw_, dh_, n0, B, float(dh_) / float(h), prevFlowTab);
    for (int l = 1; l < L; ++l) {
      const size_t ns = (size_t)lv_.w[l - 1] * lv_.h[l - 1], nd = (size_t)lv_.w[l] * lv_.h[l];
      launch_resize_linear_f32(st, (const float*)(prevPyr + (size_t)B * lv_.off[l - 1]), lv_.w[l - 1], lv_.h[l - 1], ns,
                               (float*)(prevPyr + (size_t)B * lv_.off[l]), lv_.w[l], lv_.h[l], nd, 2, B, 1.f, 0);
      launch_resize_linear_f32(st, motionPyr + (size_t)N * lv_.off[l - 1], lv_.w[l - 1], lv_.h[l - 1], ns,
                               motionPyr + (size_t)N * lv_.off[l], lv_.w[l], lv_.h[l], nd, 1, N, 1.f, 0);
    }
    // (the rescale of the previous flow at each level, PixFlow.h:147-153 — level 0's factor is exactly 1 —, is applied where the
    // level is read: launch_diffusion_adjust)
  }
  return p;
}

void FlowEngine::compute(hipStream_t st, const PixFlowConsts& pc, const FlowBatch& batch, int w, int h, int hint) {
  const FlowPrepared p = prepare(st, pc, batch, w, h);
  const int N = p.N, B = p.B, L = p.L;
  Profiler& P = *prof_;
  FlowBufs& M = *bufs_;
  const BlurTaps tFinal = gaussian_taps(3, 1.0f);
  float2* cur = M.flowA.as<float2>();
  float2* oth = M.flowB.as<float2>();
  const float invPyr = 1.0f / pc.pyrScaleFactor;
  if (capture_levels) capture_levels->clear();
  for (int l = L - 1; l >= 0; --l) {
    const int wl = lv_.w[l], hl = lv_.h[l];
    const size_t nl = (size_t)wl * hl;
    // (the rescale of the previous flow's level, PixFlow.h:147-153, is applied where it is read; level 0's factor is exactly 1)
    FlowLevelArgs a;
    a.w = wl; a.h = hl; a.N = N; a.B = B;
    a.I = level_gray(p, l); a.A = level_alpha(p, l);
    a.idx = p.idx;
    a.cur = cur; a.oth = oth;
    a.first = l == L - 1;
    a.hint = hint;
    a.handoff_fwd = (char*)M.handoff.p + p.hoff[l];
    a.handoff_bwd = (char*)M.handoff.p + p.hoff[l] + handoff_bytes(wl, hl, B);
    a.rowflags = reinterpret_cast<unsigned*>((char*)M.handoff.p + p.hoff[l] + 2 * handoff_bytes(wl, hl, B));
    a.fast = p.fast;
    a.prev = p.usePrev ? p.prevPyr + (size_t)B * lv_.off[l] : nullptr;
    a.motion = p.usePrev ? p.motionPyr + (size_t)N * lv_.off[l] : nullptr;
    a.prev_scale = level_prev_scale(l);
    level(st, pc, a);
    if (capture_levels) {
      std::vector<float> hbuf(B * nl * 2);
      S360_HIP(hipMemcpyAsync(hbuf.data(), oth, hbuf.size() * sizeof(float), hipMemcpyDeviceToHost, st));
      S360_HIP(hipStreamSynchronize(st));
      capture_levels->push_back(std::move(hbuf));
    }
    if (l > 0) {
      ProfScope ps(P, "flow_upscale");
      launch_resize_cubic_f32c2(st, oth, wl, hl, nl, cur, lv_.w[l - 1], lv_.h[l - 1],
                                (size_t)lv_.w[l - 1] * lv_.h[l - 1], B, invPyr);
    } else {
      ProfScope ps(P, "flow_final");
      // final upscale + scalar + 3x3 blur fused: the upscaled flow is evaluated while the blur's tile is loaded
      launch_upscale_blur(st, oth, wl, hl, nl, nullptr, w, h, (size_t)w * h, B, 1.0f / pc.downscaleFactor, tFinal, p.outTab);
    }
  }
}

void FlowEngine::debug_prepare(hipStream_t st, const PixFlowConsts& pc, const FlowBatch& batch, int w, int h, int fill,
                               const FlowPrepareTaps& t) {
  FlowBufs& M = *bufs_;
  const int N = (int)batch.images.size(), B = (int)batch.out.size();
  const int dw = int(w * pc.downscaleFactor), dh = int(h * pc.downscaleFactor);
  if (fill >= 0 && dw >= 2 && dh >= 2 && N >= 1 && B >= 1) {  // every buffer the preparation writes holds `fill` before it runs
    FlowLevels lv;
    lv.build(dw, dh, pc.pyrScaleFactor);
    const size_t n0 = (size_t)dw * dh;
    const bool usePrev = !batch.prev_flow.empty();
    struct { DevBuf* b; size_t bytes; } bufs[] = {{&M.down, N * n0 * sizeof(uchar4)}, {&M.gray, N * n0 * sizeof(float)},
                                                  {&M.pyrI, 2 * N * lv.total * sizeof(float)}, {&M.prevdown, N * n0 * sizeof(uchar4)},
                                                  {&M.prevPyr, B * lv.total * sizeof(float2)}, {&M.motionPyr, N * lv.total * sizeof(float)}};
    for (int k = 0; k < (usePrev ? 6 : 3); ++k) {
      bufs[k].b->ensure(bufs[k].bytes);
      S360_HIP(hipMemsetAsync(bufs[k].b->p, fill, bufs[k].b->cap, st));
    }
  }
  const FlowPrepared p = prepare(st, pc, batch, w, h);
  S360_HIP(hipStreamSynchronize(st));
  if (p.L > t.cap_levels || lv_.total > t.cap_pixels) throw Error(-1, "FlowEngine: the tap's buffers are too small for this pyramid");
  auto grab = [&](void* host, const void* dev, size_t bytes) {
    if (host) S360_HIP(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  };
  for (int l = 0; l < p.L; ++l) {
    if (t.level_w) t.level_w[l] = lv_.w[l];
    if (t.level_h) t.level_h[l] = lv_.h[l];
    if (t.factors) t.factors[l] = level_prev_scale(l);
  }
  if (t.n_levels) *t.n_levels = p.L;
  grab(t.pyr_images, p.pyrI, 2 * (size_t)N * lv_.total * sizeof(float));
  if (p.usePrev) {
    grab(t.prev_pyr, p.prevPyr, (size_t)B * lv_.total * sizeof(float2));
    grab(t.motion_pyr, p.motionPyr, (size_t)N * lv_.total * sizeof(float));
  }
}

size_t FlowEngine::handoff_bytes(int w, int h, int B) const {
  const size_t b = sweep_mode_ == 3 ? sweep_quad_handoff_bytes(w, h, B) : sweep_lock_handoff_bytes(w, h, B, sweep_lock_waves());
  return (b + 255) & ~(size_t)255;
}

bool FlowEngine::sweeps_fast(hipStream_t st, const std::vector<float>& divisors) {
  if (sweep_fast_ < 0) {
    const char* d = std::getenv("S360_SWEEP_DIV");  // "ieee": IEEE division / sqrt expansions instead of the verified fast ones (same bits)
    sweep_fast_ = !(d && std::string(d) == "ieee");
  }
  return sweep_fast_ ? sweep_verify_divisors(st, divisors) : false;
}

void FlowEngine::level(hipStream_t st, const PixFlowConsts& pc, const FlowLevelArgs& a, const FlowLevelTaps* tap) {
  Profiler& P = *prof_;
  FlowBufs& M = *bufs_;
  const int wl = a.w, hl = a.h, N = a.N, B = a.B;
  const size_t nl = (size_t)wl * hl;
  float2* const cur = a.cur;
  float2* const oth = a.oth;
  // (tests only) what a launch has left, copied to the host before the next one overwrites it
  auto grab = [&](void* host, const void* dev, size_t bytes) {
    if (!tap || !host) return;
    S360_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    S360_HIP(hipStreamSynchronize(st));
  };
  const size_t flowBytes = (size_t)B * nl * sizeof(float2);
  {
    ProfScope ps(P, "flow_gradients");
    launch_gradients(st, a.I, M.G.as<float2>(), wl, hl, nl, N, tGrad_);
  }
  if (tap) grab(tap->gradients, M.G.p, (size_t)N * nl * sizeof(float2));
  if (a.first) {
    S360_HIP(hipMemsetAsync(cur, 0, B * nl * sizeof(float2), st));
    if (pc.maxPercentage > 0 && a.hint != 0) {
      ProfScope ps(P, "flow_search_init");
      M.I1eq.ensure(B * nl * sizeof(float));
      const int dist = (24 * pc.maxPercentage + 50) / 100;
      launch_search_init(st, a.I, a.A, wl, hl, nl, B, a.idx, cur, a.hint, dist, M.I1eq.as<float>());
    }
  }
  if (tap) grab(tap->initial_flow, cur, flowBytes);
  {
    ProfScope ps(P, "flow_blur15");  // the blurred flow goes straight into the sweeps' half-records
    launch_blur_to_records(st, cur, M.rec.p, wl, hl, nl, B, tFlow_, sweep_mode_ == 3 ? nullptr : M.G.as<float2>(), a.A, a.idx,
                           a.rowflags);
  }
  if (tap && (tap->blurred_flow || tap->updated)) {  // the records decoded: both formats mark a pixel that is not updated with a NaN first word
    const size_t words = sweep_mode_ == 3 ? 2 : 4;
    std::vector<float> rec((size_t)B * nl * words);
    grab(rec.data(), M.rec.p, rec.size() * sizeof(float));
    for (size_t i = 0; i < (size_t)B * nl; ++i) {
      const float* r = &rec[i * words];
      if (tap->updated) tap->updated[i] = r[0] == r[0] ? 1 : 0;
      if (tap->blurred_flow) {
        tap->blurred_flow[2 * i] = r[words - 2];
        tap->blurred_flow[2 * i + 1] = r[words - 1];
      }
    }
  }
  if (tap) grab(tap->row_flags, a.rowflags, (size_t)B * hl * sizeof(unsigned));
  auto sweep = [&](float2* fl, int dir) {
    ProfScope ps(P, "flow_sweep");
    void* ho = dir > 0 ? a.handoff_fwd : a.handoff_bwd;
    if (sweep_mode_ == 3)
      launch_sweep_quad(st, M.rec.as<float2>(), M.G.as<float2>(), fl, ho, err_.as<unsigned>(), wl, hl, nl, B, a.idx, dir, pc,
                        a.fast, a.rowflags);
    else
      launch_sweep_lock(st, M.rec.as<float4>(), M.G.as<float2>(), fl, ho, err_.as<unsigned>(), wl, hl, nl, B, a.idx, dir, pc,
                        a.fast);
  };
  sweep(cur, +1);
  if (tap) grab(tap->sweep_forward, cur, flowBytes);
  {
    ProfScope ps(P, "flow_median");
    launch_median5_c2(st, cur, oth, wl, hl, nl, B);
  }
  if (tap) grab(tap->median_first, oth, flowBytes);
  sweep(oth, -1);
  if (tap) grab(tap->sweep_backward, oth, flowBytes);
  {
    ProfScope ps(P, "flow_median");
    launch_median5_c2(st, oth, cur, wl, hl, nl, B);
  }
  if (tap) grab(tap->median_second, cur, flowBytes);
  {
    ProfScope ps(P, "flow_diffusion");
    if (a.prev)  // ... and adjustFlowTowardPrevious in the same pass (the previous flow's level rescaled as it is read)
      launch_diffusion_adjust(st, cur, oth, wl, hl, nl, B, tFlow_, a.A, a.idx, a.prev, a.motion, a.prev_scale);
    else
      launch_diffusion(st, cur, oth, wl, hl, nl, B, tFlow_, a.A, a.idx);
  }
  if (tap) {
    if (!a.prev) grab(tap->diffused, oth, flowBytes);
    grab(tap->final_flow, oth, flowBytes);
  }
}

void FlowEngine::debug_level(hipStream_t st, const PixFlowConsts& pc, int N, int B, int w, int h, const float* gray,
                             const float* alpha, const int* i0, const int* i1, const float* init, int hint, const float* prev,
                             const float* motion, float prev_scale, const FlowLevelTaps& taps, int* info) {
  if (w < 2 || h < 2 || N < 1 || B < 1 || B > kMaxFlows) throw Error(-1, "FlowEngine: bad level");
  if ((prev != nullptr) != (motion != nullptr)) throw Error(-1, "FlowEngine: previous-frame state must be complete or absent");
  if (prev && taps.diffused) throw Error(-1, "FlowEngine: with previous state the diffusion and the adjustment are one launch");
  FlowBatch fb;  // the index arrays take the way of a batch's: the pointer tables of this one stay unused
  fb.images.assign(N, nullptr);
  for (int b = 0; b < B; ++b) {
    if (i0[b] < 0 || i0[b] >= N || i1[b] < 0 || i1[b] >= N) throw Error(-1, "FlowEngine: image index out of range");
    fb.add_flow(i0[b], i1[b], nullptr);
  }
  FlowBufs& M = *bufs_;
  const size_t nl = (size_t)w * h;
  const unsigned long long* tab = batch_tables(st, fb);
  FlowLevelArgs a;
  a.w = w; a.h = h; a.N = N; a.B = B;
  a.idx.i0 = reinterpret_cast<const int*>(tab + 2 * N + 2 * B);
  a.idx.i1 = a.idx.i0 + B;
  M.pyrI.ensure(2 * N * nl * sizeof(float));  // N grey planes, then N alpha planes, as a level of the pyramid lies
  M.G.ensure(N * nl * sizeof(float2));
  M.flowA.ensure(B * nl * sizeof(float2));
  M.flowB.ensure(B * nl * sizeof(float2));
  M.rec.ensure(B * nl * (sweep_mode_ == 3 ? sizeof(float2) : sizeof(float4)));
  const size_t hb = handoff_bytes(w, h, B);
  M.handoff.ensure(2 * hb + rowflag_bytes(h, B));
  S360_HIP(hipMemsetAsync(M.handoff.p, 0xFF, 2 * hb + rowflag_bytes(h, B), st));
  if (!err_.p) {
    err_.ensure(sizeof(unsigned));
    S360_HIP(hipMemsetAsync(err_.p, 0, sizeof(unsigned), st));
  }
  float* I = M.pyrI.as<float>();
  S360_HIP(hipMemcpyAsync(I, gray, N * nl * sizeof(float), hipMemcpyHostToDevice, st));
  S360_HIP(hipMemcpyAsync(I + N * nl, alpha, N * nl * sizeof(float), hipMemcpyHostToDevice, st));
  a.I = I;
  a.A = I + N * nl;
  a.cur = M.flowA.as<float2>();
  a.oth = M.flowB.as<float2>();
  a.first = init == nullptr;
  if (init) S360_HIP(hipMemcpyAsync(a.cur, init, B * nl * sizeof(float2), hipMemcpyHostToDevice, st));
  a.hint = hint;
  a.handoff_fwd = M.handoff.p;
  a.handoff_bwd = (char*)M.handoff.p + hb;
  a.rowflags = reinterpret_cast<unsigned*>((char*)M.handoff.p + 2 * hb);
  a.fast = sweeps_fast(st, {0.001f, (float)w, (float)h});
  a.prev = nullptr;
  a.motion = nullptr;
  a.prev_scale = prev_scale;
  if (prev) {
    M.prevPyr.ensure(B * nl * sizeof(float2));
    M.motionPyr.ensure(N * nl * sizeof(float));
    S360_HIP(hipMemcpyAsync(M.prevPyr.p, prev, B * nl * sizeof(float2), hipMemcpyHostToDevice, st));
    S360_HIP(hipMemcpyAsync(M.motionPyr.p, motion, N * nl * sizeof(float), hipMemcpyHostToDevice, st));
    a.prev = M.prevPyr.as<float2>();
    a.motion = M.motionPyr.as<float>();
  }
  S360_HIP(hipStreamSynchronize(st));  // (the caller's buffers are pageable: the copies have read them by now)
  level(st, pc, a, &taps);
  S360_HIP(hipStreamSynchronize(st));
  if (info) {
    std::memset(info, 0, kFlowLevelInfoCount * sizeof(int));
    if (sweep_mode_ == 3) {
      info[0] = sweep_quad_lanes_per_pixel(h, B);
      info[1] = sweep_quad_num_bands(h, B);
      info[2] = sweep_quad_waves(h, B);
    } else {
      info[1] = sweep_lock_num_wgs(h, sweep_lock_waves());
      info[2] = info[1] * B * (sweep_lock_waves() + 2);
    }
    info[3] = a.fast ? 1 : 0;
    info[4] = median5_tile_bx(w, h);
    info[5] = (int)take_error(st);
  }
}

unsigned FlowEngine::take_error(hipStream_t st) {
  if (!err_.p) return 0;
  unsigned v = 0;
  S360_HIP(hipMemcpyAsync(&v, err_.p, sizeof(v), hipMemcpyDeviceToHost, st));
  S360_HIP(hipStreamSynchronize(st));
  if (v) S360_HIP(hipMemsetAsync(err_.p, 0, sizeof(unsigned), st));
  return v;
}

}  // namespace s360
