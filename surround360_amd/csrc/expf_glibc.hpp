// expf_glibc.hpp — expf as glibc 2.35 computes it on x86-64 with FMA (sysdeps/ieee754/flt-32/e_expf.c through the
// multiarch FMA build): double arithmetic, 32-entry 2^(i/32) table, cubic in double, with the contractions gcc -mfma
// makes. Shared by the ISP's noise coring (isp_kernels.hip: arguments <= 0) and the preview's alpha softmax (preview.hip:
// arguments from a little below 0 to a little above softmax_coef). tools/expf_check.c compares this sequence with the
// host's expf for every float <= 0 (2 139 095 041 values) and for every float in [0, 88.8] (the overflow threshold,
// 0x1.62e42ep6 = 88.72..., lies inside): no difference. The table is built on the host with exp2().
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

namespace s360 {

// 2^(i/32) bit patterns minus i << 47 (the table of glibc's expf), for upload
inline void expf_glibc_table(unsigned long long tab[32]) {
  for (int i = 0; i < 32; ++i) {
    const double v = exp2((double)i / 32);
    unsigned long long u;
    std::memcpy(&u, &v, 8);
    tab[i] = u - ((unsigned long long)i << 47);
  }
}

__device__ __forceinline__ float expf_glibc(float x, const unsigned long long* __restrict__ tab) {
  const unsigned ux = __float_as_uint(x);
  const unsigned abstop = (ux >> 20) & 0x7ff;
  if (abstop >= (0x42b00000u >> 20)) {  // |x| >= 88 or NaN
    if (ux == 0xff800000u) return 0.0f;
    if (abstop >= (0x7f800000u >> 20)) return x + x;
    if (x > 0x1.62e42ep6f) return __uint_as_float(0x7f800000u);  // __math_oflowf
    if (x < -0x1.9fe368p6f) return 0.0f;      // underflow
    if (x < -0x1.9d1d9ep6f) return 0x1p-149f;  // __math_may_uflowf
  }
  const double kInvLn2N = 0x1.71547652b82fep+0 * 32, kShift = 0x1.8p+52;
  const double C0 = 0x1.c6af84b912394p-5 / 32 / 32 / 32, C1 = 0x1.ebfce50fac4f3p-3 / 32 / 32, C2 = 0x1.62e42ff0c52d6p-1 / 32;
  const double xd = (double)x;
  double kd = __builtin_fma(kInvLn2N, xd, kShift);
  const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
  kd -= kShift;
  const double r = __builtin_fma(kInvLn2N, xd, -kd);
  const unsigned long long t = tab[ki & 31] + (ki << (52 - 5));
  const double s = __longlong_as_double((long long)t);
  const double z = __builtin_fma(C0, r, C1);
  const double r2 = r * r;
  double y = __builtin_fma(C2, r, 1.0);
  y = __builtin_fma(z, r2, y);
  y = y * s;
  return (float)y;
}

}  // namespace s360
