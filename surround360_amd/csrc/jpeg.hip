// jpeg.hip — baseline JPEG on gfx950 (include/s360_jpeg.h, jpeg.hpp): the file host/jpeg_io.hpp's jpegio::encode writes, byte
// for byte, from a B,G,R image in device memory. The host writer is the specification; every rule here is read from it.
//
//   k_jpeg_blocks          4 MCUs of 16 x 16 pixels per workgroup, 8 threads per block: colour conversion with libjpeg's 16-bit
//                          fixed-point constants, h2v2 chroma with the alternating bias, edges replicated by clamping the source
//                          coordinates, the "islow" DCT (rows, LDS, columns) in 32-bit integers, quantisation; dummy Y blocks take
//                          the DC of the block before them -> 6 x 64 int16 per MCU in emission order
//   k_jpeg_entropy<false>  one wave per block, lane k = zigzag position k: __ballot of "non-zero" gives every lane its zero run,
//                          from it ZRL codes, symbol, code and extra bits (at most 59 bits a lane); a wave prefix sum gives the
//                          block's bit length
//   k_scan_*               exclusive scan over the blocks' bit lengths in three separate kernels (per-group totals, one group
//                          scans the totals, apply): no workgroup ever waits for another
//   k_jpeg_entropy<true>   the same codes again, ORed into a tile in LDS at the block's bit offset, then into the zeroed word
//                          buffer: whole words inside the block are stored, the first and the last — shared with the neighbours —
//                          are atomicOr'ed. Bit 0 of the stream is the most significant bit of word 0
//   k_jpeg_stuff_count /   the last partial byte filled with 1-bits, then 0x00 after every 0xFF: count per tile of 4096 bytes,
//   k_scan_* / _scatter    the same scan, scatter
//
// Everything is enqueued on the caller's stream, the memset of the word buffer included; nothing synchronises. The encoder's own
// buffers are sized for the worst case (1660 bits a block, doubled by stuffing) and every store is bounds-checked besides. The
// caller's scan buffer may be smaller (encode(.., capped): a frame slot's, render.hip): the stuffed size is known from the tile
// scan before k_jpeg_stuff_scatter runs, which then stores the whole scan or, when it does not fit, nothing; count[0] tells.
//
// Sizes: 8192 x 8192 (a frame slot's stereo equirect) is 262 144 MCUs, 1 572 864 blocks: 65 536 workgroups of k_jpeg_blocks,
// 393 216 of k_jpeg_entropy (x 256 threads: below 2^32 work-items), 1536 scan groups, at most 79 680 stream tiles; bit offsets
// reach 2.6e9 in the worst case and are unsigned 32-bit in every kernel (blk, off[], nbits, base and i of the stuffing kernels;
// byte offsets into out[] are size_t). JPEG_MAX_MCUS keeps all of them below 2^32.
//
// gfx950, VGPRs / SGPRs / LDS bytes (no scratch, no spills): k_jpeg_blocks 50/97/6240, k_jpeg_entropy<false> 11/28/0, <true>
// 15/30/896, k_scan_totals 8/14/1024, k_scan_groups 18/32/1024, k_scan_apply 10/22/1024, k_jpeg_stuff_count 5/19/1024,
// k_jpeg_stuff_scatter 24/24/1024.
#include "jpeg.hpp"

#include <cstring>
#include <vector>

#include "../../include/s360_debug_jpeg.h"
#include "../../include/s360_jpeg.h"
#include "api_guard.hpp"
#include "devmath.hpp"

namespace s360 {
namespace {

// ---- the standard tables (ITU-T T.81 Annex K, as jcparam.c holds them) ------------------------------------------------
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t kLumQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40, 57,
                           69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                           81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
const uint8_t kChrQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                           99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// what the kernels read; every entry a dword
struct JpegTab {
  uint32_t ac[2][256];  // length << 16 | code, per symbol (EncTable of the host writer; jchuff.c: jpeg_make_c_derived_tbl)
  uint32_t dc[2][16];
  uint32_t qdiv[2][64];  // q << 3, natural order
  uint32_t zz[64];
};
void huff_table(const uint8_t* bits, const uint8_t* vals, uint32_t* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = 0;
  unsigned c = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k) out[vals[k]] = (uint32_t)l << 16 | (c++ & 0xFFFFu);
    c <<= 1;
  }
}

// ---- blocks ---------------------------------------------------------------------------------------------------------
constexpr int JB_MCUS = 4, JB_THREADS = JB_MCUS * 48, JB_LD = 65;  // 8 threads per block; the LDS stride of a block, padded

// one pass of jpeg_fdct_islow (jfdctint.c) over 8 values, in the host writer's operation order; 32-bit integers suffice: with
// samples in -128..127 no product sum exceeds 1.6e9 in magnitude (the odd part of the column pass is the largest)
template <bool ROWS>
__device__ __forceinline__ void fdct_islow_1d(int* d) {
  constexpr int CB = 13, P1 = 2, SH = ROWS ? CB - P1 : CB + P1;
  constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (ROWS) {
    d[0] = (t10 + t11) * (1 << P1);
    d[4] = (t10 - t11) * (1 << P1);
  } else {
    d[0] = (t10 + t11 + (1 << (P1 - 1))) >> P1;
    d[4] = (t10 - t11 + (1 << (P1 - 1))) >> P1;
  }
  constexpr int RND = 1 << (SH - 1);
  int z1 = (t12 + t13) * F0541;
  d[2] = (z1 + t13 * F0765 + RND) >> SH;
  d[6] = (z1 + t12 * (-F1847) + RND) >> SH;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F1175;
  const int m4 = t4 * F0298, m5 = t5 * F2053, m6 = t6 * F3072, m7 = t7 * F1501;
  z1 *= -F0899;
  z2 *= -F2562;
  z3 *= -F1961;
  z4 *= -F0390;
  z3 += z5;
  z4 += z5;
  d[7] = (m4 + z1 + z3 + RND) >> SH;
  d[5] = (m5 + z2 + z4 + RND) >> SH;
  d[3] = (m6 + z2 + z3 + RND) >> SH;
  d[1] = (m7 + z1 + z4 + RND) >> SH;
}

// rgb_ycc_convert (jccolor.c): FIX(x) = (long)(x * 65536 + 0.5)
__device__ __forceinline__ int ycc_y(int b, int g, int r) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int ycc_cb(int b, int g, int r) { return (-11059 * r - 21709 * g + 32768 * b + ((128 << 16) + 32767)) >> 16; }
__device__ __forceinline__ int ycc_cr(int b, int g, int r) { return (32768 * r - 27439 * g - 5329 * b + ((128 << 16) + 32767)) >> 16; }

__global__ __launch_bounds__(JB_THREADS) void k_jpeg_blocks(const unsigned char* __restrict__ bgr, int w, int h, int mcux, int nmcu,
                                                            const JpegTab* __restrict__ tab, short* __restrict__ coef) {
  __shared__ int s[JB_MCUS * 6 * JB_LD];
  const int t = threadIdx.x, m = t / 48, b = (t % 48) >> 3, k = t & 7;
  const int mcu = (int)blockIdx.x * JB_MCUS + m;
  const int ybw = (w + 7) >> 3, ybh = (h + 7) >> 3, ch = (h + 1) >> 1;
  int* sb = s + (m * 6 + b) * JB_LD;
  int d[8];
  if (mcu < nmcu) {
    const int mx = mcu % mcux, my = mcu / mcux;
    if (b < 4) {  // Y: row k of the block; pixel (min(x, w - 1), min(y, h - 1))
      const int y = min(my * 16 + (b >> 1) * 8 + k, h - 1), x0 = mx * 16 + (b & 1) * 8;
      const unsigned char* row = bgr + (size_t)y * w * 3;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const unsigned char* p = row + (size_t)min(x0 + c, w - 1) * 3;
        d[c] = ycc_y(p[0], p[1], p[2]) - 128;
      }
    } else {  // chroma: h2v2_downsample of the full-resolution plane, whose right edge and bottom row are replicated
      const int cy = min(my * 8 + k, ch - 1);
      const unsigned char* r0 = bgr + (size_t)min(2 * cy, h - 1) * w * 3;
      const unsigned char* r1 = bgr + (size_t)min(2 * cy + 1, h - 1) * w * 3;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int xa = min(mx * 16 + 2 * c, w - 1) * 3, xb = min(mx * 16 + 2 * c + 1, w - 1) * 3;
        int sum = (c & 1) ? 2 : 1;
        if (b == 4) sum += ycc_cb(r0[xa], r0[xa + 1], r0[xa + 2]) + ycc_cb(r0[xb], r0[xb + 1], r0[xb + 2]) +
                           ycc_cb(r1[xa], r1[xa + 1], r1[xa + 2]) + ycc_cb(r1[xb], r1[xb + 1], r1[xb + 2]);
        else sum += ycc_cr(r0[xa], r0[xa + 1], r0[xa + 2]) + ycc_cr(r0[xb], r0[xb + 1], r0[xb + 2]) +
                    ycc_cr(r1[xa], r1[xa + 1], r1[xa + 2]) + ycc_cr(r1[xb], r1[xb + 1], r1[xb + 2]);
        d[c] = (sum >> 2) - 128;
      }
    }
    fdct_islow_1d<true>(d);
#pragma unroll
    for (int c = 0; c < 8; ++c) sb[k * 8 + c] = d[c];
  }
  __syncthreads();
  if (mcu < nmcu) {  // column k; forward_DCT's quantisation (jcdctmgr.c): half the divisor added to the magnitude, truncation
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = sb[r * 8 + k];
    fdct_islow_1d<false>(d);
    const uint32_t* qd = tab->qdiv[b < 4 ? 0 : 1];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const unsigned qv = qd[r * 8 + k];
      const int v = d[r];
      unsigned a = (unsigned)(v < 0 ? -v : v) + (qv >> 1);
      a = a >= qv ? a / qv : 0u;
      sb[r * 8 + k] = v < 0 ? -(int)a : (int)a;
    }
  }
  __syncthreads();
  // emission order Y00 Y01 Y10 Y11 Cb Cr. A Y block at or past the last block column / row is a dummy: zero AC, the DC of the
  // block emitted before it (jccoefct.c) — always a Y block of the same MCU, Y00 is never a dummy
  for (int i = t; i < JB_MCUS * 6 * 64; i += JB_THREADS) {
    const int bl = i >> 6, pos = i & 63, m2 = bl / 6, b2 = bl % 6, mcu2 = (int)blockIdx.x * JB_MCUS + m2;
    if (mcu2 >= nmcu) break;
    const int mx = mcu2 % mcux, my = mcu2 / mcux;
    int src = b2;
    if (b2 < 4)
      while (src > 0 && !(mx * 2 + (src & 1) < ybw && my * 2 + (src >> 1) < ybh)) --src;
    const int v = src == b2 ? s[bl * JB_LD + pos] : pos == 0 ? s[(m2 * 6 + src) * JB_LD] : 0;
    coef[((size_t)mcu2 * 6 + b2) * 64 + pos] = (short)v;
  }
}

// ---- entropy coding -------------------------------------------------------------------------------------------------
constexpr int JE_WAVES = 4, JE_TILE = 56;  // tile: 31 bits of the word the block starts in + 1660 bits = 53 words
static_assert((31 + JPEG_MAX_BLOCK_BITS + 31) / 32 <= JE_TILE - 2 && JE_TILE <= 64, "the entropy kernel's tile");

__device__ __forceinline__ int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// WRITE false: bits[blk] = the block's bit length. true: the block's bits ORed into words[] at bit offset off[blk].
template <bool WRITE>
__global__ __launch_bounds__(JE_WAVES * 64) void k_jpeg_entropy(const short* __restrict__ coef, unsigned nblk,
                                                                const JpegTab* __restrict__ tab, unsigned* __restrict__ bits,
                                                                const unsigned* __restrict__ off, unsigned* __restrict__ words,
                                                                unsigned nwords) {
  __shared__ unsigned tile[JE_WAVES][JE_TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned blk = blockIdx.x * JE_WAVES + wv;
  const bool valid = blk < nblk;  // (wave-uniform; every wave reaches every barrier)
  const unsigned b = blk % 6, mcu = blk / 6;
  const int t = b < 4 ? 0 : 1;
  int v = valid ? (int)coef[(size_t)blk * 64 + tab->zz[lane]] : 0;
  if (lane == 0 && valid) {  // DC: the difference to the block before OF THE SAME COMPONENT in emission order, 0 for the first
    int prev = 0;
    if (b >= 1 && b <= 3) prev = coef[(size_t)(blk - 1) * 64];
    else if (mcu > 0) prev = coef[(size_t)(blk - (b == 0 ? 3 : 6)) * 64];
    v -= prev;
  }
  const unsigned long long nzmask = __ballot(lane > 0 && v != 0);
  unsigned long long code = 0;
  int len = 0;
  const int nb = bit_length((unsigned)(v < 0 ? -v : v));
  const unsigned extra = (unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u);
  if (valid) {
    if (lane == 0) {
      const unsigned e = tab->dc[t][nb & 15];
      code = (unsigned long long)(e & 0xFFFFu) << nb | extra;
      len = (int)(e >> 16) + nb;
    } else if (v != 0) {
      const unsigned long long below = nzmask & ((1ull << lane) - 1ull);
      const int last = below ? 63 - __builtin_clzll(below) : 0;  // the non-zero position before this one (0: the DC)
      const int run = lane - last - 1;
      const unsigned zrl = tab->ac[t][0xF0], e = tab->ac[t][((run & 15) << 4 | nb) & 255];
      for (int i = 0; i < (run >> 4); ++i) {
        code = code << (zrl >> 16) | (zrl & 0xFFFFu);
        len += (int)(zrl >> 16);
      }
      code = (code << (e >> 16) | (e & 0xFFFFu)) << nb | extra;
      len += (int)(e >> 16) + nb;
    } else if (lane == 63) {  // a zero in the last position: the run at the end is not empty, EOB
      const unsigned e = tab->ac[t][0];
      code = e & 0xFFFFu;
      len = (int)(e >> 16);
    }
  }
  // inclusive prefix sum of the lengths over the wave
  int incl = len;
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const int o = __builtin_amdgcn_ds_bpermute(((lane - dlt) & 63) << 2, incl);
    if (lane >= dlt) incl += o;
  }
  const int total = __builtin_amdgcn_readlane(incl, 63);
  if (!WRITE) {
    if (valid && lane == 0) bits[blk] = (unsigned)total;
    return;
  }
  const unsigned o0 = valid ? off[blk] : 0u;
  const int s0 = (int)(o0 & 31u);
  if (lane < JE_TILE) tile[wv][lane] = 0u;
  __syncthreads();
  if (len > 0) {
    const unsigned long long V = code << (64 - len);  // left-aligned
    const unsigned hi = (unsigned)(V >> 32), lo = (unsigned)V;
    const int pos = s0 + incl - len, wi = pos >> 5, sh = pos & 31;
    const unsigned w0 = hi >> sh, w1 = sh ? (hi << (32 - sh)) | (lo >> sh) : lo, w2 = sh ? lo << (32 - sh) : 0u;
    if (w0) atomicOr(&tile[wv][wi], w0);
    if (w1) atomicOr(&tile[wv][wi + 1], w1);
    if (w2) atomicOr(&tile[wv][wi + 2], w2);
  }
  __syncthreads();
  const int nw = valid ? (s0 + total + 31) >> 5 : 0;
  if (lane < nw) {
    const size_t gi = (size_t)(o0 >> 5) + lane;
    if (gi < nwords) {
      const unsigned x = tile[wv][lane];
      if (lane == 0 || lane == nw - 1) {
        if (x) atomicOr(&words[gi], x);
      } else {
        words[gi] = x;
      }
    }
  }
}

// ---- exclusive scan of n dwords in three kernels -----------------------------------------------------------------------
constexpr int SC_THREADS = 256, SC_PER = JPEG_SCAN_ITEMS / SC_THREADS;

// exclusive prefix of v over the workgroup (Hillis-Steele in LDS); *total: the sum
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned* sh, unsigned* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < SC_THREADS; d <<= 1) {
    const unsigned a = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const unsigned incl = sh[t];
  *total = sh[SC_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(SC_THREADS) void k_scan_totals(const unsigned* __restrict__ in, unsigned n, unsigned* __restrict__ tot) {
  __shared__ unsigned sh[SC_THREADS];
  const unsigned base = blockIdx.x * JPEG_SCAN_ITEMS + threadIdx.x * SC_PER;
  unsigned v = 0;
#pragma unroll
  for (int i = 0; i < SC_PER; ++i)
    if (base + i < n) v += in[base + i];
  unsigned total;
  (void)block_exclusive(v, sh, &total);
  if (threadIdx.x == 0) tot[blockIdx.x] = total;
}
// one workgroup: tot[0..ng) -> exclusive offsets, *sum = the total
__global__ __launch_bounds__(SC_THREADS) void k_scan_groups(const unsigned* __restrict__ tot, unsigned ng, unsigned* __restrict__ goff,
                                                            unsigned* __restrict__ sum) {
  __shared__ unsigned sh[SC_THREADS];
  unsigned carry = 0;
  for (unsigned base = 0; base < ng; base += SC_THREADS) {
    const unsigned i = base + threadIdx.x, v = i < ng ? tot[i] : 0u;
    unsigned total;
    const unsigned ex = block_exclusive(v, sh, &total);
    if (i < ng) goff[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *sum = carry;
}
__global__ __launch_bounds__(SC_THREADS) void k_scan_apply(const unsigned* __restrict__ in, unsigned n, const unsigned* __restrict__ goff,
                                                           unsigned* __restrict__ out) {
  __shared__ unsigned sh[SC_THREADS];
  const unsigned base = blockIdx.x * JPEG_SCAN_ITEMS + threadIdx.x * SC_PER;
  unsigned x[SC_PER], v = 0;
#pragma unroll
  for (int i = 0; i < SC_PER; ++i) {
    x[i] = base + i < n ? in[base + i] : 0u;
    v += x[i];
  }
  unsigned total;
  unsigned run = goff[blockIdx.x] + block_exclusive(v, sh, &total);
#pragma unroll
  for (int i = 0; i < SC_PER; ++i) {
    if (base + i < n) out[base + i] = run;
    run += x[i];
  }
}

// ---- byte stuffing ----------------------------------------------------------------------------------------------------
constexpr int ST_THREADS = 256, ST_PER = JPEG_STUFF_TILE / ST_THREADS;
static_assert(ST_THREADS == SC_THREADS && ST_PER % 4 == 0, "the stuffing kernels use the scan's workgroup prefix");

// byte i of the stream, the last partial byte filled with 1-bits (i < the stream's byte count)
__device__ __forceinline__ unsigned stream_byte(const unsigned* __restrict__ words, unsigned i, unsigned nbits) {
  unsigned b = (words[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu;
  if ((nbits & 7u) && i == (nbits >> 3)) b |= (1u << (8 - (nbits & 7u))) - 1u;
  return b;
}
__global__ __launch_bounds__(ST_THREADS) void k_jpeg_stuff_count(const unsigned* __restrict__ words, const unsigned* __restrict__ nbitsp,
                                                                 unsigned* __restrict__ cnt) {
  __shared__ unsigned sh[ST_THREADS];
  const unsigned nbits = *nbitsp, nbytes = (nbits + 7) >> 3;
  const unsigned base = blockIdx.x * JPEG_STUFF_TILE + threadIdx.x * ST_PER;
  unsigned c = 0;
  for (int i = 0; i < ST_PER; ++i)
    if (base + i < nbytes) c += stream_byte(words, base + i, nbits) == 0xFFu;
  unsigned total;
  (void)block_exclusive(c, sh, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;  // (0 for the tiles past the end of the stream)
}
__global__ __launch_bounds__(ST_THREADS) void k_jpeg_stuff_scatter(const unsigned* __restrict__ words, const unsigned* __restrict__ nbitsp,
                                                                   const unsigned* __restrict__ toff, const unsigned* __restrict__ nff,
                                                                   unsigned char* __restrict__ out, size_t cap,
                                                                   unsigned* __restrict__ count) {
  __shared__ unsigned sh[ST_THREADS];
  const unsigned nbits = *nbitsp, nbytes = (nbits + 7) >> 3;
  const unsigned stuffed = nbytes + *nff;  // (at most twice 326 MB: 32 bits hold it)
  if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = stuffed;
  if (stuffed > cap) return;  // a scan that does not fit is not stored at all; count[0] > cap tells (uniform over the grid)
  const unsigned base = blockIdx.x * JPEG_STUFF_TILE + threadIdx.x * ST_PER;
  if (blockIdx.x * (unsigned)JPEG_STUFF_TILE >= nbytes) return;  // (uniform over the workgroup)
  unsigned x[ST_PER], c = 0;
  for (int i = 0; i < ST_PER; ++i) {
    x[i] = base + i < nbytes ? stream_byte(words, base + i, nbits) : 0u;
    c += x[i] == 0xFFu;
  }
  unsigned total;
  size_t o = (size_t)base + toff[blockIdx.x] + block_exclusive(c, sh, &total);
  for (int i = 0; i < ST_PER; ++i) {
    if (base + i >= nbytes) break;
    if (o < cap) out[o] = (unsigned char)x[i];
    ++o;
    if (x[i] == 0xFFu) {
      if (o < cap) out[o] = 0;
      ++o;
    }
  }
}

inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

void scan(const unsigned* in, unsigned n, unsigned* gtot, unsigned* goff, unsigned* out, unsigned* sum, hipStream_t st) {
  const unsigned ng = cdiv(n, JPEG_SCAN_ITEMS);
  hipLaunchKernelGGL(k_scan_totals, dim3(ng), dim3(SC_THREADS), 0, st, in, n, gtot);
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(SC_THREADS), 0, st, (const unsigned*)gtot, ng, goff, sum);
  hipLaunchKernelGGL(k_scan_apply, dim3(ng), dim3(SC_THREADS), 0, st, in, n, (const unsigned*)goff, out);
}

}  // namespace

void JpegEncoder::init(int max_w, int max_h, int quality_, hipStream_t st) {
  if (!jpeg_size_ok(max_w, max_h)) throw Error(S360_ERR_INVALID_ARG, "jpeg: image size outside 1..65535 or more than 431 220 MCUs of 16 x 16 pixels");
  init_mcus(jpeg_mcus(max_w, max_h), quality_, st);
  maxW = max_w;
  maxH = max_h;
}
void JpegEncoder::init_mcus(long long max_mcus, int quality_, hipStream_t st) {
  if (max_mcus < 1 || max_mcus > JPEG_MAX_MCUS) throw Error(S360_ERR_INVALID_ARG, "jpeg: more than 431 220 MCUs of 16 x 16 pixels");
  maxW = maxH = 65535;
  maxMcus = max_mcus;
  quality = quality_ < 1 ? 1 : quality_ > 100 ? 100 : quality_;  // as jpegio::encode clamps
  const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;  // jpeg_quality_scaling
  JpegTab tab;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const long v = ((long)(t ? kChrQ[i] : kLumQ[i]) * scale + 50L) / 100L;
      q[t][i] = (int)(v <= 0 ? 1 : v > 255 ? 255 : v);  // force_baseline
      tab.qdiv[t][i] = (uint32_t)q[t][i] << 3;
    }
  huff_table(kDcLumBits, kDcVals, tab.dc[0], 16);
  huff_table(kDcChrBits, kDcVals, tab.dc[1], 16);
  huff_table(kAcLumBits, kAcLumVals, tab.ac[0], 256);
  huff_table(kAcChrBits, kAcChrVals, tab.ac[1], 256);
  for (int i = 0; i < 64; ++i) tab.zz[i] = kZigzag[i];
  const size_t nblk = (size_t)max_mcus * 6, raw = jpeg_raw_cap_mcus(max_mcus);
  const size_t ntiles = cdiv(raw, JPEG_STUFF_TILE), nscan = nblk > ntiles ? nblk : ntiles;
  dTab.ensure(sizeof tab);
  dCoef.ensure(nblk * 64 * sizeof(int16_t));
  dBlkBits.ensure(nblk * 4);
  dBlkOff.ensure(nblk * 4);
  dGrpTot.ensure((size_t)cdiv(nscan, JPEG_SCAN_ITEMS) * 4);
  dGrpOff.ensure((size_t)cdiv(nscan, JPEG_SCAN_ITEMS) * 4);
  dWords.ensure(raw);
  dTileCnt.ensure(ntiles * 4);
  dTileOff.ensure(ntiles * 4);
  dTotals.ensure(2 * 4);
  S360_HIP(hipMemcpyAsync(dTab.p, &tab, sizeof tab, hipMemcpyHostToDevice, st));
  S360_HIP(hipStreamSynchronize(st));  // (tab goes out of scope)
}

void JpegEncoder::encode(const uint8_t* bgr, int w, int h, uint8_t* scan_out, size_t scan_cap, uint32_t* count, hipStream_t st, bool capped) {
  if (w < 1 || h < 1 || w > maxW || h > maxH || jpeg_mcus(w, h) > maxMcus)
    throw Error(S360_ERR_INVALID_ARG, "jpeg: the image is larger than the encoder was created for");
  if (!capped && scan_cap < jpeg_scan_cap(w, h)) throw Error(S360_ERR_INVALID_ARG, "jpeg: the scan buffer is smaller than jpeg_scan_cap");
  const int mcux = (w + 15) / 16, nmcu = (int)jpeg_mcus(w, h);
  const unsigned nblk = (unsigned)nmcu * 6;
  const size_t raw = jpeg_raw_cap(w, h);
  const unsigned ntiles = cdiv(raw, JPEG_STUFF_TILE);
  const JpegTab* tab = dTab.as<JpegTab>();
  unsigned* totals = dTotals.as<unsigned>();  // [0] the scan's bits, [1] its 0xFF bytes
  S360_HIP(hipMemsetAsync(dWords.p, 0, raw, st));
  hipLaunchKernelGGL(k_jpeg_blocks, dim3(cdiv(nmcu, JB_MCUS)), dim3(JB_THREADS), 0, st, bgr, w, h, mcux, nmcu, tab, dCoef.as<short>());
  hipLaunchKernelGGL(k_jpeg_entropy<false>, dim3(cdiv(nblk, JE_WAVES)), dim3(JE_WAVES * 64), 0, st, (const short*)dCoef.as<short>(), nblk,
                     tab, dBlkBits.as<unsigned>(), (const unsigned*)nullptr, (unsigned*)nullptr, 0u);
  scan(dBlkBits.as<unsigned>(), nblk, dGrpTot.as<unsigned>(), dGrpOff.as<unsigned>(), dBlkOff.as<unsigned>(), totals, st);
  hipLaunchKernelGGL(k_jpeg_entropy<true>, dim3(cdiv(nblk, JE_WAVES)), dim3(JE_WAVES * 64), 0, st, (const short*)dCoef.as<short>(), nblk,
                     tab, (unsigned*)nullptr, (const unsigned*)dBlkOff.as<unsigned>(), dWords.as<unsigned>(), (unsigned)(raw / 4));
  hipLaunchKernelGGL(k_jpeg_stuff_count, dim3(ntiles), dim3(ST_THREADS), 0, st, (const unsigned*)dWords.as<unsigned>(),
                     (const unsigned*)totals, dTileCnt.as<unsigned>());
  scan(dTileCnt.as<unsigned>(), ntiles, dGrpTot.as<unsigned>(), dGrpOff.as<unsigned>(), dTileOff.as<unsigned>(), totals + 1, st);
  hipLaunchKernelGGL(k_jpeg_stuff_scatter, dim3(ntiles), dim3(ST_THREADS), 0, st, (const unsigned*)dWords.as<unsigned>(),
                     (const unsigned*)totals, (const unsigned*)dTileOff.as<unsigned>(), (const unsigned*)(totals + 1), scan_out, scan_cap,
                     count);
  S360_HIP(hipGetLastError());
}

void JpegEncoder::header(uint8_t* out, int w, int h) const {
  uint8_t* p = out;
  const auto put = [&](std::initializer_list<int> v) { for (int x : v) *p++ = (uint8_t)x; };
  const auto put16 = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xDB});
    put16(67);
    *p++ = (uint8_t)t;
    for (int i = 0; i < 64; ++i) *p++ = (uint8_t)q[t][kZigzag[i]];
  }
  put({0xFF, 0xC0});
  put16(17);
  *p++ = 8;
  put16(h);
  put16(w);
  put({3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  const uint8_t* bitsOf[4] = {kDcLumBits, kAcLumBits, kDcChrBits, kAcChrBits};
  const uint8_t* valsOf[4] = {kDcVals, kAcLumVals, kDcVals, kAcChrVals};
  const int nvals[4] = {12, 162, 12, 162};
  const int ids[4] = {0x00, 0x10, 0x01, 0x11};
  for (int t = 0; t < 4; ++t) {
    put({0xFF, 0xC4});
    put16(2 + 1 + 16 + nvals[t]);
    *p++ = (uint8_t)ids[t];
    std::memcpy(p, bitsOf[t], 16);
    p += 16;
    std::memcpy(p, valsOf[t], nvals[t]);
    p += nvals[t];
  }
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  if (p - out != JPEG_HEADER_BYTES) throw Error(S360_ERR_STATE, "jpeg: header size");
}

}  // namespace s360

using namespace s360;

struct s360_jpeg {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t evT[2] = {nullptr, nullptr};
  JpegEncoder enc;
  DevBuf dBgr, dScan, dCount;
  uint32_t* hCount = nullptr;
  bool encoded = false;
  ~s360_jpeg() {
    if (st) (void)hipStreamSynchronize(st);
    for (hipEvent_t e : evT)
      if (e) (void)hipEventDestroy(e);
    if (hCount) (void)hipHostFree(hCount);
    if (st) (void)hipStreamDestroy(st);
  }
};

namespace {

void jpeg_init(s360_jpeg* e, int device, int max_w, int max_h, int quality) {
  need(jpeg_size_ok(max_w, max_h), "s360_jpeg_create: size outside 1..65535 or more than 431 220 MCUs of 16 x 16 pixels");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw Error(S360_ERR_NO_DEVICE, "no HIP device available (libs360 has no CPU path)");
  need(device >= 0 && device < ndev, "device index out of range");
  e->device = device;
  S360_HIP(hipSetDevice(device));
  S360_HIP(hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k) S360_HIP(hipEventCreate(&e->evT[k]));
  S360_HIP(hipHostMalloc((void**)&e->hCount, sizeof(uint32_t), hipHostMallocDefault));
  e->dBgr.ensure((size_t)max_w * max_h * 3);
  e->dScan.ensure(jpeg_scan_cap(max_w, max_h));
  e->dCount.ensure(sizeof(uint32_t));
  e->enc.init(max_w, max_h, quality, e->st);
}

// upload + encoder, enqueued; the image must fit the object
void run(s360_jpeg* e, const uint8_t* bgr, int w, int h) {
  need(w >= 1 && h >= 1 && w <= e->enc.maxW && h <= e->enc.maxH, "the image is larger than the encoder's max_w x max_h");
  S360_HIP(hipSetDevice(e->device));
  S360_HIP(hipMemcpyAsync(e->dBgr.p, bgr, (size_t)w * h * 3, hipMemcpyHostToDevice, e->st));
  S360_HIP(hipEventRecord(e->evT[0], e->st));
  e->enc.encode(e->dBgr.as<uint8_t>(), w, h, e->dScan.as<uint8_t>(), e->dScan.cap, e->dCount.as<uint32_t>(), e->st);
  S360_HIP(hipEventRecord(e->evT[1], e->st));
  e->encoded = true;
}

}  // namespace

extern "C" {

int s360_jpeg_create(s360_jpeg** out, int device, int max_w, int max_h, int quality) {
  if (!out) return S360_ERR_INVALID_ARG;
  *out = nullptr;
  s360_jpeg* e = nullptr;
  const int rc = guard([&] {
    e = new s360_jpeg;
    jpeg_init(e, device, max_w, max_h, quality);
  });
  if (rc != S360_OK) {
    delete e;
    return rc;
  }
  *out = e;
  return S360_OK;
}
void s360_jpeg_destroy(s360_jpeg* e) { delete e; }
size_t s360_jpeg_bound(int w, int h) { return jpeg_size_ok(w, h) ? jpeg_file_bound(w, h) : 0; }

int s360_jpeg_encode(s360_jpeg* e, const uint8_t* bgr, int w, int h, uint8_t* out, size_t cap, size_t* n_out) {
  return guard([&] {
    need(e && bgr && n_out && (out || cap == 0), "null argument");
    *n_out = 0;
    run(e, bgr, w, h);
    S360_HIP(hipMemcpyAsync(e->hCount, e->dCount.p, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    S360_HIP(hipStreamSynchronize(e->st));
    const size_t n = *e->hCount;
    if (n > e->dScan.cap) throw Error(S360_ERR_STATE, "s360_jpeg_encode: the scan is longer than its worst case");
    *n_out = JPEG_HEADER_BYTES + n + 2;
    need(cap >= *n_out, "s360_jpeg_encode: cap is smaller than the file (its size is in *n_out)");
    e->enc.header(out, w, h);
    S360_HIP(hipMemcpyAsync(out + JPEG_HEADER_BYTES, e->dScan.p, n, hipMemcpyDeviceToHost, e->st));
    S360_HIP(hipStreamSynchronize(e->st));
    out[JPEG_HEADER_BYTES + n] = 0xFF;
    out[JPEG_HEADER_BYTES + n + 1] = 0xD9;
  });
}

int s360_jpeg_last_time(s360_jpeg* e, float* ms) {
  return guard([&] {
    need(e && ms, "null argument");
    if (!e->encoded) throw Error(S360_ERR_STATE, "s360_jpeg_last_time: nothing was encoded");
    S360_HIP(hipEventSynchronize(e->evT[1]));
    S360_HIP(hipEventElapsedTime(ms, e->evT[0], e->evT[1]));
  });
}

// ---- test tap (include/s360_debug_jpeg.h) ---------------------------------------------------------------------------
int s360_debug_jpeg_blocks(s360_jpeg* e, const uint8_t* bgr, int w, int h, int16_t* coef_out, uint32_t* bits_out) {
  return guard([&] {
    need(e && bgr && coef_out && bits_out, "null argument");
    run(e, bgr, w, h);
    const size_t nblk = (size_t)jpeg_mcus(w, h) * 6;
    S360_HIP(hipMemcpyAsync(coef_out, e->enc.coef(), nblk * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, e->st));
    S360_HIP(hipMemcpyAsync(bits_out, e->enc.block_bits(), nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    S360_HIP(hipStreamSynchronize(e->st));
  });
}

}  // extern "C"
