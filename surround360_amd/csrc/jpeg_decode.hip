// jpeg_decode.hip — baseline JPEG camera files decoded on gfx950 (jpeg_decode.hpp, include/s360_input_jpeg.h): the read side of
// jpeg.hip. The specification is host/jpeg_io.hpp's jpegio::Reader; every rounding and every tolerated oddity is read from it.
//
// A baseline scan has no entry points, but a Huffman decoder started at a wrong bit falls into step with the right one sooner or
// later, or never (a constant image: every block is "DC 0, EOB", a decoder in the wrong block phase stays token-aligned and wrong).
// So nothing here relies on falling into step. The scan is cut into subsequences of S = kJpegSubBits bits. The state at a
// boundary is (bit position of the first token at or behind it, block index inside the MCU, zigzag position; 0 = DC expected), or
// an end / fault state. Subsequence 0 starts from the known state, every other one from the guess (its nominal start, block 0, DC).
// A subsequence whose predecessor's exit state is not the entry it decoded from decodes again from that exit and publishes its
// own. After round k subsequences 0..k hold the serial decoder's states (induction from subsequence 0), so the fixed point is
// the serial decoder's result whatever the data, and the number of subsequences bounds the loop. As in k_png_inflate's fast path
// (png_decode.hip) the rounds run where they are cheap: inside a workgroup of kJpegSyncThreads subsequences through LDS and
// __syncthreads, until a round changes nothing there; across workgroups as separate launches, each reading what its predecessor
// published in the launch before (two buffers, so a launch never reads what it writes), driven by the host from a downloaded
// counter of workgroups whose published exit changed. No workgroup waits for another through memory.
//
//   k_jpeg_unstuff      16 KiB of the stuffed scan per workgroup: count the 0x00 behind 0xFF per thread, scan in LDS, scatter. The
//                       host walks the scan's 0xFF bytes anyway to find its end, and hands over the stuffing count in front of
//                       every 16 KiB, so no scan across workgroups is needed. 0xFF followed by anything but 0x00 sets the file's
//                       status "marker inside the scan".
//   k_jpeg_sync         the rounds above; also the blocks begun per subsequence and per workgroup
//   k_jpeg_base         per file: the workgroups' first block index (serial over a file's workgroups, a dozen for 2048 x 2048), the
//                       file's status from the last exit state and the block count
//   k_jpeg_coef         every subsequence decodes once more from its final entry and writes de-zigzagged, still quantised int16
//                       coefficients into the zeroed block array (a block that spans a boundary is written by two subsequences at
//                       disjoint positions); the DC position holds the difference
//   k_jpeg_dc_*         DC differences -> values: per-component sums per chunk of 256 MCUs, a serial scan over a file's chunks, apply
//   k_jpeg_idct         8 threads per block: dequantise, jidctint.c's column pass into LDS, row pass, +128, clamp -> sample planes.
//                       64-bit products as in jpegio (damaged files' coefficients overflow 32 bits there, and must give the same)
//   k_jpeg_pixels       h2v1 / h2v2 fancy upsampling with the edges repeated, YCbCr -> RGB with jdcolor.c's 16-bit constants, and
//                       the store: packed B,G,R; a side slot (uchar4, side_src_alpha's ramp); a pole slot (uchar4, alpha 255)
//
// All files of a call share every launch: grids are (most work items of a file, files), a workgroup past its file's count returns.
// Bounds: every read of the bit stream is inside the file's unstuffed bytes plus 16 bytes of padding, and bits behind the end read
// as 0; a token is at least one bit, and the token loop ends at the subsequence's end; zigzag positions are checked against 63
// before they index; block indices against the file's block count before they address; the in-workgroup rounds are capped at the
// workgroup's size and the launches at the most workgroups of a file + 2 (both caps are the induction's own bounds, not cut-offs).
//
// S = kJpegSubBits = 4096 bits, measured (profiles/input_jpeg.txt: the 16 camera files of one frame, 2048 x 2048, PIL quality 95,
// synthetic images; entropy stage of the batch, warm, median of 10, 4:2:0 / 4:4:4): S 1024: 221 / 356 ms, 4096: 109 / 107 ms, 8192:
// 197 / 222 ms, 16384: 256 / 401 ms, 65536: 227 / 380 ms. A token is at most 32 bits (16 of code, 16 of magnitude), so an exit state
// lies at most 31 bits behind its boundary whatever S is. What the figures show: these images have long flat stretches, where a
// decoder in the wrong block phase never falls into step, so a corrected start walks down the subsequences one per pass (100 to
// 250 passes in most files at every S up to 8192: the last column of that profile) and the stretch is decoded serially by one lane at a time;
// S then only decides how the stretch is cut among workgroups, which run their chains side by side between launches. The
// developer switch S360_JPEG_SUB_BITS (64 .. 2^24; DESIGN §8, tools/README.md) overrides S for such measurements and for the tests' replay with
// short subsequences; it changes no result. Not done: a guess better than "block 0, DC"
// (e.g. one decode per block phase), which is what would shorten the chains.
// Occupancy of the token walk: it is divergent by nature, and in a propagation pass one lane of a wave works; the walk keeps the
// next 32..64 bits of the stream in a register and loads 4 bytes per 32 bits consumed, and each token's first lookup goes to the
// file's six 10-bit tables staged in LDS (12 KiB a workgroup); codes longer than 10 bits take the length loop in global memory.
//
// Resource usage as the compiler reports it (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): no kernel uses
// scratch, and none is limited below 8 waves per SIMD by its registers or LDS.
//   kernel             VGPRs  SGPRs  LDS bytes
//   k_jpeg_unstuff        10     46       1024
//   k_jpeg_sync           34     82      15616
//   k_jpeg_base            3     26          0
//   k_jpeg_coef           22     52      13312
//   k_jpeg_dc_totals      14     30       1024
//   k_jpeg_dc_chunks       4     16          0
//   k_jpeg_dc_apply       16     38       1024
//   k_jpeg_idct           36     18      16384
//   k_jpeg_pixels         16     31          0
#include "jpeg_decode.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/s360.h"
#include "render_kernels.hpp"

namespace s360 {
namespace {

typedef unsigned long long u64;
constexpr int kT = kJpegSyncThreads;

struct JFile {
  u64 in_off, u_off, coef_off, plane_off[3];
  uint8_t* dst;
  unsigned scan_len, ulen, nbits, nsub, nwg, sub0, wg0, seg0, nseg, nblocks, nmcu, chunk0, nchunk, sub_bits;
  int w, h, hs, vs, mx, my, store, feather;
};
struct JOut { unsigned status, blocks, marker, pad; };

struct JState { unsigned pos, blk, zz, flag; };  // flag: 0 decoding, kFlagEnd, or kFlagFault + JpegStatus
constexpr unsigned kFlagEnd = 1, kFlagFault = 16;
__host__ __device__ inline u64 pack(const JState& s) { return (u64)s.pos | ((u64)s.blk << 32) | ((u64)s.zz << 40) | ((u64)s.flag << 48); }
__host__ __device__ inline JState unpack(u64 v) {
  JState s;
  s.pos = (unsigned)v; s.blk = (unsigned)(v >> 32) & 255u; s.zz = (unsigned)(v >> 40) & 255u; s.flag = (unsigned)(v >> 48) & 255u;
  return s;
}

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct JZig { uint8_t z[64]; };

// exclusive prefix sum over the kT threads of a workgroup; every thread calls it
__device__ inline unsigned block_exscan(unsigned v, unsigned* sh, unsigned& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kT; d <<= 1) {
    const unsigned a = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  total = sh[kT - 1];
  const unsigned r = sh[t] - v;
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kT) void k_jpeg_unstuff(const uint8_t* __restrict__ in, uint8_t* __restrict__ unst, const JFile* __restrict__ files,
                                                      const unsigned* __restrict__ seg_stuff, JOut* __restrict__ outs) {
  __shared__ unsigned sh[kT];
  const JFile F = files[blockIdx.y];
  if (blockIdx.x >= F.nseg) return;
  const int t = threadIdx.x;
  constexpr unsigned kPer = (unsigned)(kJpegUnstuffSeg / kT);
  const uint8_t* s = in + F.in_off;
  const unsigned j0 = (unsigned)blockIdx.x * (unsigned)kJpegUnstuffSeg + (unsigned)t * kPer;
  const unsigned j1 = j0 < F.scan_len ? (F.scan_len - j0 < kPer ? F.scan_len : j0 + kPer) : j0;
  unsigned cnt = 0;
  bool marker = false;
  unsigned prev = j0 > 0 && j0 < F.scan_len ? s[j0 - 1] : 0u;
  for (unsigned j = j0; j < j1; ++j) {
    const unsigned b = s[j];
    if (b == 0u && prev == 0xFFu) ++cnt;
    if (prev == 0xFFu && b != 0u && j > 0) marker = true;
    prev = b;
  }
  if (j1 == F.scan_len && j1 > j0 && prev == 0xFFu) marker = true;  // (the byte behind the scan is no 0x00: the host ends the scan there)
  if (marker) outs[blockIdx.y].marker = 1u;
  unsigned total;
  const unsigned ex = block_exscan(cnt, sh, total);
  uint8_t* o = unst + F.u_off;
  unsigned at = j0 - (seg_stuff[F.seg0 + blockIdx.x] + ex);
  prev = j0 > 0 && j0 < F.scan_len ? s[j0 - 1] : 0u;
  for (unsigned j = j0; j < j1; ++j) {
    const unsigned b = s[j];
    if (!(b == 0u && prev == 0xFFu)) {
      if (at < F.ulen) o[at] = (uint8_t)b;
      ++at;
    }
    prev = b;
  }
}

// The six 10-bit tables of a file staged in LDS (12 KiB): every token's first lookup then costs an LDS read, not a trip to L2.
typedef uint16_t JLut[6][1024];
__device__ inline void stage_luts(const JpegTabDev& T, JLut& slut) {
  for (int k = threadIdx.x; k < 6 * 512; k += kT)
    reinterpret_cast<unsigned*>(slut[k >> 9])[k & 511] = reinterpret_cast<const unsigned*>(T.h[k >> 9].lut)[k & 511];
  __syncthreads();
}
// One Huffman symbol from the 16 bits in the top half of w: the symbol and its length, or length 0 (no code matches).
__device__ inline unsigned huff_lookup(const uint16_t* lut, const JpegHuffDev& H, unsigned w, unsigned& len) {
  const unsigned e = lut[w >> 22];
  if (e) {
    len = e >> 8;
    return e & 255u;
  }
  for (int l = 11; l <= 16; ++l) {
    const int code = (int)(w >> (32 - l));
    if (H.maxcode[l] >= 0 && code <= H.maxcode[l] && code >= H.mincode[l]) {
      len = (unsigned)l;
      return H.vals[(H.valptr[l] + code - H.mincode[l]) & 255];
    }
  }
  len = 0;
  return 0;
}
__device__ inline int extend(unsigned v, unsigned s) { return s && v < (1u << (s - 1)) ? (int)v - (int)(1u << s) + 1 : (int)v; }

// The serial decoder from state s up to the first token that starts at or behind bit `limit` (<= F.nbits), or to an end / fault
// state. Returns the blocks begun. W: writes the coefficients; `first` is the index of the first block begun here, the block in
// progress at entry is first - 1.
template <bool W>
__device__ inline unsigned decode_span(const uint8_t* __restrict__ u, const JpegTabDev& T, const JLut& slut, const JZig& Z, const JFile& F, JState& s, unsigned limit,
                                       int16_t* __restrict__ coef, unsigned first) {
  const unsigned hv = (unsigned)(F.hs * F.vs), bpm = hv + 2u, nbits = F.nbits;
  unsigned begun = 0, cur = first - 1u;
  if (limit > nbits) limit = nbits;
  // The next 32..64 bits of the stream in a register, left-aligned: one 4-byte load per 32 bits consumed instead of a window load
  // per token (with one lane of a wave at work, as in a propagation round, nothing hides a load's latency). `next` is the next
  // byte to load: at most 8 bytes behind the byte of pos, so a load ends less than 12 bytes behind the last byte of the stream.
  u64 buf = 0;
  unsigned avail = 0, next = s.pos >> 3;
  if (s.flag == 0u && s.pos < limit) {
    __builtin_memcpy(&buf, u + next, 8);
    buf = __builtin_bswap64(buf) << (s.pos & 7u);
    avail = 64u - (s.pos & 7u);
    next += 8u;
  }
  while (s.flag == 0u && s.pos < limit) {  // (a token is at least one bit: at most limit - pos turns)
    const unsigned rem = nbits - s.pos;
    if (avail < 32u) {
      unsigned v4;
      __builtin_memcpy(&v4, u + next, 4);
      buf |= (u64)__builtin_bswap32(v4) << (32u - avail);
      avail += 32u;
      next += 4u;
    }
    unsigned w = (unsigned)(buf >> 32);
    if (rem < 32u) w &= ~(0xFFFFFFFFu >> rem);  // bits behind the end read as 0, as the host's reader fills them
    const unsigned comp = s.blk < hv ? 0u : s.blk - hv + 1u;
    unsigned len;
    const unsigned tb = 2u * comp + (s.zz ? 1u : 0u);
    const unsigned sym = huff_lookup(slut[tb], T.h[tb], w, len);
    if (len == 0u) {  // no code: an incomplete token at the end is judged by k_jpeg_base, anywhere else it is a fault
      s.flag = rem < 16u ? kFlagEnd : kFlagFault + kJpegBadCode;
      break;
    }
    if (len > rem) { s.flag = kFlagEnd; break; }
    unsigned adv;  // the token's bits: at most 32
    if (s.zz == 0u) {
      if (sym > 11u) { s.flag = kFlagFault + kJpegBadCode; break; }
      if (len + sym > rem) { s.flag = kFlagEnd; break; }
      const unsigned v = sym ? (w << len) >> (32u - sym) : 0u;
      cur = first + begun;
      ++begun;
      if (W && cur < F.nblocks) coef[(size_t)cur * 64] = (int16_t)extend(v, sym);
      s.zz = 1u;
      adv = len + sym;
    } else {
      const unsigned r = sym >> 4, sz = sym & 15u;
      bool done;
      if (sz == 0u) {
        done = r != 15u || s.zz + 16u > 63u;  // EOB, or a ZRL that runs off the block (the host's loop just ends there)
        s.zz += 16u;
        adv = len;
      } else {
        const unsigned k = s.zz + r;
        if (len + sz > rem) { s.flag = kFlagEnd; break; }
        if (k > 63u) { s.flag = kFlagFault + kJpegBadRun; break; }
        if (W && cur < F.nblocks) coef[(size_t)cur * 64 + Z.z[k]] = (int16_t)extend((w << len) >> (32u - sz), sz);
        s.zz = k + 1u;
        adv = len + sz;
        done = s.zz > 63u;
      }
      if (done) {
        s.zz = 0u;
        s.blk = s.blk + 1u == bpm ? 0u : s.blk + 1u;
      }
    }
    s.pos += adv;
    buf <<= adv;
    avail -= adv;
  }
  if (s.flag == 0u && s.pos >= nbits) s.flag = kFlagEnd;
  return begun;
}

__global__ __launch_bounds__(kT) void k_jpeg_sync(const uint8_t* __restrict__ unst, const JFile* __restrict__ files, const JpegTabDev* __restrict__ tabs,
                                                   const JZig* __restrict__ zig, u64* __restrict__ entry, u64* __restrict__ exitv,
                                                   unsigned* __restrict__ nblk, u64* wg_exit, unsigned G, unsigned* __restrict__ wg_blocks,
                                                   unsigned* __restrict__ wg_iters, unsigned* __restrict__ changed, unsigned round,
                                                   const JOut* __restrict__ outs) {
  __shared__ u64 sh[kT];
  __shared__ unsigned shn[kT];
  __shared__ JLut slut;
  const JFile F = files[blockIdx.y];
  if (blockIdx.x >= F.nwg || outs[blockIdx.y].marker) return;
  const int t = threadIdx.x;
  const unsigned g = F.wg0 + blockIdx.x, li = blockIdx.x * (unsigned)kT + (unsigned)t;
  const bool valid = li < F.nsub;
  const size_t i = (size_t)F.sub0 + li;
  const u64* prevbuf = wg_exit + (size_t)(round & 1u) * G;
  u64* nextbuf = wg_exit + (size_t)((round + 1u) & 1u) * G;
  JState st0 = {0u, 0u, 0u, 0u};
  u64 e_in = 0, e_out = 0;
  unsigned nb = 0;
  bool need;
  if (round == 0u) {
    st0.pos = li * F.sub_bits;  // (li < nsub: below nbits)
    e_in = pack(st0);
    need = valid;
  } else {
    const u64 incoming = blockIdx.x == 0u ? pack(st0) : prevbuf[g - 1u];
    if (valid) { e_in = entry[i]; e_out = exitv[i]; nb = nblk[i]; }
    need = t == 0 && incoming != e_in;
    if (need) e_in = incoming;
    if (__syncthreads_and(!need)) {  // this workgroup's entry is what it decoded from: everything it published stands
      if (t == 0) nextbuf[g] = prevbuf[g];
      return;
    }
  }
  const uint8_t* u = unst + F.u_off;
  const JpegTabDev& T = tabs[blockIdx.y];
  stage_luts(T, slut);
  const unsigned limit = valid ? (li + 1u) * F.sub_bits : 0u;  // (li + 1 < nsub: below nbits; the last one is clamped to nbits)
  unsigned iters = 0;
  for (int it = 0; it <= kT; ++it) {  // after pass k threads 0..k-1 hold their final states: at most kT + 1 passes
    if (need) {
      JState s = unpack(e_in);
      nb = decode_span<false>(u, T, slut, *zig, F, s, li + 1u < F.nsub ? limit : F.nbits, nullptr, 0u);
      e_out = pack(s);
    }
    sh[t] = e_out;
    __syncthreads();
    const u64 ne = t == 0 ? e_in : sh[t - 1];
    ++iters;
    need = valid && ne != e_in;
    e_in = ne;
    if (__syncthreads_and(!need)) break;
  }
  if (valid) { entry[i] = e_in; exitv[i] = e_out; nblk[i] = nb; }
  shn[t] = valid ? nb : 0u;
  __syncthreads();
  for (int d = kT / 2; d > 0; d >>= 1) {
    if (t < d) shn[t] += shn[t + d];
    __syncthreads();
  }
  if (t == 0) {
    const unsigned left = F.nsub - blockIdx.x * (unsigned)kT, last = left < (unsigned)kT ? left - 1u : (unsigned)kT - 1u;
    const u64 pub = sh[last];
    // (workgroup 0 of a file starts from the known state: a file of one workgroup is final after the first launch)
    if (round == 0u ? F.nwg > 1u : pub != prevbuf[g]) atomicAdd(&changed[round], 1u);
    nextbuf[g] = pub;
    wg_blocks[g] = shn[0];
    wg_iters[g] = (round ? wg_iters[g] : 0u) + iters;
  }
}

__global__ __launch_bounds__(64) void k_jpeg_base(const JFile* __restrict__ files, const u64* __restrict__ exitv, const unsigned* __restrict__ wg_blocks,
                                                   unsigned* __restrict__ wg_base, JOut* __restrict__ outs) {
  if (threadIdx.x != 0) return;
  const JFile F = files[blockIdx.x];
  JOut& O = outs[blockIdx.x];
  if (O.marker) { O.status = kJpegMarker; return; }
  unsigned run = 0;
  for (unsigned k = 0; k < F.nwg; ++k) {
    wg_base[F.wg0 + k] = run;
    const unsigned b = wg_blocks[F.wg0 + k];
    run = run + b < run ? 0xFFFFFFFFu : run + b;
  }
  const JState s = unpack(exitv[(size_t)F.sub0 + F.nsub - 1u]);
  const unsigned left = F.nbits - (s.pos < F.nbits ? s.pos : F.nbits);
  unsigned status = kJpegOk;
  if (s.flag >= kFlagFault) status = s.flag - kFlagFault;
  else if (run < F.nblocks) status = s.zz == 0u && left < 8u ? kJpegBlocksMissing : kJpegShort;
  else if (run > F.nblocks) status = kJpegLeftOver;
  else if (s.zz != 0u) status = kJpegShort;
  else if (left >= 8u) status = kJpegLeftOver;
  O.status = status;
  O.blocks = run;
}

__global__ __launch_bounds__(kT) void k_jpeg_coef(const uint8_t* __restrict__ unst, const JFile* __restrict__ files, const JpegTabDev* __restrict__ tabs,
                                                   const JZig* __restrict__ zig, const u64* __restrict__ entry, const unsigned* __restrict__ nblk,
                                                   const unsigned* __restrict__ wg_base, const JOut* __restrict__ outs, int16_t* __restrict__ coef) {
  __shared__ unsigned sh[kT];
  __shared__ JLut slut;
  const JFile F = files[blockIdx.y];
  if (blockIdx.x >= F.nwg || outs[blockIdx.y].status) return;
  stage_luts(tabs[blockIdx.y], slut);
  const unsigned li = blockIdx.x * (unsigned)kT + threadIdx.x;
  const bool valid = li < F.nsub;
  const size_t i = (size_t)F.sub0 + li;
  unsigned total;
  const unsigned first = wg_base[F.wg0 + blockIdx.x] + block_exscan(valid ? nblk[i] : 0u, sh, total);
  if (!valid) return;
  JState s = unpack(entry[i]);
  decode_span<true>(unst + F.u_off, tabs[blockIdx.y], slut, *zig, F, s, li + 1u < F.nsub ? (li + 1u) * F.sub_bits : F.nbits, coef + F.coef_off * 64, first);
}

// The DC differences of MCU m per component (Y: all of its blocks)
__device__ inline void mcu_dc_sums(const int16_t* __restrict__ coef, const JFile& F, unsigned m, int sum[3]) {
  const unsigned hv = (unsigned)(F.hs * F.vs), bpm = hv + 2u;
  const int16_t* c = coef + (F.coef_off + (size_t)m * bpm) * 64;
  sum[0] = 0;
  for (unsigned k = 0; k < hv; ++k) sum[0] += c[(size_t)k * 64];
  sum[1] = c[(size_t)hv * 64];
  sum[2] = c[(size_t)(hv + 1u) * 64];
}
__global__ __launch_bounds__(kT) void k_jpeg_dc_totals(const int16_t* __restrict__ coef, const JFile* __restrict__ files, const JOut* __restrict__ outs,
                                                        int* __restrict__ chunks) {
  __shared__ unsigned sh[kT];
  const JFile F = files[blockIdx.y];
  if (blockIdx.x >= F.nchunk || outs[blockIdx.y].status) return;
  const unsigned m = blockIdx.x * (unsigned)kT + threadIdx.x;
  int sum[3] = {0, 0, 0};
  if (m < F.nmcu) mcu_dc_sums(coef, F, m, sum);
  for (int c = 0; c < 3; ++c) {
    unsigned total;
    block_exscan((unsigned)sum[c], sh, total);  // (two's complement: the sum of the differences modulo 2^32)
    if (threadIdx.x == 0) chunks[((size_t)F.chunk0 + blockIdx.x) * 4 + c] = (int)total;
  }
}
__global__ __launch_bounds__(64) void k_jpeg_dc_chunks(const JFile* __restrict__ files, const JOut* __restrict__ outs, int* __restrict__ chunks) {
  const JFile F = files[blockIdx.x];
  if (threadIdx.x >= 3 || outs[blockIdx.x].status) return;
  unsigned run = 0;
  for (unsigned k = 0; k < F.nchunk; ++k) {
    int& v = chunks[((size_t)F.chunk0 + k) * 4 + threadIdx.x];
    const unsigned add = (unsigned)v;
    v = (int)run;
    run += add;
  }
}
__global__ __launch_bounds__(kT) void k_jpeg_dc_apply(const int16_t* __restrict__ coef, const JFile* __restrict__ files, const JOut* __restrict__ outs,
                                                       const int* __restrict__ chunks, int* __restrict__ dc) {
  __shared__ unsigned sh[kT];
  const JFile F = files[blockIdx.y];
  if (blockIdx.x >= F.nchunk || outs[blockIdx.y].status) return;
  const unsigned m = blockIdx.x * (unsigned)kT + threadIdx.x;
  int sum[3] = {0, 0, 0};
  if (m < F.nmcu) mcu_dc_sums(coef, F, m, sum);
  unsigned pre[3];
  for (int c = 0; c < 3; ++c) {
    unsigned total;
    pre[c] = block_exscan((unsigned)sum[c], sh, total) + (unsigned)chunks[((size_t)F.chunk0 + blockIdx.x) * 4 + c];
  }
  if (m >= F.nmcu) return;
  const unsigned hv = (unsigned)(F.hs * F.vs), bpm = hv + 2u;
  const size_t b0 = F.coef_off + (size_t)m * bpm;
  unsigned y = pre[0];
  for (unsigned k = 0; k < hv; ++k) {
    y += (unsigned)(int)coef[(b0 + k) * 64];
    dc[b0 + k] = (int)y;
  }
  dc[b0 + hv] = (int)(pre[1] + (unsigned)sum[1]);
  dc[b0 + hv + 1u] = (int)(pre[2] + (unsigned)sum[2]);
}

// jidctint.c's one-dimensional pass on v[0..7] (the even part, the odd part), as jpegio::Reader::idct writes it out
__device__ inline void idct_1d(const long long v[8], long long o[8]) {
  const long long F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137, F1961 = 16069,
                  F2053 = 16819, F2562 = 20995, F3072 = 25172;
  long long z2 = v[2], z3 = v[6];
  long long z1 = (z2 + z3) * F0541;
  long long tmp2 = z1 + z3 * (-F1847), tmp3 = z1 + z2 * F0765;
  long long tmp0 = (v[0] + v[4]) * 8192, tmp1 = (v[0] - v[4]) * 8192;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  long long z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * F1175;
  tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
  z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3;
  o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
  o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1;
  o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}
constexpr int kIdctBlocks = kT / 8;
__global__ __launch_bounds__(kT) void k_jpeg_idct(const int16_t* __restrict__ coef, const int* __restrict__ dc, const JFile* __restrict__ files,
                                                   const JpegTabDev* __restrict__ tabs, const JOut* __restrict__ outs, uint8_t* __restrict__ planes) {
  __shared__ long long ws[kIdctBlocks][64];
  const JFile F = files[blockIdx.y];
  if ((u64)blockIdx.x * kIdctBlocks >= F.nblocks || outs[blockIdx.y].status) return;
  const int t = threadIdx.x, lb = t >> 3, c = t & 7;
  const unsigned b = blockIdx.x * (unsigned)kIdctBlocks + (unsigned)lb;
  const bool active = b < F.nblocks;
  const unsigned hv = (unsigned)(F.hs * F.vs), bpm = hv + 2u, m = b / bpm, k = b % bpm, comp = k < hv ? 0u : k - hv + 1u;
  if (active) {
    const int16_t* in = coef + (F.coef_off + b) * 64;
    const uint16_t* q = tabs[blockIdx.y].q[comp];
    long long v[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = (long long)in[r * 8 + c] * q[r * 8 + c];
    if (c == 0) v[0] = (long long)dc[F.coef_off + b] * q[0];
    idct_1d(v, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[lb][r * 8 + c] = (o[r] + (1ll << 10)) >> 11;  // CONST_BITS - PASS1_BITS
  }
  __syncthreads();
  if (!active) return;
  long long v[8], o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = ws[lb][c * 8 + j];  // row c of the block
  idct_1d(v, o);
  const unsigned mxy = (unsigned)F.mx;
  unsigned bx, by, stride;
  if (comp == 0u) {
    bx = (m % mxy) * (unsigned)F.hs + k % (unsigned)F.hs;
    by = (m / mxy) * (unsigned)F.vs + k / (unsigned)F.hs;
    stride = mxy * (unsigned)F.hs * 8u;
  } else {
    bx = m % mxy; by = m / mxy; stride = mxy * 8u;
  }
  const u64 plane = comp == 0u ? F.plane_off[0] : comp == 1u ? F.plane_off[1] : F.plane_off[2];  // (a run-time index would put F in scratch)
  uint8_t* out = planes + plane + ((size_t)by * 8 + (size_t)c) * stride + (size_t)bx * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    long long x = ((o[j] + (1ll << 17)) >> 18) + 128;  // CONST_BITS + PASS1_BITS + 3
    out[j] = (uint8_t)(x < 0 ? 0 : x > 255 ? 255 : x);
  }
}

// a chroma sample at (x, y) of the full-size image: jdsample.c's fancy upsampling as jpegio::Reader::upsample applies it
__device__ inline int chroma_at(const uint8_t* __restrict__ p, int stride, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(size_t)y * stride + x];
  const int n = dw, i = x >> 1;
  if (vs == 1) {
    const uint8_t* in = p + (size_t)y * stride;
    if (x & 1) return i == n - 1 ? in[n - 1] : (in[i] * 3 + in[i + 1] + 2) >> 2;
    return i == 0 ? in[0] : (in[i] * 3 + in[i - 1] + 1) >> 2;
  }
  const int r = y >> 1, r1 = (y & 1) ? r + 1 : r - 1;
  const uint8_t* in0 = p + (size_t)(r < dh - 1 ? r : dh - 1) * stride;
  const uint8_t* in1 = p + (size_t)(r1 < 0 ? 0 : r1 > dh - 1 ? dh - 1 : r1) * stride;
  const int cs = in0[i] * 3 + in1[i];
  if (x & 1) return i == n - 1 ? (cs * 4 + 7) >> 4 : (cs * 3 + in0[i + 1] * 3 + in1[i + 1] + 7) >> 4;
  return i == 0 ? (cs * 4 + 8) >> 4 : (cs * 3 + in0[i - 1] * 3 + in1[i - 1] + 8) >> 4;
}
__global__ __launch_bounds__(256) void k_jpeg_pixels(const uint8_t* __restrict__ planes, const JFile* __restrict__ files, const JOut* __restrict__ outs) {
  const JFile F = files[blockIdx.z];
  const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
  if (x >= F.w || y >= F.h || outs[blockIdx.z].status) return;
  const int ystride = F.mx * F.hs * 8, cstride = F.mx * 8;
  const int dw = (F.w + F.hs - 1) / F.hs, dh = (F.h + F.vs - 1) / F.vs;
  const int Y = planes[F.plane_off[0] + (size_t)y * ystride + x];
  const int cb = chroma_at(planes + F.plane_off[1], cstride, dw, dh, F.hs, F.vs, x, y) & 255;
  const int cr = chroma_at(planes + F.plane_off[2], cstride, dw, dh, F.hs, F.vs, x, y) & 255;
  // jdcolor.c build_ycc_rgb_table: SCALEBITS 16 (>> of a negative int is arithmetic here as on the host)
  const int r = Y + ((91881 * (cr - 128) + 32768) >> 16), b = Y + ((116130 * (cb - 128) + 32768) >> 16);
  const int g = Y + ((-22554 * (cb - 128) + 32768 - 46802 * (cr - 128)) >> 16);
  const unsigned B = (unsigned)(b < 0 ? 0 : b > 255 ? 255 : b), G = (unsigned)(g < 0 ? 0 : g > 255 ? 255 : g), R = (unsigned)(r < 0 ? 0 : r > 255 ? 255 : r);
  const size_t p = (size_t)y * (size_t)F.w + (size_t)x;
  if (F.store == kJpegStoreBytes) {
    uint8_t* o = F.dst + p * 3;
    o[0] = (uint8_t)B; o[1] = (uint8_t)G; o[2] = (uint8_t)R;
  } else {
    const unsigned a = F.store == kJpegStoreSide ? (unsigned)side_src_alpha(y, F.h, F.feather, 255) : 255u;
    reinterpret_cast<unsigned*>(F.dst)[p] = B | (G << 8) | (R << 16) | (a << 24);
  }
}

const char* const kStatusText[] = {"ok", "invalid Huffman code", "a run past coefficient 63", "the scan ends short", "blocks missing at the end",
                                   "bits left over beyond the padding", "a marker inside the scan"};

// ---- the container -----------------------------------------------------------------------------------------------------
struct HuffHost {
  uint8_t bits[17] = {0}, vals[256] = {0};
  bool defined = false;
};
void build_huff(const HuffHost& t, JpegHuffDev& H) {
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    H.valptr[l] = k;
    H.mincode[l] = code;
    code += t.bits[l];
    k += t.bits[l];
    H.maxcode[l] = t.bits[l] ? code - 1 : -1;
    code <<= 1;
  }
  H.valptr[0] = H.mincode[0] = 0;
  H.maxcode[0] = -1;
  std::memcpy(H.vals, t.vals, 256);
  for (unsigned p = 0; p < 1024; ++p) {  // jpegio's decode_sym on these 10 bits
    H.lut[p] = 0;
    for (int l = 1; l <= 10; ++l) {
      const int c = (int)(p >> (10 - l));
      if (H.maxcode[l] >= 0 && c <= H.maxcode[l] && c >= H.mincode[l]) {
        H.lut[p] = (uint16_t)((l << 8) | t.vals[(H.valptr[l] + c - H.mincode[l]) & 255]);
        break;
      }
    }
  }
}
}  // namespace

bool jpeg_in_parse(const uint8_t* d, size_t n, JpegInInfo& I) {
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return false;
  size_t pos = 2;
  bool sof = false;
  int w = 0, h = 0, adobe = -1;
  struct Comp { int id, hh, vv, tq, td, ta; } comp[3] = {};
  uint8_t q[4][64];
  bool qdef[4] = {false, false, false, false};
  HuffHost dc[4], ac[4];
  auto be16 = [&](size_t p) -> size_t { return ((size_t)d[p] << 8) | d[p + 1]; };
  for (;;) {
    // the next marker, as jpegio::Reader::marker finds it
    while (pos < n && d[pos] != 0xFF) ++pos;
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos >= n) return false;
    const int m = d[pos++];
    if (m == 0xD9) return false;
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
    if (pos + 2 > n) return false;
    const size_t len = be16(pos);
    if (len < 2 || pos + len > n) return false;
    const size_t seg = pos + 2, end = pos + len;
    if (m == 0xC0) {
      if (sof || end - seg < 6 + 9 || d[seg] != 8 || d[seg + 5] != 3) return false;
      h = (int)be16(seg + 1);
      w = (int)be16(seg + 3);
      if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 28)) return false;
      for (int i = 0; i < 3; ++i) {
        Comp& c = comp[i];
        c.id = d[seg + 6 + i * 3];
        c.hh = d[seg + 7 + i * 3] >> 4;
        c.vv = d[seg + 7 + i * 3] & 15;
        c.tq = d[seg + 8 + i * 3];
        if (c.tq > 3) return false;
      }
      if (comp[1].hh != 1 || comp[1].vv != 1 || comp[2].hh != 1 || comp[2].vv != 1) return false;
      if (!((comp[0].hh == 2 && comp[0].vv == 2) || (comp[0].hh == 2 && comp[0].vv == 1) || (comp[0].hh == 1 && comp[0].vv == 1))) return false;
      sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
      return false;  // extended, progressive, lossless, arithmetic, hierarchical
    } else if (m == 0xC4) {
      size_t p = seg;
      while (p < end) {
        const int tc = d[p] >> 4, th = d[p] & 15;
        ++p;
        if (tc > 1 || th > 3 || p + 16 > end) return false;
        HuffHost& t = tc ? ac[th] : dc[th];
        int cnt = 0;
        for (int l = 1; l <= 16; ++l) { t.bits[l] = d[p + l - 1]; cnt += t.bits[l]; }
        p += 16;
        if (cnt > 256 || p + (size_t)cnt > end) return false;
        std::memset(t.vals, 0, sizeof t.vals);
        std::memcpy(t.vals, d + p, (size_t)cnt);
        p += (size_t)cnt;
        t.defined = true;
      }
    } else if (m == 0xDB) {
      size_t p = seg;
      while (p < end) {
        const int pq = d[p] >> 4, tq = d[p] & 15;
        ++p;
        if (tq > 3 || pq != 0 || p + 64 > end) return false;  // 8-bit tables only
        for (int i = 0; i < 64; ++i) q[tq][kZigzag[i]] = d[p + i];
        p += 64;
        qdef[tq] = true;
      }
    } else if (m == 0xDD) {
      if (end - seg < 2 || be16(seg) != 0) return false;  // restart intervals are the host decoder's
    } else if (m == 0xE1) {  // EXIF: orientation tag 0x0112 of IFD0 (jpegio::Reader::check_exif)
      if (end - seg >= 14 && std::memcmp(d + seg, "Exif\0\0", 6) == 0) {
        const size_t t = seg + 6;
        const bool le = d[t] == 'I';
        auto u16 = [&](size_t o) -> unsigned { return o + 1 < end ? (le ? d[o] | d[o + 1] << 8 : d[o] << 8 | d[o + 1]) : 0u; };
        auto u32 = [&](size_t o) -> unsigned { return o + 3 < end ? (le ? u16(o) | u16(o + 2) << 16 : u16(o) << 16 | u16(o + 2)) : 0u; };
        const size_t ifd = t + u32(t + 4);
        const unsigned cnt = u16(ifd);
        for (unsigned i = 0; i < cnt; ++i) {
          const size_t e = ifd + 2 + (size_t)i * 12;
          if (e + 12 > end) break;
          if (u16(e) == 0x0112) {
            if (u16(e + 8) > 1) return false;
            break;
          }
        }
      }
    } else if (m == 0xEE) {
      if (end - seg >= 12 && std::memcmp(d + seg, "Adobe", 5) == 0) adobe = d[seg + 11];
    } else if (m == 0xDA) {
      if (!sof || adobe == 0 || end - seg < 1 + 6 + 3 || d[seg] != 3) return false;
      for (int i = 0; i < 3; ++i) {
        const int id = d[seg + 1 + i * 2], t = d[seg + 2 + i * 2];
        if (id != comp[i].id) return false;
        comp[i].td = t >> 4;
        comp[i].ta = t & 15;
        if (comp[i].td > 3 || comp[i].ta > 3 || !dc[comp[i].td].defined || !ac[comp[i].ta].defined || !qdef[comp[i].tq]) return false;
      }
      if (d[seg + 7] != 0 || d[seg + 8] != 63 || d[seg + 9] != 0) return false;
      pos = end;
      break;
    }
    pos = end;
  }
  // the entropy-coded segment: up to the first 0xFF that is followed by neither 0x00 (stuffing) nor RSTn / 0xFF (which the device
  // reports as a marker inside the scan), or to the end of the file; the stuffing bytes counted on the way
  I.scan_off = pos;
  I.seg_stuff.clear();
  I.seg_stuff.push_back(0);
  size_t stuff = 0, p = pos, endp = n;
  auto seg_mark = [&](size_t upto) {  // every segment that starts at or before scan byte `upto` has its count
    while (I.seg_stuff.size() * kJpegUnstuffSeg <= upto) I.seg_stuff.push_back((uint32_t)stuff);
  };
  while (p < n) {
    const uint8_t* f = static_cast<const uint8_t*>(std::memchr(d + p, 0xFF, n - p));
    if (!f) break;
    const size_t j = (size_t)(f - d);
    if (j + 1 >= n) { endp = j; break; }
    const uint8_t b2 = d[j + 1];
    if (b2 == 0) {
      seg_mark(j + 1 - pos);  // segments up to the one the stuffing byte lies in: it is not in front of its own segment
      ++stuff;
      p = j + 2;
    } else if ((b2 >= 0xD0 && b2 <= 0xD7) || b2 == 0xFF) {
      p = j + 1;
    } else {
      endp = j;
      break;
    }
  }
  I.scan_len = endp - pos;
  if (I.scan_len >= ((size_t)1 << 29)) return false;
  seg_mark(I.scan_len ? I.scan_len - 1 : 0);
  I.seg_stuff.resize(std::max<size_t>(1, (I.scan_len + kJpegUnstuffSeg - 1) / kJpegUnstuffSeg));
  I.nstuff = stuff;
  I.w = w; I.h = h; I.hs = comp[0].hh; I.vs = comp[0].vv;
  for (int c = 0; c < 3; ++c) {
    build_huff(dc[comp[c].td], I.tab.h[2 * c]);
    build_huff(ac[comp[c].ta], I.tab.h[2 * c + 1]);
    for (int i = 0; i < 64; ++i) I.tab.q[c][i] = q[comp[c].tq][i];
  }
  return true;
}

unsigned jpeg_sub_bits() {
  unsigned v = kJpegSubBits;
  if (const char* e = std::getenv("S360_JPEG_SUB_BITS")) {  // developer switch: tools/input_jpeg_time.py sweeps it
    const long x = std::atol(e);
    if (x >= 64 && x <= (1l << 24)) v = (unsigned)x;
  }
  return v;
}

void jpeg_decode_run(hipStream_t st, JpegDecodeBufs& D, const std::vector<const uint8_t*>& files, const std::vector<JpegInInfo>& info,
                     const std::vector<JpegDecodeDst>& dst, const std::vector<hipEvent_t>& before, JpegDecodeStats& stats, int16_t* coef_tap,
                     int tap_image) {
  const size_t nf = info.size();
  stats = JpegDecodeStats();
  if (!nf) return;
  if (nf > 65535) throw Error(S360_ERR_INVALID_ARG, "jpeg decode: more than 65535 files in one call");
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const unsigned sub_bits = jpeg_sub_bits();
  std::vector<JFile> jf(nf);
  size_t in_bytes = 0, u_bytes = 0, nsub = 0, nwg = 0, nseg = 0, nblk = 0, nchunk = 0, plane_bytes = 0;
  unsigned max_seg = 0, max_wg = 0, max_chunk = 0, max_iblk = 0;
  int max_w = 0, max_h = 0;
  std::vector<unsigned> seg_stuff;
  for (size_t i = 0; i < nf; ++i) {
    const JpegInInfo& P = info[i];
    const JpegDecodeDst& T = dst[i];
    if (T.store != kJpegStoreBytes && T.store != kJpegStoreSide && T.store != kJpegStorePole)
      throw Error(S360_ERR_INVALID_ARG, "jpeg decode: image " + std::to_string(i) + ": no such store");
    if (T.store != kJpegStoreBytes && (reinterpret_cast<uintptr_t>(T.p) & 3)) throw Error(S360_ERR_INVALID_ARG, "jpeg decode: image not 4-byte aligned");
    JFile& F = jf[i];
    std::memset(&F, 0, sizeof F);
    F.w = P.w; F.h = P.h; F.hs = P.hs; F.vs = P.vs;
    F.mx = (P.w + 8 * P.hs - 1) / (8 * P.hs);
    F.my = (P.h + 8 * P.vs - 1) / (8 * P.vs);
    F.store = T.store; F.feather = T.feather; F.dst = T.p;
    const size_t mcus = (size_t)F.mx * F.my, blocks = jpeg_in_blocks(P);
    if (blocks > 0x7fffffffu) throw Error(S360_ERR_INVALID_ARG, "jpeg decode: image " + std::to_string(i) + ": too many blocks");
    F.nmcu = (unsigned)mcus;
    F.nblocks = (unsigned)blocks;
    F.scan_len = (unsigned)P.scan_len;
    F.ulen = (unsigned)(P.scan_len - P.nstuff);
    F.nbits = F.ulen * 8u;
    F.sub_bits = sub_bits;
    F.nsub = std::max(1u, (unsigned)(((u64)F.nbits + sub_bits - 1u) / sub_bits));
    F.nwg = (F.nsub + kT - 1) / kT;
    F.nseg = (unsigned)P.seg_stuff.size();
    F.nchunk = (F.nmcu + kT - 1) / kT;
    F.in_off = in_bytes; in_bytes += up16(P.scan_len + 1);
    F.u_off = u_bytes; u_bytes += up16((size_t)F.ulen + 16);
    F.sub0 = (unsigned)nsub; nsub += F.nsub;
    F.wg0 = (unsigned)nwg; nwg += F.nwg;
    F.seg0 = (unsigned)nseg; nseg += F.nseg;
    F.chunk0 = (unsigned)nchunk; nchunk += F.nchunk;
    F.coef_off = nblk; nblk += blocks;
    const size_t ysz = mcus * (size_t)(P.hs * P.vs) * 64, csz = mcus * 64;
    F.plane_off[0] = plane_bytes; F.plane_off[1] = plane_bytes + up16(ysz); F.plane_off[2] = F.plane_off[1] + up16(csz);
    plane_bytes = F.plane_off[2] + up16(csz);
    if (nsub > 0x7fffffffu || nseg > 0x7fffffffu) throw Error(S360_ERR_INVALID_ARG, "jpeg decode: the files' scans are too long for one call");
    seg_stuff.insert(seg_stuff.end(), P.seg_stuff.begin(), P.seg_stuff.end());
    max_seg = std::max(max_seg, F.nseg); max_wg = std::max(max_wg, F.nwg); max_chunk = std::max(max_chunk, F.nchunk);
    max_iblk = std::max(max_iblk, (F.nblocks + kIdctBlocks - 1) / kIdctBlocks);
    max_w = std::max(max_w, P.w); max_h = std::max(max_h, P.h);
  }
  const unsigned max_rounds = max_wg + 2u;
  // where everything lies
  D.in.ensure(in_bytes + 16);
  D.unst.ensure(u_bytes + 16);
  D.files.ensure(nf * sizeof(JFile));
  D.tabs.ensure(nf * sizeof(JpegTabDev) + sizeof(JZig));
  D.segs.ensure(nseg * sizeof(unsigned));
  const size_t sub_exit = up16(nsub * sizeof(u64)), sub_nblk = 2 * sub_exit;
  D.subs.ensure(sub_nblk + nsub * sizeof(unsigned));
  const size_t wg_u32 = up16(2 * nwg * sizeof(u64));
  D.wgs.ensure(wg_u32 + 3 * up16(nwg * sizeof(unsigned)));
  const size_t cnt_changed = up16(nf * sizeof(JOut)), cnt_bytes = cnt_changed + (size_t)max_rounds * sizeof(unsigned);
  D.counters.ensure(cnt_bytes);
  D.coef.ensure(nblk * 64 * sizeof(int16_t));
  D.dc.ensure(nblk * sizeof(int));
  D.chunks.ensure(nchunk * 4 * sizeof(int));
  D.planes.ensure(plane_bytes);
  for (hipEvent_t& e : D.ev)
    if (!e) S360_HIP(hipEventCreate(&e));

  // (from here on copies from this function's locals may be pending on the stream: an error waits for them before it unwinds)
  std::vector<JpegTabDev> tabs(nf);
  JZig zig;
  try {
  uint8_t* din = D.in.as<uint8_t>();
  for (size_t i = 0; i < nf; ++i)
    if (info[i].scan_len) S360_HIP(hipMemcpyAsync(din + jf[i].in_off, files[i] + info[i].scan_off, info[i].scan_len, hipMemcpyHostToDevice, st));
  S360_HIP(hipMemcpyAsync(D.files.p, jf.data(), nf * sizeof(JFile), hipMemcpyHostToDevice, st));
  for (size_t i = 0; i < nf; ++i) tabs[i] = info[i].tab;
  std::memcpy(zig.z, kZigzag, 64);
  S360_HIP(hipMemcpyAsync(D.tabs.p, tabs.data(), nf * sizeof(JpegTabDev), hipMemcpyHostToDevice, st));
  JZig* dzig = reinterpret_cast<JZig*>(D.tabs.as<uint8_t>() + nf * sizeof(JpegTabDev));
  S360_HIP(hipMemcpyAsync(dzig, &zig, sizeof zig, hipMemcpyHostToDevice, st));
  S360_HIP(hipMemcpyAsync(D.segs.p, seg_stuff.data(), nseg * sizeof(unsigned), hipMemcpyHostToDevice, st));
  S360_HIP(hipMemsetAsync(D.counters.p, 0, cnt_bytes, st));
  S360_HIP(hipMemsetAsync(D.coef.p, 0, nblk * 64 * sizeof(int16_t), st));

  const JFile* dfiles = D.files.as<JFile>();
  const JpegTabDev* dtabs = D.tabs.as<JpegTabDev>();
  JOut* douts = D.counters.as<JOut>();
  unsigned* dchanged = reinterpret_cast<unsigned*>(D.counters.as<uint8_t>() + cnt_changed);
  u64* dentry = D.subs.as<u64>();
  u64* dexit = reinterpret_cast<u64*>(D.subs.as<uint8_t>() + sub_exit);
  unsigned* dnblk = reinterpret_cast<unsigned*>(D.subs.as<uint8_t>() + sub_nblk);
  u64* dwg_exit = D.wgs.as<u64>();
  unsigned* dwg_blocks = reinterpret_cast<unsigned*>(D.wgs.as<uint8_t>() + wg_u32);
  unsigned* dwg_base = reinterpret_cast<unsigned*>(D.wgs.as<uint8_t>() + wg_u32 + up16(nwg * sizeof(unsigned)));
  unsigned* dwg_iters = reinterpret_cast<unsigned*>(D.wgs.as<uint8_t>() + wg_u32 + 2 * up16(nwg * sizeof(unsigned)));
  const unsigned nfu = (unsigned)nf;

  S360_HIP(hipEventRecord(D.ev[0], st));
  hipLaunchKernelGGL(k_jpeg_unstuff, dim3(max_seg, nfu), dim3(kT), 0, st, (const uint8_t*)din, D.unst.as<uint8_t>(), dfiles,
                     (const unsigned*)D.segs.as<unsigned>(), douts);
  unsigned rounds = 0;
  for (;;) {
    if (rounds >= max_rounds) throw Error(S360_ERR_STATE, "jpeg decode: the synchronisation did not end within its bound");
    hipLaunchKernelGGL(k_jpeg_sync, dim3(max_wg, nfu), dim3(kT), 0, st, (const uint8_t*)D.unst.as<uint8_t>(), dfiles, dtabs, (const JZig*)dzig,
                       dentry, dexit, dnblk, dwg_exit, (unsigned)nwg, dwg_blocks, dwg_iters, dchanged, rounds, (const JOut*)douts);
    S360_HIP(hipGetLastError());
    unsigned changed = 0;
    S360_HIP(hipMemcpyAsync(&changed, dchanged + rounds, sizeof changed, hipMemcpyDeviceToHost, st));
    S360_HIP(hipStreamSynchronize(st));
    ++rounds;
    if (!changed) break;
  }
  hipLaunchKernelGGL(k_jpeg_base, dim3(nfu), dim3(64), 0, st, dfiles, (const u64*)dexit, (const unsigned*)dwg_blocks, dwg_base, douts);
  hipLaunchKernelGGL(k_jpeg_coef, dim3(max_wg, nfu), dim3(kT), 0, st, (const uint8_t*)D.unst.as<uint8_t>(), dfiles, dtabs, (const JZig*)dzig,
                     (const u64*)dentry, (const unsigned*)dnblk, (const unsigned*)dwg_base, (const JOut*)douts, D.coef.as<int16_t>());
  hipLaunchKernelGGL(k_jpeg_dc_totals, dim3(max_chunk, nfu), dim3(kT), 0, st, (const int16_t*)D.coef.as<int16_t>(), dfiles, (const JOut*)douts,
                     D.chunks.as<int>());
  hipLaunchKernelGGL(k_jpeg_dc_chunks, dim3(nfu), dim3(64), 0, st, dfiles, (const JOut*)douts, D.chunks.as<int>());
  hipLaunchKernelGGL(k_jpeg_dc_apply, dim3(max_chunk, nfu), dim3(kT), 0, st, (const int16_t*)D.coef.as<int16_t>(), dfiles, (const JOut*)douts,
                     (const int*)D.chunks.as<int>(), D.dc.as<int>());
  S360_HIP(hipEventRecord(D.ev[1], st));
  hipLaunchKernelGGL(k_jpeg_idct, dim3(max_iblk, nfu), dim3(kT), 0, st, (const int16_t*)D.coef.as<int16_t>(), (const int*)D.dc.as<int>(), dfiles,
                     dtabs, (const JOut*)douts, D.planes.as<uint8_t>());
  for (hipEvent_t e : before)
    if (e) S360_HIP(hipStreamWaitEvent(st, e, 0));
  hipLaunchKernelGGL(k_jpeg_pixels, dim3((unsigned)(max_w + 63) / 64u, (unsigned)(max_h + 3) / 4u, nfu), dim3(64, 4), 0, st,
                     (const uint8_t*)D.planes.as<uint8_t>(), dfiles, (const JOut*)douts);
  S360_HIP(hipEventRecord(D.ev[2], st));
  S360_HIP(hipGetLastError());
  std::vector<JOut> outs(nf);
  std::vector<unsigned> iters(nwg);
  S360_HIP(hipMemcpyAsync(outs.data(), douts, nf * sizeof(JOut), hipMemcpyDeviceToHost, st));
  S360_HIP(hipMemcpyAsync(iters.data(), dwg_iters, nwg * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  S360_HIP(hipStreamSynchronize(st));
  float ms0 = 0, ms1 = 0;
  S360_HIP(hipEventElapsedTime(&ms0, D.ev[0], D.ev[1]));
  S360_HIP(hipEventElapsedTime(&ms1, D.ev[1], D.ev[2]));
  stats.files = nf;
  stats.subsequences = nsub;
  stats.rounds = rounds;
  stats.ms_entropy = ms0;
  stats.ms_pixels = ms1;
  stats.file_rounds.assign(nf, 0);
  for (size_t i = 0; i < nf; ++i) {
    if (!outs[i].marker)
      for (unsigned k = 0; k < jf[i].nwg; ++k) stats.file_rounds[i] = std::max(stats.file_rounds[i], iters[jf[i].wg0 + k]);
    stats.most_file_rounds = std::max<unsigned long long>(stats.most_file_rounds, stats.file_rounds[i]);
  }
  for (size_t i = 0; i < nf; ++i)
    if (const unsigned s = outs[i].status)
      throw JpegDecodeError((int)i, s, "jpeg decode: image " + std::to_string(i) + ": " + (s < sizeof kStatusText / sizeof *kStatusText ? kStatusText[s] : "error"));
  if (coef_tap && tap_image >= 0 && (size_t)tap_image < nf) {
    const JFile& F = jf[(size_t)tap_image];
    std::vector<int> dcv(F.nblocks);
    S360_HIP(hipMemcpyAsync(coef_tap, D.coef.as<int16_t>() + F.coef_off * 64, (size_t)F.nblocks * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    S360_HIP(hipMemcpyAsync(dcv.data(), D.dc.as<int>() + F.coef_off, (size_t)F.nblocks * sizeof(int), hipMemcpyDeviceToHost, st));
    S360_HIP(hipStreamSynchronize(st));
    for (unsigned b = 0; b < F.nblocks; ++b) coef_tap[(size_t)b * 64] = (int16_t)dcv[b];
  }
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
}

}  // namespace s360
