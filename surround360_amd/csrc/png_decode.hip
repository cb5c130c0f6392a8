// png_decode.hip — banded PNG files inflated and unfiltered on the device: the read side of png.hip.
//
// What it replaces: pngio::read_into's parallel band path (host/png_io.hpp:171-221) for the 36 B,G,R,A state images a per-frame
// caller reads back (TRSP:215-235): host threads inflate 919 MB of scanlines per 8K frame and the pixels are uploaded; here the
// 123 MB of file bytes are uploaded and the scanlines never exist on the host.
//
// The file: what png.hip and host/png_io.hpp write — an "sbNd" chunk (rows per band), an IDAT with the zlib header, ONE IDAT PER
// BAND, each a complete byte-aligned raw-deflate segment, an IDAT with the Adler-32 of all filtered scanlines. The host parses the
// container (png_parse_banded) and hands the device a table: per band its segment, its rows, its image.
//
// k_png_inflate — a workgroup of ONE wave per band; the band's filtered scanlines go to a scratch buffer.
//   general path  always correct, serial: stored, fixed and dynamic blocks, any number of them, any distance inside the band's own
//                 output. Lane 0 parses a block header; the 64 lanes build the decode tables in LDS from the code lengths (counts
//                 by atomics, the canonical rank of every symbol, a 10-bit lookup table for the literal/length code and puff-style
//                 count/symbol arrays for codes longer than that and for the distance code); lane 0 walks the tokens. Stored
//                 blocks are copies by all lanes.
//   fast path     for what png.hip writes (and zlib at Z_RLE, Z_FIXED, Z_HUFFMAN_ONLY): one Huffman block, closed by the empty
//                 stored block or final, every match at distance 1. The block body is taken in windows of 64 x 256 bits. Lane i
//                 starts at bit 256 i of the window (lane 0 at the true start), decodes whole tokens up to the first token
//                 boundary at or beyond lane i + 1's nominal start and records its exit bit, output bytes and last literal. Lane
//                 i + 1 takes lane i's exit as its start and decodes again if that changed; a ballot ends the loop when nothing
//                 changed. After round k lanes 0..k are right, so the loop ends within 65 rounds with the serial result whatever
//                 the data; how soon the codes resynchronise decides the speed only. A prefix sum of the counts gives the output
//                 offsets, a scan of "last literal" the byte a lane that starts with a match repeats; every lane then decodes its
//                 span once more and writes its bytes. A band that shows anything else (a second block, another distance, an
//                 invalid code, too much or too little output) is REDONE on the general path by the same wave, which also names
//                 the error.
//   Both paths read the segment through an LDS stage of 520 dwords and write through an LDS window of 16 KB that goes to HBM as
//   whole dwords, coalesced, when it is full. Every read is bounded by the segment's length (rounded to a dword), every write by
//   rows x line, every loop by one of the two (a token takes at least one bit, a block three); a band that would cross either
//   bound, ends short, has an invalid code-length set, a reserved block type or a bad LEN/NLEN sets its status word and stops.
// k_png_unfilter — a workgroup of 256 threads per band, a thread per pixel: Sub (type 1) is a running byte-wise sum per channel
//   along the row = a wave scan over the pixels' dwords with byte-wise adds, the waves' totals and the tile's carry through LDS;
//   type 0 rows are copied; R and B swap on the way out, alpha stays; any other filter type sets the band's status (unsupported,
//   as the host's parallel reader bails out). It also sums the band's Adler-32 pieces (s1, s2) for the host to combine.
//   The band's image picks one instantiation of unfilter_band<layout, store>. Layouts: 3 and 4 bytes per pixel (8-bit R,G,B(,A)) and
//   6 (16-bit R,G,B, high byte first, Sub at a distance of 6: what k_png_band<6> of png.hip writes for the camera images); a pixel's
//   6 bytes start at any byte offset and are loaded as two or three dwords, each of which holds a byte of that pixel. Stores: packed
//   8-bit B,G,R(,A) (a 16-bit file keeps its high bytes: png_set_strip_16), packed little-endian uint16 B,G,R, and a frame's source
//   slots written directly — a side slot, uchar4 with side_src_alpha's row ramp (render_kernels.hpp, shared with
//   k_prepare_side_src), and a pole slot, uchar4 with alpha 255 — with no B,G,R intermediate (s360_frame_upload_png). The Adler-32
//   is over all 6 bytes whatever the store keeps; the stores that keep high bytes scan byte lanes 0, 2, 4 packed into one dword.
//   Resources (gfx950, -Rpass-analysis=kernel-resource-usage): 45 VGPRs, 71 SGPRs, 40 bytes of LDS, no scratch, 8 waves per SIMD
//   (with layouts 3 and 4 alone: 43 VGPRs, 76 SGPRs, 24 bytes of LDS); k_png_inflate is unchanged at 181 VGPRs, 106 SGPRs,
//   21 884 bytes of LDS, no scratch.
//   Two kernels, not one: the fused form (unfilter out of the LDS window) was not built, so there is no measurement of it.
// Measured (profiles/state_png_read.txt, the 36 state images of an 8K frame, 6000 bands, all on the fast path): k_png_inflate
// 85.5-86.7 ms, k_png_unfilter 0.76 ms. The round count (rounds up to the last one in which a lane decoded again, + 1) says why the
// inflate is slow: in 3203 of the 6000 bands some window took all 65 rounds and in 5465 more than 60 — these codes do NOT resynchronise
// within a lane's 256 bits, a wrong start moves down the lanes one per round and the window is decoded serially, 64 times over. A
// span of 1024 bits resynchronises more often (74 bands at 3 rounds) and is slower, 125.8-128.5 ms (profiles/state_png_read_span1024.txt):
// not adopted.
#include "png_decode.hpp"

#include <cstring>
#include <string>

#include "../../include/s360.h"
#include "render_kernels.hpp"

namespace s360 {

namespace {
constexpr int kWinBytes = 16384;                 // the output window in LDS
constexpr unsigned kSpan = 256;                  // fast path: bits of the block body per lane and window
constexpr int kCinWords = 64 * kSpan / 32 + 8;   // staged dwords of the segment: a window + the last lane's overrun (< 48 bits) + slack
constexpr int kLutBits = 10;
constexpr unsigned kAdler = 65521u;
constexpr unsigned kRetry = 0xFFFFu;             // fast path: redo the band on the general path

enum Status : unsigned {
  kOk = 0, kInputShort = 1, kOutputOver = 2, kBadLengths = 3, kBadBlockType = 4, kBadStoredLen = 5, kBadCode = 6, kBadDistance = 7,
  kOutputShort = 8, kBadFilter = 9
};
const char* const kStatusText[] = {"ok", "the segment ends short", "more output than rows x line", "invalid code-length set",
                                   "reserved block type", "stored block LEN/NLEN mismatch", "invalid code", "distance beyond the band's output",
                                   "less output than rows x line", "unsupported filter type"};

struct DecBand {
  unsigned long long comp_off, filt_off;  // the segment in the files' buffer; the band's filtered scanlines in the scratch (16-byte aligned)
  unsigned comp_len, n, y0, rows;         // n = rows x line
  int img, pad;
};
struct DecImage {
  uint8_t* dst;
  int w, h, pix;  // pix: bytes per pixel in the file (3, 4, or 6 for 16-bit R,G,B)
  unsigned line;
  int store, feather;  // PngStore; kPngStoreSide: side_alpha_feather_size
};
struct DecOut {
  unsigned status, s1, s2, path, rounds, pad;  // path: 1 fast, 2 general, 3 stored blocks only
};

struct DSmem {
  unsigned win[kWinBytes / 4];
  unsigned cin[kCinWords];
  unsigned short lut[1 << kLutBits];  // literal/length code, codes of up to 10 bits: symbol << 4 | length (0: longer or invalid)
  unsigned short sortedL[288], sortedD[32], sortedC[20];
  unsigned cntL[16], cntD[16], cntC[16];
  unsigned short offL[16], offD[16], nextL[16];
  unsigned char lens[320];  // code lengths: literal/length symbols at 0, distance symbols at 288
  unsigned char cl[20];
  unsigned ctl[16];
};
struct Band {
  const unsigned* words;  // the segment's dwords from the aligned address in front of it
  const uint8_t* bytes;   // the same address as bytes
  unsigned nwords, startbit, endbit, n;
  uint8_t* out;
};

__device__ inline int lane_id() { return (int)threadIdx.x & 63; }
__device__ inline unsigned shfl_up(unsigned v, int d) {
  const int l = lane_id();
  const unsigned t = (unsigned)__builtin_amdgcn_ds_bpermute(((l - d) & 63) << 2, (int)v);
  return l >= d ? t : v;
}
__device__ inline unsigned scan_add(unsigned v) {
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = shfl_up(v, d);
    if (lane_id() >= d) v += t;
  }
  return v;
}
__device__ inline unsigned rev_bits(unsigned c, int n) {
  unsigned r = 0;
  for (int i = 0; i < n; ++i) { r = (r << 1) | (c & 1u); c >>= 1; }
  return r;
}

// dwords [w0, w0 + kCinWords) of the segment into S.cin (zero behind the segment's end)
__device__ inline void stage(DSmem& S, const Band& X, unsigned w0) {
  __syncthreads();
  for (int i = lane_id(); i < kCinWords; i += 64) {
    const unsigned w = w0 + (unsigned)i;
    S.cin[i] = w < X.nwords ? X.words[w] : 0u;
  }
  __syncthreads();
}
// >= 32 bits of the segment from bit `bitpos` on, low bit first (the index is clamped to the stage: no read outside S.cin)
__device__ inline unsigned peek(const DSmem& S, unsigned w0, unsigned bitpos) {
  const unsigned i = min((bitpos >> 5) - w0, (unsigned)kCinWords - 2u), sh = bitpos & 31u;
  return (unsigned)(((((unsigned long long)S.cin[i + 1]) << 32) | S.cin[i]) >> sh);
}
// canonical decode from count / sorted-symbol arrays, one bit at a time (puff.c's way): the symbol, its length in n; -1: no such code
__device__ inline int slow_decode(const unsigned* cnt, const unsigned short* sorted, unsigned v, int& n) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)(v & 1u);
    v >>= 1;
    const int c = (int)cnt[l];
    if (code - c < first) { n = l; return sorted[index + (code - first)]; }
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}
// One token at `bitpos`: 0..255 a literal, 256 end of block, 257 a match (len, dist), -1 an invalid code. Advances bitpos.
__device__ inline int next_token(const DSmem& S, unsigned w0, unsigned& bitpos, unsigned& len, unsigned& dist) {
  unsigned v = peek(S, w0, bitpos);
  int sym, n = 0;
  const unsigned e = S.lut[v & ((1u << kLutBits) - 1u)];
  if (e & 15u) { sym = (int)(e >> 4); n = (int)(e & 15u); }
  else {
    sym = slow_decode(S.cntL, S.sortedL, v, n);
    if (sym < 0) return -1;
  }
  bitpos += (unsigned)n;
  if (sym <= 256) return sym;
  if (sym > 285) return -1;
  v >>= n;  // >= 17 bits left, at most 5 needed
  unsigned eb = 0;
  if (sym < 265) len = (unsigned)sym - 254u;
  else if (sym == 285) len = 258u;
  else {
    eb = (unsigned)(sym - 261) >> 2;
    len = 3u + ((4u + ((unsigned)(sym - 261) & 3u)) << eb) + (v & ((1u << eb) - 1u));
  }
  bitpos += eb;
  v = peek(S, w0, bitpos);
  const int ds = slow_decode(S.cntD, S.sortedD, v, n);
  if (ds < 0 || ds > 29) return -1;
  bitpos += (unsigned)n;
  v >>= n;  // >= 17 bits left, at most 13 needed
  if (ds < 4) { dist = (unsigned)ds + 1u; return 257; }
  eb = ((unsigned)ds >> 1) - 1u;
  dist = 1u + ((2u + ((unsigned)ds & 1u)) << eb) + (v & ((1u << eb) - 1u));
  bitpos += eb;
  return 257;
}

// counts, first codes and offsets of one code (lane 0); false: over-subscribed, or incomplete with more than one code
__device__ inline bool code_shape(const unsigned* cnt, unsigned short* off, unsigned short* next) {
  int left = 1, maxl = 0;
  unsigned code = 0, o = 0;
  for (int l = 1; l <= 15; ++l) {
    left = (left << 1) - (int)cnt[l];
    if (left < 0) return false;
    if (cnt[l]) maxl = l;
    off[l] = (unsigned short)o;
    o += cnt[l];
    code = (code + (l > 1 ? cnt[l - 1] : 0u)) << 1;
    if (next) next[l] = (unsigned short)code;
  }
  return left == 0 || maxl <= 1;
}
// The decode tables of a block from S.lens, by all lanes. Returns the status (the same in every lane).
__device__ inline unsigned build_tables(DSmem& S) {
  const int lane = lane_id();
  __syncthreads();
  if (lane < 16) { S.cntL[lane] = 0u; S.cntD[lane] = 0u; }
  for (int i = lane; i < (1 << kLutBits); i += 64) S.lut[i] = 0;
  __syncthreads();
  for (int s = lane; s < 320; s += 64) {
    const int l = S.lens[s];
    if (l) atomicAdd(s < 288 ? &S.cntL[l] : &S.cntD[l], 1u);
  }
  __syncthreads();
  if (lane == 0) {
    const bool okL = code_shape(S.cntL, S.offL, S.nextL), okD = code_shape(S.cntD, S.offD, nullptr);
    S.ctl[0] = (okL && okD && S.lens[256] != 0) ? kOk : kBadLengths;  // (no end-of-block code: zlib's "missing end-of-block")
  }
  __syncthreads();
  const unsigned status = S.ctl[0];
  if (status) return status;
  for (int s = lane; s < 320; s += 64) {
    const int l = S.lens[s];
    if (!l) continue;
    const int base = s < 288 ? 0 : 288;
    unsigned before = 0;
    for (int j = base; j < s; ++j) before += S.lens[j] == l ? 1u : 0u;
    if (s < 288) {
      S.sortedL[S.offL[l] + before] = (unsigned short)s;
      if (l <= kLutBits) {
        const unsigned r = rev_bits((unsigned)S.nextL[l] + before, l);
        for (unsigned k = r; k < (1u << kLutBits); k += 1u << l) S.lut[k] = (unsigned short)((s << 4) | l);
      }
    } else {
      S.sortedD[S.offD[l] + before] = (unsigned short)(s - 288);
    }
  }
  __syncthreads();
  return kOk;
}
__device__ inline void fixed_lengths(DSmem& S) {
  for (int s = lane_id(); s < 320; s += 64) S.lens[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
}
// A block header at `bitpos`, by lane 0 out of the stage at w0: S.ctl[0] status, [1] BTYPE, [2] BFINAL, [3] the bit behind the
// header, [4] a stored block's LEN; a dynamic block's code lengths go to S.lens. `room`: bytes the band's output may still take.
__device__ inline void parse_header(DSmem& S, const Band& X, unsigned w0, unsigned bitpos, unsigned room) {
  unsigned v = peek(S, w0, bitpos);
  const unsigned bfinal = v & 1u, btype = (v >> 1) & 3u;
  unsigned status = kOk, slen = 0;
  bitpos += 3;
  if (btype == 3) status = kBadBlockType;
  else if (btype == 0) {
    bitpos = (bitpos + 7u) & ~7u;
    if (bitpos + 32u > X.endbit) status = kInputShort;
    else {
      v = peek(S, w0, bitpos);
      slen = v & 0xffffu;
      bitpos += 32;
      if ((slen ^ 0xffffu) != (v >> 16)) status = kBadStoredLen;
      else if (8u * slen > X.endbit - bitpos) status = kInputShort;
      else if (slen > room) status = kOutputOver;
    }
  } else if (btype == 2) {
    v = peek(S, w0, bitpos);
    const unsigned hlit = (v & 31u) + 257u, hdist = ((v >> 5) & 31u) + 1u, hclen = ((v >> 10) & 15u) + 4u;
    bitpos += 14;
    if (hlit > 286u || hdist > 30u) status = kBadLengths;
    else {
      for (int i = 0; i < 20; ++i) S.cl[i] = 0;
      for (int i = 0; i < 16; ++i) S.cntC[i] = 0u;
      for (int i = 0; i < 320; ++i) S.lens[i] = 0;
      for (unsigned i = 0; i < hclen; ++i) {
        // the order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const unsigned j = i - 4u, sym = i < 3 ? 16u + i : i == 3 ? 0u : (j & 1u) ? 7u - (j >> 1) : 8u + (j >> 1);
        const unsigned l = peek(S, w0, bitpos) & 7u;
        bitpos += 3;
        S.cl[sym] = (unsigned char)l;
        if (l) S.cntC[l] += 1u;
      }
      unsigned short* offC = S.offD;  // (build_tables makes the distance code's offsets afterwards)
      int left = 1;
      unsigned o = 0;
      for (int l = 1; l <= 15; ++l) {  // (the code-length code must be complete: zlib's rule for it)
        left = (left << 1) - (int)S.cntC[l];
        offC[l] = (unsigned short)o;
        o += S.cntC[l];
        if (left < 0) break;
      }
      if (left != 0) status = kBadLengths;
      else {
        for (int l = 1; l <= 7; ++l)
          for (unsigned s = 0, k = 0; s < 19; ++s)
            if (S.cl[s] == l) S.sortedC[offC[l] + k++] = (unsigned short)s;
        unsigned k = 0, prev = 0;
        const unsigned total = hlit + hdist;
        while (k < total && !status) {
          int n = 0;
          const unsigned vv = peek(S, w0, bitpos);
          const int sym = slow_decode(S.cntC, S.sortedC, vv, n);
          if (sym < 0) { status = kBadLengths; break; }
          bitpos += (unsigned)n;
          unsigned rep = 1, val = (unsigned)sym;
          if (sym == 16) {
            if (k == 0) { status = kBadLengths; break; }
            val = prev;
            rep = 3u + ((vv >> n) & 3u);
            bitpos += 2;
          } else if (sym == 17) {
            val = 0;
            rep = 3u + ((vv >> n) & 7u);
            bitpos += 3;
          } else if (sym == 18) {
            val = 0;
            rep = 11u + ((vv >> n) & 127u);
            bitpos += 7;
          }
          if (k + rep > total) { status = kBadLengths; break; }
          for (unsigned q = 0; q < rep; ++q, ++k) S.lens[k < hlit ? k : 288u + (k - hlit)] = (unsigned char)val;
          prev = val;
        }
        if (!status && bitpos > X.endbit) status = kInputShort;
      }
    }
  }
  S.ctl[0] = status; S.ctl[1] = btype; S.ctl[2] = bfinal; S.ctl[3] = bitpos; S.ctl[4] = slen;
}
// the window's first `nbytes` bytes to the band's output at `wb`, as whole dwords (the band's scratch is padded to 16 bytes)
__device__ inline void flush(DSmem& S, const Band& X, unsigned wb, unsigned nbytes) {
  unsigned* g = reinterpret_cast<unsigned*>(X.out + wb);
  const unsigned nw = (nbytes + 3u) >> 2;
  for (unsigned i = (unsigned)lane_id(); i < nw; i += 64u) g[i] = S.win[i];
  __syncthreads();
}

// ---- the general path ------------------------------------------------------------------------------------------------------
__device__ unsigned general_path(DSmem& S, const Band& X, bool& stored_only) {
  const int lane = lane_id();
  constexpr unsigned W = kWinBytes;
  uint8_t* winb = reinterpret_cast<uint8_t*>(S.win);
  unsigned bitpos = X.startbit, opos = 0, status = kOk;
  stored_only = true;
  for (;;) {  // blocks: each takes at least 3 bits
    if (bitpos + 3u > X.endbit) break;  // the segment is used up (a sync-flushed band has no final block)
    const unsigned w0 = bitpos >> 5;
    stage(S, X, w0);
    if (lane == 0) parse_header(S, X, w0, bitpos, X.n - opos);
    __syncthreads();
    status = S.ctl[0];
    if (status) break;
    const unsigned btype = S.ctl[1], bfinal = S.ctl[2], slen = S.ctl[4];
    bitpos = S.ctl[3];
    if (btype == 0) {  // a copy by all lanes, through the window
      const uint8_t* src = X.bytes + (bitpos >> 3);
      for (unsigned done = 0; done < slen;) {
        const unsigned wb = opos & ~(W - 1u), k = min(wb + W - opos, slen - done);
        for (unsigned i = (unsigned)lane; i < k; i += 64u) winb[opos - wb + i] = src[done + i];
        __syncthreads();
        opos += k;
        done += k;
        if ((opos & (W - 1u)) == 0u) flush(S, X, wb, W);
      }
      bitpos += 8u * slen;
    } else {
      stored_only = false;
      if (btype == 1) fixed_lengths(S);
      status = build_tables(S);
      if (status) break;
      unsigned pend = 0, pdist = 0;  // lane 0: what is left of a match that crossed the window's end
      bool eob = false;
      while (!eob) {  // rounds: each ends at a full window (16 KB of output), a used-up stage (2 KB of input) or the block's end
        const unsigned s0 = bitpos >> 5;
        stage(S, X, s0);
        if (lane == 0) {
          const unsigned wb = opos & ~(W - 1u), wend = wb + W;
          unsigned reason = 0, st = kOk;  // reason 1: end of block, 2: the window is full
          for (;;) {
            for (; pend && opos < wend; ++opos, --pend) {
              const unsigned sp = opos - pdist;
              winb[opos - wb] = sp >= wb ? winb[sp - wb] : X.out[sp];
            }
            if (opos == wend) { reason = 2; break; }
            if ((bitpos >> 5) - s0 > (unsigned)kCinWords - 4u) break;
            unsigned len = 0, dist = 0;
            const int tok = next_token(S, s0, bitpos, len, dist);
            if (tok < 0) { st = kBadCode; break; }
            if (bitpos > X.endbit) { st = kInputShort; break; }
            if (tok == 256) { reason = 1; break; }
            if (tok < 256) {
              if (opos >= X.n) { st = kOutputOver; break; }
              winb[opos - wb] = (uint8_t)tok;
              ++opos;
            } else {
              if (dist > opos) { st = kBadDistance; break; }
              if (len > X.n - opos) { st = kOutputOver; break; }
              pend = len;
              pdist = dist;
            }
          }
          S.ctl[0] = st; S.ctl[1] = reason; S.ctl[3] = bitpos; S.ctl[5] = opos;
        }
        __syncthreads();
        status = S.ctl[0];
        if (status) break;
        eob = S.ctl[1] == 1u;
        bitpos = S.ctl[3];
        opos = S.ctl[5];
        if (S.ctl[1] == 2u) flush(S, X, opos - W, W);
      }
      if (status) break;
    }
    if (bfinal) break;
  }
  if (!status) {
    const unsigned wb = opos & ~(W - 1u);
    if (opos > wb) flush(S, X, wb, opos - wb);
    if (opos != X.n) status = kOutputShort;
  }
  return status;
}

// ---- the fast path ---------------------------------------------------------------------------------------------------------
constexpr unsigned kFEob = 1u, kFErr = 2u, kFDone = 4u;
constexpr unsigned kNoStart = 0xFFFFFFFFu;

__device__ unsigned fast_path(DSmem& S, const Band& X, unsigned& most_rounds) {
  const int lane = lane_id();
  constexpr unsigned W = kWinBytes;
  uint8_t* winb = reinterpret_cast<uint8_t*>(S.win);
  if (X.startbit + 3u > X.endbit) return kRetry;
  stage(S, X, X.startbit >> 5);
  if (lane == 0) parse_header(S, X, X.startbit >> 5, X.startbit, X.n);
  __syncthreads();
  if (S.ctl[0] || S.ctl[1] == 0u) return kRetry;  // (the general path names the error; stored blocks are its copies)
  const unsigned bfinal = S.ctl[2];
  unsigned wstart = S.ctl[3];
  if (S.ctl[1] == 1u) fixed_lengths(S);
  if (build_tables(S)) return kRetry;

  unsigned opos = 0;
  int lastb = -1;  // the last byte of the output so far
  for (;;) {       // windows of 64 x kSpan bits: each advances by at least that much or ends the block
    if (wstart >= X.endbit) return kRetry;
    const unsigned w0 = wstart >> 5;
    stage(S, X, w0);
    const unsigned stop = wstart + ((unsigned)lane + 1u) * kSpan;
    unsigned start = wstart + (unsigned)lane * kSpan, exitb = 0, cnt = 0, flags = 0, round = 0;
    int lastlit = -1;
    bool redo = true;
    unsigned decoded = 0;  // rounds up to the last one in which a lane decoded its span (again)
    for (; round < 66u; ++round) {
      // (behind the lane that saw the end of the block, "nothing left" walks down the lanes one per round: rounds without a decode,
      // which the statistic leaves out — it is about how soon the codes resynchronise)
      if (__ballot(redo && start != kNoStart)) decoded = round + 1u;
      if (redo) {
        cnt = 0; lastlit = -1; flags = 0; exitb = start;
        if (start == kNoStart) flags = kFDone;
        else {
          unsigned bp = start;
          while (bp < stop) {
            if (bp >= X.endbit) { flags = kFErr; break; }
            unsigned len = 0, dist = 0;
            const int tok = next_token(S, w0, bp, len, dist);
            if (tok < 0 || bp > X.endbit) { flags = kFErr; break; }
            if (tok == 256) { flags = kFEob; break; }
            if (tok < 256) { lastlit = tok; ++cnt; }
            else if (dist != 1u) { flags = kFErr; break; }
            else cnt += len;
          }
          exitb = bp;
        }
      }
      const unsigned pe = shfl_up(exitb, 1), pf = shfl_up(flags, 1);
      const unsigned ns = lane == 0 ? start : (pf & (kFEob | kFErr | kFDone)) ? kNoStart : pe;
      redo = ns != start;
      start = ns;
      if (!__ballot(redo)) break;
    }
    most_rounds = max(most_rounds, decoded + 1u);  // + the round that found no start changed
    if (__ballot((flags & kFErr) != 0u)) return kRetry;
    // output offsets, the byte in front of every lane's span
    const unsigned incl = scan_add(cnt);
    unsigned ll = (unsigned)lastlit;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = shfl_up(ll, d);
      if (lane >= d && (int)ll < 0) ll = t;
    }
    int cur = (int)shfl_up(ll, 1);
    if (lane == 0 || cur < 0) cur = lastb;
    const unsigned long long eobs = __ballot((flags & kFEob) != 0u);
    __syncthreads();
    if (lane == 63) { S.ctl[7] = incl; S.ctl[8] = exitb; S.ctl[9] = (int)ll < 0 ? (unsigned)lastb : ll; }
    if (eobs && lane == __ffsll((long long)eobs) - 1) S.ctl[10] = exitb;
    __syncthreads();
    const unsigned total = S.ctl[7];
    if (total > X.n - opos) return kRetry;
    // every lane's span once more, its bytes into the window
    const unsigned target = opos + total;
    unsigned bp = start, myo = opos + incl - cnt, pend = 0;
    const bool active = !(flags & kFDone);
    bool err = false;
    for (;;) {  // passes: one per output window the bytes reach into
      const unsigned wb = opos & ~(W - 1u), wend = wb + W;
      if (active && !err)
        for (;;) {
          for (; pend && myo < wend; ++myo, --pend) winb[myo - wb] = (uint8_t)cur;
          if (pend || bp >= exitb) break;
          unsigned len = 0, dist = 0;
          const int tok = next_token(S, w0, bp, len, dist);
          if (tok == 256 || tok < 0) break;
          if (tok < 256) { cur = tok; pend = 1; }
          else if (cur < 0) { err = true; break; }  // a match in front of the band's first byte
          else pend = len;
        }
      __syncthreads();
      const unsigned reached = min(target, wend);
      if (reached == wend) flush(S, X, wb, W);
      opos = reached;
      if (opos == target) break;
    }
    if (__ballot(err)) return kRetry;
    lastb = (int)S.ctl[9];
    if (eobs) { wstart = S.ctl[10]; break; }
    wstart = S.ctl[8];
  }
  {
    const unsigned wb = opos & ~(W - 1u);
    if (opos > wb) flush(S, X, wb, opos - wb);
  }
  if (opos != X.n) return kRetry;  // more blocks, or too little: the general path finds out
  if (!bfinal) {  // what must follow: the empty stored block of a sync flush, then nothing
    const unsigned p = (wstart + 3u + 7u) & ~7u;
    if (p + 32u != X.endbit) return kRetry;
    stage(S, X, wstart >> 5);
    if ((peek(S, wstart >> 5, wstart) & 7u) != 0u || peek(S, wstart >> 5, p) != 0xFFFF0000u) return kRetry;
  }
  return kOk;
}

__global__ __launch_bounds__(64) void k_png_inflate(const uint8_t* __restrict__ comp, const DecBand* __restrict__ bands,
                                                     uint8_t* __restrict__ filt, DecOut* __restrict__ outs, unsigned* __restrict__ stats) {
  __shared__ DSmem S;
  const DecBand B = bands[blockIdx.x];
  Band X;
  const unsigned long long a0 = B.comp_off & ~3ull;
  X.bytes = comp + a0;
  X.words = reinterpret_cast<const unsigned*>(comp + a0);
  X.startbit = 8u * (unsigned)(B.comp_off - a0);
  X.endbit = X.startbit + 8u * B.comp_len;
  X.nwords = (X.endbit + 31u) >> 5;
  X.n = B.n;
  X.out = filt + B.filt_off;
  if (threadIdx.x < 16) S.ctl[threadIdx.x] = 0u;
  unsigned rounds = 0, path = 1;
  unsigned status = fast_path(S, X, rounds);
  if (status == kRetry) {
    bool stored_only = true;
    status = general_path(S, X, stored_only);
    path = stored_only ? 3u : 2u;
  }
  if (threadIdx.x == 0) {
    DecOut o;
    o.status = status; o.s1 = 0; o.s2 = 0; o.path = path; o.rounds = rounds; o.pad = 0;
    outs[blockIdx.x] = o;
    atomicAdd(&stats[path - 1u], 1u);
    if (path == 1u) {
      atomicMax(&stats[3], rounds);
      atomicAdd(&stats[4 + min(rounds, 65u)], 1u);
    }
  }
}

// ---- unfilter, R <-> B, Adler-32 pieces ---------------------------------------------------------------------------------------
__device__ inline unsigned badd(unsigned a, unsigned b) {  // four byte-wise sums mod 256
  return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
}
constexpr int kUT = 256;
// Sub over one tile of a row: x[] becomes the byte-wise running sum of the pixels up to this thread's (a wave scan, the waves' totals
// and the tile's carry through LDS), carry[] the sum up to the tile's last pixel. NX dwords per pixel, every byte a lane of its own.
template <int NX>
__device__ inline void sub_scan(unsigned (&x)[NX], unsigned (&carry)[NX], unsigned (*wtot)[kUT / 64], int lane, int wv) {
  for (int d = 1; d < 64; d <<= 1)
    for (int k = 0; k < NX; ++k) {
      const unsigned q = (unsigned)__builtin_amdgcn_ds_bpermute(((lane - d) & 63) << 2, (int)x[k]);
      if (lane >= d) x[k] = badd(x[k], q);
    }
  if (lane == 63)
    for (int k = 0; k < NX; ++k) wtot[k][wv] = x[k];
  __syncthreads();
  for (int k = 0; k < NX; ++k) {
    unsigned pre = carry[k], all = carry[k];
    for (int j = 0; j < kUT / 64; ++j) {
      if (j < wv) pre = badd(pre, wtot[k][j]);
      all = badd(all, wtot[k][j]);
    }
    x[k] = badd(x[k], pre);
    carry[k] = all;
  }
  __syncthreads();
}
// One band of an image of L bytes per pixel (3: R,G,B; 4: R,G,B,A; 6: R,G,B of 16 bits, high byte first) into store S. The
// Adler-32 pieces are over every byte of the scanlines whatever the store keeps. Sub has no carries between byte lanes, so the
// stores that keep a 16-bit file's high bytes scan byte lanes 0, 2 and 4 only, packed into one dword: the scan of layout 3.
template <int L, int S>
__device__ inline void unfilter_band(const uint8_t* __restrict__ src, const DecBand& B, const DecImage& I, DecOut* __restrict__ out,
                                     unsigned (*wtot)[kUT / 64], unsigned* acc) {
  constexpr int NX = (L == 6 && S == kPngStoreU16) ? 2 : 1;
  static_assert(S == kPngStoreBytes || (S == kPngStoreU16 && L == 6) || ((S == kPngStoreSide || S == kPngStorePole) && L != 4), "no such store");
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const unsigned line = I.line, n = B.n;
  const unsigned* srcw = reinterpret_cast<const unsigned*>(src);  // 16-byte aligned, padded to 16 bytes behind n
  unsigned long long sum = 0, wsum = 0;
  for (unsigned r = 0; r < B.rows; ++r) {
    const unsigned rowoff = r * line;
    const unsigned f = src[rowoff];
    if (f > 1u) {  // (the same for every thread)
      if (t == 0) out->status = kBadFilter;
      return;
    }
    if (t == 0) { sum += f; wsum += (unsigned long long)(n - rowoff) * f; }
    const int y = (int)(B.y0 + r);
    const size_t drow = (size_t)y * (size_t)I.w;
    const unsigned alpha = S == kPngStoreSide ? (unsigned)side_src_alpha(y, I.h, I.feather, 255) : 255u;
    unsigned carry[NX] = {};
    for (int p0 = 0; p0 < I.w; p0 += kUT) {
      const int p = p0 + t;
      unsigned x[NX] = {};
      if (p < I.w) {
        const unsigned boff = rowoff + 1u + (unsigned)L * (unsigned)p, sh = 8u * (boff & 3u), wi = boff >> 2;
        const unsigned w0 = srcw[wi];
        if (L == 6) {
          // 6 bytes from any byte offset: two dwords, a third only where the pixel reaches into it (every dword read holds a
          // byte of this pixel, so none lies behind the band's padded scanlines)
          const unsigned w1 = srcw[wi + 1u], w2 = (boff & 3u) == 3u ? srcw[wi + 2u] : 0u;
          const unsigned lo = (unsigned)(((((unsigned long long)w1) << 32) | w0) >> sh);
          const unsigned hi = (unsigned)(((((unsigned long long)w2) << 32) | w1) >> sh) & 0xffffu;
          const unsigned b0 = lo & 255u, b1 = (lo >> 8) & 255u, b2 = (lo >> 16) & 255u, b3 = lo >> 24, b4 = hi & 255u, b5 = hi >> 8;
          const unsigned s = b0 + b1 + b2 + b3 + b4 + b5;
          sum += s;
          wsum += (unsigned long long)(n - boff) * s - (b1 + 2u * b2 + 3u * b3 + 4u * b4 + 5u * b5);
          if (NX == 2) { x[0] = lo; x[NX - 1] = hi; }
          else x[0] = b0 | (b2 << 8) | (b4 << 16);
        } else {
          const unsigned hi = (boff & 3u) + (unsigned)L > 4u ? srcw[wi + 1u] : 0u;
          unsigned v = (unsigned)(((((unsigned long long)hi) << 32) | w0) >> sh);
          if (L == 3) v &= 0xffffffu;
          const unsigned b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24, s = b0 + b1 + b2 + b3;
          sum += s;
          wsum += (unsigned long long)(n - boff) * s - (b1 + 2u * b2 + 3u * b3);
          x[0] = v;
        }
      }
      if (f == 1u) sub_scan<NX>(x, carry, wtot, lane, wv);
      if (p < I.w) {
        const unsigned v = x[0];  // bytes R, G, B (, A)
        if (S == kPngStoreU16) {
          const unsigned h2 = x[NX - 1];
          unsigned short* o = reinterpret_cast<unsigned short*>(I.dst) + (drow + (size_t)p) * 3;
          o[0] = (unsigned short)(((h2 & 255u) << 8) | ((h2 >> 8) & 255u));
          o[1] = (unsigned short)(((v >> 8) & 0xff00u) | (v >> 24));
          o[2] = (unsigned short)(((v & 255u) << 8) | ((v >> 8) & 255u));
        } else if (S == kPngStoreSide || S == kPngStorePole) {
          reinterpret_cast<unsigned*>(I.dst)[drow + (size_t)p] = (v & 0xff00u) | ((v >> 16) & 255u) | ((v & 255u) << 16) | (alpha << 24);
        } else if (L == 4) {
          reinterpret_cast<unsigned*>(I.dst)[drow + (size_t)p] = (v & 0xff00ff00u) | ((v >> 16) & 255u) | ((v & 255u) << 16);
        } else {
          uint8_t* o = I.dst + (drow + (size_t)p) * 3;
          o[0] = (uint8_t)(v >> 16); o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)v;
        }
      }
    }
    wsum %= kAdler;
  }
  atomicAdd(&acc[0], (unsigned)(sum % kAdler));
  atomicAdd(&acc[1], (unsigned)(wsum % kAdler));
  __syncthreads();
  if (t == 0) { out->s1 = acc[0] % kAdler; out->s2 = acc[1] % kAdler; }
}
// A workgroup per band; the band's image says which instantiation runs (the same for every thread of the workgroup).
__global__ __launch_bounds__(kUT) void k_png_unfilter(const uint8_t* __restrict__ filt, const DecBand* __restrict__ bands,
                                                       const DecImage* __restrict__ imgs, DecOut* __restrict__ outs) {
  __shared__ unsigned wtot[2][kUT / 64];
  __shared__ unsigned acc[2];
  const int b = blockIdx.x, t = threadIdx.x;
  if (outs[b].status) return;
  const DecBand B = bands[b];
  const DecImage I = imgs[B.img];
  const uint8_t* src = filt + B.filt_off;  // 16-byte aligned
  if (t < 2) acc[t] = 0u;
  __syncthreads();
  switch (I.store * 8 + I.pix) {
    case kPngStoreBytes * 8 + 3: unfilter_band<3, kPngStoreBytes>(src, B, I, outs + b, wtot, acc); break;
    case kPngStoreBytes * 8 + 4: unfilter_band<4, kPngStoreBytes>(src, B, I, outs + b, wtot, acc); break;
    case kPngStoreBytes * 8 + 6: unfilter_band<6, kPngStoreBytes>(src, B, I, outs + b, wtot, acc); break;
    case kPngStoreU16 * 8 + 6: unfilter_band<6, kPngStoreU16>(src, B, I, outs + b, wtot, acc); break;
    case kPngStoreSide * 8 + 3: unfilter_band<3, kPngStoreSide>(src, B, I, outs + b, wtot, acc); break;
    case kPngStoreSide * 8 + 6: unfilter_band<6, kPngStoreSide>(src, B, I, outs + b, wtot, acc); break;
    case kPngStorePole * 8 + 3: unfilter_band<3, kPngStorePole>(src, B, I, outs + b, wtot, acc); break;
    case kPngStorePole * 8 + 6: unfilter_band<6, kPngStorePole>(src, B, I, outs + b, wtot, acc); break;
    default:  // (png_decode_run refuses every other pair)
      if (t == 0) outs[b].status = kBadFilter;
  }
}

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
bool parse_banded(const uint8_t* file, size_t n, PngBandedInfo& info, bool allow16);
}  // namespace

bool png_parse_banded(const uint8_t* file, size_t n, PngBandedInfo& info) { return parse_banded(file, n, info, false); }
bool png_parse_banded_input(const uint8_t* file, size_t n, PngBandedInfo& info) { return parse_banded(file, n, info, true); }

namespace {
bool parse_banded(const uint8_t* file, size_t n, PngBandedInfo& info, bool allow16) {
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  if (!file || n < 8 || std::memcmp(file, sig, 8) != 0) return false;
  size_t pos = 8;
  uint32_t w = 0, h = 0, band_rows = 0;
  int ctype = -1, depth = 8;
  bool have_ihdr = false;
  std::vector<std::pair<size_t, size_t>> idat;
  while (pos + 12 <= n) {
    const uint32_t len = be32(file + pos);
    const uint8_t* type = file + pos + 4;
    const uint8_t* data = file + pos + 8;
    if (len > n || pos + 12 + len > n) break;
    if (!std::memcmp(type, "IHDR", 4)) {
      if (len < 13) return false;
      w = be32(data); h = be32(data + 4);
      if (w == 0 || h == 0 || w > 65535u || h > 65535u) return false;
      if ((data[9] != 2 && data[9] != 6) || data[10] != 0 || data[11] != 0 || data[12] != 0) return false;
      if (data[8] != 8 && !(allow16 && data[8] == 16 && data[9] == 2)) return false;
      ctype = data[9];
      depth = data[8];
      have_ihdr = true;
    } else if (!std::memcmp(type, "sbNd", 4) && len == 4) band_rows = std::min<uint32_t>(be32(data), 65535u);
    else if (!std::memcmp(type, "IDAT", 4)) idat.emplace_back(pos + 8, (size_t)len);
    else if (!std::memcmp(type, "IEND", 4)) break;
    pos += 12 + len;
  }
  if (!have_ihdr || band_rows == 0 || idat.size() < 3 || idat[0].second != 2 || idat.back().second != 4) return false;
  const size_t nb = idat.size() - 2;
  if (nb != ((size_t)h + band_rows - 1) / band_rows) return false;
  const size_t ch = ctype == 6 ? 4 : 3, line = 1 + ch * (size_t)(depth / 8) * (size_t)w;
  if (std::min<size_t>(band_rows, h) * line > ((size_t)1 << 30)) return false;
  for (size_t i = 1; i + 1 < idat.size(); ++i)
    if (idat[i].second >= ((size_t)1 << 28)) return false;
  info.w = (int)w; info.h = (int)h; info.channels = (int)ch; info.band_rows = (int)band_rows; info.nbands = (int)nb;
  info.depth = depth;
  info.bands.assign(idat.begin() + 1, idat.end() - 1);
  info.adler = be32(file + idat.back().first);
  return true;
}
}  // namespace

void png_decode_run(hipStream_t st, PngDecodeBufs& D, const std::vector<const uint8_t*>& files, const std::vector<PngBandedInfo>& info,
                    const std::vector<uint8_t*>& dst, unsigned long long* stats, Profiler* prof) {
  std::vector<PngDecodeDst> d(dst.size());
  for (size_t i = 0; i < dst.size(); ++i) d[i].p = dst[i];
  png_decode_run(st, D, files, info, d, {}, stats, prof);
}
void png_decode_run(hipStream_t st, PngDecodeBufs& D, const std::vector<const uint8_t*>& files, const std::vector<PngBandedInfo>& info,
                    const std::vector<PngDecodeDst>& dst, const std::vector<hipEvent_t>& before, unsigned long long* stats, Profiler* prof) {
  const size_t nimg = info.size();
  if (!nimg) return;
  // where every file, every band's scanlines and the tables lie
  std::vector<size_t> file_off(nimg);
  std::vector<DecImage> imgs(nimg);
  std::vector<DecBand> bands;
  size_t in_bytes = 0, filt_bytes = 0;
  for (size_t i = 0; i < nimg; ++i) {
    const PngBandedInfo& P = info[i];
    const PngDecodeDst& T = dst[i];
    const int pix = P.channels * (P.depth / 8);
    const bool slot = T.store == kPngStoreSide || T.store == kPngStorePole;
    if (!(T.store == kPngStoreBytes || (T.store == kPngStoreU16 && P.depth == 16) || (slot && P.channels == 3)) || (pix != 3 && pix != 4 && pix != 6))
      throw Error(S360_ERR_INVALID_ARG, "png decode: image " + std::to_string(i) + ": no such store for this file");
    if ((P.channels == 4 || slot) && (reinterpret_cast<uintptr_t>(T.p) & 3)) throw Error(S360_ERR_INVALID_ARG, "png decode: image not 4-byte aligned");
    if (T.store == kPngStoreU16 && (reinterpret_cast<uintptr_t>(T.p) & 1)) throw Error(S360_ERR_INVALID_ARG, "png decode: image not 2-byte aligned");
    size_t end = 0;
    for (const auto& b : P.bands) end = std::max(end, b.first + b.second);
    file_off[i] = in_bytes;
    in_bytes += (end + 15) & ~(size_t)15;
    const unsigned line = 1u + (unsigned)pix * (unsigned)P.w;
    imgs[i] = DecImage{T.p, P.w, P.h, pix, line, T.store, T.feather};
    for (int b = 0; b < P.nbands; ++b) {
      const int y0 = b * P.band_rows, rows = std::min(P.band_rows, P.h - y0);
      DecBand R;
      R.comp_off = file_off[i] + P.bands[(size_t)b].first;
      R.comp_len = (unsigned)P.bands[(size_t)b].second;
      R.filt_off = filt_bytes;
      R.n = (unsigned)rows * line;
      R.y0 = (unsigned)y0;
      R.rows = (unsigned)rows;
      R.img = (int)i;
      R.pad = 0;
      filt_bytes += ((size_t)R.n + 15) & ~(size_t)15;
      bands.push_back(R);
    }
  }
  const size_t nb = bands.size();
  if (nb > 0x7fffffffu) throw Error(S360_ERR_INVALID_ARG, "png decode: too many bands");
  const size_t tab_bands = 0, tab_imgs = (nb * sizeof(DecBand) + 15) & ~(size_t)15, tab_bytes = tab_imgs + nimg * sizeof(DecImage);
  const size_t out_stats = (nb * sizeof(DecOut) + 15) & ~(size_t)15, out_bytes = out_stats + kPngDecodeStatWords * sizeof(unsigned);
  D.in.ensure(in_bytes + 16);
  D.filt.ensure(filt_bytes + 16);
  D.table.ensure(tab_bytes);
  D.outs.ensure(out_bytes);
  uint8_t* din = D.in.as<uint8_t>();
  for (size_t i = 0; i < nimg; ++i) {
    size_t end = 0;
    for (const auto& b : info[i].bands) end = std::max(end, b.first + b.second);
    S360_HIP(hipMemcpyAsync(din + file_off[i], files[i], end, hipMemcpyHostToDevice, st));
  }
  uint8_t* dtab = D.table.as<uint8_t>();
  S360_HIP(hipMemcpyAsync(dtab + tab_bands, bands.data(), nb * sizeof(DecBand), hipMemcpyHostToDevice, st));
  S360_HIP(hipMemcpyAsync(dtab + tab_imgs, imgs.data(), nimg * sizeof(DecImage), hipMemcpyHostToDevice, st));
  S360_HIP(hipMemsetAsync(D.outs.p, 0, out_bytes, st));
  const DecBand* dbands = reinterpret_cast<const DecBand*>(dtab + tab_bands);
  const DecImage* dimgs = reinterpret_cast<const DecImage*>(dtab + tab_imgs);
  DecOut* douts = D.outs.as<DecOut>();
  unsigned* dstats = reinterpret_cast<unsigned*>(D.outs.as<uint8_t>() + out_stats);
  Profiler none;
  Profiler& pr = prof ? *prof : none;
  {
    ProfScope ps(pr, "png_inflate");
    hipLaunchKernelGGL(k_png_inflate, dim3((unsigned)nb), dim3(64), 0, st, (const uint8_t*)din, dbands, D.filt.as<uint8_t>(), douts, dstats);
  }
  for (hipEvent_t e : before)
    if (e) S360_HIP(hipStreamWaitEvent(st, e, 0));
  {
    ProfScope ps(pr, "png_unfilter");
    hipLaunchKernelGGL(k_png_unfilter, dim3((unsigned)nb), dim3(kUT), 0, st, (const uint8_t*)D.filt.as<uint8_t>(), dbands, dimgs, douts);
  }
  S360_HIP(hipGetLastError());
  std::vector<uint8_t> res(out_bytes);
  S360_HIP(hipMemcpyAsync(res.data(), D.outs.p, out_bytes, hipMemcpyDeviceToHost, st));
  S360_HIP(hipStreamSynchronize(st));
  const DecOut* O = reinterpret_cast<const DecOut*>(res.data());
  const unsigned* sw = reinterpret_cast<const unsigned*>(res.data() + out_stats);
  if (stats)
    for (int k = 0; k < kPngDecodeStatWords; ++k) stats[k] = sw[k];
  // every band's status; the file's Adler-32 from the bands' pieces: A = 1 + sum of bytes, B = N + sum of (N - index) * byte
  size_t b0 = 0;
  for (size_t i = 0; i < nimg; ++i) {
    const PngBandedInfo& P = info[i];
    for (int b = 0; b < P.nbands; ++b)
      if (const unsigned s = O[b0 + (size_t)b].status)
        throw PngDecodeError((int)i, "png decode: image " + std::to_string(i) + ": band " + std::to_string(b) + ": " +
                                              (s < sizeof kStatusText / sizeof *kStatusText ? kStatusText[s] : "error"));
    unsigned long long A = 1, Bs = 0, after = 0;
    for (int b = P.nbands - 1; b >= 0; --b) {
      const DecOut& o = O[b0 + (size_t)b];
      A = (A + o.s1) % kAdler;
      Bs = (Bs + o.s2 + (after % kAdler) * o.s1) % kAdler;
      after += bands[b0 + (size_t)b].n;
    }
    Bs = (Bs + after % kAdler) % kAdler;
    if ((uint32_t)((Bs << 16) | A) != P.adler)
      throw PngDecodeError((int)i, "png decode: image " + std::to_string(i) + ": Adler-32 mismatch (the scanlines are damaged)");
    b0 += (size_t)P.nbands;
  }
}

}  // namespace s360
