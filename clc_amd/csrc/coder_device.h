// coder_device.h — the arithmetic that the device coders share (entropy.hip, ar_context.hip, gmm.hip, rans_lanes.hip), one definition each.
//
// The encoder and every decoder stay in step only if these pieces are equal bit for bit wherever they run: the bounded scale and Phi,
// the scale index, the place of a pixel-list row in the map, the words of a span, and the 64-lane decoder of the lanes stream.  The host
// coder (rans_host.cpp) is the oracle the device code is held to and shares nothing with this file.
#pragma once
#include "common.h"

namespace coder {

constexpr float kScaleBound = 0.11f;   // LowerBound(scale, 0.11) of the Gaussian-conditional models
constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;

// LowerBound's forward, torch.max(x, bound): a NaN x stays NaN (fmaxf would return the bound); every other x gives fmaxf's bits.
// The coder's index path keeps fmaxf on purpose: encoder and decoder code a NaN scale as the bound.
__device__ __forceinline__ float bound_below(float x, float bound) { return x < bound ? bound : x; }

__device__ __forceinline__ float std_cum(float x) { return 0.5f * erfcf(-kInvSqrt2 * x); }

// The row of the coder's table for a scale sg that is already bounded below (fmaxf(scale, kScaleBound)):
// n_scales - 1 - #{k < n_scales - 1: sg <= tb[k]}, counted linearly.  A NaN compares false everywhere and gets the last row.
__device__ __forceinline__ int scale_index_linear(float sg, const float* tb, int n_scales) {
  int idx = n_scales - 1;
  for (int k = 0; k < n_scales - 1; ++k) idx -= (sg <= tb[k]) ? 1 : 0;
  return idx;
}

// Row p of a pixel list [P][2] = (h, w) in image b of a [B][H][W] map: the pixel's number (b H + h) W + w, or -1 outside the map —
// such a pixel is neither read nor written.
__device__ __forceinline__ long pixel_of(const int32_t* pix, int p, int b, int H, int W) {
  const int h = pix[2 * p], w = pix[2 * p + 1];
  if (h < 0 || h >= H || w < 0 || w >= W) return -1;
  return ((long)b * H + h) * W + w;
}

// The words of one stream: spans[2 wid] is its first word in `words`, spans[2 wid + 1] its count.  A negative first or count reads
// nothing, and a word at or past the count is zero (a truncated stream decodes as if padded with zeros).
struct WordSpan {
  const uint32_t* w; uint32_t count;
  __device__ __forceinline__ void open(const uint32_t* words, const int32_t* spans, int wid) {
    const int first = spans[2 * wid], cnt = spans[2 * wid + 1];
    w = words + (first > 0 ? first : 0);
    count = (first >= 0 && cnt > 0) ? (uint32_t)cnt : 0u;
  }
  __device__ __forceinline__ uint32_t word(uint32_t i) const { return i < count ? w[i] : 0u; }
};

// The decoder of one wave stream of the lanes format (rans_lanes.hip has the format): lane l of the wave IS rANS lane l, one symbol per
// lane and round.  Per lane the arithmetic is rans_host.cpp's (the symbol update, renorm and get_bits of clc_rans_decoder_decode); every
// loop is bounded by a constant.  A state in memory is kStateWords words: 64 x (x low, x high), pos, pad.
struct LaneCoder {
  static constexpr int kLanes = 64;
  static constexpr uint64_t kL = 1ull << 31;
  static constexpr int kStateWords = 2 * kLanes + 2;
  uint64_t x; uint32_t pos;   // the lane's state; the wave's place in the span
  WordSpan span;
  unsigned long long below;   // the lanes before this one
  uint32_t* st;
  __device__ __forceinline__ void open(const uint32_t* words, const int32_t* spans, uint32_t* state, int wid, int lane) {
    span.open(words, spans, wid);
    st = state + (long)kStateWords * wid;
    x = (uint64_t)st[2 * lane] | ((uint64_t)st[2 * lane + 1] << 32);
    pos = st[2 * kLanes];
    below = (1ull << lane) - 1ull;
  }
  // renorm of the lanes that `need` it: they take the next words in ascending lane order
  __device__ __forceinline__ void take(bool need) {
    const unsigned long long m = __ballot(need);
    if (need) {
      const uint32_t v = span.word(pos + (uint32_t)__popcll(m & below));
      x = (x << 32) | v;
    }
    pos += (uint32_t)__popcll(m);
  }
  // One round: an active lane decodes one symbol of the row cdf[0 .. maxv + 1] and returns its value before the row's offset is added
  // (an escaped value wraps as the host coder's does); an inactive lane takes no part and returns 0.
  __device__ __forceinline__ uint32_t round(const int32_t* cdf, int maxv, bool active) {
    // sub-step 0, the symbol: the largest s <= max_value with cdf[s] <= cf
    int s = 0;
    if (active) {
      const uint32_t cf = (uint32_t)x & 0xFFFFu;
      int lo = 0, hi = maxv;
#pragma unroll 1
      for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if ((uint32_t)cdf[mid] <= cf) lo = mid; else hi = mid - 1;
      }
      s = lo;
      const uint32_t start = (uint32_t)cdf[s], freq = (uint32_t)(cdf[s + 1] - cdf[s]);
      x = (uint64_t)freq * (x >> 16) + cf - start;
    }
    take(active && x < kL);
    const bool esc = active && s == maxv;
    uint32_t value = (uint32_t)s;
    if (__ballot(esc)) {   // the tail's escape: sub-steps 1 .. — the count (one nibble; a second after a 15), then the payload nibbles
      int nb = 0, base = 2;
      uint32_t raw = 0;
#pragma unroll 1
      for (int t = 1; t < 19; ++t) {
        const bool cnt_op = esc && (t == 1 || (t == 2 && nb == 15));
        const int k = t - base;
        const bool pay_op = esc && !cnt_op && t >= 2 && k < (nb < 16 ? nb : 16);
        const bool op = cnt_op || pay_op;
        if (!__ballot(op)) break;
        const uint32_t v = (uint32_t)x & 15u;
        if (op) x >>= 4;
        take(op && x < kL);
        if (cnt_op) { nb += (int)v; if (t == 2) base = 3; }
        if (pay_op && k < 8) raw |= v << (4 * k);
      }
      if (esc) value = (raw & 1u) ? ~(raw >> 1) : (raw >> 1) + (uint32_t)maxv;   // (-v - 1 == ~v)
    }
    return value;
  }
  __device__ __forceinline__ void close(int lane) {
    st[2 * lane] = (uint32_t)x;
    st[2 * lane + 1] = (uint32_t)(x >> 32);
    if (lane == 0) st[2 * kLanes] = pos;
  }
};

}  // namespace coder
