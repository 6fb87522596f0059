// rans_lanes.hip — the lane-interleaved rANS coder of the "lanes" stream on the device (include/clc_hip.h: clc_rans_lanes_*).
//
// One wave per (image, wave stream); lane l of the wave IS rANS lane l of the stream.  The 64 states advance together, one symbol per
// lane and round; the only thing the lanes share is the word array, and who takes (decoder) or writes (encoder) the next words of a
// sub-step is decided by a ballot of the lanes that renormalise and a prefix popcount: ascending lane order forward, which the encoder
// mirrors by writing backward with the highest lane first.  The arithmetic per lane is rans_host.cpp's (enc_put, enc_put_bits, the
// escape; the symbol update, renorm and get_bits of clc_rans_decoder_decode), and the host coder of the same format
// (clc_rans_lanes_encode_host, clc_rans_lanes_decoder_*) is the oracle: same words, same symbols, same final states.
//
// No LDS, no barrier, no atomics, no wave waits on another; every loop is bounded by a constant or by the symbol count.
#include "common.h"

namespace {
constexpr int kLanes = 64;
constexpr uint64_t kL = 1ull << 31;

struct LanesTables {
  const int32_t* cdfs; int cdf_stride, n_rows;
  const int32_t* cdf_sizes;
  const int32_t* offsets;
};

struct LanesDecArgs {
  const int32_t* indexes; long ld_idx;
  int n, W;
  LanesTables t;
  const uint32_t* words;
  const int32_t* spans;
  uint32_t* state;   // per (b, w): 64 x (x low, x high), pos, pad
  int32_t* symbols; long ld_sym;
};

constexpr int kStateWords = 2 * kLanes + 2;

__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(64) void rans_lanes_decode_kernel(const LanesDecArgs a) {
  const int lane = threadIdx.x;
  const int wid = blockIdx.x;   // (b, w)
  const int b = wid / a.W, w = wid - b * a.W;
  const int first = a.spans[2 * wid], cnt = a.spans[2 * wid + 1];
  const uint32_t* wp = a.words + (first > 0 ? first : 0);
  const uint32_t count = (first >= 0 && cnt > 0) ? (uint32_t)cnt : 0u;   // (a negative first or count reads nothing)
  uint32_t* st = a.state + (long)kStateWords * wid;
  uint64_t x = (uint64_t)st[2 * lane] | ((uint64_t)st[2 * lane + 1] << 32);
  uint32_t pos = st[2 * kLanes];
  const int32_t* idx = a.indexes + (long)b * a.ld_idx;
  int32_t* out = a.symbols + (long)b * a.ld_sym;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int chunks = (a.n + kLanes - 1) / kLanes;
  // renorm of the lanes that `need` it: they take the next words in ascending lane order; a word at or past the count is zero
  auto take = [&](bool need) {
    const unsigned long long m = __ballot(need);
    if (need) {
      const uint32_t i = pos + (uint32_t)__popcll(m & below);
      const uint32_t v = i < count ? wp[i] : 0u;
      x = (x << 32) | v;
    }
    pos += (uint32_t)__popcll(m);
  };
  // the next round's row is known before this round's state is: fetched one round ahead
  int ci_next = 0, size_next = 2, off_next = 0;
  auto fetch = [&](int q) {
    const long j = (long)q * kLanes + lane;
    if (q < chunks && j < a.n) {
      ci_next = clamp_int(idx[j], 0, a.t.n_rows - 1);   // an index outside the table is clamped into it
      size_next = clamp_int(a.t.cdf_sizes[ci_next], 2, a.t.cdf_stride);
      off_next = a.t.offsets[ci_next];
    }
  };
  fetch(w);
#pragma unroll 1
  for (int q = w; q < chunks; q += a.W) {
    const long j = (long)q * kLanes + lane;
    const bool active = j < a.n;
    const int ci = ci_next, size = size_next, off = off_next;
    fetch(q + a.W);
    const int32_t* cdf = a.t.cdfs + (long)ci * a.t.cdf_stride;
    const int maxv = size - 2;
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
    if (active) out[j] = (int32_t)(value + (uint32_t)off);
  }
  st[2 * lane] = (uint32_t)x;
  st[2 * lane + 1] = (uint32_t)(x >> 32);
  if (lane == 0) st[2 * kLanes] = pos;
}

struct LanesEncArgs {
  const int32_t* symbols;
  const int32_t* indexes; long ld;
  LanesTables t;
  uint32_t* out;
  const int32_t* regions;   // [B][W][2]: first word, capacity
  int32_t* result;          // [B][W][2]: first word, count — or (code < 0, 0)
  int W;
  clc_rans_lanes_segments segs;
};

__global__ __launch_bounds__(64) void rans_lanes_encode_kernel(const LanesEncArgs a) {
  const int lane = threadIdx.x;
  const int wid = blockIdx.x;   // (b, w)
  const int b = wid / a.W, w = wid - b * a.W;
  const int rfirst = a.regions[2 * wid], rcap = a.regions[2 * wid + 1];
  if (rfirst < 0 || rcap < 2 * kLanes) {   // not even the states fit: nothing is written
    if (lane == 0) { a.result[2 * wid] = CLC_RANS_LANES_OVERFLOW; a.result[2 * wid + 1] = 0; }
    return;
  }
  uint32_t* region = a.out + rfirst;
  int ptr = rcap;   // the next free slot is ptr - 1; below zero: overflow, and nothing more is written
  const int32_t* sym = a.symbols + (long)b * a.ld;
  const int32_t* idx = a.indexes + (long)b * a.ld;
  const unsigned long long above = lane == 63 ? 0ull : ~((2ull << lane) - 1ull);
  uint64_t x = kL;
  bool zero_freq = false;
  long at = 0;
  for (int p = 0; p < a.segs.P; ++p) at += a.segs.n[p];
#pragma unroll 1
  for (int p = a.segs.P - 1; p >= 0; --p) {
    const int n = a.segs.n[p];
    at -= n;
    const int chunks = (n + kLanes - 1) / kLanes;
    if (chunks <= w) continue;
#pragma unroll 1
    for (int q = chunks - 1 - (chunks - 1 - w) % a.W; q >= 0; q -= a.W) {   // the wave's chunks of the segment, last first
      const int j = q * kLanes + lane;
      const bool active = j < n;
      uint32_t start = 0, freq = 1, raw = 0;
      int nops = 0, nb = 0;
      if (active) {
        const int ci = clamp_int(idx[at + j], 0, a.t.n_rows - 1);
        const int maxv = clamp_int(a.t.cdf_sizes[ci], 2, a.t.cdf_stride) - 2;
        const int32_t* cdf = a.t.cdfs + (long)ci * a.t.cdf_stride;
        int value = (int)((uint32_t)sym[at + j] - (uint32_t)a.t.offsets[ci]);
        bool esc = false;
        if (value < 0) { raw = (uint32_t)(-2 * (long)value - 1); value = maxv; esc = true; }
        else if (value >= maxv) { raw = (uint32_t)(2 * ((long)value - maxv)); value = maxv; esc = true; }
        start = (uint32_t)cdf[value] & 0xFFFFu;
        freq = (uint32_t)(cdf[value + 1] - cdf[value]) & 0xFFFFu;
        nops = 1;
        if (esc) {   // a payload has at most 8 nibbles, so one count nibble
#pragma unroll
          for (int k = 0; k < 8; ++k) nb += (raw >> (4 * k)) != 0 ? 1 : 0;
          nops = 2 + nb;
        }
      }
      if (__ballot(active && freq == 0)) zero_freq = true;
      if (freq == 0) freq = 1;   // (the result is the error code; the division stays defined)
      int t_hi = 0;
      if (__ballot(nops > 1)) {
        t_hi = 1;
#pragma unroll
        for (int k = 2; k < 10; ++k) t_hi = __ballot(nops > k) ? k : t_hi;
      }
#pragma unroll 1
      for (int t = t_hi; t >= 0; --t) {   // sub-steps descending; inside one the highest lane writes first, i.e. at the highest address
        const bool in = t < nops;
        const uint64_t x_max = t == 0 ? ((uint64_t)freq << 47) : (1ull << 59);   // ((L >> 16) << 32) * freq, and the same at freq = 2^12
        const bool emit = in && x >= x_max;
        const unsigned long long m = __ballot(emit);
        if (emit) {
          const int slot = ptr - 1 - __popcll(m & above);
          if (slot >= 0) region[slot] = (uint32_t)x;
          x >>= 32;
        }
        ptr -= __popcll(m);
        if (in) {
          if (t == 0) x = ((x / freq) << 16) + (x % freq) + start;
          else x = (x << 4) | (t == 1 ? (uint32_t)nb : ((raw >> (4 * (t - 2))) & 15u));
        }
      }
    }
  }
  // the 64 final states in front: lane l's low word at 2 l, its high word at 2 l + 1
  ptr -= 2 * kLanes;
  if (ptr >= 0) {
    region[ptr + 2 * lane] = (uint32_t)x;
    region[ptr + 2 * lane + 1] = (uint32_t)(x >> 32);
  }
  if (lane == 0) {
    const int code = zero_freq ? CLC_RANS_LANES_ZERO_FREQ : (ptr < 0 ? CLC_RANS_LANES_OVERFLOW : 0);
    a.result[2 * wid] = code ? code : rfirst + ptr;
    a.result[2 * wid + 1] = code ? 0 : rcap - ptr;
  }
}

bool lanes_tables_ok(const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets) {
  return cdfs && cdf_sizes && offsets && cdf_stride >= 2 && n_rows >= 1;
}
}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int clc_rans_lanes_decode_step(const int32_t* indexes, long ld_idx, int n, int B, const int32_t* cdfs, int cdf_stride, int n_rows,
                                          const int32_t* cdf_sizes, const int32_t* offsets, const uint32_t* words, const int32_t* spans,
                                          clc_rans_lanes_state* state, int W, int32_t* symbols, long ld_sym, clc_stream_t stream) {
  static_assert(sizeof(clc_rans_lanes_state) == 4 * kStateWords, "rans_lanes_decode_kernel: a state is 64 x u64 and (pos, pad)");
  CLC_CHECK(indexes && words && spans && state && symbols, "clc_rans_lanes_decode_step: null pointer");
  CLC_CHECK(cdfs && cdf_sizes && offsets, "clc_rans_lanes_decode_step: null table pointer");
  CLC_CHECK(cdf_stride >= 2 && n_rows >= 1, "clc_rans_lanes_decode_step: the table needs cdf_stride >= 2 and n_rows >= 1 (got %d, %d)", cdf_stride, n_rows);
  CLC_CHECK(W >= 1 && W <= CLC_RANS_LANES_MAX_W, "clc_rans_lanes_decode_step: W must be between 1 and %d waves (got %d)", CLC_RANS_LANES_MAX_W, W);
  CLC_CHECK(n >= 0 && B > 0, "clc_rans_lanes_decode_step: n must not be negative and B must be positive (got %d, %d)", n, B);
  CLC_CHECK(ld_idx >= n && ld_sym >= n, "clc_rans_lanes_decode_step: ld_idx or ld_sym < n");
  CLC_CHECK((long)B * W < (1l << 24), "clc_rans_lanes_decode_step: B * W must be below 2^24");
  if (n == 0) return 0;   // an empty segment contributes nothing
  LanesDecArgs a = {};
  a.indexes = indexes; a.ld_idx = ld_idx; a.n = n; a.W = W;
  a.t = {cdfs, cdf_stride, n_rows, cdf_sizes, offsets};
  a.words = words; a.spans = spans; a.state = reinterpret_cast<uint32_t*>(state); a.symbols = symbols; a.ld_sym = ld_sym;
  hipLaunchKernelGGL(rans_lanes_decode_kernel, dim3(B * W), dim3(kLanes), 0, ST, a);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, long ld, int B, clc_rans_lanes_segments segs, int W,
                                            const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets,
                                            uint32_t* out, const int32_t* regions, int32_t* result, clc_stream_t stream) {
  CLC_CHECK(symbols && indexes && out && regions && result, "clc_rans_lanes_encode: null pointer");
  CLC_CHECK(cdfs && cdf_sizes && offsets, "clc_rans_lanes_encode: null table pointer");
  CLC_CHECK(cdf_stride >= 2 && n_rows >= 1, "clc_rans_lanes_encode: the table needs cdf_stride >= 2 and n_rows >= 1 (got %d, %d)", cdf_stride, n_rows);
  CLC_CHECK(W >= 1 && W <= CLC_RANS_LANES_MAX_W, "clc_rans_lanes_encode: W must be between 1 and %d waves (got %d)", CLC_RANS_LANES_MAX_W, W);
  CLC_CHECK(B > 0, "clc_rans_lanes_encode: B must be positive (got %d)", B);
  CLC_CHECK(segs.P >= 0 && segs.P <= CLC_RANS_LANES_MAX_SEGMENTS, "clc_rans_lanes_encode: P must be between 0 and %d segments (got %d)",
            CLC_RANS_LANES_MAX_SEGMENTS, segs.P);
  long total = 0;
  for (int p = 0; p < segs.P; ++p) {
    CLC_CHECK(segs.n[p] >= 0, "clc_rans_lanes_encode: segment %d has a negative length (%d)", p, segs.n[p]);
    total += segs.n[p];
  }
  CLC_CHECK(total < (1l << 27), "clc_rans_lanes_encode: %ld symbols per image; a region's 128 + 10 n words must stay below 2^31", total);
  CLC_CHECK(ld >= total, "clc_rans_lanes_encode: ld < the segments' total (%ld < %ld)", ld, total);
  CLC_CHECK((long)B * W < (1l << 24), "clc_rans_lanes_encode: B * W must be below 2^24");
  LanesEncArgs a = {};
  a.symbols = symbols; a.indexes = indexes; a.ld = ld;
  a.t = {cdfs, cdf_stride, n_rows, cdf_sizes, offsets};
  a.out = out; a.regions = regions; a.result = result; a.W = W; a.segs = segs;
  hipLaunchKernelGGL(rans_lanes_encode_kernel, dim3(B * W), dim3(kLanes), 0, ST, a);
  CLC_LAUNCH_CHECK();
  return 0;
}
