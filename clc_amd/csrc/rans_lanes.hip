// rans_lanes.hip — the lane-interleaved rANS coder of the "lanes" stream on the device (include/clc_hip.h: clc_rans_lanes_*).
//
// One wave per (image, wave stream); lane l of the wave IS rANS lane l of the stream.  The 64 states advance together, one symbol per
// lane and round; the only thing the lanes share is the word array, and who takes (decoder) or writes (encoder) the next words of a
// sub-step is decided by a ballot of the lanes that renormalise and a prefix popcount: ascending lane order forward, which the encoder
// mirrors by writing backward with the highest lane first.  The arithmetic per lane is rans_host.cpp's (enc_put, enc_put_bits, the
// escape; the symbol update, renorm and get_bits of clc_rans_decoder_decode), and the host coder of the same format
// (clc_rans_lanes_encode_host, clc_rans_lanes_decoder_*) is the oracle: same words, same symbols, same final states.
//
// No atomics, no wave waits on another; every loop is bounded by a constant or by the symbol count.  The two kernels of the table-coded
// stream use no LDS and no barrier; rans_lanes_decode_gauss_kernel keeps the scale table in LDS (one barrier before its first round).
//
// The decoder has one owner, coder::LaneCoder (coder_device.h): the open and write-back of span and state, the ballot-and-popcount renorm,
// a round's symbol search and state update, the escape.  Both decode kernels run their rounds through it and own what surrounds a round:
// which row it decodes from (fetched one round ahead of the state; read, or formed from the scale) and where the value goes.
//
// Two kernels are templates over the one thing their entries differ in.  The encoder reads its segment lengths from a by-value struct
// (clc_rans_lanes_encode, P <= 32) or from device memory (clc_rans_lanes_encode_list, any P).  The Gaussian step lands a (row, channel)
// in a dense [rows][ldh] map (clc_rans_lanes_decode_gauss) or, through a pixel list, in an NHWC latent (clc_ar_lanes_decode).
#include "coder_device.h"

namespace {
using namespace coder;
constexpr int kLanes = LaneCoder::kLanes;
constexpr uint64_t kL = LaneCoder::kL;
constexpr int kStateWords = LaneCoder::kStateWords;

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

__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(64) void rans_lanes_decode_kernel(const LanesDecArgs a) {
  const int lane = threadIdx.x;
  const int wid = blockIdx.x;   // (b, w)
  const int b = wid / a.W, w = wid - b * a.W;
  LaneCoder d;
  d.open(a.words, a.spans, a.state, wid, lane);
  const int32_t* idx = a.indexes + (long)b * a.ld_idx;
  int32_t* out = a.symbols + (long)b * a.ld_sym;
  const int chunks = (a.n + kLanes - 1) / kLanes;
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
    const uint32_t value = d.round(a.t.cdfs + (long)ci * a.t.cdf_stride, size - 2, active);
    if (active) out[j] = (int32_t)(value + (uint32_t)off);
  }
  d.close(lane);
}

struct LanesSegList { int P; const int32_t* n; };   // clc_rans_lanes_segments with the lengths in device memory

template <class Segs>
struct LanesEncArgs {
  const int32_t* symbols;
  const int32_t* indexes; long ld;
  LanesTables t;
  uint32_t* out;
  const int32_t* regions;   // [B][W][2]: first word, capacity
  int32_t* result;          // [B][W][2]: first word, count — or (code < 0, 0)
  int W;
  Segs segs;   // .P lengths .n[p]; a negative length counts as 0
};

template <class Segs>
__global__ __launch_bounds__(64) void rans_lanes_encode_kernel(const LanesEncArgs<Segs> a) {
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
  for (int p = 0; p < a.segs.P; ++p) at += a.segs.n[p] > 0 ? a.segs.n[p] : 0;
#pragma unroll 1
  for (int p = a.segs.P - 1; p >= 0; --p) {
    const int n = a.segs.n[p] > 0 ? a.segs.n[p] : 0;
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

// ---- the slice step of the Gaussian-conditional models: index, decode, de-quantise in one launch ----
// rans_lanes_decode_kernel with the row index formed here (quantize_build_indexes_kernel's, entropy.hip) and the symbol leaving as
// y_hat = (float)symbol + mu.
//
// WHERE a (row, channel) lands is the template's parameter.  LanesDenseRows: at r * ldh + c, the slice models' map.  LanesPixelList: the
// rows of an image are the pixels of a step of the context model's schedule, row p of image b lands at pixel pix[p] = (h, w) of the
// NHWC latent, pixel_of(...) * ldh + c (ar_commit_kernel's place), and a pair outside the map is decoded and not written.
constexpr int kMaxScales = 256;

struct LanesGaussArgs {
  const float* scale; long ldsc;
  const float* mu; long ldmu;
  int C, n, W;
  const float* table; int n_scales;
  LanesTables t;
  const uint32_t* words;
  const int32_t* spans;
  uint32_t* state;
  float* y_hat; long ldh;
  int32_t* symbols; long ld_sym;   // symbols may be null
  const float* step;               // [C]: the quantisation step per channel; read by the kStep instantiations only
};

struct LanesDenseRows {
  static constexpr bool kEveryRow = true;   // every row has a place
  __device__ __forceinline__ long at(int, long r, int, int c, long ldh) const { return r * ldh + c; }
};

struct LanesPixelList {
  static constexpr bool kEveryRow = false;
  const int32_t* pix;   // [P][2]: (h, w) of the image's row p
  int H, W;
  __device__ __forceinline__ long at(int b, long, int p, int c, long ldh) const {   // negative: outside the map (c - ldh, and c < C <= ldh)
    return pixel_of(pix, p, b, H, W) * ldh + c;
  }
};

// kStep (variable-rate coding; clc_rans_lanes_decode_gauss_step): the row index is that of max(scale, 0.11) / step[c] and the symbol
// leaves as y_hat = (float)symbol * step[c] + mu, a rounded multiply and a rounded add — clc_quantize_build_indexes_step's expression.  The
// step of a round is fetched where its scale (for the index) and its mu (for the value) are; words, spans, states, clamps and loop
// bounds are the unit-step kernel's, and with kStep false every added line is compiled out.
template <class Landing, bool kStep = false>
__global__ __launch_bounds__(64) void rans_lanes_decode_gauss_kernel(const LanesGaussArgs a, const Landing place) {
  __shared__ float tb[kMaxScales];
  const int lane = threadIdx.x;
  const int ns1 = a.n_scales - 1;
  for (int i = lane; i < ns1; i += kLanes) tb[i] = a.table[i];
  __syncthreads();
  const int wid = blockIdx.x;   // (b, w)
  const int b = wid / a.W, w = wid - b * a.W;
  LaneCoder d;
  d.open(a.words, a.spans, a.state, wid, lane);
  const long row0 = (long)b * (a.n / a.C);   // the image's first row of the [rows][C] maps
  const int chunks = (a.n + kLanes - 1) / kLanes;
  // A round's row does not depend on the coder state, but finding it is a chain of its own — the scale's load, a search of up to eight
  // dependent LDS reads, the loads of cdf size and offset — and one wave alone hides none of it behind anything.  So the wave's rounds
  // run in GROUPS of kGroup: at a group's last round the indexes of the next group's rounds are searched together (kGroup independent
  // searches, step by step side by side, so that one LDS latency serves them all) from scales that were loaded a whole group earlier,
  // and the scales of the group after that are requested.  Per round what is left is the (size, offset, mu) fetch one round ahead, as
  // in rans_lanes_decode_kernel.
  constexpr int kGroup = 4;
  int top = 1;   // the largest power of two <= ns1
  while (2 * top <= ns1) top *= 2;
  // (pixel, channel) of a lane's symbol advance by a constant from one of the wave's rounds to the next: no division inside the loop
  const int step_p = (a.W * kLanes) / a.C, step_c = (a.W * kLanes) % a.C;
  struct Place { int p, c; };
  auto advance = [&](Place& at) {
    at.p += step_p; at.c += step_c;
    if (at.c >= a.C) { at.c -= a.C; at.p += 1; }
  };
  const int j0 = w * kLanes + lane;   // (< 2^10 + 64)
  Place ahead = {j0 / a.C, j0 % a.C}, row = ahead;   // of the next round load_scales / fetch_row is called for
  float sc[kGroup] = {};
  float sq[kStep ? kGroup : 1];   // kStep: the steps of the group's rounds
  auto load_scales = [&](int q0) {   // the scales of rounds q0, q0 + W, ...: called for consecutive groups
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
      const long q = (long)q0 + (long)g * a.W;
      const long j = q * kLanes + lane;
      sc[g] = 0.f;
      if constexpr (kStep) sq[g] = 1.f;
      if (q < chunks && j < a.n) {
        sc[g] = a.scale[(row0 + ahead.p) * a.ldsc + ahead.c];
        if constexpr (kStep) sq[g] = a.step[ahead.c];
      }
      advance(ahead);
    }
  };
  // n_scales - 1 - #{k < n_scales - 1: sg <= table[k]}.  Over a non-decreasing table the k that do NOT count are a prefix, and its
  // length is the index: the largest pos with !(sg <= table[pos - 1]), built from the top bit down.  (A NaN scale: every pos, ns1.)
  auto search = [&]() -> uint32_t {   // -> the kGroup indexes, a byte each
    float sg[kGroup];
    int pos[kGroup];
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
      sg[g] = fmaxf(sc[g], kScaleBound);
      if constexpr (kStep) sg[g] = sg[g] / sq[g];
      pos[g] = 0;
    }
#pragma unroll 1
    for (int step = top; step >= 1; step >>= 1) {
#pragma unroll
      for (int g = 0; g < kGroup; ++g) {
        const int t = pos[g] + step;
        const float e = tb[(t < ns1 ? t : ns1) - 1];
        if (t <= ns1 && !(sg[g] <= e)) pos[g] = t;
      }
    }
    uint32_t pack = 0;
#pragma unroll
    for (int g = 0; g < kGroup; ++g) pack |= (uint32_t)pos[g] << (8 * g);
    return pack;
  };
  int ci_next = 0, size_next = 2, off_next = 0;
  long at_next = 0;
  float mu_next = 0.f, step_next = 1.f;
  auto fetch_row = [&](int q, int index) {   // called for consecutive rounds
    const long j = (long)q * kLanes + lane;
    if (q < chunks && j < a.n) {
      const long r = row0 + row.p;
      const int c = row.c;
      ci_next = clamp_int(index, 0, a.t.n_rows - 1);   // an index outside the cdf table is clamped into it
      size_next = clamp_int(a.t.cdf_sizes[ci_next], 2, a.t.cdf_stride);
      off_next = a.t.offsets[ci_next];
      mu_next = a.mu[r * a.ldmu + c];
      if constexpr (kStep) step_next = a.step[c];
      at_next = place.at(b, r, row.p, c, a.ldh);
    }
    advance(row);
  };
  load_scales(w);
  uint32_t pack = search();
  load_scales(w + kGroup * a.W);
  fetch_row(w, (int)(pack & 255u));
  int g = 0;   // the round's place in its group
#pragma unroll 1
  for (int q = w; q < chunks; q += a.W) {
    const long j = (long)q * kLanes + lane;
    const bool active = j < a.n;
    const int ci = ci_next, size = size_next, off = off_next;
    const long at = at_next;
    const float m_ = mu_next, s_ = step_next;
    g = (g + 1) & (kGroup - 1);
    if (g == 0) {   // (uniform) the next round opens a group
      pack = search();
      load_scales(q + a.W + kGroup * a.W);
    }
    fetch_row(q + a.W, (int)((pack >> (8 * g)) & 255u));
    const uint32_t value = d.round(a.t.cdfs + (long)ci * a.t.cdf_stride, size - 2, active);
    if (active) {
      const int32_t sym = (int32_t)(value + (uint32_t)off);
      if constexpr (kStep) {
        if (Landing::kEveryRow || at >= 0) a.y_hat[at] = (float)sym * s_ + m_;
      } else {
        if (Landing::kEveryRow || at >= 0) a.y_hat[at] = (float)sym + m_;
      }
      if (a.symbols) a.symbols[(long)b * a.ld_sym + j] = sym;
    }
  }
  d.close(lane);
}

// ---- the encoder's wave streams, back to back ----
struct LanesPackArgs {
  const uint32_t* words; long n_words;
  const int32_t* result;   // [B][W][2]: first word, count — or (code < 0, 0)
  int n_streams;
  uint32_t* packed; long capacity;
  int32_t* header;         // [n_streams + 1]: counts (negative codes as they are), total
};

__device__ __forceinline__ long wave_sum(long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kLanes);
  return v;
}

__global__ __launch_bounds__(64) void rans_lanes_pack_kernel(const LanesPackArgs a) {
  const int lane = threadIdx.x;
  const int wid = blockIdx.x;
  auto count_of = [&](int i) -> long {
    const int f = a.result[2 * i], c = a.result[2 * i + 1];
    return (f >= 0 && c > 0) ? (long)c : 0l;   // (a code carries no words)
  };
  // the wave's own prefix over the counts before it: no wave reads what another wrote
  long before = 0;
  for (int i = lane; i < wid; i += kLanes) before += count_of(i);
  before = wave_sum(before);
  const int first = a.result[2 * wid];
  const long cnt = count_of(wid);
  for (long i = lane; i < cnt; i += kLanes) {
    const long src = (long)first + i, dst = before + i;
    if (dst < a.capacity && src < a.n_words) a.packed[dst] = a.words[src];
  }
  if (lane == 0) a.header[wid] = first < 0 ? first : (int32_t)cnt;
  if (wid == 0) {   // (uniform per wave) the total, reported whether or not it fits
    long total = 0;
    for (int i = lane; i < a.n_streams; i += kLanes) total += count_of(i);
    total = wave_sum(total);
    if (lane == 0) a.header[a.n_streams] = (int32_t)(total < 0x7fffffffl ? total : 0x7fffffffl);
  }
}

// what every coder entry checks of its table, its wave count and its grid, under the entry's name `who`
int lanes_entry_ok(const char* who, const LanesTables& t, int W, int B) {
  CLC_CHECK(t.cdfs && t.cdf_sizes && t.offsets, "%s: null table pointer", who);
  CLC_CHECK(t.cdf_stride >= 2 && t.n_rows >= 1, "%s: the table needs cdf_stride >= 2 and n_rows >= 1 (got %d, %d)", who, t.cdf_stride, t.n_rows);
  CLC_CHECK(W >= 1 && W <= CLC_RANS_LANES_MAX_W, "%s: W must be between 1 and %d waves (got %d)", who, CLC_RANS_LANES_MAX_W, W);
  CLC_CHECK((long)B * W < (1l << 24), "%s: B * W must be below 2^24", who);
  return 0;
}

// the launch of clc_rans_lanes_decode_gauss and clc_ar_lanes_decode, which differ in where a (row, channel) lands
template <class Landing>
int launch_decode_gauss(const float* scale, long ldsc, const float* mu, long ldmu, int C, int n, int B, const float* scale_table, int n_scales,
                        const LanesTables& t, const uint32_t* words, const int32_t* spans, clc_rans_lanes_state* state, int W, float* y_hat, long ldh,
                        int32_t* symbols, long ld_sym, const Landing& place, hipStream_t st, const float* step = nullptr) {
  LanesGaussArgs a = {};
  a.scale = scale; a.ldsc = ldsc; a.mu = mu; a.ldmu = ldmu; a.C = C; a.n = n; a.W = W;
  a.table = scale_table; a.n_scales = n_scales;
  a.t = t;
  a.words = words; a.spans = spans; a.state = reinterpret_cast<uint32_t*>(state);
  a.y_hat = y_hat; a.ldh = ldh; a.symbols = symbols; a.ld_sym = ld_sym; a.step = step;
  bool stepped = false;
  if constexpr (Landing::kEveryRow) {   // (the context models' pixel-list landing has no step entry: no such instantiation)
    if (step) {
      hipLaunchKernelGGL((rans_lanes_decode_gauss_kernel<Landing, true>), dim3(B * W), dim3(kLanes), 0, st, a, place);
      stepped = true;
    }
  }
  if (!stepped) hipLaunchKernelGGL((rans_lanes_decode_gauss_kernel<Landing, false>), dim3(B * W), dim3(kLanes), 0, st, a, place);
  CLC_LAUNCH_CHECK();
  return 0;
}
}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int clc_rans_lanes_decode_step(const int32_t* indexes, long ld_idx, int n, int B, const int32_t* cdfs, int cdf_stride, int n_rows,
                                          const int32_t* cdf_sizes, const int32_t* offsets, const uint32_t* words, const int32_t* spans,
                                          clc_rans_lanes_state* state, int W, int32_t* symbols, long ld_sym, clc_stream_t stream) {
  static_assert(sizeof(clc_rans_lanes_state) == 4 * kStateWords, "rans_lanes_decode_kernel: a state is 64 x u64 and (pos, pad)");
  CLC_CHECK(indexes && words && spans && state && symbols, "clc_rans_lanes_decode_step: null pointer");
  const LanesTables t = {cdfs, cdf_stride, n_rows, cdf_sizes, offsets};
  if (lanes_entry_ok("clc_rans_lanes_decode_step", t, W, B)) return -1;
  CLC_CHECK(n >= 0 && B > 0, "clc_rans_lanes_decode_step: n must not be negative and B must be positive (got %d, %d)", n, B);
  CLC_CHECK(ld_idx >= n && ld_sym >= n, "clc_rans_lanes_decode_step: ld_idx or ld_sym < n");
  if (n == 0) return 0;   // an empty segment contributes nothing
  LanesDecArgs a = {};
  a.indexes = indexes; a.ld_idx = ld_idx; a.n = n; a.W = W;
  a.t = t;
  a.words = words; a.spans = spans; a.state = reinterpret_cast<uint32_t*>(state); a.symbols = symbols; a.ld_sym = ld_sym;
  hipLaunchKernelGGL(rans_lanes_decode_kernel, dim3(B * W), dim3(kLanes), 0, ST, a);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, long ld, int B, clc_rans_lanes_segments segs, int W,
                                            const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets,
                                            uint32_t* out, const int32_t* regions, int32_t* result, clc_stream_t stream) {
  CLC_CHECK(symbols && indexes && out && regions && result, "clc_rans_lanes_encode: null pointer");
  const LanesTables t = {cdfs, cdf_stride, n_rows, cdf_sizes, offsets};
  if (lanes_entry_ok("clc_rans_lanes_encode", t, W, B)) return -1;
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
  LanesEncArgs<clc_rans_lanes_segments> a = {};
  a.symbols = symbols; a.indexes = indexes; a.ld = ld;
  a.t = t;
  a.out = out; a.regions = regions; a.result = result; a.W = W; a.segs = segs;
  hipLaunchKernelGGL(rans_lanes_encode_kernel<clc_rans_lanes_segments>, dim3(B * W), dim3(kLanes), 0, ST, a);
  CLC_LAUNCH_CHECK();
  return 0;
}

// clc_rans_lanes_decode_gauss and clc_rans_lanes_decode_gauss_step: one set of checks under the entry's name; step == nullptr is the unit step
static int decode_gauss_entry(const char* who, const float* scale, long ldsc, const float* mu, long ldmu, const float* step, int C, int n, int B,
                              const float* scale_table, int n_scales, const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes,
                              const int32_t* offsets, const uint32_t* words, const int32_t* spans, clc_rans_lanes_state* state, int W,
                              float* y_hat, long ldh, int32_t* symbols, long ld_sym, hipStream_t st) {
  CLC_CHECK(scale && mu && scale_table && words && spans && state && y_hat, "%s: null pointer", who);
  const LanesTables t = {cdfs, cdf_stride, n_rows, cdf_sizes, offsets};
  if (lanes_entry_ok(who, t, W, B)) return -1;
  CLC_CHECK(n_scales > 1 && n_scales <= kMaxScales, "%s: n_scales must be between 2 and %d (got %d)", who, kMaxScales, n_scales);
  CLC_CHECK(n >= 0 && B > 0, "%s: n must not be negative and B must be positive (got %d, %d)", who, n, B);
  CLC_CHECK(n < (1 << 30), "%s: n must be below 2^30 symbols per image (got %d)", who, n);
  CLC_CHECK(C > 0 && n % C == 0, "%s: n must be whole rows of C > 0 channels (got n = %d, C = %d)", who, n, C);
  CLC_CHECK(ldsc >= C && ldmu >= C && ldh >= C, "%s: ldsc, ldmu or ldh < C", who);
  CLC_CHECK(!symbols || ld_sym >= n, "%s: ld_sym < n", who);
  if (n == 0) return 0;   // an empty segment contributes nothing
  return launch_decode_gauss(scale, ldsc, mu, ldmu, C, n, B, scale_table, n_scales, t, words, spans, state, W, y_hat, ldh, symbols, ld_sym,
                             LanesDenseRows{}, st, step);
}

extern "C" int clc_rans_lanes_decode_gauss(const float* scale, long ldsc, const float* mu, long ldmu, int C, int n, int B, const float* scale_table,
                                           int n_scales, const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes,
                                           const int32_t* offsets, const uint32_t* words, const int32_t* spans, clc_rans_lanes_state* state, int W,
                                           float* y_hat, long ldh, int32_t* symbols, long ld_sym, clc_stream_t stream) {
  return decode_gauss_entry("clc_rans_lanes_decode_gauss", scale, ldsc, mu, ldmu, nullptr, C, n, B, scale_table, n_scales, cdfs, cdf_stride, n_rows,
                            cdf_sizes, offsets, words, spans, state, W, y_hat, ldh, symbols, ld_sym, ST);
}

extern "C" int clc_rans_lanes_decode_gauss_step(const float* scale, long ldsc, const float* mu, long ldmu, const float* step, int C, int n, int B,
                                                const float* scale_table, int n_scales, const int32_t* cdfs, int cdf_stride, int n_rows,
                                                const int32_t* cdf_sizes, const int32_t* offsets, const uint32_t* words, const int32_t* spans,
                                                clc_rans_lanes_state* state, int W, float* y_hat, long ldh, int32_t* symbols, long ld_sym,
                                                clc_stream_t stream) {
  CLC_CHECK(step, "clc_rans_lanes_decode_gauss_step: step is NULL (the unit-step entry is clc_rans_lanes_decode_gauss)");
  return decode_gauss_entry("clc_rans_lanes_decode_gauss_step", scale, ldsc, mu, ldmu, step, C, n, B, scale_table, n_scales, cdfs, cdf_stride, n_rows,
                            cdf_sizes, offsets, words, spans, state, W, y_hat, ldh, symbols, ld_sym, ST);
}

extern "C" int clc_ar_lanes_decode(const float* gp, long ldg, int M, const int32_t* pix, int P, int B, int H, int W_map, const float* scale_table,
                                   int n_scales, const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets,
                                   const uint32_t* words, const int32_t* spans, clc_rans_lanes_state* state, int W, float* y_hat, long ldh,
                                   int32_t* symbols, long ld_sym, clc_stream_t stream) {
  CLC_CHECK(gp && scale_table && words && spans && state && y_hat, "clc_ar_lanes_decode: null pointer");
  const LanesTables t = {cdfs, cdf_stride, n_rows, cdf_sizes, offsets};
  if (lanes_entry_ok("clc_ar_lanes_decode", t, W, B)) return -1;
  CLC_CHECK(n_scales > 1 && n_scales <= kMaxScales, "clc_ar_lanes_decode: n_scales must be between 2 and %d (got %d)", kMaxScales, n_scales);
  CLC_CHECK(P >= 0 && B > 0 && H > 0 && W_map > 0 && M > 0, "clc_ar_lanes_decode: P must not be negative and B, H, W and M must be positive (got %d, %d, %d, %d, %d)",
            P, B, H, W_map, M);
  CLC_CHECK((long)P * M < (1l << 30), "clc_ar_lanes_decode: n = P * M must be below 2^30 symbols per image (got %ld)", (long)P * M);
  CLC_CHECK(P == 0 || pix, "clc_ar_lanes_decode: null pixel list");
  CLC_CHECK(ldg >= 2l * M, "clc_ar_lanes_decode: ldg < 2 M (scales first, means second)");
  CLC_CHECK(ldh >= M, "clc_ar_lanes_decode: ldh < M");
  CLC_CHECK((long)B * H * W_map < (1l << 31), "clc_ar_lanes_decode: B * H * W must be below 2^31");
  const int n = P * M;
  CLC_CHECK(!symbols || ld_sym >= n, "clc_ar_lanes_decode: ld_sym < n");
  if (n == 0) return 0;   // an empty step contributes nothing
  return launch_decode_gauss(gp, ldg, gp + M, ldg, M, n, B, scale_table, n_scales, t, words, spans, state, W, y_hat, ldh, symbols, ld_sym,
                             LanesPixelList{pix, H, W_map}, ST);
}

extern "C" int clc_rans_lanes_encode_list(const int32_t* symbols, const int32_t* indexes, long ld, int B, const int32_t* seg_len, int P, int W,
                                          const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets,
                                          uint32_t* out, const int32_t* regions, int32_t* result, clc_stream_t stream) {
  CLC_CHECK(symbols && indexes && out && regions && result, "clc_rans_lanes_encode_list: null pointer");
  const LanesTables t = {cdfs, cdf_stride, n_rows, cdf_sizes, offsets};
  if (lanes_entry_ok("clc_rans_lanes_encode_list", t, W, B)) return -1;
  CLC_CHECK(B > 0, "clc_rans_lanes_encode_list: B must be positive (got %d)", B);
  CLC_CHECK(P >= 0, "clc_rans_lanes_encode_list: P must not be negative (got %d)", P);
  CLC_CHECK(P == 0 || seg_len, "clc_rans_lanes_encode_list: null segment list");
  CLC_CHECK(ld >= 0 && ld < (1l << 27), "clc_rans_lanes_encode_list: ld must be between 0 and 2^27 - 1 (got %ld); a region's 128 + 10 n words must stay below 2^31", ld);
  LanesEncArgs<LanesSegList> a = {};
  a.symbols = symbols; a.indexes = indexes; a.ld = ld;
  a.t = t;
  a.out = out; a.regions = regions; a.result = result; a.W = W; a.segs = {P, seg_len};
  hipLaunchKernelGGL(rans_lanes_encode_kernel<LanesSegList>, dim3(B * W), dim3(kLanes), 0, ST, a);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_rans_lanes_pack(const uint32_t* words, long n_words, const int32_t* result, int B, int W, uint32_t* packed, long capacity,
                                   int32_t* header, clc_stream_t stream) {
  CLC_CHECK(words && result && packed && header, "clc_rans_lanes_pack: null pointer");
  CLC_CHECK(W >= 1 && W <= CLC_RANS_LANES_MAX_W, "clc_rans_lanes_pack: W must be between 1 and %d waves (got %d)", CLC_RANS_LANES_MAX_W, W);
  CLC_CHECK(B > 0, "clc_rans_lanes_pack: B must be positive (got %d)", B);
  CLC_CHECK((long)B * W < (1l << 24), "clc_rans_lanes_pack: B * W must be below 2^24");
  CLC_CHECK(n_words >= 0 && n_words < (1l << 31), "clc_rans_lanes_pack: n_words must be between 0 and 2^31 - 1 (got %ld)", n_words);
  CLC_CHECK(capacity >= 0 && capacity < (1l << 31), "clc_rans_lanes_pack: capacity must be between 0 and 2^31 - 1 words (got %ld)", capacity);
  LanesPackArgs a = {};
  a.words = words; a.n_words = n_words; a.result = result; a.n_streams = B * W; a.packed = packed; a.capacity = capacity; a.header = header;
  hipLaunchKernelGGL(rans_lanes_pack_kernel, dim3(B * W), dim3(kLanes), 0, ST, a);
  CLC_LAUNCH_CHECK();
  return 0;
}
