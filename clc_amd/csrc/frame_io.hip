// frame_io.hip — video frames in and out of the model's layout (gfx950): planar YUV 4:2:0 integer samples <-> pixel-major f32 RGB,
// and the exact sum of squared sample differences of two planes (PSNR).  Definition: DESIGN 30; ABI: include/clc_hip.h.
//
// SAMPLES.  8-bit planes are bytes; 9 .. 16-bit planes are 16-bit words read as UNSIGNED (the caller's int16 tensor is a container:
// at 16 bits 65535 is the pattern 0xFFFF).  Y is [N][H][W], U and V are [N][H/2][W/2], dense.  A sample above max = 2^bit_depth - 1
// is the caller's error and is not looked for (it converts as the number it is).
//
// COLOUR.  BT.709, full range, Kr, Kg, Kb = 0.2126, 0.7152, 0.0722; every constant below is the double expression rounded ONCE to
// f32.  THE f32 OPERATION ORDER (the Makefile compiles with -ffp-contract=off, so nothing else is fused):
//   sample -> float:   s = (float)sample * (1 / max)
//   x2 chroma sample:  the output sample a quarter of a step from tap n towards tap a1 (b = the tap behind n, a2 = the one after a1),
//                        bilinear:  fmaf(1/4, a1, 3/4 * n)
//                        bicubic:   fmaf(-27/256, b, fmaf(-9/256, a2, fmaf(67/256, a1, 225/256 * n)))      (torch's A = -0.75)
//                      tap indices clamped to the plane; ROWS first (each needed column), then along the row.
//   YCbCr -> RGB:      r = fmaf(2 - 2 Kr, cr - 0.5, y);  b = fmaf(2 - 2 Kb, cb - 0.5, y);  g = fmaf(-Kb, b, fmaf(-Kr, r, y)) * (1 / Kg)
//   RGB -> YCbCr:      r, g, b clamped to [0, 1];  y = fmaf(Kb, b, fmaf(Kg, g, Kr * r));
//                      cb = fmaf(0.5 / (1 - Kb), b - y, 0.5);  cr = fmaf(0.5 / (1 - Kr), r - y, 0.5)
//   2x2 chroma mean:   ((c00 + c01) + (c10 + c11)) * 0.25     (cxy: row x, column y of the block)
//   float -> sample:   (integer) rintf(fminf(fmaxf(v, 0), 1) * max)      (round half to even; a NaN stores 0)
// At 8 bits neutral chroma is 0.5 * 255 = 127.5, an exact tie: a grey frame lands on 127 or 128 by the last bit of b - y.  That is
// the definition's, not an error.
//
// SHAPE.  One thread per chroma sample (a 2x2 luma block), R = 8 / sizeof(sample) adjacent blocks of one block row per lane: a lane's
// luma samples of a row are 16 bytes, its chroma samples 8, its RGB pixels 2 R x 12 bytes = 12 (6) 16-byte accesses.  A run takes
// the wide path when it lies wholly inside the true image and the call's pointers and widths keep those accesses aligned (dense
// 3-channel RGB: ld == 3); every other run — the tail of a row, the replicate padding of clc_yuv420_to_rgb, an unaligned call —
// goes block by block through clamped scalar accesses.  Both paths do the same operations in the same order: a pixel's bits do
// not depend on the path, the padding, or the batch around its image.  No LDS, no scratch, no atomics in the two converters.
//
// clc_plane_sse: stage 1, one wave per block, each block a fixed range of one image, 64-bit integer partial sums by wave
// shuffles; stage 2, one wave per image over its partials.  Integer sums: exact, and the same whatever the order.
#include <algorithm>

#include "common.h"

namespace {

constexpr int TPB = 256;

constexpr double KR = 0.2126, KG = 0.7152, KB = 0.0722;
constexpr float kKr = (float)KR, kKg = (float)KG, kKb = (float)KB;
constexpr float kCr2R = (float)(2.0 - 2.0 * KR), kCb2B = (float)(2.0 - 2.0 * KB), kInvKg = (float)(1.0 / KG);
constexpr float kB2Cb = (float)(0.5 / (1.0 - KB)), kR2Cr = (float)(0.5 / (1.0 - KR));
constexpr float kCubN = 225.f / 256.f, kCubA1 = 67.f / 256.f, kCubA2 = -9.f / 256.f, kCubB = -27.f / 256.f;   // exact in f32

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct F3 { float x, y, z; };

__device__ __forceinline__ int clampi(int i, int n) { return min(max(i, 0), n - 1); }

// the x2 sample a quarter of a step from n towards a1 (MODE 0: bilinear, b and a2 unused; 1: bicubic)
template <int MODE> __device__ __forceinline__ float interp(float b, float n, float a1, float a2) {
  if constexpr (MODE == 0) return fmaf(0.25f, a1, 0.75f * n);
  else return fmaf(kCubB, b, fmaf(kCubA2, a2, fmaf(kCubA1, a1, kCubN * n)));
}

__device__ __forceinline__ F3 to_rgb(float y, float cb, float cr) {
  const float r = fmaf(kCr2R, cr - 0.5f, y), b = fmaf(kCb2B, cb - 0.5f, y);
  return {r, fmaf(-kKb, b, fmaf(-kKr, r, y)) * kInvKg, b};
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ F3 to_ycc(float r, float g, float b) {
  r = clamp01(r); g = clamp01(g); b = clamp01(b);
  const float y = fmaf(kKb, b, fmaf(kKg, g, kKr * r));
  return {y, fmaf(kB2Cb, b - y, 0.5f), fmaf(kR2Cr, r - y, 0.5f)};
}
__device__ __forceinline__ unsigned quant(float v, float maxv) { return (unsigned)rintf(clamp01(v) * maxv); }

// sample k of a run of samples held in 32-bit words (k is a constant after unrolling)
template <typename T> __device__ __forceinline__ unsigned word_sample(const unsigned* w, int k) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  return (w[k / PER] >> (BITS * (k % PER))) & ((1u << BITS) - 1u);
}

// ------------------------------------------------------------------------------------------------ YUV 4:2:0 -> RGB
struct ToRgbArgs {
  const void *y, *u, *v;
  float* rgb; long ld;
  int N, H, W, Hp, Wp, vec;
  float inv_max;
};

// one chroma plane at full-resolution pixel (sh, sw) of an image: the clamped scalar path
template <typename T, int MODE> __device__ __forceinline__ float chroma_at(const T* p, int CH, int CW, int sh, int sw, float s) {
  const int cr = sh >> 1, cc = sw >> 1, sy = (sh & 1) ? 1 : -1, sx = (sw & 1) ? 1 : -1;
  const long rn = (long)cr * CW, ra1 = (long)clampi(cr + sy, CH) * CW;
  const long rb = (long)clampi(cr - sy, CH) * CW, ra2 = (long)clampi(cr + 2 * sy, CH) * CW;
  float col[4] = {0.f, 0.f, 0.f, 0.f};   // the row's taps: behind, near, ahead 1, ahead 2 — each the rows' interpolation of its column
#pragma unroll
  for (int k = MODE ? 0 : 1; k < (MODE ? 4 : 3); ++k) {
    const int c = clampi(cc + (k - 1) * sx, CW);
    col[k] = interp<MODE>(MODE ? (float)p[rb + c] * s : 0.f, (float)p[rn + c] * s, (float)p[ra1 + c] * s, MODE ? (float)p[ra2 + c] * s : 0.f);
  }
  return interp<MODE>(col[0], col[1], col[2], col[3]);
}

template <typename T, int MODE> __global__ void __launch_bounds__(TPB) yuv420_to_rgb_kernel(const ToRgbArgs a) {
  constexpr int R = 8 / (int)sizeof(T), NT = MODE ? 2 : 1, NC = R + 2 * NT, ROWS = 2 * NT + 1;
  const int CH = a.H >> 1, CW = a.W >> 1, CHp = a.Hp >> 1, CWp = a.Wp >> 1, runs = (CWp + R - 1) / R;
  const long i = (long)blockIdx.x * TPB + threadIdx.x, total = (long)a.N * CHp * runs;
  if (i >= total) return;
  const int c0 = (int)(i % runs) * R, ch = (int)((i / runs) % CHp);
  const long n = i / ((long)runs * CHp);
  const T* yp = static_cast<const T*>(a.y) + n * a.H * a.W;
  const T* up = static_cast<const T*>(a.u) + n * CH * CW;
  const T* vp = static_cast<const T*>(a.v) + n * CH * CW;
  float* out = a.rgb + (n * a.Hp * a.Wp) * a.ld;
  const float s = a.inv_max;

  if (a.vec && ch < CH && c0 + R <= CW) {
    // the rows' interpolation of columns c0 - NT .. c0 + R + NT - 1 (clamped), for the upper (dy = 0) and lower output row
    float vert[2][2][NC];   // [plane][dy][column]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      const T* p = pl ? vp : up;
      float raw[ROWS][NC];
#pragma unroll
      for (int ri = 0; ri < ROWS; ++ri) {
        const T* row = p + (long)clampi(ch - NT + ri, CH) * CW;
        const u32x2 w = *reinterpret_cast<const u32x2*>(row + c0);
        const unsigned ww[2] = {w[0], w[1]};
#pragma unroll
        for (int k = 0; k < R; ++k) raw[ri][NT + k] = (float)word_sample<T>(ww, k) * s;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
          raw[ri][k] = (float)row[clampi(c0 - NT + k, CW)] * s;
          raw[ri][NT + R + k] = (float)row[clampi(c0 + R + k, CW)] * s;
        }
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        vert[pl][0][j] = interp<MODE>(raw[NT + 1][j], raw[NT][j], raw[NT - 1][j], MODE ? raw[NT - MODE * 2][j] : 0.f);
        vert[pl][1][j] = interp<MODE>(raw[NT - 1][j], raw[NT][j], raw[NT + 1][j], MODE ? raw[NT + MODE * 2][j] : 0.f);
      }
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int h = 2 * ch + dy;
      const u32x4 w = *reinterpret_cast<const u32x4*>(yp + (long)h * a.W + 2 * c0);
      const unsigned ww[4] = {w[0], w[1], w[2], w[3]};
      float px[2 * R * 3];
#pragma unroll
      for (int j = 0; j < 2 * R; ++j) {
        const int jc = NT + (j >> 1), sx = (j & 1) ? 1 : -1;
        const float* cu = vert[0][dy];
        const float* cv = vert[1][dy];
        const float cb = interp<MODE>(MODE ? cu[jc - MODE * sx] : 0.f, cu[jc], cu[jc + sx], MODE ? cu[jc + MODE * 2 * sx] : 0.f);
        const float cr = interp<MODE>(MODE ? cv[jc - MODE * sx] : 0.f, cv[jc], cv[jc + sx], MODE ? cv[jc + MODE * 2 * sx] : 0.f);
        const F3 q = to_rgb((float)word_sample<T>(ww, j) * s, cb, cr);
        px[3 * j] = q.x; px[3 * j + 1] = q.y; px[3 * j + 2] = q.z;
      }
      f32x4* dst = reinterpret_cast<f32x4*>(out + ((long)h * a.Wp + 2 * c0) * 3);
#pragma unroll
      for (int k = 0; k < 2 * R * 3 / 4; ++k) dst[k] = (f32x4){px[4 * k], px[4 * k + 1], px[4 * k + 2], px[4 * k + 3]};
    }
    return;
  }
  // block by block: the tail of a row, the padding (output pixel (h, w) = converted pixel (min(h, H - 1), min(w, W - 1))), unaligned calls
  for (int k = 0; k < R; ++k) {
    const int c = c0 + k;
    if (c >= CWp) break;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int h = 2 * ch + (d >> 1), w = 2 * c + (d & 1), sh = min(h, a.H - 1), sw = min(w, a.W - 1);
      const F3 q = to_rgb((float)yp[(long)sh * a.W + sw] * s, chroma_at<T, MODE>(up, CH, CW, sh, sw, s), chroma_at<T, MODE>(vp, CH, CW, sh, sw, s));
      float* o = out + ((long)h * a.Wp + w) * a.ld;
      o[0] = q.x; o[1] = q.y; o[2] = q.z;
    }
  }
}

// ------------------------------------------------------------------------------------------------ RGB -> YUV 4:2:0
struct ToYuvArgs {
  const float* rgb; long ld;
  int N, H, W, Hp, Wp, vec;
  void *y, *u, *v;
  float maxv;
};

template <typename T> __global__ void __launch_bounds__(TPB) rgb_to_yuv420_kernel(const ToYuvArgs a) {
  constexpr int R = 8 / (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  const int CH = a.H >> 1, CW = a.W >> 1, runs = (CW + R - 1) / R;
  const long i = (long)blockIdx.x * TPB + threadIdx.x, total = (long)a.N * CH * runs;
  if (i >= total) return;
  const int c0 = (int)(i % runs) * R, ch = (int)((i / runs) % CH);
  const long n = i / ((long)runs * CH);
  const float* in = a.rgb + (n * a.Hp * a.Wp) * a.ld;   // the crop: the top-left H x W of the Hp x Wp frame
  T* yp = static_cast<T*>(a.y) + n * a.H * a.W;
  T* up = static_cast<T*>(a.u) + n * CH * CW;
  T* vp = static_cast<T*>(a.v) + n * CH * CW;

  if (a.vec && c0 + R <= CW) {
    float sb[2][R], sr[2][R];   // per block and row: cb and cr of its two pixels, added
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int h = 2 * ch + dy;
      const f32x4* src = reinterpret_cast<const f32x4*>(in + ((long)h * a.Wp + 2 * c0) * 3);
      float px[2 * R * 3];
#pragma unroll
      for (int k = 0; k < 2 * R * 3 / 4; ++k) {
        const f32x4 t = src[k];
        px[4 * k] = t[0]; px[4 * k + 1] = t[1]; px[4 * k + 2] = t[2]; px[4 * k + 3] = t[3];
      }
      unsigned yw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const F3 p0 = to_ycc(px[6 * k], px[6 * k + 1], px[6 * k + 2]), p1 = to_ycc(px[6 * k + 3], px[6 * k + 4], px[6 * k + 5]);
        yw[(2 * k) / PER] |= quant(p0.x, a.maxv) << (BITS * ((2 * k) % PER));
        yw[(2 * k + 1) / PER] |= quant(p1.x, a.maxv) << (BITS * ((2 * k + 1) % PER));
        sb[dy][k] = p0.y + p1.y;
        sr[dy][k] = p0.z + p1.z;
      }
      *reinterpret_cast<u32x4*>(yp + (long)h * a.W + 2 * c0) = (u32x4){yw[0], yw[1], yw[2], yw[3]};
    }
    unsigned uw[2] = {0u, 0u}, vw[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < R; ++k) {
      uw[k / PER] |= quant((sb[0][k] + sb[1][k]) * 0.25f, a.maxv) << (BITS * (k % PER));
      vw[k / PER] |= quant((sr[0][k] + sr[1][k]) * 0.25f, a.maxv) << (BITS * (k % PER));
    }
    *reinterpret_cast<u32x2*>(up + (long)ch * CW + c0) = (u32x2){uw[0], uw[1]};
    *reinterpret_cast<u32x2*>(vp + (long)ch * CW + c0) = (u32x2){vw[0], vw[1]};
    return;
  }
  for (int k = 0; k < R; ++k) {
    const int c = c0 + k;
    if (c >= CW) break;
    float sb[2], sr[2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int h = 2 * ch + dy;
      const float* p = in + ((long)h * a.Wp + 2 * c) * a.ld;
      const F3 p0 = to_ycc(p[0], p[1], p[2]), p1 = to_ycc(p[a.ld], p[a.ld + 1], p[a.ld + 2]);
      yp[(long)h * a.W + 2 * c] = (T)quant(p0.x, a.maxv);
      yp[(long)h * a.W + 2 * c + 1] = (T)quant(p1.x, a.maxv);
      sb[dy] = p0.y + p1.y;
      sr[dy] = p0.z + p1.z;
    }
    up[(long)ch * CW + c] = (T)quant((sb[0] + sb[1]) * 0.25f, a.maxv);
    vp[(long)ch * CW + c] = (T)quant((sr[0] + sr[1]) * 0.25f, a.maxv);
  }
}

// ------------------------------------------------------------------------------------------------ sum of squared differences
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

constexpr int kSseWave = 64, kSseMaxBlocks = 1024;
constexpr long kSseChunk = 4096;   // samples per block at least
inline int sse_blocks(long n) { return (int)std::min((long)kSseMaxBlocks, std::max(1L, (n + kSseChunk - 1) / kSseChunk)); }

// block (x, image y): units [x * per, min(units, (x + 1) * per)) of the image, a unit = 16 bytes of samples (VEC) or one sample
template <typename T, bool VEC>
__global__ void __launch_bounds__(kSseWave) plane_sse_partial_kernel(const T* a, const T* b, long n, int nb, unsigned long long* part) {
  constexpr int E = 16 / (int)sizeof(T);
  const long units = VEC ? n / E : n, per = (units + nb - 1) / nb;
  const long lo = (long)blockIdx.x * per, hi = min(units, lo + per);
  const T* pa = a + (long)blockIdx.y * n;
  const T* pb = b + (long)blockIdx.y * n;
  unsigned long long acc = 0;
  for (long i = lo + threadIdx.x; i < hi; i += kSseWave) {
    if constexpr (VEC) {
      const u32x4 va = reinterpret_cast<const u32x4*>(pa)[i], vb = reinterpret_cast<const u32x4*>(pb)[i];
      const unsigned wa[4] = {va[0], va[1], va[2], va[3]}, wb[4] = {vb[0], vb[1], vb[2], vb[3]};
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const long d = (long)word_sample<T>(wa, k) - (long)word_sample<T>(wb, k);
        acc += (unsigned long long)(d * d);
      }
    } else {
      const long d = (long)pa[i] - (long)pb[i];
      acc += (unsigned long long)(d * d);
    }
  }
  acc = wave_sum_u64(acc);
  if (threadIdx.x == 0) part[(long)blockIdx.y * nb + blockIdx.x] = acc;
}

__global__ void __launch_bounds__(kSseWave) plane_sse_final_kernel(const unsigned long long* part, int nb, long long* out) {
  unsigned long long acc = 0;
  for (int i = threadIdx.x; i < nb; i += kSseWave) acc += part[(long)blockIdx.x * nb + i];
  acc = wave_sum_u64(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = (long long)acc;
}

int check_frame(const char* who, int bit_depth, int N, int H, int W, int Hp, int Wp, long ld, const void* rgb, const void* y, const void* u, const void* v) {
  CLC_CHECK(bit_depth >= 8 && bit_depth <= 16, "%s: bit_depth must be 8 .. 16 (got bit_depth=%d)", who, bit_depth);
  CLC_CHECK(N >= 1 && H >= 2 && W >= 2, "%s: N must be positive and H, W at least 2 (got N=%d H=%d W=%d)", who, N, H, W);
  CLC_CHECK(H % 2 == 0 && W % 2 == 0, "%s: H and W must be even, 4:2:0 has one chroma sample per 2x2 block (got H=%d W=%d)", who, H, W);
  CLC_CHECK(Hp >= H && Wp >= W && Hp % 2 == 0 && Wp % 2 == 0, "%s: Hp and Wp must be even with Hp >= H and Wp >= W (got Hp=%d Wp=%d for H=%d W=%d)", who, Hp,
            Wp, H, W);
  CLC_CHECK(ld >= 3, "%s: ld < 3 (got ld=%ld)", who, ld);
  CLC_CHECK(rgb != nullptr && y != nullptr && u != nullptr && v != nullptr, "%s: rgb, y, u or v is NULL", who);
  CLC_CHECK((reinterpret_cast<uintptr_t>(rgb) & 3) == 0, "%s: rgb must be 4-byte aligned", who);
  if (bit_depth > 8)
    CLC_CHECK(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v)) & 1) == 0,
              "%s: 16-bit sample planes must be 2-byte aligned", who);
  CLC_CHECK((long)N * Hp * Wp < (1L << 31), "%s: N*Hp*Wp must stay below 2^31 (got %ld)", who, (long)N * Hp * Wp);
  return 0;
}

// the wide path's alignment: every 16-byte luma / RGB access and every 8-byte chroma access of every run
bool wide_ok(int bit_depth, int W, int Wp, long ld, const void* rgb, const void* y, const void* u, const void* v) {
  const int sz = bit_depth > 8 ? 2 : 1;
  return ld == 3 && Wp % 4 == 0 && (W * sz) % 16 == 0 && aligned16(rgb) && aligned16(y) && (reinterpret_cast<uintptr_t>(u) & 7) == 0 &&
         (reinterpret_cast<uintptr_t>(v) & 7) == 0;
}

inline unsigned blocks_for(long n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

extern "C" {

int clc_yuv420_to_rgb(const void* y, const void* u, const void* v, int bit_depth, int N, int H, int W, int mode, float* rgb, long ld, int Hp, int Wp,
                      clc_stream_t stream) {
  if (check_frame("clc_yuv420_to_rgb", bit_depth, N, H, W, Hp, Wp, ld, rgb, y, u, v) < 0) return -1;
  CLC_CHECK(mode == CLC_CHROMA_BILINEAR || mode == CLC_CHROMA_BICUBIC, "clc_yuv420_to_rgb: mode must be CLC_CHROMA_BILINEAR or CLC_CHROMA_BICUBIC (got mode=%d)",
            mode);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ToRgbArgs a = {y, u, v, rgb, ld, N, H, W, Hp, Wp, wide_ok(bit_depth, W, Wp, ld, rgb, y, u, v) ? 1 : 0,
                       (float)(1.0 / (double)((1 << bit_depth) - 1))};
  const int R = bit_depth > 8 ? 4 : 8;
  const unsigned grid = blocks_for((long)N * (Hp / 2) * ((Wp / 2 + R - 1) / R));
  if (bit_depth == 8) {
    if (mode == CLC_CHROMA_BILINEAR) yuv420_to_rgb_kernel<uint8_t, 0><<<grid, TPB, 0, st>>>(a);
    else yuv420_to_rgb_kernel<uint8_t, 1><<<grid, TPB, 0, st>>>(a);
  } else {
    if (mode == CLC_CHROMA_BILINEAR) yuv420_to_rgb_kernel<uint16_t, 0><<<grid, TPB, 0, st>>>(a);
    else yuv420_to_rgb_kernel<uint16_t, 1><<<grid, TPB, 0, st>>>(a);
  }
  CLC_LAUNCH_CHECK();
  return 0;
}

int clc_rgb_to_yuv420(const float* rgb, long ld, int Hp, int Wp, int N, int H, int W, int bit_depth, void* y, void* u, void* v, clc_stream_t stream) {
  if (check_frame("clc_rgb_to_yuv420", bit_depth, N, H, W, Hp, Wp, ld, rgb, y, u, v) < 0) return -1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ToYuvArgs a = {rgb, ld, N, H, W, Hp, Wp, wide_ok(bit_depth, W, Wp, ld, rgb, y, u, v) ? 1 : 0, y, u, v, (float)((1 << bit_depth) - 1)};
  const int R = bit_depth > 8 ? 4 : 8;
  const unsigned grid = blocks_for((long)N * (H / 2) * ((W / 2 + R - 1) / R));
  if (bit_depth == 8) rgb_to_yuv420_kernel<uint8_t><<<grid, TPB, 0, st>>>(a);
  else rgb_to_yuv420_kernel<uint16_t><<<grid, TPB, 0, st>>>(a);
  CLC_LAUNCH_CHECK();
  return 0;
}

size_t clc_plane_sse_workspace_bytes(int N, long n) {
  if (N < 1 || n < 1 || n >= (1L << 31)) {
    clc_set_error("clc_plane_sse_workspace_bytes: N must be positive and n between 1 and 2^31 - 1 samples per image (got N=%d n=%ld)", N, n);
    return 0;
  }
  return (size_t)N * sse_blocks(n) * sizeof(unsigned long long);
}

int clc_plane_sse(const void* a, const void* b, int bit_depth, int N, long n, int64_t* out, void* ws, size_t ws_bytes, clc_stream_t stream) {
  CLC_CHECK(bit_depth >= 8 && bit_depth <= 16, "clc_plane_sse: bit_depth must be 8 .. 16 (got bit_depth=%d)", bit_depth);
  CLC_CHECK(N >= 1 && N <= 65535 && n >= 1 && n < (1L << 31), "clc_plane_sse: N must be 1 .. 65535 and n between 1 and 2^31 - 1 samples per image (got N=%d n=%ld)",
            N, n);
  CLC_CHECK(a != nullptr && b != nullptr && out != nullptr, "clc_plane_sse: a, b or out is NULL");
  const int sz = bit_depth > 8 ? 2 : 1;
  CLC_CHECK(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & (sz - 1)) == 0, "clc_plane_sse: 16-bit sample planes must be 2-byte aligned");
  CLC_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0, "clc_plane_sse: out must be 8-byte aligned");
  const int nb = sse_blocks(n);
  CLC_CHECK(ws != nullptr && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_bytes >= (size_t)N * nb * 8,
            "clc_plane_sse: ws must be 8-byte aligned with ws_bytes >= %zu (got %zu)", (size_t)N * nb * 8, ws_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* part = static_cast<unsigned long long*>(ws);
  const bool vec = aligned16(a) && aligned16(b) && (n * sz) % 16 == 0;
  const dim3 grid(nb, N);
  if (sz == 1) {
    if (vec) plane_sse_partial_kernel<uint8_t, true><<<grid, kSseWave, 0, st>>>(static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), n, nb, part);
    else plane_sse_partial_kernel<uint8_t, false><<<grid, kSseWave, 0, st>>>(static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), n, nb, part);
  } else {
    if (vec) plane_sse_partial_kernel<uint16_t, true><<<grid, kSseWave, 0, st>>>(static_cast<const uint16_t*>(a), static_cast<const uint16_t*>(b), n, nb, part);
    else plane_sse_partial_kernel<uint16_t, false><<<grid, kSseWave, 0, st>>>(static_cast<const uint16_t*>(a), static_cast<const uint16_t*>(b), n, nb, part);
  }
  plane_sse_final_kernel<<<N, kSseWave, 0, st>>>(part, nb, reinterpret_cast<long long*>(out));
  CLC_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
