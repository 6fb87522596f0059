// row_gemm.hip — the batch-invariant row GEMM of the space-channel context model (ELIC, He et al., CVPR 2022) on gfx950: the 1x1
// "parameter aggregation" layers of the coder, out[r][n] = act(bias[n] + sum_k in(r, k) w[n][k]) for the rows r = b * P + p of a pixel
// list, on the matrix cores.  The contract is clc_ar_linear's (ar_context.hip); that kernel re-reads its eight rows and its filter row
// per wave and is built for the one-to-forty-row steps of mbt2018, this one for the 768 .. 6 144 rows x 704 .. 1 408 -> 640 -> 512 layers
// a checkerboard pass of a channel group has.  f32 operands, f32 accumulation on v_mfma_f32_32x32x2_f32, wave64.  The structure is
// ckbd_context.hip's / conv5.hip's (128 rows x 64 output channels per workgroup of four waves, 32 channels of one range per K-step,
// [rows][32 + 4] LDS images of both operands, two stages, one barrier per step, register-staged loads, one tile variant); what differs
// is the row space — the pixel list, one "tap": the row's own pixel (CLC_AR_SRC_PIXEL) or its dense row (CLC_AR_SRC_DENSE) — and that
// there is no partner store.
//
// A row past the end, or a row whose pixel lies outside the map, is zero-filled on load and never stored (clc_ar_linear neither reads
// nor writes such a pixel either).
//
// ORDER RULE.  Every output element sums its ranges in order; within a range the 32-channel chunks ascending; the last chunk of a range
// is zero-filled on both operands past C and never skipped; inside a chunk by MFMA and lane half as conv5.hip does (lane half h takes
// k = 8 ks + 4 h + {0..3} for ks = 0..3, each k one MFMA into the one accumulator).  bias + sum, then the activation.  The order is a
// function of (C_1, ..., C_nsrc) alone: not of P, B, the row's place in the list, the tile it lands in or the grid — rows share filter
// registers, never an accumulator.  A stream written from a batch of 8 therefore decodes one image at a time.
// This is NOT the order of clc_ar_linear: the two kernels are not interchangeable inside one stream.
//
// Every loop bound is fixed by the arguments, no workgroup waits on another; stream-ordered, graph-capturable, allocation- and
// sync-free, no workspace.
#include "common.h"

namespace {

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int kBM = 128;                        // rows per workgroup
constexpr int kBN = 64;                         // output channels per workgroup
constexpr int kKC = 32;                         // channels per K-step
constexpr int kPitch = kKC + 4;                 // LDS row pitch: 16-lane b128 reads of 16 rows hit 64 different banks
constexpr int kStage = (kBM + kBN) * kPitch;    // floats per stage
constexpr int kLds = 2 * kStage * 4;            // 55 296 B: two workgroups per CU
constexpr int kMaxSrc = 4;

struct RgParams {
  clc_ar_src s[kMaxSrc];
  int nsrc;
  const int32_t* pix;
  int P, B, H, W;
  const float* w; const float* bias; float* out;
  int N, K, act, ldo, vec_store;
  int rows;    // B * P
  int total;   // K-steps: sum over the ranges of ceil(C / 32)
};

// the pixel of row m, or -1 for a row past the end / a pixel outside the map
__device__ __forceinline__ int pixel_of(const RgParams& p, int m) {
  if (m >= p.rows) return -1;
  const int b = m / p.P, e = m - b * p.P;
  const int h = p.pix[2 * e], w = p.pix[2 * e + 1];
  if ((unsigned)h >= (unsigned)p.H || (unsigned)w >= (unsigned)p.W) return -1;
  return (b * p.H + h) * p.W + w;
}

__global__ __launch_bounds__(256) void row_gemm_kernel(const RgParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  const int wp = wave & 1, wc = wave >> 1;   // the wave's 64-row half / 32-channel half of the 128 x 64 tile
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  const int lrow = tid >> 3, lcol = (tid & 7) << 2;   // loader role: rows lrow + 32 i, columns lcol .. lcol + 3 of the chunk

  int pixel[4];   // the loader's four rows (< 0: zero-filled)
#pragma unroll
  for (int i = 0; i < 4; ++i) pixel[i] = pixel_of(p, m0 + lrow + 32 * i);

  f32x4 vx[4], vw[2];
  auto load = [&](int s, int kc, int kofs) {
    const clc_ar_src src = p.s[s];
    const int k = kc * kKC + lcol;
    const bool kin = k < src.C;   // C % 4 == 0: the whole 16-byte group is inside or outside
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (pixel[i] >= 0 && kin) {
        const size_t row = src.kind == CLC_AR_SRC_DENSE ? (size_t)(m0 + lrow + 32 * i) : (size_t)pixel[i];
        vx[i] = *reinterpret_cast<const f32x4*>(src.p + row * src.ld + k);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + lrow + 32 * i;
      vw[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (n < p.N && kin) vw[i] = *reinterpret_cast<const f32x4*>(p.w + (size_t)n * p.K + kofs + k);
    }
  };
  auto store = [&](int buf) {
    float* X = sm + buf * kStage;
    float* Wm = X + kBM * kPitch;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(X + (lrow + 32 * i) * kPitch + lcol) = vx[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(Wm + (lrow + 32 * i) * kPitch + lcol) = vw[i];
  };

  f32x16 acc[2];   // [row tile of the wave]
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;

  int s = 0, kc = 0, kofs = 0;   // block-uniform: the range, the chunk inside it, the range's first filter column
  load(0, 0, 0);
  store(0);
  __syncthreads();
  for (int step = 0; step < p.total; ++step) {
    const int cur = step & 1;
    int ns = s, nkc = kc + 1, nkofs = kofs;
    if (nkc * kKC >= p.s[s].C) { nkofs += p.s[s].C; ++ns; nkc = 0; }
    const bool more = step + 1 < p.total;   // block-uniform
    if (more) load(ns, nkc, nkofs);
    const float* X = sm + cur * kStage + (wp * 64 + li) * kPitch + 4 * h;
    const float* Wm = sm + cur * kStage + (kBM + wc * 32 + li) * kPitch + 4 * h;
#pragma unroll
    for (int ks = 0; ks < kKC / 8; ++ks) {
      // lane half h takes k = 8 ks + 4 h + {0..3}: any k order serves as long as both operands use the same one
      const f32x4 a = *reinterpret_cast<const f32x4*>(Wm + 8 * ks);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(X + 8 * ks), b1 = *reinterpret_cast<const f32x4*>(X + 32 * kPitch + 8 * ks);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = MFMA(a[e], b0[e], acc[0]);
        acc[1] = MFMA(a[e], b1[e], acc[1]);
      }
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    s = ns; kc = nkc; kofs = nkofs;
  }

  // epilogue: bias, activation, store (a lane: one row, channels 8 q + 4 h + {0..3} of the wave's 32)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int m = m0 + wp * 64 + b * 32 + li;
    if (pixel_of(p, m) < 0) continue;
    float* op = p.out + (size_t)m * p.ldo;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + wc * 32 + 8 * q + 4 * h;
      if (n >= p.N) continue;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bj = (p.bias && n + j < p.N) ? p.bias[n + j] : 0.f;
        v[j] = apply_act(bj + acc[b][4 * q + j], p.act);
      }
      if (p.vec_store) {
        *reinterpret_cast<f32x4*>(op + n) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n + j < p.N) op[n + j] = v[j];
      }
    }
  }
}

}  // namespace

extern "C" int clc_row_gemm(const clc_ar_src* srcs, int nsrc, const int32_t* pix, int P, int B, int H, int W, const float* w, const float* bias,
                            int N, int act, float* out, int ldo, clc_stream_t stream) {
  CLC_CHECK(srcs && pix && w && out, "clc_row_gemm: null pointer (srcs, pix, w or out)");
  CLC_CHECK(nsrc >= 1 && nsrc <= kMaxSrc, "clc_row_gemm: nsrc must be 1 to 4 (got %d)", nsrc);
  CLC_CHECK(P > 0 && B > 0 && H > 0 && W > 0 && N > 0, "clc_row_gemm: P, B, H, W and N must be positive (P=%d B=%d H=%d W=%d N=%d)", P, B, H, W, N);
  CLC_CHECK(act == CLC_ACT_NONE || act == CLC_ACT_LRELU || act == CLC_ACT_RELU,
            "clc_row_gemm: act must be CLC_ACT_NONE, CLC_ACT_LRELU or CLC_ACT_RELU (got %d)", act);
  CLC_CHECK(ldo >= N, "clc_row_gemm: ldo < N (ldo=%d N=%d)", ldo, N);
  CLC_CHECK((long)B * H * W < (1l << 31), "clc_row_gemm: B * H * W must be below 2^31 (got %ld)", (long)B * H * W);
  CLC_CHECK((long)B * P < (1l << 31) - kBM, "clc_row_gemm: B * P must be below 2^31 (got %ld)", (long)B * P);
  RgParams p;
  p.nsrc = nsrc;
  p.total = 0;
  long K = 0;
  for (int s = 0; s < nsrc; ++s) {
    const clc_ar_src& r = srcs[s];
    CLC_CHECK(r.kind != CLC_AR_SRC_TAPS, "clc_row_gemm: range %d is CLC_AR_SRC_TAPS: the gather stays with clc_ar_linear", s);
    CLC_CHECK(r.kind == CLC_AR_SRC_DENSE || r.kind == CLC_AR_SRC_PIXEL, "clc_row_gemm: range %d has unknown kind %d", s, r.kind);
    CLC_CHECK(r.p, "clc_row_gemm: range %d has a null pointer", s);
    CLC_CHECK(r.C > 0 && r.C % 4 == 0, "clc_row_gemm: C %% 4 != 0 (range %d has C = %d)", s, r.C);
    CLC_CHECK(r.ld >= r.C && r.ld % 4 == 0, "clc_row_gemm: ld %% 4 != 0 or ld < C (range %d has ld = %d, C = %d)", s, r.ld, r.C);
    CLC_CHECK(aligned16(r.p), "clc_row_gemm: range %d is not 16-byte aligned", s);
    p.s[s] = r;
    K += r.C;
    p.total += (r.C + kKC - 1) / kKC;
  }
  for (int s = nsrc; s < kMaxSrc; ++s) p.s[s] = p.s[0];
  CLC_CHECK(K < (1l << 31), "clc_row_gemm: K = sum of C must be below 2^31 (got %ld)", K);
  CLC_CHECK(aligned16(w), "clc_row_gemm: the filter w is not 16-byte aligned");
  p.pix = pix; p.P = P; p.B = B; p.H = H; p.W = W;
  p.w = w; p.bias = bias; p.out = out;
  p.N = N; p.K = (int)K; p.act = act; p.ldo = ldo;
  p.vec_store = N % 4 == 0 && ldo % 4 == 0 && aligned16(out);
  p.rows = (int)((long)B * P);
  const long ntile = ((long)N + kBN - 1) / kBN;
  CLC_CHECK(ntile <= 65535, "clc_row_gemm: N must be at most 65535 * 64 (got %d)", N);
  static PerDeviceOnce attr_once;
  if (attr_once.first())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&row_gemm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  dim3 grid((p.rows + kBM - 1) / kBM, (unsigned)ntile);
  hipLaunchKernelGGL(row_gemm_kernel, grid, dim3(256), kLds, (hipStream_t)stream, p);
  CLC_LAUNCH_CHECK();
  return 0;
}
