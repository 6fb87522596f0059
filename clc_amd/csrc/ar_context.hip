// ar_context.hip — the sequential part of the autoregressive context model (mbt2018, JointAutoregressiveHierarchicalPriors) on gfx950.
//
// The coder evaluates, per latent pixel, gather(12 live taps of the 5x5 mask-A window) -> M -> 2M, then 4M -> 10M/3 -> 8M/3 -> 2M, then
// quantise and index.  The encoder does it for all pixels of a wavefront step at once, the decoder for one pixel at a time, and both must
// arrive at the same float bits or the arithmetic decoder loses sync.  So the small-row GEMM here sums every output element in an order
// that is a function of the K of each range ALONE:
//
//   one wave per (output channel n, block of kRows rows); lane l owns the 16-byte K-chunks q = l, l + 64, l + 128, ... of a range, in
//   that order, and folds each chunk's four products into ONE accumulator per row with four fmaf in element order; a second range
//   continues the same accumulators; then the 64 lane sums are added by the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum), then
//   bias + sum, then the activation.
//
// Nothing in that sentence mentions the row count, the row's place in the list, the pixel's place in the map, the batch or the grid:
// rows only share the filter registers of their wave, never an accumulator.  A tap outside the map is the operand 0.0f, and
// fmaf(0, w, acc) == acc for every finite w, so a border pixel's bits do not depend on how its zeros are produced either.
//
// Work per step is tiny (M = 192: 7.5 MB of filters, a few hundred rows at most): launch- and latency-bound, so plain f32 VALU FMAs,
// no LDS, no barrier, nothing that waits on another workgroup.  Stream-ordered, allocation-free, graph-capturable.
#include "coder_device.h"

namespace {
using namespace coder;

constexpr int kRows = 8;   // rows that share one wave's filter registers
constexpr long kMaxRowBlocksY = 32;   // grid.y: beyond 256 rows a workgroup walks several row blocks

struct ArLinArgs {
  clc_ar_src s[2];
  int nsrc;
  const int32_t* pix;
  int P, B, H, W;
  const float* w;
  const float* bias;
  int N, K, act;
  float* out;
  int ldo;
  long rows;
};

// live tap t = 0..11 of mask A in (kh, kw) ascending order -> offset of the tap from the window's centre
__device__ __forceinline__ void tap_offset(int t, int& dh, int& dw) {
  if (t < 10) {
    const int kh = t / 5;
    dh = kh - 2;
    dw = t - 5 * kh - 2;
  } else {
    dh = 0;
    dw = t - 12;
  }
}

__global__ __launch_bounds__(256) void ar_linear_kernel(const ArLinArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.N) return;   // wave-uniform; the kernel has no barrier
  const float* wrow = a.w + (size_t)n * a.K;
  const float bn = a.bias ? a.bias[n] : 0.f;
  const long nblk = (a.rows + kRows - 1) / kRows;
  for (long rb = blockIdx.y; rb < nblk; rb += gridDim.y) {
    int ph[kRows], pw[kRows];
    long pixel[kRows];
    bool ok[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const long r = rb * kRows + i;
      ok[i] = r < a.rows;
      ph[i] = pw[i] = 0;
      pixel[i] = 0;
      if (ok[i]) {
        const int b = (int)(r / a.P), p = (int)(r - (long)b * a.P);
        ph[i] = a.pix[2 * p];
        pw[i] = a.pix[2 * p + 1];
        ok[i] = ph[i] >= 0 && ph[i] < a.H && pw[i] >= 0 && pw[i] < a.W;   // a pixel outside the map is neither read nor written
        pixel[i] = ((long)b * a.H + ph[i]) * a.W + pw[i];
      }
    }
    float acc[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i) acc[i] = 0.f;
    int kofs = 0;
    for (int s = 0; s < a.nsrc; ++s) {
      const clc_ar_src src = a.s[s];
      const int K = src.kind == CLC_AR_SRC_TAPS ? 12 * src.C : src.C;
      for (int q = lane; q < (K >> 2); q += 64) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wrow + kofs + 4 * q);
        int c = 4 * q, dh = 0, dw = 0;
        if (src.kind == CLC_AR_SRC_TAPS) {
          const int t = c / src.C;
          c -= t * src.C;
          tap_offset(t, dh, dw);
        }
        f32x4 xv[kRows];
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
          xv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (!ok[i]) continue;
          if (src.kind == CLC_AR_SRC_DENSE) {
            xv[i] = *reinterpret_cast<const f32x4*>(src.p + (size_t)(rb * kRows + i) * src.ld + c);
          } else {
            const int hh = ph[i] + dh, ww = pw[i] + dw;
            if (hh >= 0 && hh < a.H && ww >= 0 && ww < a.W)
              xv[i] = *reinterpret_cast<const f32x4*>(src.p + (size_t)(pixel[i] + (long)dh * a.W + dw) * src.ld + c);
          }
        }
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
          float v = acc[i];
          v = fmaf(xv[i][0], wv[0], v);
          v = fmaf(xv[i][1], wv[1], v);
          v = fmaf(xv[i][2], wv[2], v);
          v = fmaf(xv[i][3], wv[3], v);
          acc[i] = v;
        }
      }
      kofs += K;
    }
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const float v = wave_sum(acc[i]);
      if (lane == 0 && ok[i]) a.out[(size_t)(rb * kRows + i) * a.ldo + n] = apply_act(bn + v, a.act);
    }
  }
}

// mode 0 (encode): symbols / indexes at the pixel's raster place of [B][H*W][M], y_hat into the map; mode 1 (decode): indexes to the
// dense [rows][M] buffer.  The index is quantize_build_indexes_kernel's (entropy.hip): coder::scale_index_linear.
// y and y_hat may be the same map (each element is read and then written by one thread).
__global__ __launch_bounds__(256) void ar_finish_kernel(const float* __restrict__ gp, int ldg, int M, const int32_t* __restrict__ pix, int P, int H, int W,
                                                      const float* __restrict__ table, int n_scales, const float* y, int ldy, float* y_hat, int ldh,
                                                      int32_t* __restrict__ symbols, int32_t* __restrict__ indexes, int mode, long rows) {
  __shared__ float tb[256];
  for (int i = threadIdx.x; i < n_scales; i += 256) tb[i] = table[i];
  __syncthreads();
  const long total = rows * M;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / M;
    const int c = (int)(i - r * M);
    const int idx = scale_index_linear(fmaxf(gp[r * ldg + c], kScaleBound), tb, n_scales);
    if (mode == 1) {
      indexes[i] = idx;
      continue;
    }
    const int b = (int)(r / P), p = (int)(r - (long)b * P);
    const long px = pixel_of(pix, p, b, H, W);
    if (px < 0) continue;
    const float m = gp[r * ldg + M + c];
    const float q = rintf(y[px * ldy + c] - m);
    symbols[px * M + c] = (int32_t)q;
    indexes[px * M + c] = idx;
    y_hat[px * ldh + c] = q + m;
  }
}

__global__ __launch_bounds__(256) void ar_commit_kernel(const int32_t* __restrict__ symbols, const float* __restrict__ gp, int ldg, int M,
                                                      const int32_t* __restrict__ pix, int P, int H, int W, float* __restrict__ y_hat, int ldh, long rows) {
  const long total = rows * M;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / M;
    const int c = (int)(i - r * M);
    const int b = (int)(r / P), p = (int)(r - (long)b * P);
    const long px = pixel_of(pix, p, b, H, W);
    if (px < 0) continue;
    const float q = (float)symbols[i];   // the encoder's rintf(y - m): an integer-valued float either way
    y_hat[px * ldh + c] = q + gp[r * ldg + M + c];
  }
}

int grid_rows(long total) { return (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048); }

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int clc_ar_linear(const clc_ar_src* srcs, int nsrc, const int32_t* pix, int P, int B, int H, int W, const float* w, const float* bias,
                             int N, int act, float* out, int ldo, clc_stream_t stream) {
  CLC_CHECK(srcs && pix && w && out, "clc_ar_linear: null pointer");
  CLC_CHECK(nsrc == 1 || nsrc == 2, "clc_ar_linear: nsrc must be 1 or 2 (got %d)", nsrc);
  CLC_CHECK(P > 0 && B > 0 && H > 0 && W > 0 && N > 0, "clc_ar_linear: P, B, H, W and N must be positive");
  CLC_CHECK(act == CLC_ACT_NONE || act == CLC_ACT_LRELU, "clc_ar_linear: act must be CLC_ACT_NONE or CLC_ACT_LRELU (got %d)", act);
  CLC_CHECK(ldo >= N, "clc_ar_linear: ldo < N");
  CLC_CHECK((long)B * H * W < (1l << 31), "clc_ar_linear: B * H * W must be below 2^31");
  ArLinArgs a;
  a.nsrc = nsrc;
  a.K = 0;
  for (int s = 0; s < nsrc; ++s) {
    const clc_ar_src& r = srcs[s];
    CLC_CHECK(r.kind == CLC_AR_SRC_DENSE || r.kind == CLC_AR_SRC_PIXEL || r.kind == CLC_AR_SRC_TAPS, "clc_ar_linear: range %d has unknown kind %d", s, r.kind);
    CLC_CHECK(r.p, "clc_ar_linear: range %d has a null pointer", s);
    CLC_CHECK(r.C > 0 && r.C % 4 == 0, "clc_ar_linear: C %% 4 != 0 (range %d has C = %d)", s, r.C);
    CLC_CHECK(r.ld >= r.C && r.ld % 4 == 0, "clc_ar_linear: ld %% 4 != 0 or ld < C (range %d has ld = %d, C = %d)", s, r.ld, r.C);
    CLC_CHECK(aligned16(r.p), "clc_ar_linear: range %d is not 16-byte aligned", s);
    a.s[s] = r;
    a.K += r.kind == CLC_AR_SRC_TAPS ? 12 * r.C : r.C;
  }
  if (nsrc == 1) a.s[1] = a.s[0];
  CLC_CHECK(aligned16(w), "clc_ar_linear: the filter is not 16-byte aligned");
  a.pix = pix; a.P = P; a.B = B; a.H = H; a.W = W;
  a.w = w; a.bias = bias; a.N = N; a.act = act; a.out = out; a.ldo = ldo;
  a.rows = (long)B * P;
  const long nblk = (a.rows + kRows - 1) / kRows;
  hipLaunchKernelGGL(ar_linear_kernel, dim3((N + 3) / 4, (unsigned)(nblk < kMaxRowBlocksY ? nblk : kMaxRowBlocksY)), dim3(256), 0, ST, a);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_ar_finish(const float* gp, int ldg, int M, const int32_t* pix, int P, int B, int H, int W, const float* scale_table, int n_scales,
                             const float* y, int ldy, float* y_hat, int ldh, int32_t* symbols, int32_t* indexes, int mode, clc_stream_t stream) {
  CLC_CHECK(gp && pix && scale_table && indexes, "clc_ar_finish: null pointer");
  CLC_CHECK(mode == CLC_AR_ENCODE || mode == CLC_AR_DECODE, "clc_ar_finish: mode must be CLC_AR_ENCODE or CLC_AR_DECODE (got %d)", mode);
  CLC_CHECK(P > 0 && B > 0 && H > 0 && W > 0 && M > 0, "clc_ar_finish: P, B, H, W and M must be positive");
  CLC_CHECK(ldg >= 2 * M, "clc_ar_finish: ldg < 2 M (scales first, means second)");
  CLC_CHECK(n_scales > 1 && n_scales <= 256, "clc_ar_finish: n_scales out of range");
  CLC_CHECK((long)B * H * W < (1l << 31), "clc_ar_finish: B * H * W must be below 2^31");
  if (mode == CLC_AR_ENCODE) CLC_CHECK(y && y_hat && symbols && ldy >= M && ldh >= M, "clc_ar_finish: encode mode needs y, y_hat, symbols and ldy, ldh >= M");
  const long rows = (long)B * P;
  hipLaunchKernelGGL(ar_finish_kernel, dim3(grid_rows(rows * M)), dim3(256), 0, ST, gp, ldg, M, pix, P, H, W, scale_table, n_scales, y, ldy, y_hat,
                     ldh, symbols, indexes, mode, rows);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_ar_commit(const int32_t* symbols, const float* gp, int ldg, int M, const int32_t* pix, int P, int B, int H, int W, float* y_hat,
                             int ldh, clc_stream_t stream) {
  CLC_CHECK(symbols && gp && pix && y_hat, "clc_ar_commit: null pointer");
  CLC_CHECK(P > 0 && B > 0 && H > 0 && W > 0 && M > 0, "clc_ar_commit: P, B, H, W and M must be positive");
  CLC_CHECK(ldg >= 2 * M && ldh >= M, "clc_ar_commit: ldg < 2 M or ldh < M");
  CLC_CHECK((long)B * H * W < (1l << 31), "clc_ar_commit: B * H * W must be below 2^31");
  const long rows = (long)B * P;
  hipLaunchKernelGGL(ar_commit_kernel, dim3(grid_rows(rows * M)), dim3(256), 0, ST, symbols, gp, ldg, M, pix, P, H, W, y_hat, ldh, rows);
  CLC_LAUNCH_CHECK();
  return 0;
}
