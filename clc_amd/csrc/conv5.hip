// conv5.hip — 5x5 / pad-2 convolutions (stride 1 or 2) on gfx950: the conv(k=5, s=2) / deconv(k=5, s=2) layers of the hyperprior
// baselines (clc_amd/models/hyperprior.py).  f32 operands, f32 accumulation on v_mfma_f32_32x32x2_f32, wave64.
//
//   conv5_kernel         forward AND transposed (data gradient = ConvTranspose2d forward) as one implicit GEMM: M = output pixels,
//                        N = Cout, K = (tap, Cin).  A workgroup owns 128 pixels x 64 output channels; a K-step is one tap x 32 input
//                        channels; both operands go through [rows][32 + 4] LDS images, two stages (the global loads of step s + 1 are
//                        in registers while step s multiplies) — the structure of kmeans_assign_kernel.  The FILTER is the A operand and
//                        the PIXELS the B operand, so a lane owns one pixel and 4 consecutive channels per accumulator quad: 16-B stores.
//                        Filter layout [Cout][25][Cin]: the forward filter as it is, for transposed = 1 the image clc_filter_transpose
//                        makes.  transposed + stride 2: blockIdx.z = output parity class (y & 1, x & 1); a class visits only its live
//                        taps (kh = y mod 2, kw = x mod 2: 3x3, 3x2, 2x3, 2x2 of the 25), none of the structural zeros.
//                        Taps that fall outside the image are zero-filled, never skipped: the K order of an output element is
//                        (tap ascending, channel chunks ascending, k inside a chunk by lane half) for EVERY element — a function of
//                        (Cin, class) alone, not of the batch size, the image's place in the batch or the tile it lands in.
//   conv5_wgrad_kernel   dw[co][t][ci] = sum_m dy[m][co] x[pix(m, t)][ci]: a workgroup owns (tap, 64 co, 64 ci) and walks ALL N*OH*OW
//                        pixels in chunks of 32 in ascending order — a single pass, every dw element written once by one lane (no
//                        atomics, no slabs).  The pixel-major operands are transposed on their way into the [channel][32 + 4] images.
//                        dbias = clc_colsum of dy.
#include "common.h"

namespace {

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int kBM = 128;                        // pixels per workgroup
constexpr int kBN = 64;                         // output channels per workgroup
constexpr int kKC = 32;                         // channels per K-step
constexpr int kPitch = kKC + 4;                 // LDS row pitch: 16-lane b128 reads of 16 rows hit 64 different banks
constexpr int kStage = (kBM + kBN) * kPitch;    // floats per stage
constexpr int kFwdLds = 2 * kStage * 4;         // 55 296 B: two workgroups per CU
constexpr int kWT = 64;                         // filter-gradient tile: 64 co x 64 ci
constexpr int kWStage = 2 * kWT * kPitch;
constexpr int kWgradLds = 2 * kWStage * 4;      // 36 864 B

__device__ __forceinline__ int row_of(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }   // C/D layout of the 32x32 MFMAs

struct C5Params {
  const float* x; const float* w; const float* bias; float* y;
  int N, H, W, Cin, ldx, OH, OW, Cout, ldy;
  int stride, transposed, act, vec_store;
  int M;    // rows of the GEMM (per parity class)
};

__global__ __launch_bounds__(256) void conv5_kernel(const C5Params p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  const int wp = wave & 1, wc = wave >> 1;   // the wave's 64-pixel half / 32-channel half of the 128 x 64 tile
  const int m0 = blockIdx.x * kBM, co0 = blockIdx.y * kBN;
  const int lrow = tid >> 3, lcol = (tid & 7) << 2;   // loader role: rows lrow + 32 i, columns lcol .. lcol + 3 of the chunk
  const bool par = p.transposed && p.stride == 2;     // parity classes
  const int py = par ? (int)(blockIdx.z >> 1) : 0, px = par ? (int)(blockIdx.z & 1) : 0;
  const int GH = par ? p.OH >> 1 : p.OH, GW = par ? p.OW >> 1 : p.OW;   // the class's pixel grid
  const int kh0 = py, kw0 = px, kstep = par ? 2 : 1;
  const int nkh = par ? 3 - py : 5, nkw = par ? 3 - px : 5;
  const int nchunk = (p.Cin + kKC - 1) / kKC;
  const int total = nkh * nkw * nchunk;

  // the loader's four pixels: image base row and the coordinate a tap offsets
  int pbase[4], by[4], bx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + lrow + 32 * i;
    const int mm = m < p.M ? m : 0;
    const int n = mm / (GH * GW), r = mm - n * (GH * GW);
    const int gy = r / GW, gx = r - gy * GW;
    pbase[i] = m < p.M ? n * p.H : -1;
    if (!p.transposed) { by[i] = gy * p.stride - 2; bx[i] = gx * p.stride - 2; }
    else if (par) { by[i] = 2 * gy + py + 2; bx[i] = 2 * gx + px + 2; }
    else { by[i] = gy + 2; bx[i] = gx + 2; }
  }

  f32x4 vx[4], vw[2];
  auto load = [&](int kh, int kw, int kc) {
    const int k = kc * kKC + lcol;
    const int t = kh * 5 + kw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // forward: iy = oy s - 2 + kh.  transposed: iy = (y + 2 - kh) / s (a live tap of the class makes it divisible; -2 >> 1 = -1 is rejected below)
      int iy = p.transposed ? by[i] - kh : by[i] + kh, ix = p.transposed ? bx[i] - kw : bx[i] + kw;
      if (par) { iy >>= 1; ix >>= 1; }
      if (pbase[i] >= 0 && k < p.Cin && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
        vx[i] = *reinterpret_cast<const f32x4*>(p.x + ((size_t)(pbase[i] + iy) * p.W + ix) * p.ldx + k);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int co = co0 + lrow + 32 * i;
      vw[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (co < p.Cout && k < p.Cin) vw[i] = *reinterpret_cast<const f32x4*>(p.w + ((size_t)co * 25 + t) * p.Cin + k);
    }
  };
  auto store = [&](int buf) {
    float* P = sm + buf * kStage;
    float* Wm = P + kBM * kPitch;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(P + (lrow + 32 * i) * kPitch + lcol) = vx[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(Wm + (lrow + 32 * i) * kPitch + lcol) = vw[i];
  };

  f32x16 acc[2];   // [pixel tile of the wave]
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;

  int ikh = 0, ikw = 0, kc = 0;
  load(kh0, kw0, 0);
  store(0);
  __syncthreads();
  for (int s = 0; s < total; ++s) {
    const int cur = s & 1;
    int nkc = kc + 1, nikw = ikw, nikh = ikh;
    if (nkc == nchunk) { nkc = 0; if (++nikw == nkw) { nikw = 0; ++nikh; } }
    const bool more = s + 1 < total;   // block-uniform
    if (more) load(kh0 + kstep * nikh, kw0 + kstep * nikw, nkc);
    const float* P = sm + cur * kStage + (wp * 64 + li) * kPitch + 4 * h;
    const float* Wm = sm + cur * kStage + (kBM + wc * 32 + li) * kPitch + 4 * h;
#pragma unroll
    for (int ks = 0; ks < kKC / 8; ++ks) {
      // lane half h takes k = 8 ks + 4 h + {0..3}: any k order serves as long as both operands use the same one
      const f32x4 a = *reinterpret_cast<const f32x4*>(Wm + 8 * ks);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(P + 8 * ks), b1 = *reinterpret_cast<const f32x4*>(P + 32 * kPitch + 8 * ks);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = MFMA(a[e], b0[e], acc[0]);
        acc[1] = MFMA(a[e], b1[e], acc[1]);
      }
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    kc = nkc; ikw = nikw; ikh = nikh;
  }

  // epilogue: bias, activation, store (a lane: one pixel, channels 8 q + 4 h + {0..3} of the wave's 32)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int m = m0 + wp * 64 + b * 32 + li;
    if (m >= p.M) continue;
    const int n = m / (GH * GW), r = m - n * (GH * GW);
    const int gy = r / GW, gx = r - gy * GW;
    const int oy = par ? 2 * gy + py : gy, ox = par ? 2 * gx + px : gx;
    float* yp = p.y + ((size_t)(n * p.OH + oy) * p.OW + ox) * p.ldy;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = co0 + wc * 32 + 8 * q + 4 * h;
      if (co >= p.Cout) continue;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bj = (p.bias && co + j < p.Cout) ? p.bias[co + j] : 0.f;
        v[j] = apply_act(acc[b][4 * q + j] + bj, p.act);
      }
      if (p.vec_store) {
        *reinterpret_cast<f32x4*>(yp + co) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (co + j < p.Cout) yp[co + j] = v[j];
      }
    }
  }
}

struct W5Params {
  const float* x; const float* dy; float* dw;
  int N, H, W, Cin, ldx, OH, OW, Cout, lddy;
  int stride, accumulate, vec_dy, nci;
  int K;    // N * OH * OW
};

__global__ __launch_bounds__(256) void conv5_wgrad_kernel(const W5Params p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  const int wa = wave & 1, wb = wave >> 1;   // the wave's 32-co / 32-ci quarter of the 64 x 64 tile
  const int t = blockIdx.x / p.nci, ci0 = (blockIdx.x - t * p.nci) * kWT, co0 = blockIdx.y * kWT;
  const int kh = t / 5, kw = t - kh * 5;
  const int lp = tid >> 3, lc = (tid & 7) << 2;   // loader role: pixel lp of the chunk, channels lc + 32 j .. + 3
  const int nsteps = (p.K + kKC - 1) / kKC;
  const int img = p.OH * p.OW;

  f32x4 vd[2], vx[2];
  auto load = [&](int s) {
    const int m = s * kKC + lp;
    vd[0] = vd[1] = vx[0] = vx[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (m >= p.K) return;
    const int n = m / img, r = m - n * img;
    const int oy = r / p.OW, ox = r - oy * p.OW;
    const float* dp = p.dy + (size_t)m * p.lddy;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int co = co0 + lc + 32 * j;
      if (p.vec_dy) {
        if (co < p.Cout) vd[j] = *reinterpret_cast<const f32x4*>(dp + co);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (co + e < p.Cout) vd[j][e] = dp[co + e];
      }
    }
    const int iy = oy * p.stride - 2 + kh, ix = ox * p.stride - 2 + kw;
    if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
      const float* xp = p.x + ((size_t)(n * p.H + iy) * p.W + ix) * p.ldx;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ci = ci0 + lc + 32 * j;
        if (ci < p.Cin) vx[j] = *reinterpret_cast<const f32x4*>(xp + ci);
      }
    }
  };
  auto store = [&](int buf) {   // transposed deposit: [channel][pixel of the chunk]
    float* A = sm + buf * kWStage;
    float* B = A + kWT * kPitch;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        A[(lc + 32 * j + e) * kPitch + lp] = vd[j][e];
        B[(lc + 32 * j + e) * kPitch + lp] = vx[j][e];
      }
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  load(0);
  store(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < nsteps;   // block-uniform
    if (more) load(s + 1);
    const float* A = sm + cur * kWStage + (wa * 32 + li) * kPitch + 4 * h;
    const float* B = sm + cur * kWStage + (kWT + wb * 32 + li) * kPitch + 4 * h;
#pragma unroll
    for (int ks = 0; ks < kKC / 8; ++ks) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(A + 8 * ks), b = *reinterpret_cast<const f32x4*>(B + 8 * ks);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = MFMA(a[e], b[e], acc);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
  }

  const int ci = ci0 + wb * 32 + li;
  if (ci >= p.Cin) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int co = co0 + wa * 32 + row_of(i, h);
    if (co >= p.Cout) continue;
    float* o = p.dw + ((size_t)co * 25 + t) * p.Cin + ci;
    *o = p.accumulate ? *o + acc[i] : acc[i];
  }
}

}  // namespace

// clc_conv2d with ks == 5 (conv_igemm.hip dispatches here before any of its own rules)
int clc_conv5_launch(const clc_conv_desc* d, hipStream_t st) {
  CLC_CHECK(d && d->x && d->w && d->y, "clc_conv2d(ks=5): null pointer");
  CLC_CHECK(d->stride == 1 || d->stride == 2, "clc_conv2d(ks=5): stride must be 1 or 2 (got %d)", d->stride);
  CLC_CHECK(d->pad == 2, "clc_conv2d(ks=5): pad must be 2 (got %d)", d->pad);
  CLC_CHECK(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->OH > 0 && d->OW > 0, "clc_conv2d(ks=5): bad dims");
  if (!d->transposed) {
    CLC_CHECK(d->OH == (d->H + 4 - 5) / d->stride + 1 && d->OW == (d->W + 4 - 5) / d->stride + 1,
              "clc_conv2d(ks=5): output dims %dx%d inconsistent with input %dx%d s=%d", d->OH, d->OW, d->H, d->W, d->stride);
  } else {
    CLC_CHECK(d->H == (d->OH + 4 - 5) / d->stride + 1 && d->W == (d->OW + 4 - 5) / d->stride + 1,
              "clc_conv2d(ks=5,transposed): dY dims %dx%d inconsistent with dX %dx%d", d->H, d->W, d->OH, d->OW);
    CLC_CHECK(d->stride == 1 || (d->OH % 2 == 0 && d->OW % 2 == 0), "clc_conv2d(ks=5,transposed,s2): odd dX dims");
  }
  // the 5x5 kernel has bias + activation epilogues only: every other descriptor field is refused by name
  CLC_CHECK(!d->shuffle, "clc_conv2d(ks=5): shuffle is not supported");
  CLC_CHECK(d->norm == CLC_NORM_NONE && !d->mul, "clc_conv2d(ks=5): norm / mul is not supported");
  CLC_CHECK(!d->res, "clc_conv2d(ks=5): res is not supported");
  CLC_CHECK(!d->w2 && !d->w3 && !d->w4, "clc_conv2d(ks=5): w2 / w3 / w4 (filter sets) are not supported");
  CLC_CHECK(!d->xs, "clc_conv2d(ks=5): xs (fused activation backward) is not supported");
  CLC_CHECK(!d->res_gate && !d->out_gate, "clc_conv2d(ks=5): res_gate / out_gate are not supported");
  CLC_CHECK(!d->y_pre, "clc_conv2d(ks=5): y_pre is not supported");
  CLC_CHECK(!d->w_packed && !d->w_wino, "clc_conv2d(ks=5): w_packed / w_wino are not supported");
  CLC_CHECK(d->in_op == CLC_IN_NONE, "clc_conv2d(ks=5): in_op is not supported");
  CLC_CHECK(d->act == CLC_ACT_NONE || d->act == CLC_ACT_LRELU || d->act == CLC_ACT_RELU, "clc_conv2d(ks=5): act must be none, LeakyReLU or ReLU (got %d)", d->act);
  CLC_CHECK(d->Cin % 4 == 0 && d->ldx % 4 == 0 && d->ldx >= d->Cin && aligned16(d->x) && aligned16(d->w),
            "clc_conv2d(ks=5): needs the aligned path (Cin %% 4 == 0, ldx %% 4 == 0, 16-byte aligned x / w; got Cin=%d ldx=%d)", d->Cin, d->ldx);
  CLC_CHECK(d->ldy >= d->Cout, "clc_conv2d(ks=5): ldy < Cout");
  const size_t x_bytes = ((size_t)d->N * d->H * d->W - 1) * d->ldx * 4 + (size_t)d->Cin * 4;
  const size_t y_bytes = ((size_t)d->N * d->OH * d->OW - 1) * d->ldy * 4 + (size_t)d->Cout * 4;
  CLC_CHECK(x_bytes < (1ull << 31) && y_bytes < (1ull << 31) && (size_t)d->Cout * 25 * d->Cin * 4 < (1ull << 31), "clc_conv2d(ks=5): tensor larger than 2 GiB");

  C5Params p;
  p.x = d->x; p.w = d->w; p.bias = d->bias; p.y = d->y;
  p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.ldx = d->ldx;
  p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout; p.ldy = d->ldy;
  p.stride = d->stride; p.transposed = d->transposed ? 1 : 0; p.act = d->act;
  p.vec_store = d->Cout % 4 == 0 && d->ldy % 4 == 0 && aligned16(d->y);
  const int classes = (d->transposed && d->stride == 2) ? 4 : 1;
  p.M = classes == 4 ? d->N * (d->OH / 2) * (d->OW / 2) : d->N * d->OH * d->OW;
  static PerDeviceOnce attr_once;
  if (attr_once.first())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv5_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kFwdLds);
  dim3 grid((p.M + kBM - 1) / kBM, (p.Cout + kBN - 1) / kBN, classes);
  hipLaunchKernelGGL(conv5_kernel, grid, dim3(256), kFwdLds, st, p);
  CLC_LAUNCH_CHECK();
  return kBM * 1000 + kBN;
}

size_t clc_conv5_wgrad_workspace_bytes(const clc_wgrad_desc* d) {
  return d->dbias ? clc_colsum_workspace_bytes((long)d->N * d->OH * d->OW, d->Cout) : 0;
}

// clc_conv2d_wgrad with ks == 5: launched in line, never part of a grouped launch
int clc_conv5_wgrad_launch(const clc_wgrad_desc* d, hipStream_t st) {
  CLC_CHECK(d && d->x && d->dy && d->dw, "clc_conv2d_wgrad(ks=5): null pointer");
  CLC_CHECK(d->stride == 1 || d->stride == 2, "clc_conv2d_wgrad(ks=5): stride must be 1 or 2");
  CLC_CHECK(d->pad == 2, "clc_conv2d_wgrad(ks=5): pad must be 2");
  CLC_CHECK(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "clc_conv2d_wgrad(ks=5): bad dims");
  CLC_CHECK(d->OH == (d->H + 4 - 5) / d->stride + 1 && d->OW == (d->W + 4 - 5) / d->stride + 1 && d->OH > 0 && d->OW > 0,
            "clc_conv2d_wgrad(ks=5): output dims inconsistent");
  CLC_CHECK(d->ldx >= d->Cin && d->lddy >= d->Cout, "clc_conv2d_wgrad(ks=5): ld too small");
  CLC_CHECK(!d->dys, "clc_conv2d_wgrad(ks=5): dys (fused activation backward) is not supported");
  CLC_CHECK(d->in_op == CLC_IN_NONE, "clc_conv2d_wgrad(ks=5): in_op is not supported");
  CLC_CHECK(d->Cin % 4 == 0 && d->ldx % 4 == 0 && aligned16(d->x), "clc_conv2d_wgrad(ks=5): needs the aligned path (Cin %% 4 == 0, ldx %% 4 == 0; got Cin=%d ldx=%d)", d->Cin, d->ldx);
  const long K = (long)d->N * d->OH * d->OW;
  const size_t xb = ((size_t)d->N * d->H * d->W - 1) * d->ldx * 4 + (size_t)d->Cin * 4;
  const size_t db = ((size_t)K - 1) * d->lddy * 4 + (size_t)d->Cout * 4;
  CLC_CHECK(xb < (1ull << 31) && db < (1ull << 31) && K < (1l << 31) - 64, "clc_conv2d_wgrad(ks=5): tensor larger than 2 GiB");
  CLC_CHECK(!d->dbias || (d->workspace && d->workspace_bytes >= clc_conv5_wgrad_workspace_bytes(d)), "clc_conv2d_wgrad(ks=5): workspace too small");
  W5Params p;
  p.x = d->x; p.dy = d->dy; p.dw = d->dw;
  p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.ldx = d->ldx;
  p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout; p.lddy = d->lddy;
  p.stride = d->stride; p.accumulate = d->accumulate ? 1 : 0;
  p.vec_dy = d->Cout % 4 == 0 && d->lddy % 4 == 0 && aligned16(d->dy);
  p.nci = (d->Cin + kWT - 1) / kWT;
  p.K = (int)K;
  hipLaunchKernelGGL(conv5_wgrad_kernel, dim3(25 * p.nci, (d->Cout + kWT - 1) / kWT), dim3(256), kWgradLds, st, p);
  CLC_LAUNCH_CHECK();
  if (d->dbias) {
    if (clc_colsum(d->dy, d->lddy, K, d->Cout, d->dbias, p.accumulate, d->workspace, d->workspace_bytes, (clc_stream_t)st) < 0) return -1;
  }
  return 5;
}
