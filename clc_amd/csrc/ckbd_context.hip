// ckbd_context.hip — the checkerboard context layer (He et al., CVPR 2021) on gfx950: a 5x5 / pad-2 / stride-1 convolution whose 12 live
// taps are the (kh + kw)-odd ones, evaluated at the NON-ANCHOR pixels ((h + w) even) only and exactly 0 at the anchors ((h + w) odd).
// A live tap of a non-anchor lands on an anchor or outside the map, so the layer reads anchors only.  f32 operands, f32 accumulation on
// v_mfma_f32_32x32x2_f32, wave64.  The structure is conv5.hip's (128 rows x 64 output channels per workgroup, one tap x 32 input channels
// per K-step, [rows][32 + 4] LDS images, two stages, one barrier per step); what differs is the row space, the tap walk and the partner store.
//
//   ckbd_conv_kernel    forward AND transposed (data gradient) as one implicit GEMM: N = Cout, K = (12 taps, Cin).  The rows are the SLOTS
//                       (b, h, j) of an H x ceil(W / 2) grid per image; a slot's pixel is w = 2 j + ((h + phase) & 1): phase 0 = non-anchors
//                       (forward), phase 1 = anchors (transposed).  A slot with w >= W is padding: zero-filled on load, never stored.  Filter
//                       [Cout][12][Cin], taps in (kh, kw) ascending order: (0,1) (0,3) (1,0) (1,2) (1,4) (2,1) (2,3) (3,0) (3,2) (3,4) (4,1)
//                       (4,3).  transposed = 1: dx at an anchor p = sum_t dy[p - offset_t] w^T with the [Cin][12][Cout] image
//                       clc_filter_transpose makes; p - offset_t is a non-anchor, so an anchor's dy is never read.  (The tap set is symmetric
//                       under (kh, kw) -> (4 - kh, 4 - kw): reading at minus the offset of tap t is reading at the offset of tap 11 - t.)
//                       For each of its slots and its channel tile a workgroup also writes zeros to the slot's PARTNER pixel of the other
//                       parity (w' = 2 j + ((h + phase + 1) & 1), if inside the map): one launch defines the whole output map, no memset.
//                       Taps outside the map are zero-filled, never skipped: the K order of an output element is (tap ascending, 32-channel
//                       chunks ascending, inside a chunk by MFMA and lane half) for EVERY element — a function of Cin alone, not of the
//                       batch size, the image's place in the batch, the map size or the tile it lands in.  The two-pass coder rests on this.
//   ckbd_wgrad_kernel   dw[co][t][ci] = sum_slots dy[slot][co] x[slot + offset_t][ci] over the non-anchor slots of all images: a workgroup
//                       owns (tap, 64 co, 64 ci) and walks the slots in ascending chunks of 32 — a single pass, every dw element written
//                       once by one lane (no atomics, no slabs, no reduce launch).  An anchor's dy is never read.
#include "common.h"

namespace {

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int kBM = 128;                        // slots per workgroup
constexpr int kBN = 64;                         // output channels per workgroup
constexpr int kKC = 32;                         // channels per K-step
constexpr int kPitch = kKC + 4;                 // LDS row pitch: 16-lane b128 reads of 16 rows hit 64 different banks
constexpr int kStage = (kBM + kBN) * kPitch;    // floats per stage
constexpr int kFwdLds = 2 * kStage * 4;         // 55 296 B: two workgroups per CU
constexpr int kWT = 64;                         // filter-gradient tile: 64 co x 64 ci
constexpr int kWStage = 2 * kWT * kPitch;
constexpr int kWgradLds = 2 * kWStage * 4;      // 36 864 B
constexpr int kTaps = 12;

__device__ __forceinline__ int row_of(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }   // C/D layout of the 32x32 MFMAs

// the live taps in (kh, kw) ascending order: rows 0, 2, 4 hold kw = 1, 3, rows 1, 3 hold kw = 0, 2, 4
__device__ __forceinline__ void next_tap(int& kh, int& kw) {
  kw += 2;
  if (kw > 4) { ++kh; kw = (kh & 1) ? 0 : 1; }
}
__device__ __forceinline__ void tap_of(int t, int& kh, int& kw) {
  // t: 0 1 | 2 3 4 | 5 6 | 7 8 9 | 10 11
  const int pair = t / 5, r = t - pair * 5;   // a row pair holds 2 + 3 taps
  kh = 2 * pair + (r >= 2);
  kw = r < 2 ? 2 * r + 1 : 2 * (r - 2);
}

struct CkParams {
  const float* x; const float* w; const float* bias; float* y;
  int B, H, W, Wh, Cin, ldx, Cout, ldy;
  int transposed, phase, act, vec_store;
  int M;    // slots: B * H * Wh
};

__global__ __launch_bounds__(256) void ckbd_conv_kernel(const CkParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  const int wp = wave & 1, wc = wave >> 1;   // the wave's 64-slot half / 32-channel half of the 128 x 64 tile
  const int m0 = blockIdx.x * kBM, co0 = blockIdx.y * kBN;
  const int lrow = tid >> 3, lcol = (tid & 7) << 2;   // loader role: rows lrow + 32 i, columns lcol .. lcol + 3 of the chunk
  const int nchunk = (p.Cin + kKC - 1) / kKC;
  const int total = kTaps * nchunk;
  const int img = p.H * p.Wh;

  // the loader's four slots: image base row and the pixel a tap offsets (pbase < 0: padding slot or past the end)
  int pbase[4], by[4], bx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + lrow + 32 * i;
    const int mm = m < p.M ? m : 0;
    const int n = mm / img, r = mm - n * img;
    const int gy = r / p.Wh, gj = r - gy * p.Wh;
    const int gx = 2 * gj + ((gy + p.phase) & 1);
    pbase[i] = (m < p.M && gx < p.W) ? n * p.H : -1;
    by[i] = gy; bx[i] = gx;
  }

  f32x4 vx[4], vw[2];
  auto load = [&](int t, int kh, int kw, int kc) {
    const int k = kc * kKC + lcol;
    const int dy = p.transposed ? 2 - kh : kh - 2, dx = p.transposed ? 2 - kw : kw - 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const int iy = by[i] + dy, ix = bx[i] + dx;
      if (pbase[i] >= 0 && k < p.Cin && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
        vx[i] = *reinterpret_cast<const f32x4*>(p.x + ((size_t)(pbase[i] + iy) * p.W + ix) * p.ldx + k);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int co = co0 + lrow + 32 * i;
      vw[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (co < p.Cout && k < p.Cin) vw[i] = *reinterpret_cast<const f32x4*>(p.w + ((size_t)co * kTaps + t) * p.Cin + k);
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

  f32x16 acc[2];   // [slot tile of the wave]
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;

  int t = 0, kh = 0, kw = 1, kc = 0;
  load(0, 0, 1, 0);
  store(0);
  __syncthreads();
  for (int s = 0; s < total; ++s) {
    const int cur = s & 1;
    int nkc = kc + 1, nt = t, nkh = kh, nkw = kw;
    if (nkc == nchunk) { nkc = 0; ++nt; next_tap(nkh, nkw); }
    const bool more = s + 1 < total;   // block-uniform
    if (more) load(nt, nkh, nkw, nkc);
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
    kc = nkc; t = nt; kh = nkh; kw = nkw;
  }

  // epilogue: bias, activation, store (a lane: one slot, channels 8 q + 4 h + {0..3} of the wave's 32) — and zeros to the slot's partner
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int m = m0 + wp * 64 + b * 32 + li;
    if (m >= p.M) continue;
    const int n = m / img, r = m - n * img;
    const int gy = r / p.Wh, gj = r - gy * p.Wh;
    const int par = (gy + p.phase) & 1;
    const int ox = 2 * gj + par, zx = 2 * gj + (par ^ 1);
    float* row = p.y + (size_t)(n * p.H + gy) * p.W * p.ldy;
    float* yp = row + (size_t)ox * p.ldy;
    float* zp = row + (size_t)zx * p.ldy;
    const bool live = ox < p.W, partner = zx < p.W;
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
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      if (p.vec_store) {
        if (live) *reinterpret_cast<f32x4*>(yp + co) = v;
        if (partner) *reinterpret_cast<f32x4*>(zp + co) = z;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (co + j < p.Cout) {
            if (live) yp[co + j] = v[j];
            if (partner) zp[co + j] = 0.f;
          }
      }
    }
  }
}

struct CkWParams {
  const float* x; const float* dy; float* dw;
  int B, H, W, Wh, Cin, ldx, Cout, lddy;
  int accumulate, vec_dy, nci;
  int K;    // slots: B * H * Wh
};

__global__ __launch_bounds__(256) void ckbd_wgrad_kernel(const CkWParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  const int wa = wave & 1, wb = wave >> 1;   // the wave's 32-co / 32-ci quarter of the 64 x 64 tile
  const int t = blockIdx.x / p.nci, ci0 = (blockIdx.x - t * p.nci) * kWT, co0 = blockIdx.y * kWT;
  int kh, kw;
  tap_of(t, kh, kw);
  const int lp = tid >> 3, lc = (tid & 7) << 2;   // loader role: slot lp of the chunk, channels lc + 32 j .. + 3
  const int nsteps = (p.K + kKC - 1) / kKC;
  const int img = p.H * p.Wh;

  f32x4 vd[2], vx[2];
  auto load = [&](int s) {
    const int m = s * kKC + lp;
    vd[0] = vd[1] = vx[0] = vx[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (m >= p.K) return;
    const int n = m / img, r = m - n * img;
    const int oy = r / p.Wh, oj = r - oy * p.Wh;
    const int ox = 2 * oj + (oy & 1);   // the non-anchor of the slot
    if (ox >= p.W) return;              // padding slot
    const float* dp = p.dy + ((size_t)(n * p.H + oy) * p.W + ox) * p.lddy;
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
    const int iy = oy - 2 + kh, ix = ox - 2 + kw;
    if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
      const float* xp = p.x + ((size_t)(n * p.H + iy) * p.W + ix) * p.ldx;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ci = ci0 + lc + 32 * j;
        if (ci < p.Cin) vx[j] = *reinterpret_cast<const f32x4*>(xp + ci);
      }
    }
  };
  auto store = [&](int buf) {   // transposed deposit: [channel][slot of the chunk]
    float* A = sm + buf * kWStage;
    float* Bm = A + kWT * kPitch;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        A[(lc + 32 * j + e) * kPitch + lp] = vd[j][e];
        Bm[(lc + 32 * j + e) * kPitch + lp] = vx[j][e];
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
    const float* Bm = sm + cur * kWStage + (kWT + wb * 32 + li) * kPitch + 4 * h;
#pragma unroll
    for (int ks = 0; ks < kKC / 8; ++ks) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(A + 8 * ks), b = *reinterpret_cast<const f32x4*>(Bm + 8 * ks);
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
    float* o = p.dw + ((size_t)co * kTaps + t) * p.Cin + ci;
    *o = p.accumulate ? *o + acc[i] : acc[i];
  }
}

}  // namespace

extern "C" int clc_ckbd_conv(const clc_ckbd_desc* d, clc_stream_t stream) {
  CLC_CHECK(d && d->x && d->w && d->y, "clc_ckbd_conv: null pointer");
  CLC_CHECK(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "clc_ckbd_conv: bad dims (B=%d H=%d W=%d Cin=%d Cout=%d)", d->B, d->H, d->W, d->Cin, d->Cout);
  CLC_CHECK(d->transposed == 0 || d->transposed == 1, "clc_ckbd_conv: transposed must be 0 or 1 (got %d)", d->transposed);
  CLC_CHECK(d->act == CLC_ACT_NONE || d->act == CLC_ACT_LRELU, "clc_ckbd_conv: act must be none or LeakyReLU (got %d)", d->act);
  CLC_CHECK(d->Cin % 4 == 0 && d->ldx % 4 == 0 && d->ldx >= d->Cin,
            "clc_ckbd_conv: needs the aligned path (Cin %% 4 == 0, ldx %% 4 == 0, ldx >= Cin; got Cin=%d ldx=%d)", d->Cin, d->ldx);
  CLC_CHECK(aligned16(d->x) && aligned16(d->w), "clc_ckbd_conv: x and w must be 16-byte aligned");
  CLC_CHECK(d->ldy >= d->Cout, "clc_ckbd_conv: ldy < Cout (ldy=%d Cout=%d)", d->ldy, d->Cout);
  const int Wh = (d->W + 1) / 2;
  const long pixels = (long)d->B * d->H * d->W, slots = (long)d->B * d->H * Wh;
  CLC_CHECK(pixels < (1l << 31) && slots < (1l << 31) - kBM, "clc_ckbd_conv: B * H * W must stay below 2^31 (got %ld)", pixels);
  CLC_CHECK((long)d->Cout * kTaps * d->Cin < (1l << 31), "clc_ckbd_conv: filter larger than 2^31 elements");

  CkParams p;
  p.x = d->x; p.w = d->w; p.bias = d->bias; p.y = d->y;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Wh = Wh; p.Cin = d->Cin; p.ldx = d->ldx; p.Cout = d->Cout; p.ldy = d->ldy;
  p.transposed = d->transposed; p.phase = d->transposed; p.act = d->act;
  p.vec_store = d->Cout % 4 == 0 && d->ldy % 4 == 0 && aligned16(d->y);
  p.M = (int)slots;
  static PerDeviceOnce attr_once;
  if (attr_once.first())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ckbd_conv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kFwdLds);
  dim3 grid((p.M + kBM - 1) / kBM, (p.Cout + kBN - 1) / kBN);
  hipLaunchKernelGGL(ckbd_conv_kernel, grid, dim3(256), kFwdLds, (hipStream_t)stream, p);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_ckbd_wgrad(const clc_ckbd_wgrad_desc* d, clc_stream_t stream) {
  CLC_CHECK(d && d->x && d->dy && d->dw, "clc_ckbd_wgrad: null pointer");
  CLC_CHECK(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "clc_ckbd_wgrad: bad dims (B=%d H=%d W=%d Cin=%d Cout=%d)", d->B, d->H, d->W, d->Cin, d->Cout);
  CLC_CHECK(d->Cin % 4 == 0 && d->ldx % 4 == 0 && d->ldx >= d->Cin,
            "clc_ckbd_wgrad: needs the aligned path (Cin %% 4 == 0, ldx %% 4 == 0, ldx >= Cin; got Cin=%d ldx=%d)", d->Cin, d->ldx);
  CLC_CHECK(aligned16(d->x), "clc_ckbd_wgrad: x must be 16-byte aligned");
  CLC_CHECK(d->lddy >= d->Cout, "clc_ckbd_wgrad: lddy < Cout (lddy=%d Cout=%d)", d->lddy, d->Cout);
  const int Wh = (d->W + 1) / 2;
  const long pixels = (long)d->B * d->H * d->W, slots = (long)d->B * d->H * Wh;
  CLC_CHECK(pixels < (1l << 31) && slots < (1l << 31) - 64, "clc_ckbd_wgrad: B * H * W must stay below 2^31 (got %ld)", pixels);
  CLC_CHECK((long)d->Cout * kTaps * d->Cin < (1l << 31), "clc_ckbd_wgrad: filter larger than 2^31 elements");

  CkWParams p;
  p.x = d->x; p.dy = d->dy; p.dw = d->dw;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Wh = Wh; p.Cin = d->Cin; p.ldx = d->ldx; p.Cout = d->Cout; p.lddy = d->lddy;
  p.accumulate = d->accumulate ? 1 : 0;
  p.vec_dy = d->Cout % 4 == 0 && d->lddy % 4 == 0 && aligned16(d->dy);
  p.nci = (d->Cin + kWT - 1) / kWT;
  p.K = (int)slots;
  hipLaunchKernelGGL(ckbd_wgrad_kernel, dim3(kTaps * p.nci, (d->Cout + kWT - 1) / kWT), dim3(256), kWgradLds, (hipStream_t)stream, p);
  CLC_LAUNCH_CHECK();
  return 0;
}
