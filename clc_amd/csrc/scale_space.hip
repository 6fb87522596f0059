// scale_space.hip — the two operators of the scale-space-flow video model (ssf2020; Agustsson et al., CVPR 2020), forward and
// backward (gfx950): the scale-space VOLUME of a frame (a Gaussian pyramid brought back to full resolution) and the trilinear
// WARP through it (F.grid_sample of the 5-D volume, padding_mode="border", align_corners=False).  Definition: DESIGN 29.
//
// LAYOUT.  Frames, flows and gradients are pixel-major (NHWC) with a leading dimension, like everything else.  The volume is
// [N][H][W][D][4] f32: depth and channel innermost, the three channels padded to one 16-byte voxel (lane 3 is written 0 and never
// read), so the two depth neighbours of a pixel are 32 contiguous bytes and the D = L + 1 slices of a pixel one 96-byte run at the
// default L = 5: a trilinear sample is four 32-byte reads.  Every kernel gives one thread one pixel (or voxel) with all three
// channels; the intermediate maps of the pyramid are [pixels][4] in the caller's workspace.
//
// VOLUME.  V0 = x, V1 = blur(x), then per level: 2x2 average pool, blur, and i bilinear x2 upsamplings (F.interpolate,
// align_corners=False) for slice i + 1.  blur = separable Gaussian (taps by value in the descriptor) with replicate padding,
// each axis one fmaf chain over the taps in ascending order.  The backward pass is the adjoint chain in GATHER form: every output
// element has one owner thread and a fixed summation order (the adjoint of the replicate-padded blur folds the taps that the
// clamp sent to an edge pixel into that pixel's weight; the adjoint of the upsampling reads its 4 x 4 fine pixels).
//
// WARP.  ix = w + flow_x W / 2 (= ((gx + 1) W - 1) / 2 with gx = (2 w + 1) / W - 1 + flow_x, one rounding instead of four),
// likewise iy; iz = ((gz + 1) D - 1) / 2; each clamped to [0, size - 1]; the coordinate gradient is 0 where the clamp is active
// (torch's rule: unclamped index <= 0 or >= size - 1).  dflow and dscale are gathers.  dvolume is a SCATTER made deterministic
// without float atomics:
//   1. per pixel, the key = linear index of its clamped lower corner voxel, the value = the pixel id, and its three fractions;
//   2. ONE stable radix sort of (key, pixel id) pairs over the batch (rocPRIM, caller's temporary storage): pixels are generated in
//      index order, so each corner's bucket is ordered by pixel id — alone or inside a batch;
//   3. bucket bounds from the sorted keys (each bound has one writer);
//   4. one thread per voxel walks the (up to) 8 corner buckets that can touch it in a fixed order and sums weight x dy.
// Cost: the sort is O(P) (P = N H W pixels, ceil(log2(N H W D)) key bits), the bounds O(P), the gather O(8 P) bucket entries in
// total; the longest serial chain is 8 x the largest bucket (border clamping can send every pixel of an image to one voxel: H W
// entries on one thread — linear, never quadratic).
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace {

constexpr int TPB = 256;

struct F3 { float x, y, z; };
struct Taps { int n; float v[CLC_SS_MAX_TAPS]; };

// S4 / D4: the buffer is [pixels][4] (volume slices and workspace maps: one aligned 16-byte access); else 3 floats at a leading dimension
template <bool V4> __device__ __forceinline__ F3 ldp(const float* p) {
  if constexpr (V4) { const f32x4 v = *reinterpret_cast<const f32x4*>(p); return {v[0], v[1], v[2]}; }
  else return {p[0], p[1], p[2]};
}
template <bool V4> __device__ __forceinline__ void stp(float* p, F3 v) {
  if constexpr (V4) *reinterpret_cast<f32x4*>(p) = (f32x4){v.x, v.y, v.z, 0.f};
  else { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
}
__device__ __forceinline__ F3 fma3(float w, F3 a, F3 acc) { return {fmaf(w, a.x, acc.x), fmaf(w, a.y, acc.y), fmaf(w, a.z, acc.z)}; }

// a map: element (n, h, w) at p + ((n * H + h) * W + w) * ld
struct Map { float* p; long ld; };
struct CMap { const float* p; long ld; };

// ---- copy (V0 = x) ----
template <bool S4, bool D4> __global__ void __launch_bounds__(TPB) ss_copy_kernel(CMap s, Map d, long npix) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x;
  if (i >= npix) return;
  stp<D4>(d.p + i * d.ld, ldp<S4>(s.p + i * s.ld));
}

// ---- blur along one axis, replicate padding: out[i] = sum_k g[k] in[clamp(i + k - r)], k ascending ----
template <bool S4, bool D4, bool VERT> __global__ void __launch_bounds__(TPB) ss_blur_kernel(CMap s, Map d, int N, int H, int W, Taps t) {
  __shared__ float g[CLC_SS_MAX_TAPS];
  if ((int)threadIdx.x < t.n) g[threadIdx.x] = t.v[threadIdx.x];
  __syncthreads();
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)N * H * W;
  if (i >= npix) return;
  const int w = (int)(i % W), h = (int)((i / W) % H);
  const int r = t.n >> 1, len = VERT ? H : W, pos = VERT ? h : w;
  const long step = VERT ? (long)W : 1, base = i - (long)pos * step;
  F3 acc = {0.f, 0.f, 0.f};
  for (int k = 0; k < t.n; ++k) {
    const int q = min(max(pos + k - r, 0), len - 1);
    acc = fma3(g[k], ldp<S4>(s.p + (base + (long)q * step) * s.ld), acc);
  }
  stp<D4>(d.p + i * d.ld, acc);
}

// ---- adjoint of the blur along one axis: dx[s] = sum_o w(o, s) dy[o], o ascending; w = the taps k with clamp(o + k - r) == s
// (one tap inside the map; at an edge pixel every tap the clamp sent there); + add[s] first when add is given ----
template <bool S4, bool D4, bool A4, bool VERT>
__global__ void __launch_bounds__(TPB) ss_blur_adj_kernel(CMap s, Map d, CMap add, int N, int H, int W, Taps t) {
  __shared__ float g[CLC_SS_MAX_TAPS];
  if ((int)threadIdx.x < t.n) g[threadIdx.x] = t.v[threadIdx.x];
  __syncthreads();
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)N * H * W;
  if (i >= npix) return;
  const int w = (int)(i % W), h = (int)((i / W) % H);
  const int r = t.n >> 1, len = VERT ? H : W, pos = VERT ? h : w;
  const long step = VERT ? (long)W : 1, base = i - (long)pos * step;
  F3 acc = {0.f, 0.f, 0.f};
  if (add.p != nullptr) acc = ldp<A4>(add.p + i * add.ld);
  const int o_lo = max(pos - r, 0), o_hi = min(pos + r, len - 1);
  for (int o = o_lo; o <= o_hi; ++o) {
    const int kc = pos - o + r;   // the tap that lands on pos without the clamp
    const int k_lo = pos == 0 ? 0 : kc, k_hi = pos == len - 1 ? t.n - 1 : kc;
    float wgt = 0.f;
    for (int k = k_lo; k <= k_hi; ++k) wgt += g[k];
    acc = fma3(wgt, ldp<S4>(s.p + (base + (long)o * step) * s.ld), acc);
  }
  stp<D4>(d.p + i * d.ld, acc);
}

// ---- 2x2 average pool (H, W even): [N, H, W] -> [N, H/2, W/2]; threads over the output ----
template <bool S4, bool D4> __global__ void __launch_bounds__(TPB) ss_pool_kernel(CMap s, Map d, int N, int OH, int OW) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)N * OH * OW;
  if (i >= npix) return;
  const int w = (int)(i % OW), h = (int)((i / OW) % OH);
  const long n = i / ((long)OW * OH), W = 2L * OW;
  const long p00 = (n * 2 * OH + 2 * h) * W + 2 * w;
  const F3 a = ldp<S4>(s.p + p00 * s.ld), b = ldp<S4>(s.p + (p00 + 1) * s.ld), c = ldp<S4>(s.p + (p00 + W) * s.ld), e = ldp<S4>(s.p + (p00 + W + 1) * s.ld);
  stp<D4>(d.p + i * d.ld, {((a.x + b.x) + (c.x + e.x)) * 0.25f, ((a.y + b.y) + (c.y + e.y)) * 0.25f, ((a.z + b.z) + (c.z + e.z)) * 0.25f});
}

// ---- adjoint of the pool, plus the other gradient of the same map: out[n, h, w] = add[n, h, w] + 0.25 s[n, h/2, w/2]; threads over the fine map ----
template <bool S4, bool D4, bool A4> __global__ void __launch_bounds__(TPB) ss_pool_adj_kernel(CMap s, Map d, CMap add, int N, int H, int W) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)N * H * W;
  if (i >= npix) return;
  const int w = (int)(i % W), h = (int)((i / W) % H);
  const long n = i / ((long)W * H);
  const F3 a = ldp<A4>(add.p + i * add.ld), c = ldp<S4>(s.p + ((n * (H / 2) + h / 2) * (W / 2) + w / 2) * s.ld);
  stp<D4>(d.p + i * d.ld, fma3(0.25f, c, a));
}

// ---- bilinear x2, align_corners=False (F.interpolate): [N, H, W] -> [N, 2H, 2W]; threads over the output ----
__device__ __forceinline__ void up_src(int o, int len, int& i0, int& i1, float& l0, float& l1) {
  const float sc = fmaxf(((float)o + 0.5f) * 0.5f - 0.5f, 0.f);
  i0 = (int)sc;
  i1 = min(i0 + 1, len - 1);
  l1 = sc - (float)i0;
  l0 = 1.f - l1;
}
template <bool S4, bool D4> __global__ void __launch_bounds__(TPB) ss_up_kernel(CMap s, Map d, int N, int H, int W) {
  const int OH = 2 * H, OW = 2 * W;
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)N * OH * OW;
  if (i >= npix) return;
  const int ow = (int)(i % OW), oh = (int)((i / OW) % OH);
  const long n = i / ((long)OW * OH);
  int h0, h1, w0, w1;
  float lh0, lh1, lw0, lw1;
  up_src(oh, H, h0, h1, lh0, lh1);
  up_src(ow, W, w0, w1, lw0, lw1);
  const long r0 = (n * H + h0) * W, r1 = (n * H + h1) * W;
  const F3 a = ldp<S4>(s.p + (r0 + w0) * s.ld), b = ldp<S4>(s.p + (r0 + w1) * s.ld), c = ldp<S4>(s.p + (r1 + w0) * s.ld), e = ldp<S4>(s.p + (r1 + w1) * s.ld);
  stp<D4>(d.p + i * d.ld, {lh0 * (lw0 * a.x + lw1 * b.x) + lh1 * (lw0 * c.x + lw1 * e.x), lh0 * (lw0 * a.y + lw1 * b.y) + lh1 * (lw0 * c.y + lw1 * e.y),
                           lh0 * (lw0 * a.z + lw1 * b.z) + lh1 * (lw0 * c.z + lw1 * e.z)});
}

// ---- adjoint of the upsampling: [N, 2H, 2W] -> [N, H, W]; coarse pixel h reads fine rows 2h - 1 .. 2h + 2 with weights
// 1/4 (h > 0), 3/4 (1 at h == 0), 3/4 (1 at h == H - 1), 1/4 (h < H - 1); columns likewise; rows outer, columns inner, ascending ----
__device__ __forceinline__ void up_adj_w(int p, int len, float (&wq)[4]) {
  wq[0] = p > 0 ? 0.25f : 0.f;
  wq[1] = p == 0 ? 1.f : 0.75f;
  wq[2] = p == len - 1 ? 1.f : 0.75f;
  wq[3] = p < len - 1 ? 0.25f : 0.f;
}
template <bool S4, bool D4> __global__ void __launch_bounds__(TPB) ss_up_adj_kernel(CMap s, Map d, int N, int H, int W) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)N * H * W;
  if (i >= npix) return;
  const int w = (int)(i % W), h = (int)((i / W) % H);
  const long n = i / ((long)W * H);
  float wh[4], ww[4];
  up_adj_w(h, H, wh);
  up_adj_w(w, W, ww);
  F3 acc = {0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int fh = 2 * h - 1 + a;
    if (wh[a] == 0.f) continue;   // (outside the fine map exactly then)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int fw = 2 * w - 1 + b;
      if (ww[b] == 0.f) continue;
      acc = fma3(wh[a] * ww[b], ldp<S4>(s.p + ((n * 2 * H + fh) * (2L * W) + fw) * s.ld), acc);
    }
  }
  stp<D4>(d.p + i * d.ld, acc);
}

// ---- warp ----
// the clamped coordinate: lower index, upper index (clamped: its weight is 0 there), fraction, and whether the clamp is inactive
struct Coord { int i0, i1; float f, live; };
__device__ __forceinline__ Coord clamp_coord(float iu, int size) {
  const float m = (float)(size - 1);
  Coord c;
  c.live = (iu > 0.f && iu < m) ? 1.f : 0.f;
  const float ic = fminf(fmaxf(iu, 0.f), m);   // (a NaN lands on 0: the indices stay inside the volume whatever the input)
  const float fl = floorf(ic);
  c.i0 = (int)fl;
  c.f = ic - fl;
  c.i1 = min(c.i0 + 1, size - 1);
  return c;
}
struct WarpArgs {
  const float* vol; int N, H, W, D;
  const float* flow; long ldf;
  const float* scale; long lds;
};
__device__ __forceinline__ void warp_coords(const WarpArgs& a, long i, int h, int w, Coord& cx, Coord& cy, Coord& cz) {
  const float fx = a.flow[i * a.ldf], fy = a.flow[i * a.ldf + 1], gz = a.scale[i * a.lds];
  cx = clamp_coord(fmaf(fx, 0.5f * (float)a.W, (float)w), a.W);
  cy = clamp_coord(fmaf(fy, 0.5f * (float)a.H, (float)h), a.H);
  cz = clamp_coord(fmaf(gz, 0.5f * (float)a.D, 0.5f * (float)(a.D - 1)), a.D);
}
__device__ __forceinline__ F3 vox(const WarpArgs& a, long n, int y, int x, int z) {
  return ldp<true>(a.vol + ((((n * a.H + y) * a.W + x) * a.D + z) << 2));
}
// the 8 corner weights, index = 4 dz + 2 dy + dx
__device__ __forceinline__ void corner_weights(float fx, float fy, float fz, float (&wt)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) wt[c] = ((c & 1) ? fx : 1.f - fx) * ((c & 2) ? fy : 1.f - fy) * ((c & 4) ? fz : 1.f - fz);
}

__global__ void __launch_bounds__(TPB) ss_warp_fwd_kernel(WarpArgs a, float* y, long ldy) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)a.N * a.H * a.W;
  if (i >= npix) return;
  const int w = (int)(i % a.W), h = (int)((i / a.W) % a.H);
  const long n = i / ((long)a.W * a.H);
  Coord cx, cy, cz;
  warp_coords(a, i, h, w, cx, cy, cz);
  float wt[8];
  corner_weights(cx.f, cy.f, cz.f, wt);
  F3 acc = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 8; ++c) acc = fma3(wt[c], vox(a, n, (c & 2) ? cy.i1 : cy.i0, (c & 1) ? cx.i1 : cx.i0, (c & 4) ? cz.i1 : cz.i0), acc);
  stp<false>(y + i * ldy, acc);
}

// dflow / dscale of a pixel (gathers), and — when the volume takes a gradient — the pixel's sort key, id and fractions
__global__ void __launch_bounds__(TPB) ss_warp_bwd_pixel_kernel(WarpArgs a, const float* dy, long lddy, float* dflow, long lddf, float* dscale, long ldds,
                                                                unsigned* keys, unsigned* ids, f32x4* frac) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x, npix = (long)a.N * a.H * a.W;
  if (i >= npix) return;
  const int w = (int)(i % a.W), h = (int)((i / a.W) % a.H);
  const long n = i / ((long)a.W * a.H);
  Coord cx, cy, cz;
  warp_coords(a, i, h, w, cx, cy, cz);
  if (keys != nullptr) {
    keys[i] = (unsigned)((((n * a.H + cy.i0) * a.W + cx.i0) * a.D) + cz.i0);
    ids[i] = (unsigned)i;
    frac[i] = (f32x4){cx.f, cy.f, cz.f, 0.f};
  }
  if (dflow == nullptr && dscale == nullptr) return;
  const F3 g = ldp<false>(dy + i * lddy);
  F3 v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = vox(a, n, (c & 2) ? cy.i1 : cy.i0, (c & 1) ? cx.i1 : cx.i0, (c & 4) ? cz.i1 : cz.i0);
  const float ax[2] = {1.f - cx.f, cx.f}, ay[2] = {1.f - cy.f, cy.f}, az[2] = {1.f - cz.f, cz.f};
  float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int bx = c & 1, by = (c >> 1) & 1, bz = c >> 2;
    const float dot = fmaf(g.z, v[c].z, fmaf(g.y, v[c].y, g.x * v[c].x));
    gx = fmaf((bx ? 1.f : -1.f) * (ay[by] * az[bz]), dot, gx);
    gy = fmaf((by ? 1.f : -1.f) * (ax[bx] * az[bz]), dot, gy);
    gz = fmaf((bz ? 1.f : -1.f) * (ax[bx] * ay[by]), dot, gz);
  }
  if (dflow != nullptr) {
    dflow[i * lddf] = gx * (0.5f * (float)a.W) * cx.live;
    dflow[i * lddf + 1] = gy * (0.5f * (float)a.H) * cy.live;
  }
  if (dscale != nullptr) dscale[i * ldds] = gz * (0.5f * (float)a.D) * cz.live;
}

// bucket bounds from the sorted keys: first[k] = position of the first entry with key k, last[k] = one past its last (0, 0: empty)
__global__ void __launch_bounds__(TPB) ss_bounds_kernel(const unsigned* keys, long n, unsigned* first, unsigned* last) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned k = keys[i];
  if (i == 0 || keys[i - 1] != k) first[k] = (unsigned)i;
  if (i == n - 1 || keys[i + 1] != k) last[k] = (unsigned)(i + 1);
}

// dvolume: one thread per voxel; corners in the order dz, dy, dx = 0/1 (the voxel as the pixel's lower corner first), each bucket in
// ascending pixel id
__global__ void __launch_bounds__(TPB) ss_warp_bwd_volume_kernel(int N, int H, int W, int D, const unsigned* ids, const f32x4* frac, const unsigned* first,
                                                                 const unsigned* last, const float* dy, long lddy, float* dvol) {
  const long v = (long)blockIdx.x * TPB + threadIdx.x, nvox = (long)N * H * W * D;
  if (v >= nvox) return;
  const int z = (int)(v % D), x = (int)((v / D) % W), y = (int)((v / ((long)D * W)) % H);
  F3 acc = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int bx = c & 1, by = (c >> 1) & 1, bz = c >> 2;
    if (x - bx < 0 || y - by < 0 || z - bz < 0) continue;
    const long k = v - ((long)by * W + bx) * D - bz;
    const unsigned lo = first[k], hi = last[k];
    for (unsigned j = lo; j < hi; ++j) {
      const unsigned p = ids[j];
      const f32x4 f = frac[p];
      const float wgt = (bx ? f[0] : 1.f - f[0]) * (by ? f[1] : 1.f - f[1]) * (bz ? f[2] : 1.f - f[2]);
      acc = fma3(wgt, ldp<false>(dy + (long)p * lddy), acc);
    }
  }
  stp<true>(dvol + (v << 2), acc);
}

inline unsigned blocks_for(long n) { return (unsigned)((n + TPB - 1) / TPB); }

// the workspace of the volume passes: two full-resolution maps and three half-resolution ones, [pixels][4] each
struct VolWs { float* full[2]; float* half[3]; };
inline long half_pixels(const clc_ss_desc* d) { return ((long)d->N * d->H * d->W + 3) / 4; }
inline size_t vol_ws_bytes(const clc_ss_desc* d) { return (size_t)(2 * (long)d->N * d->H * d->W + 3 * half_pixels(d)) * 16; }
inline VolWs vol_ws(const clc_ss_desc* d, void* ws) {
  float* p = static_cast<float*>(ws);
  const long full = (long)d->N * d->H * d->W * 4, half = half_pixels(d) * 4;
  return {{p, p + full}, {p + 2 * full, p + 2 * full + half, p + 2 * full + 2 * half}};
}

int check_desc(const clc_ss_desc* d, const char* who) {
  CLC_CHECK(d != nullptr, "%s: desc is NULL", who);
  CLC_CHECK(d->N >= 1 && d->H >= 1 && d->W >= 1, "%s: N, H, W must be positive (got N=%d H=%d W=%d)", who, d->N, d->H, d->W);
  CLC_CHECK(d->levels >= 1 && d->levels <= CLC_SS_MAX_LEVELS, "%s: levels must be 1..%d (got %d)", who, CLC_SS_MAX_LEVELS, d->levels);
  const int m = 1 << (d->levels - 1);
  CLC_CHECK(d->H % m == 0 && d->W % m == 0, "%s: H and W must be divisible by 2^(levels-1) = %d (got H=%d W=%d)", who, m, d->H, d->W);
  CLC_CHECK(d->ntaps >= 1 && d->ntaps <= CLC_SS_MAX_TAPS && (d->ntaps & 1), "%s: ntaps must be odd, 1..%d (got %d)", who, CLC_SS_MAX_TAPS, d->ntaps);
  CLC_CHECK((long)d->N * d->H * d->W * (d->levels + 1) < (1L << 31), "%s: N*H*W*(levels+1) must stay below 2^31 (got %ld)", who,
            (long)d->N * d->H * d->W * (d->levels + 1));
  return 0;
}

Taps taps_of(const clc_ss_desc* d) {
  Taps t;
  t.n = d->ntaps;
  for (int k = 0; k < CLC_SS_MAX_TAPS; ++k) t.v[k] = k < d->ntaps ? d->taps[k] : 0.f;
  return t;
}

int check_warp(const char* who, const float* vol, int N, int H, int W, int D, const float* flow, int ldf, const float* scale, int lds) {
  CLC_CHECK(N >= 1 && H >= 1 && W >= 1 && D >= 1, "%s: N, H, W, D must be positive (got N=%d H=%d W=%d D=%d)", who, N, H, W, D);
  CLC_CHECK((long)N * H * W * D < (1L << 31), "%s: N*H*W*D must stay below 2^31 (got %ld)", who, (long)N * H * W * D);
  CLC_CHECK(vol != nullptr && aligned16(vol), "%s: vol must be a 16-byte aligned [N][H][W][D][4] buffer", who);
  CLC_CHECK(flow != nullptr && ldf >= 2, "%s: flow is NULL or ldf < 2 (got ldf=%d)", who, ldf);
  CLC_CHECK(scale != nullptr && lds >= 1, "%s: scale is NULL or lds < 1 (got lds=%d)", who, lds);
  return 0;
}

using SortConfig = rocprim::default_config;
hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const unsigned* kin, unsigned* kout, const unsigned* vin, unsigned* vout, size_t n, unsigned bits,
                      hipStream_t st) {
  return rocprim::radix_sort_pairs<SortConfig>(tmp, tmp_bytes, kin, kout, vin, vout, n, 0u, bits, st, false);
}
inline unsigned key_bits(long nvox) {
  unsigned b = 1;
  while (b < 32 && (1L << b) < nvox) ++b;
  return b;
}
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
// warp backward workspace: keys in / out, ids in / out [P] u32, fractions [P] x 16 B, first / last [P D] u32, the sort's temporary storage
struct WarpWs { unsigned *kin, *kout, *vin, *vout, *first, *last; f32x4* frac; void* tmp; size_t tmp_bytes, total; };
int warp_ws(int N, int H, int W, int D, void* ws, WarpWs& o) {
  const size_t P = (size_t)N * H * W, V = P * D;
  size_t tmp = 0;
  const hipError_t e = sort_pairs(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, P, key_bits((long)V), nullptr);
  CLC_CHECK(e == hipSuccess, "clc_ss_warp_bwd: radix sort size query failed: %s", hipGetErrorString(e));
  char* p = static_cast<char*>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += up256(bytes); return q; };
  o.frac = reinterpret_cast<f32x4*>(take(P * 16));
  o.kin = reinterpret_cast<unsigned*>(take(P * 4));
  o.kout = reinterpret_cast<unsigned*>(take(P * 4));
  o.vin = reinterpret_cast<unsigned*>(take(P * 4));
  o.vout = reinterpret_cast<unsigned*>(take(P * 4));
  o.first = reinterpret_cast<unsigned*>(take(V * 4));   // (first and last are adjacent: one memset)
  o.last = reinterpret_cast<unsigned*>(take(V * 4));
  o.tmp = take(tmp > 0 ? tmp : 1);
  o.tmp_bytes = tmp;
  o.total = off;
  return 0;
}

}  // namespace

extern "C" {

size_t clc_ss_volume_workspace_bytes(const clc_ss_desc* d) {
  if (check_desc(d, "clc_ss_volume_workspace_bytes") < 0) return 0;
  return vol_ws_bytes(d);
}

int clc_ss_volume_fwd(const clc_ss_desc* d, const float* x, int ldx, float* vol, void* ws, size_t ws_bytes, clc_stream_t stream) {
  if (check_desc(d, "clc_ss_volume_fwd") < 0) return -1;
  CLC_CHECK(x != nullptr && ldx >= 3, "clc_ss_volume_fwd: x is NULL or ldx < 3 (got ldx=%d)", ldx);
  CLC_CHECK(vol != nullptr && aligned16(vol), "clc_ss_volume_fwd: vol must be a 16-byte aligned [N][H][W][D][4] buffer");
  CLC_CHECK(ws != nullptr && aligned16(ws) && ws_bytes >= vol_ws_bytes(d), "clc_ss_volume_fwd: ws must be 16-byte aligned with ws_bytes >= %zu (got %zu)",
            vol_ws_bytes(d), ws_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = d->N, H = d->H, W = d->W, L = d->levels, D = L + 1;
  const long P = (long)N * H * W, vld = 4L * D;
  const Taps t = taps_of(d);
  const VolWs b = vol_ws(d, ws);
  ss_copy_kernel<false, true><<<blocks_for(P), TPB, 0, st>>>(CMap{x, ldx}, Map{vol, vld}, P);
  ss_blur_kernel<false, true, false><<<blocks_for(P), TPB, 0, st>>>(CMap{x, ldx}, Map{b.full[0], 4}, N, H, W, t);
  ss_blur_kernel<true, true, true><<<blocks_for(P), TPB, 0, st>>>(CMap{b.full[0], 4}, Map{vol + 4, vld}, N, H, W, t);
  CMap cur = {vol + 4, vld};   // t_i at (h, w)
  int h = H, w = W;
  for (int i = 1; i < L; ++i) {
    h >>= 1; w >>= 1;
    const long p = (long)N * h * w;
    ss_pool_kernel<true, true><<<blocks_for(p), TPB, 0, st>>>(cur, Map{b.half[0], 4}, N, h, w);
    ss_blur_kernel<true, true, false><<<blocks_for(p), TPB, 0, st>>>(CMap{b.half[0], 4}, Map{b.full[0], 4}, N, h, w, t);
    ss_blur_kernel<true, true, true><<<blocks_for(p), TPB, 0, st>>>(CMap{b.full[0], 4}, Map{b.half[1], 4}, N, h, w, t);
    cur = {b.half[1], 4};
    // slice i + 1: i upsamplings, the last one into the volume; the intermediate maps (at most H/2 x W/2) alternate between full[1] and half[2]
    CMap s = cur;
    int uh = h, uw = w;
    for (int u = 0; u < i; ++u) {
      const bool lastu = u == i - 1;
      const Map dst = lastu ? Map{vol + 4L * (i + 1), vld} : Map{(u & 1) ? b.half[2] : b.full[1], 4};
      ss_up_kernel<true, true><<<blocks_for((long)N * uh * uw * 4), TPB, 0, st>>>(s, dst, N, uh, uw);
      s = {dst.p, dst.ld};
      uh *= 2; uw *= 2;
    }
  }
  CLC_LAUNCH_CHECK();
  return 0;
}

int clc_ss_volume_bwd(const clc_ss_desc* d, const float* dvol, float* dx, int lddx, void* ws, size_t ws_bytes, clc_stream_t stream) {
  if (check_desc(d, "clc_ss_volume_bwd") < 0) return -1;
  CLC_CHECK(dx != nullptr && lddx >= 3, "clc_ss_volume_bwd: dx is NULL or lddx < 3 (got lddx=%d)", lddx);
  CLC_CHECK(dvol != nullptr && aligned16(dvol), "clc_ss_volume_bwd: dvol must be a 16-byte aligned [N][H][W][D][4] buffer");
  CLC_CHECK(ws != nullptr && aligned16(ws) && ws_bytes >= vol_ws_bytes(d), "clc_ss_volume_bwd: ws must be 16-byte aligned with ws_bytes >= %zu (got %zu)",
            vol_ws_bytes(d), ws_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = d->N, H = d->H, W = d->W, L = d->levels, D = L + 1;
  const long P = (long)N * H * W, vld = 4L * D;
  const Taps t = taps_of(d);
  const VolWs b = vol_ws(d, ws);
  // pull(s, k): the adjoint of k upsamplings applied to slice s -> a map at (H >> k, W >> k); k == 0 is the slice itself.
  // Intermediate maps alternate between half[1] and half[2] (the first one, H/2 x W/2, fits a half map).
  auto pull = [&](int slice, int k) -> CMap {
    CMap s = {dvol + 4L * slice, vld};
    int uh = H, uw = W;
    for (int u = 0; u < k; ++u) {
      uh >>= 1; uw >>= 1;
      const Map dst = {(u & 1) ? b.half[2] : b.half[1], 4};
      ss_up_adj_kernel<true, true><<<blocks_for((long)N * uh * uw), TPB, 0, st>>>(s, dst, N, uh, uw);
      s = {dst.p, dst.ld};
    }
    return s;
  };
  // G = d t_L at (H >> (L - 1)); then for k = L - 1 .. 1: d t_k = pull(slice k, k - 1) + pool^T(blur^T(d t_{k+1}))
  CMap G = pull(L, L - 1);
  for (int k = L - 1; k >= 1; --k) {
    const int h = H >> k, w = W >> k;   // the map t_{k+1} lives on
    const long p = (long)N * h * w;
    ss_blur_adj_kernel<true, true, true, true><<<blocks_for(p), TPB, 0, st>>>(G, Map{b.full[1], 4}, CMap{nullptr, 0}, N, h, w, t);
    ss_blur_adj_kernel<true, true, true, false><<<blocks_for(p), TPB, 0, st>>>(CMap{b.full[1], 4}, Map{b.half[0], 4}, CMap{nullptr, 0}, N, h, w, t);
    const CMap add = pull(k, k - 1);   // (after G has been consumed: pull writes half[1] / half[2], G may live there)
    ss_pool_adj_kernel<true, true, true><<<blocks_for(p * 4), TPB, 0, st>>>(CMap{b.half[0], 4}, Map{b.full[0], 4}, add, N, 2 * h, 2 * w);
    G = {b.full[0], 4};
  }
  // dx = dV0 + blur^T(d t_1): the vertical adjoint first (the forward blurred rows, then columns)
  ss_blur_adj_kernel<true, true, true, true><<<blocks_for(P), TPB, 0, st>>>(G, Map{b.full[1], 4}, CMap{nullptr, 0}, N, H, W, t);
  ss_blur_adj_kernel<true, false, true, false><<<blocks_for(P), TPB, 0, st>>>(CMap{b.full[1], 4}, Map{dx, lddx}, CMap{dvol, vld}, N, H, W, t);
  CLC_LAUNCH_CHECK();
  return 0;
}

int clc_ss_warp_fwd(const float* vol, int N, int H, int W, int D, const float* flow, int ldf, const float* scale, int lds, float* y, int ldy,
                    clc_stream_t stream) {
  if (check_warp("clc_ss_warp_fwd", vol, N, H, W, D, flow, ldf, scale, lds) < 0) return -1;
  CLC_CHECK(y != nullptr && ldy >= 3, "clc_ss_warp_fwd: y is NULL or ldy < 3 (got ldy=%d)", ldy);
  const WarpArgs a = {vol, N, H, W, D, flow, ldf, scale, lds};
  ss_warp_fwd_kernel<<<blocks_for((long)N * H * W), TPB, 0, static_cast<hipStream_t>(stream)>>>(a, y, ldy);
  CLC_LAUNCH_CHECK();
  return 0;
}

size_t clc_ss_warp_bwd_workspace_bytes(int N, int H, int W, int D) {
  if (N < 1 || H < 1 || W < 1 || D < 1 || (long)N * H * W * D >= (1L << 31)) {
    clc_set_error("clc_ss_warp_bwd_workspace_bytes: N, H, W, D must be positive with N*H*W*D below 2^31 (got N=%d H=%d W=%d D=%d)", N, H, W, D);
    return 0;
  }
  WarpWs o;
  if (warp_ws(N, H, W, D, nullptr, o) < 0) return 0;
  return o.total;
}

int clc_ss_warp_bwd(const float* vol, int N, int H, int W, int D, const float* flow, int ldf, const float* scale, int lds, const float* dy, int lddy,
                    float* dflow, int lddf, float* dscale, int ldds, float* dvol, void* ws, size_t ws_bytes, clc_stream_t stream) {
  if (check_warp("clc_ss_warp_bwd", vol, N, H, W, D, flow, ldf, scale, lds) < 0) return -1;
  CLC_CHECK(dy != nullptr && lddy >= 3, "clc_ss_warp_bwd: dy is NULL or lddy < 3 (got lddy=%d)", lddy);
  CLC_CHECK(dflow == nullptr || lddf >= 2, "clc_ss_warp_bwd: lddf < 2 (got %d)", lddf);
  CLC_CHECK(dscale == nullptr || ldds >= 1, "clc_ss_warp_bwd: ldds < 1 (got %d)", ldds);
  CLC_CHECK(dflow != nullptr || dscale != nullptr || dvol != nullptr, "clc_ss_warp_bwd: dflow, dscale and dvol are all NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long P = (long)N * H * W, V = P * D;
  const WarpArgs a = {vol, N, H, W, D, flow, ldf, scale, lds};
  WarpWs o = {};
  if (dvol != nullptr) {
    CLC_CHECK(aligned16(dvol), "clc_ss_warp_bwd: dvol must be 16-byte aligned");
    CLC_CHECK(ws != nullptr && (reinterpret_cast<uintptr_t>(ws) & 255) == 0, "clc_ss_warp_bwd: ws must be 256-byte aligned when dvol is wanted");
    if (warp_ws(N, H, W, D, ws, o) < 0) return -1;
    CLC_CHECK(ws_bytes >= o.total, "clc_ss_warp_bwd: ws_bytes must be >= %zu (got %zu)", o.total, ws_bytes);
  }
  ss_warp_bwd_pixel_kernel<<<blocks_for(P), TPB, 0, st>>>(a, dy, lddy, dflow, lddf, dscale, ldds, o.kin, o.vin, o.frac);
  CLC_LAUNCH_CHECK();
  if (dvol == nullptr) return 0;
  size_t tmp_bytes = o.tmp_bytes;
  const hipError_t e = sort_pairs(o.tmp, tmp_bytes, o.kin, o.kout, o.vin, o.vout, (size_t)P, key_bits(V), st);
  CLC_CHECK(e == hipSuccess, "clc_ss_warp_bwd: radix sort failed: %s", hipGetErrorString(e));
  const hipError_t m = hipMemsetAsync(o.first, 0, (size_t)(reinterpret_cast<char*>(o.last) - reinterpret_cast<char*>(o.first)) + (size_t)V * 4, st);
  CLC_CHECK(m == hipSuccess, "clc_ss_warp_bwd: hipMemsetAsync failed: %s", hipGetErrorString(m));
  ss_bounds_kernel<<<blocks_for(P), TPB, 0, st>>>(o.kout, P, o.first, o.last);
  ss_warp_bwd_volume_kernel<<<blocks_for(V), TPB, 0, st>>>(N, H, W, D, o.vout, o.frac, o.first, o.last, dy, lddy, dvol);
  CLC_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
