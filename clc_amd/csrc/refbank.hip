// Reference bank of the codec (clc_amd/refbank.py): preparing reference images, gathering cached reference latents, and a content
// fingerprint of the reference encoder's weights that keys the cache.
//
// clc_ref_prepare is a context-model kernel: its outputs feed the reference encoder, whose latents steer the slice loop's means and
// scales, so a change to its arithmetic needs a new kernel generation (rans_host.cpp: kGeneration).
#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

// ---- clc_ref_prepare: pad(F.interpolate(r, (h, w), mode="bilinear", align_corners=False), 128), channels_last
// ATen's source-index rule (area_pixel_compute_source_index, align_corners=False): src = scale * (dst + 0.5) - 0.5 clamped at 0, with
// scale = in / out.  Index, weights and blend in double, rounded once to fp32 (the float64 recipe to within half an ulp); one thread per
// output pixel, all three channels.
__global__ __launch_bounds__(256) void ref_prepare_kernel(const clc_ref_src* __restrict__ table, int H, int W, int h, int w, int top, int left,
                                                          float* __restrict__ out) {
  const int n = blockIdx.y;
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= (long)H * W) return;
  const int oy = (int)(pix / W), ox = (int)(pix - (long)oy * W);
  float* o = out + ((long)n * H * W + pix) * 3;
  const int y = oy - top, x = ox - left;
  const clc_ref_src e = table[n];
  if (y < 0 || y >= h || x < 0 || x >= w || e.src == nullptr || e.h < 1 || e.w < 1) {
    o[0] = 0.f;
    o[1] = 0.f;
    o[2] = 0.f;
    return;
  }
  const long plane = (long)e.h * e.w;
  if (e.h == h && e.w == w) {   // the identity resize: an exact copy
    const float* s = e.src + (long)y * w + x;
    o[0] = s[0];
    o[1] = s[plane];
    o[2] = s[2 * plane];
    return;
  }
  const double sh = (double)e.h / (double)h, sw = (double)e.w / (double)w;
  double fy = sh * (y + 0.5) - 0.5, fx = sw * (x + 0.5) - 0.5;
  fy = fy < 0.0 ? 0.0 : fy;
  fx = fx < 0.0 ? 0.0 : fx;
  int y0 = (int)fy, x0 = (int)fx;
  y0 = y0 > e.h - 1 ? e.h - 1 : y0;
  x0 = x0 > e.w - 1 ? e.w - 1 : x0;
  const int y1 = y0 + (y0 < e.h - 1 ? 1 : 0), x1 = x0 + (x0 < e.w - 1 ? 1 : 0);
  const double ly1 = fy - y0, ly0 = 1.0 - ly1, lx1 = fx - x0, lx0 = 1.0 - lx1;
  const long i00 = (long)y0 * e.w + x0, i01 = (long)y0 * e.w + x1, i10 = (long)y1 * e.w + x0, i11 = (long)y1 * e.w + x1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* s = e.src + c * plane;
    const double v = ly0 * (lx0 * (double)s[i00] + lx1 * (double)s[i01]) + ly1 * (lx0 * (double)s[i10] + lx1 * (double)s[i11]);
    o[c] = (float)v;
  }
}

// ---- clc_gather_slots: out[r*B + b] = arena[idx[b*R + r]], one slot of `slot_vec` float4 per image; an index outside the arena writes NaN
__global__ __launch_bounds__(256) void gather_slots_kernel(const float4* __restrict__ arena, long slot_vec, int n_slots, const int* __restrict__ idx,
                                                           int B, int R, float4* __restrict__ out) {
  const int j = blockIdx.y;   // output image r*B + b
  const int r = j / B, b = j - r * B;
  const int s = idx[b * R + r];
  float4* o = out + (long)j * slot_vec;
  const bool ok = s >= 0 && s < n_slots;
  const float4* src = arena + (long)(ok ? s : 0) * slot_vec;
  const float nan = __builtin_nanf("");
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < slot_vec; i += (long)gridDim.x * blockDim.x)
    o[i] = ok ? src[i] : make_float4(nan, nan, nan, nan);
}

// ---- clc_fingerprint: sum over every 32-bit word of mix((global word index << 32) | word), mod 2^64.  A sum of per-word terms does
// not depend on which thread or block adds which word, so the value is the same for any grid.
__device__ __forceinline__ uint64_t fp_mix(uint64_t z) {   // splitmix64's finaliser: a bijection of 64-bit words
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void fingerprint_partials_kernel(const clc_fp_entry* __restrict__ table, int n, uint64_t* __restrict__ partials) {
  __shared__ uint64_t red[256];
  uint64_t acc = 0;
  const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (int k = 0; k < n; ++k) {
    const clc_fp_entry e = table[k];
    const unsigned char* p = (const unsigned char*)e.ptr;
    const long nw = (long)((e.nbytes + 3) / 4);
    const long full = (long)(e.nbytes / 4);
    for (long i = t0; i < nw; i += stride) {
      uint32_t word;
      if (i < full) {
        word = ((const uint32_t*)p)[i];
      } else {   // a tail of 1..3 bytes, zero-extended
        word = 0;
        for (long q = 4 * i; q < (long)e.nbytes; ++q) word |= (uint32_t)p[q] << (8 * (q - 4 * i));
      }
      acc += fp_mix(((uint64_t)(e.word_offset + i) << 32) | word);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void fingerprint_finish_kernel(const uint64_t* __restrict__ partials, int n_partials, uint64_t* __restrict__ out) {
  __shared__ uint64_t red[256];
  uint64_t acc = 0;
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x) acc += partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

}  // namespace

extern "C" int clc_ref_prepare(const clc_ref_src* table, int N, int h, int w, float* out, clc_stream_t stream) {
  CLC_CHECK(table && out && N > 0 && N <= 65535 && h > 0 && w > 0 && h <= 65535 && w <= 65535, "clc_ref_prepare: bad args");
  const int H = (h + 127) / 128 * 128, W = (w + 127) / 128 * 128;
  const int top = (H - h) / 2, left = (W - w) / 2;   // clc_amd.eval.pad: centred, the odd pixel at the bottom / right
  const long pix = (long)H * W;
  hipLaunchKernelGGL(ref_prepare_kernel, dim3((unsigned)((pix + 255) / 256), N), dim3(256), 0, ST, table, H, W, h, w, top, left, out);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_gather_slots(const float* arena, long slot_elems, int n_slots, const int32_t* idx, int B, int R, float* out, clc_stream_t stream) {
  CLC_CHECK(arena && idx && out && slot_elems > 0 && n_slots > 0 && B > 0 && R > 0 && (long)B * R <= 65535, "clc_gather_slots: bad args");
  CLC_CHECK(slot_elems % 4 == 0 && aligned16(arena) && aligned16(out), "clc_gather_slots: slots must hold a multiple of 4 floats, 16-byte aligned");
  const long vec = slot_elems / 4;
  long gx = (vec + 255) / 256;
  gx = gx > 256 ? 256 : gx;
  hipLaunchKernelGGL(gather_slots_kernel, dim3((unsigned)gx, B * R), dim3(256), 0, ST, (const float4*)arena, vec, n_slots, idx, B, R, (float4*)out);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_fingerprint(const clc_fp_entry* table, int n, uint64_t* partials, int n_partials, uint64_t* out, clc_stream_t stream) {
  CLC_CHECK(table && partials && out && n > 0 && n_partials > 0 && n_partials <= 4096, "clc_fingerprint: bad args");
  hipLaunchKernelGGL(fingerprint_partials_kernel, dim3(n_partials), dim3(256), 0, ST, table, n, partials);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(fingerprint_finish_kernel, dim3(1), dim3(256), 0, ST, partials, n_partials, out);
  CLC_LAUNCH_CHECK();
  return 0;
}
