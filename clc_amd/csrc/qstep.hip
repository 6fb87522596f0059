// qstep.hip — the Gaussian-conditional kernels with a quantisation step per channel (variable-rate coding; gfx950).
//
// A file of its own beside entropy.hip, not a template over its kernels: the unit-step kernels of entropy.hip stay the instantiations
// they were (same registers, same bits), and what the two files must agree on — the bounded scale, Phi, the scale index — is
// coder_device.h's, one definition each.  With step == 1.0f every expression below reduces exactly ((y - mu) / 1, 1 * u, 0.5f * 1,
// q * 1 are exact), so the outputs equal the unit-step kernels' bit for bit.
//
//   sigma = max(scale, 0.11);  t = (y - mu) / step[c];  q = rintf(t);  y_hat = q * step[c] + mu  (a rounded multiply, a rounded add)
//   y_in  = y + step[c] * u (mode 0, training) | y_hat (mode 1, eval);  v = |y_in - mu|;  h = 0.5f * step[c]
//   lik   = max(Phi((h - v) / sigma) - Phi((-h - v) / sigma), 1e-9)
//
// Bytes per latent element are the unit-step kernels' (the step vector is C floats, cache resident); the backward adds a per-channel
// sum, and the rate sweep reads y, mu, scale once (12 B) for K candidates of 2 erfcf + 1 log2f each.
#include "coder_device.h"

namespace {
using namespace coder;

constexpr float kLikBound = 1e-9f;
constexpr int kMaxCandidates = 16;

inline int grid_for(long n) { long b = (n + 1023) / 1024; return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b)); }

// the eval-mode likelihood before its bound, shared by the forward kernel and the rate sweep: q = rintf((y - mu) / step)
__device__ __forceinline__ float lik_of(float v, float sg, float h) { return std_cum((h - v) / sg) - std_cum((-h - v) / sg); }

// the element order, grid and partials of gauss_lik_fwd_kernel (entropy.hip): bits_partial of a unit step equals that kernel's
__global__ __launch_bounds__(256) void gauss_lik_step_fwd_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ mu, int ldmu,
                                                               const float* __restrict__ scale, int ldsc, const float* __restrict__ noise, int ldn,
                                                               const float* __restrict__ step, float* __restrict__ lik, int ldl,
                                                               float* __restrict__ y_hat, int ldh, long rows, int C, int mode,
                                                               float* __restrict__ bits_partial) {
  __shared__ float sm[4];
  const long total = rows * C;
  float bits = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    const float yv = y[r * ldy + c], m = mu[r * ldmu + c], s = step[c];
    const float rq = rintf((yv - m) / s);
    const float deq = rq * s + m;
    const float yin = (mode == 0) ? yv + s * noise[r * ldn + c] : deq;
    const float sg = bound_below(scale[r * ldsc + c], kScaleBound);
    const float lb = bound_below(lik_of(fabsf(yin - m), sg, 0.5f * s), kLikBound);
    lik[r * ldl + c] = lb;
    if (y_hat) y_hat[r * ldh + c] = deq;
    bits += log2f(lb);
  }
  if (bits_partial) {
    bits = wave_sum(bits);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) bits_partial[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  }
}

// ---- the thread-keeps-its-channel tiling of the backward kernel and the rate sweep ----
// A block of 256 threads is cl channel lanes x (256 / cl) row lanes, cl = min(64, the power of two >= C): consecutive lanes read
// consecutive channels (whole lines at C >= 64), and a thread walks rows only, so what belongs to its channel — the step, the running
// per-channel sums — stays in registers.
struct ChanTile {
  int cl, rl;   // channel lanes, row lanes
};
inline ChanTile chan_tile(int C) {
  int cl = 1;
  while (cl < C && cl < 64) cl *= 2;
  return {cl, 256 / cl};
}
constexpr int kSweepRows = 4;   // rows a thread walks at least before another row block is opened: the rate sweep (16 candidates a row)
constexpr int kGradRows = 8;    // ... the backward kernel: fewer row blocks, a shorter second stage
constexpr int kMaxRowBlocks = 512;
inline int row_blocks(long rows, int rl, int per_thread) {
  const long b = (rows + (long)rl * per_thread - 1) / ((long)rl * per_thread);
  return (int)(b < 1 ? 1 : (b > kMaxRowBlocks ? kMaxRowBlocks : b));
}

// gauss_lik_bwd_kernel with the step; dstep's stage 1: part[blockIdx.y][c] = the block's sum for channel c, row lanes added in
// ascending order by the block's first row lane.  g_hat: the upstream gradient of y_hat (added to dy; times q - t into dstep).
__global__ __launch_bounds__(256) void gauss_lik_step_bwd_kernel(const float* __restrict__ dlik, int lddl, const float* __restrict__ y, int ldy,
                                                               const float* __restrict__ mu, int ldmu, const float* __restrict__ scale, int ldsc,
                                                               const float* __restrict__ noise, int ldn, const float* __restrict__ step,
                                                               float* __restrict__ dy, int lddy, float* __restrict__ dmu, int lddmu,
                                                               float* __restrict__ dscale, int lddsc, long rows, int C, int mode,
                                                               const float* __restrict__ g_hat, int ldg, int cl, float* __restrict__ part) {
  __shared__ float sm[256];
  const int rl = 256 / cl;
  const int lc = threadIdx.x & (cl - 1), lr = threadIdx.x / cl;
  const int c = blockIdx.x * cl + lc;
  float acc = 0.f;
  if (c < C) {
    const float s = step[c], h = 0.5f * s;
    for (long r = (long)blockIdx.y * rl + lr; r < rows; r += (long)gridDim.y * rl) {
      const float yv = y[r * ldy + c], m = mu[r * ldmu + c], sc = scale[r * ldsc + c];
      const float t = (yv - m) / s, rq = rintf(t);
      const float w = (mode == 0) ? noise[r * ldn + c] : rq;   // d(y_in - mu) / dstep
      const float yin = (mode == 0) ? yv + s * w : rq * s + m;
      const float sg = bound_below(sc, kScaleBound);
      const float d = yin - m, v = fabsf(d);
      const float a = (h - v) / sg, b = (-h - v) / sg;
      const float l = std_cum(a) - std_cum(b);
      float g = dlik[r * lddl + c];
      if (!(g - g == 0.f)) g = g - g;   // an upstream gradient that is not finite: NaN in every gradient of the element, as under autograd
      if (!(l >= kLikBound || g < 0.f)) g = g - g;   // LowerBound(lik, 1e-9): pass if lik >= bound or grad < 0, else 0 * g (+0, or NaN if g is)
      const float pa = kInvSqrt2Pi * expf(-0.5f * a * a), pb = kInvSqrt2Pi * expf(-0.5f * b * b);
      const float dl_dv = (pb - pa) / sg;
      const float dl_dsg = (pb * b - pa * a) / sg;
      float gs = g * dl_dsg;
      if (!(sc >= kScaleBound || gs < 0.f)) gs = gs - gs;   // LowerBound(scale, 0.11)
      dscale[r * lddsc + c] = gs;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      const float gv = g * dl_dv * sgn;   // d/d(y_in - mu)
      const float gy = (mode == 0) ? gv : 0.f;
      const float gh = g_hat ? g_hat[r * ldg + c] : 0.f;
      if (dy) dy[r * lddy + c] = g_hat ? gy + gh : gy;
      if (dmu) dmu[r * lddmu + c] = (mode == 0) ? -gv : -(gv - gv);   // eval: gv - gv, zero or NaN (mu enters y_in - mu twice)
      // the three ways the step reaches the loss: the half width, y_in, y_hat
      acc += (g * (0.5f * (pa + pb) / sg) + gv * w) + gh * (rq - t);
    }
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  if (lr == 0 && c < C) {
    float sum = sm[lc];
    for (int k = 1; k < rl; ++k) sum += sm[k * cl + lc];
    part[(long)blockIdx.y * C + c] = sum;
  }
}

// stage 2, a block per 64 channels: the row blocks are cut into four consecutive quarters of ceil(nby / 4), thread (quarter s, channel c)
// adds its quarter in ascending order, and the channel's first thread adds the four sums in ascending order — a fixed tree of nby alone
__global__ __launch_bounds__(256) void step_grad_final_kernel(const float* __restrict__ part, int nby, int C, float* __restrict__ dstep) {
  __shared__ float sm[256];
  const int lc = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lc;
  const int seg = (nby + 3) >> 2;
  const int j0 = s * seg, j1 = (j0 + seg < nby) ? j0 + seg : nby;
  float sum = 0.f;
  if (c < C)
    for (int j = j0; j < j1; ++j) sum += part[(long)j * C + c];
  sm[threadIdx.x] = sum;
  __syncthreads();
  if (s == 0 && c < C) dstep[c] = ((sm[lc] + sm[64 + lc]) + sm[128 + lc]) + sm[192 + lc];
}

__global__ __launch_bounds__(256) void quantize_build_indexes_step_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ mu, int ldmu,
                                                                        const float* __restrict__ scale, int ldsc, const float* __restrict__ step,
                                                                        const float* __restrict__ table, int n_scales,
                                                                        int32_t* __restrict__ symbols, int32_t* __restrict__ indexes,
                                                                        float* __restrict__ y_hat, int ldh, long rows, int C) {
  __shared__ float tb[256];
  for (int i = threadIdx.x; i < n_scales; i += 256) tb[i] = table[i];
  __syncthreads();
  const long total = rows * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    const float m = mu[r * ldmu + c], s = step[c];
    const float q = rintf((y[r * ldy + c] - m) / s);
    const int idx = scale_index_linear(fmaxf(scale[r * ldsc + c], kScaleBound) / s, tb, n_scales);
    symbols[i] = (int32_t)q;
    indexes[i] = idx;
    if (y_hat) y_hat[r * ldh + c] = q * s + m;
  }
}

// ---- the rate sweep: bits[b][k] = - sum over image b of log2 lik_eval under steps[k] ----
// grid (channel tiles, row blocks of ONE image, B): what a block sums, and in which order, is a function of (rows_per_image, C) alone —
// candidate k has its own accumulator all the way (thread, wave, block, final), so neither K nor B enters any sum.
__global__ __launch_bounds__(256) void gauss_rate_sweep_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ mu, int ldmu,
                                                             const float* __restrict__ scale, int ldsc, const float* __restrict__ steps, int K,
                                                             long rows_per_image, int C, int cl, float* __restrict__ part) {
  __shared__ float sm[4][kMaxCandidates];
  const int rl = 256 / cl;
  const int lc = threadIdx.x & (cl - 1), lr = threadIdx.x / cl;
  const int c = blockIdx.x * cl + lc;
  const long row0 = (long)blockIdx.z * rows_per_image;
  float s[kMaxCandidates], acc[kMaxCandidates];
#pragma unroll
  for (int k = 0; k < kMaxCandidates; ++k) {
    s[k] = (k < K && c < C) ? steps[k * C + c] : 1.f;
    acc[k] = 0.f;
  }
  if (c < C) {
    for (long r = (long)blockIdx.y * rl + lr; r < rows_per_image; r += (long)gridDim.y * rl) {
      const long at = row0 + r;
      const float yv = y[at * ldy + c], m = mu[at * ldmu + c];
      const float sg = bound_below(scale[at * ldsc + c], kScaleBound);
      const float d = yv - m;
#pragma unroll
      for (int k = 0; k < kMaxCandidates; ++k) {
        if (k < K) {   // (uniform)
          const float deq = rintf(d / s[k]) * s[k] + m;
          acc[k] -= log2f(bound_below(lik_of(fabsf(deq - m), sg, 0.5f * s[k]), kLikBound));
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxCandidates; ++k) {
    if (k < K) {
      const float v = wave_sum(acc[k]);
      if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][k] = v;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    const int k = threadIdx.x;
    const long blk = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[blk * K + k] = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
  }
}

// stage 2: one block per image, thread k adds the image's partials in ascending block order
__global__ __launch_bounds__(64) void rate_sweep_final_kernel(const float* __restrict__ part, int per_image, int K, float* __restrict__ bits) {
  const int k = threadIdx.x;
  if (k >= K) return;
  const float* p = part + (long)blockIdx.x * per_image * K;
  float sum = p[k];
  for (int j = 1; j < per_image; ++j) sum += p[(long)j * K + k];
  bits[(long)blockIdx.x * K + k] = sum;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int clc_gauss_lik_step_fwd(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc, const float* noise,
                                      int ldn, const float* step, float* lik, int ldl, float* y_hat, int ldh, long rows, int C, int mode,
                                      float* bits_partial, int n_partials, clc_stream_t stream) {
  CLC_CHECK(y && mu && scale && lik && rows > 0 && C > 0, "clc_gauss_lik_step_fwd: y, mu, scale or lik is NULL, or rows / C is not positive");
  CLC_CHECK(step, "clc_gauss_lik_step_fwd: step is NULL (the unit-step entry is clc_gauss_lik_fwd)");
  CLC_CHECK(mode == 0 || mode == 1, "clc_gauss_lik_step_fwd: mode must be 0 (training) or 1 (eval) (got %d)", mode);
  CLC_CHECK(mode == 1 || noise, "clc_gauss_lik_step_fwd: training mode needs noise");
  CLC_CHECK(ldy >= C && ldmu >= C && ldsc >= C && ldl >= C && (mode == 1 || ldn >= C) && (!y_hat || ldh >= C),
            "clc_gauss_lik_step_fwd: a leading dimension is below C = %d", C);
  const int nb = grid_for(rows * C);
  CLC_CHECK(!bits_partial || n_partials == nb, "clc_gauss_lik_step_fwd: n_partials must be clc_gauss_lik_partials() = %d", nb);
  hipLaunchKernelGGL(gauss_lik_step_fwd_kernel, dim3(nb), dim3(256), 0, ST, y, ldy, mu, ldmu, scale, ldsc, noise, ldn, step, lik, ldl, y_hat, ldh,
                     rows, C, mode, bits_partial);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t clc_gauss_lik_step_bwd_workspace_bytes(long rows, int C) {
  if (rows <= 0 || C <= 0) {
    clc_set_error("clc_gauss_lik_step_bwd_workspace_bytes: rows and C must be positive (got rows=%ld C=%d)", rows, C);
    return 0;
  }
  return (size_t)row_blocks(rows, chan_tile(C).rl, kGradRows) * (size_t)C * sizeof(float);
}

extern "C" int clc_gauss_lik_step_bwd(const float* dlik, int lddl, const float* y, int ldy, const float* mu, int ldmu, const float* scale,
                                      int ldsc, const float* noise, int ldn, const float* step, float* dy, int lddy, float* dmu, int lddmu,
                                      float* dscale, int lddsc, float* dstep, long rows, int C, int mode, const float* g_hat, int ldg, void* ws,
                                      size_t ws_bytes, clc_stream_t stream) {
  CLC_CHECK(dlik && y && mu && scale && dscale && rows > 0 && C > 0,
            "clc_gauss_lik_step_bwd: dlik, y, mu, scale or dscale is NULL, or rows / C is not positive");
  CLC_CHECK(step && dstep, "clc_gauss_lik_step_bwd: step or dstep is NULL (the unit-step entry is clc_gauss_lik_bwd)");
  CLC_CHECK(mode == 0 || mode == 1, "clc_gauss_lik_step_bwd: mode must be 0 (training) or 1 (eval) (got %d)", mode);
  CLC_CHECK(mode == 1 || noise, "clc_gauss_lik_step_bwd: training mode needs noise");
  CLC_CHECK(lddl >= C && ldy >= C && ldmu >= C && ldsc >= C && lddsc >= C && (mode == 1 || ldn >= C) && (!dy || lddy >= C) &&
                (!dmu || lddmu >= C) && (!g_hat || ldg >= C),
            "clc_gauss_lik_step_bwd: a leading dimension is below C = %d", C);
  const ChanTile t = chan_tile(C);
  const int nby = row_blocks(rows, t.rl, kGradRows);
  const size_t need = (size_t)nby * (size_t)C * sizeof(float);
  CLC_CHECK(ws && (reinterpret_cast<uintptr_t>(ws) & 3) == 0 && ws_bytes >= need,
            "clc_gauss_lik_step_bwd: ws must be 4-byte aligned with ws_bytes >= clc_gauss_lik_step_bwd_workspace_bytes() = %zu (got %zu)", need, ws_bytes);
  float* part = static_cast<float*>(ws);
  hipLaunchKernelGGL(gauss_lik_step_bwd_kernel, dim3((C + t.cl - 1) / t.cl, nby), dim3(256), 0, ST, dlik, lddl, y, ldy, mu, ldmu, scale, ldsc, noise,
                     ldn, step, dy, lddy, dmu, lddmu, dscale, lddsc, rows, C, mode, g_hat, ldg, t.cl, part);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(step_grad_final_kernel, dim3((C + 63) / 64), dim3(256), 0, ST, part, nby, C, dstep);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_quantize_build_indexes_step(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc, const float* step,
                                               const float* scale_table, int n_scales, int32_t* symbols, int32_t* indexes, float* y_hat, int ldh,
                                               long rows, int C, clc_stream_t stream) {
  CLC_CHECK(y && mu && scale && scale_table && symbols && indexes && rows > 0 && C > 0,
            "clc_quantize_build_indexes_step: y, mu, scale, scale_table, symbols or indexes is NULL, or rows / C is not positive");
  CLC_CHECK(step, "clc_quantize_build_indexes_step: step is NULL (the unit-step entry is clc_quantize_build_indexes)");
  CLC_CHECK(n_scales > 1 && n_scales <= 256, "clc_quantize_build_indexes_step: n_scales must be between 2 and 256 (got %d)", n_scales);
  CLC_CHECK(ldy >= C && ldmu >= C && ldsc >= C && (!y_hat || ldh >= C), "clc_quantize_build_indexes_step: a leading dimension is below C = %d", C);
  hipLaunchKernelGGL(quantize_build_indexes_step_kernel, dim3(grid_for(rows * C)), dim3(256), 0, ST, y, ldy, mu, ldmu, scale, ldsc, step,
                     scale_table, n_scales, symbols, indexes, y_hat, ldh, rows, C);
  CLC_LAUNCH_CHECK();
  return 0;
}

static int sweep_blocks(long rows_per_image, int C, ChanTile* t) {
  *t = chan_tile(C);
  return ((C + t->cl - 1) / t->cl) * row_blocks(rows_per_image, t->rl, kSweepRows);
}

extern "C" size_t clc_gauss_rate_sweep_workspace_bytes(int B, long rows_per_image, int C, int K) {
  if (B < 1 || B > 65535 || rows_per_image <= 0 || C <= 0 || K < 1 || K > kMaxCandidates) {
    clc_set_error("clc_gauss_rate_sweep_workspace_bytes: B must be 1 .. 65535, rows_per_image and C positive, K 1 .. %d (got B=%d rows_per_image=%ld C=%d K=%d)",
                  kMaxCandidates, B, rows_per_image, C, K);
    return 0;
  }
  ChanTile t;
  return (size_t)B * (size_t)sweep_blocks(rows_per_image, C, &t) * (size_t)K * sizeof(float);
}

extern "C" int clc_gauss_rate_sweep(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc, const float* steps, int K, int B,
                                    long rows_per_image, int C, float* bits, void* ws, size_t ws_bytes, clc_stream_t stream) {
  CLC_CHECK(y && mu && scale && steps && bits, "clc_gauss_rate_sweep: y, mu, scale, steps or bits is NULL");
  CLC_CHECK(K >= 1 && K <= kMaxCandidates, "clc_gauss_rate_sweep: K must be 1 .. %d candidates (got %d)", kMaxCandidates, K);
  CLC_CHECK(B >= 1 && B <= 65535 && rows_per_image > 0 && C > 0,
            "clc_gauss_rate_sweep: B must be 1 .. 65535 and rows_per_image, C positive (got B=%d rows_per_image=%ld C=%d)", B, rows_per_image, C);
  CLC_CHECK(ldy >= C && ldmu >= C && ldsc >= C, "clc_gauss_rate_sweep: a leading dimension is below C = %d", C);
  ChanTile t;
  const int per_image = sweep_blocks(rows_per_image, C, &t);
  const size_t need = (size_t)B * (size_t)per_image * (size_t)K * sizeof(float);
  CLC_CHECK(ws && (reinterpret_cast<uintptr_t>(ws) & 3) == 0 && ws_bytes >= need,
            "clc_gauss_rate_sweep: ws must be 4-byte aligned with ws_bytes >= clc_gauss_rate_sweep_workspace_bytes() = %zu (got %zu)", need, ws_bytes);
  float* part = static_cast<float*>(ws);
  const int gx = (C + t.cl - 1) / t.cl;
  hipLaunchKernelGGL(gauss_rate_sweep_kernel, dim3(gx, per_image / gx, B), dim3(256), 0, ST, y, ldy, mu, ldmu, scale, ldsc, steps, K, rows_per_image,
                     C, t.cl, part);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(rate_sweep_final_kernel, dim3(B), dim3(64), 0, ST, part, per_image, K, bits);
  CLC_LAUNCH_CHECK();
  return 0;
}
