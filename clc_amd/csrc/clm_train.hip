// clm_train.hip — recorded forward and backward of the Conditional Latent Matching ops (clm.hip holds the inference forward).
//
// Similarity column sums (CLM.py:107-109 + :14-20), per batch item, yt / yr = [HW][C] rows, s[p][q] = yt[p].yr[q] / tau:
//   forward   S[p][q] = exp(s - m[p]) / l[p]                 w[q] = sum_p S[p][q]
//   backward  D[p] = sum_q S[p][q] g[q]                      ds[p][q] = S[p][q] (g[q] - D[p])
//             dyt[p][:] = 1/tau sum_q ds[p][q] yr[q][:]      dyr[q][:] = 1/tau sum_p ds[p][q] yt[p][:]
// The [HW x HW] matrix is never stored: every kernel below recomputes 32 x 32 tiles of s on v_mfma_f32_32x32x2_f32 from the saved row
// statistics (m, l), flash-attention style.  All five kernels have ONE shape: a workgroup owns 32 rows of one matrix (the "block"
// rows, an LDS image shared by its 4 waves) and its waves stream over 32-row tiles of the other matrix (A operand, straight from
// global memory, 16 B per lane and k-step).  The tile X[r][j] = stream[r] . block[j] arrives with the block index j on the lane and
// the stream index r in the 16 accumulator registers, so
//   * per-block-row reductions (softmax statistics, D, column sums) are per-LANE sums over registers and tiles;
//   * the output product out[j][c] = sum_r X[r][j] stream[r][c] sums over the register index: X is the A operand of the next MFMA
//     as it stands (A[i = j][k = lane half] = X[reg][j]), no transpose, no LDS round trip.
//   kernel         block rows   streams   reads        writes
//   stats          yt (p)       yr (q)                 m[p], l[p]
//   colsum         yr (q)       yt (p)    m, l         w[q]
//   drow           yt (p)       yr (q)    m, l, g      D[p]
//   grad<dyt>      yt (p)       yr (q)    m, l, g, D   dyt[p][:]
//   grad<dyr>      yr (q)       yt (p)    m, l, g, D   dyr[q][:]
// Every output element has one owner and every sum a fixed order (lane -> lane half -> wave): no floating-point atomics, the same
// bits on every run.  Workspace: D only (B*HW floats).  Channel tiles of the output product are a template bound: grad<4|8|12>
// cover C <= 128 | 256 | 384 (64 | 128 | 192 accumulator registers per lane); the recorded path refuses C > 384.
//
// The three streaming backward kernels (scale_rows, deform, fuse) follow; the deform input gradient is a scatter made deterministic
// by bucketing its (source pixel, tap, corner) list by destination pixel with integer counters and ordering each bucket by source
// index before one wave per destination pixel gathers it.
#include "common.h"

namespace {

constexpr int kMaxHW = 4096;
constexpr int kMaxC = 384;

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int ldb_of(int C) { return ((C + 7) & ~7) + 4; }   // LDS row pitch: zero-padded to a multiple of 8, + 4 against bank conflicts
__device__ __forceinline__ int row_of(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }   // C/D layout of the 32x32 MFMAs

// rows row0 .. row0+31 of src -> img[32][ldb]; rows past HW and columns past C are zero
__device__ __forceinline__ void load_block(float* img, const float* __restrict__ src, int ld, int row0, int HW, int C, int ldb, int tid) {
  const int q4 = ldb >> 2;
  for (int i = tid; i < 32 * q4; i += 256) {
    const int r = i / q4, c = (i - r * q4) << 2;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + r < HW && c < C) v = *reinterpret_cast<const f32x4*>(src + (size_t)(row0 + r) * ld + c);
    *reinterpret_cast<f32x4*>(img + r * ldb + c) = v;
  }
}

// X[r][j] = sum_k stream[r][k] block[j][k]  (lane: column j = lane & 31; rows row_of(reg, lane >> 5)).  k order: lane half h takes
// k = 8 s + 4 h + {0..3} of step s — any order serves as long as both operands use the same one.
__device__ __forceinline__ f32x16 s_tile(const float* __restrict__ srow, const float* brow, int C, int h) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int nk = (C + 7) >> 3;
  // Software pipeline over groups of four k-steps: the global loads of group g + 1 are issued before the 16 MFMAs of group g, so a
  // wave that has its SIMD to itself (grids of about one workgroup per CU) does not sit out a full memory latency per group.
  auto load_a = [&](int step) -> f32x4 {
    const int k = 8 * step + 4 * h;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (step < nk && k < C) a = *reinterpret_cast<const f32x4*>(srow + k);
    return a;
  };
  f32x4 cur[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) cur[u] = load_a(u);
  for (int s = 0; s < nk; s += 4) {
    f32x4 nxt[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) nxt[u] = load_a(s + 4 + u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (s + u < nk) b[u] = *reinterpret_cast<const f32x4*>(brow + 8 * (s + u) + 4 * h);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s + u < nk) {   // wave-uniform
        acc = MFMA(cur[u][0], b[u][0], acc);
        acc = MFMA(cur[u][1], b[u][1], acc);
        acc = MFMA(cur[u][2], b[u][2], acc);
        acc = MFMA(cur[u][3], b[u][3], acc);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
  }
  return acc;
}

// m[p] = max_q s[p][q], l[p] = sum_q exp(s[p][q] - m[p])
__global__ __launch_bounds__(256) void clm_stats_kernel(const float* __restrict__ yt, int ldy, const float* __restrict__ yr, int ldr, int HW, int C,
                                                        float inv_tau, float* __restrict__ m_out, float* __restrict__ l_out) {
  extern __shared__ float sm[];
  const int ldb = ldb_of(C);
  float* red = sm + 32 * ldb;   // [2][8][32]
  const int b = blockIdx.y, j0 = blockIdx.x * 32, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  load_block(sm, yt + (size_t)b * HW * ldy, ldy, j0, HW, C, ldb, tid);
  __syncthreads();
  float mx = -INFINITY, l = 0.f;
  const int ntiles = (HW + 31) >> 5;
  for (int t = wave; t < ntiles; t += 4) {
    const int r = min(t * 32 + li, HW - 1);
    const f32x16 X = s_tile(yr + ((size_t)b * HW + r) * ldr, sm + li * ldb, C, h);
    float v[16], tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      v[i] = (t * 32 + row_of(i, h) < HW) ? X[i] * inv_tau : -INFINITY;
      tm = fmaxf(tm, v[i]);
    }
    if (tm > -INFINITY) {
      const float nm = fmaxf(mx, tm);
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) sum += expf(v[i] - nm);
      l = l * expf(mx - nm) + sum;
      mx = nm;
    }
  }
  red[(wave * 2 + h) * 32 + li] = mx;
  red[256 + (wave * 2 + h) * 32 + li] = l;
  __syncthreads();
  if (tid < 32 && j0 + tid < HW) {
    float M = -INFINITY;
    for (int k = 0; k < 8; ++k) M = fmaxf(M, red[k * 32 + tid]);
    float L = 0.f;
    for (int k = 0; k < 8; ++k) {
      const float mk = red[k * 32 + tid];
      if (mk > -INFINITY) L += red[256 + k * 32 + tid] * expf(mk - M);
    }
    m_out[(size_t)b * HW + j0 + tid] = M;
    l_out[(size_t)b * HW + j0 + tid] = L;
  }
}

// MODE 0: w[q] = sum_p S[p][q]           block rows = yr (q), stream = yt (p)
// MODE 1: D[p] = sum_q S[p][q] g[q]      block rows = yt (p), stream = yr (q)
template <int MODE>
__global__ __launch_bounds__(256) void clm_rowsum_kernel(const float* __restrict__ blk, int ldk, const float* __restrict__ str, int lds, int HW, int C,
                                                         float inv_tau, const float* __restrict__ m, const float* __restrict__ l,
                                                         const float* __restrict__ g, float* __restrict__ out) {
  extern __shared__ float sm[];
  const int ldb = ldb_of(C);
  float* red = sm + 32 * ldb;   // [8][32]
  const int b = blockIdx.y, j0 = blockIdx.x * 32, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  load_block(sm, blk + (size_t)b * HW * ldk, ldk, j0, HW, C, ldb, tid);
  __syncthreads();
  const size_t vb = (size_t)b * HW;
  const bool jok = j0 + li < HW;
  float mj = 0.f, lj = 1.f;
  if (MODE == 1 && jok) { mj = m[vb + j0 + li]; lj = l[vb + j0 + li]; }
  float acc = 0.f;
  const int ntiles = (HW + 31) >> 5;
  for (int t = wave; t < ntiles; t += 4) {
    const int r = min(t * 32 + li, HW - 1);
    const f32x16 X = s_tile(str + (vb + r) * lds, sm + li * ldb, C, h);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int rr = t * 32 + row_of(i, h);
      if (rr < HW) {
        if (MODE == 0) acc += expf(X[i] * inv_tau - m[vb + rr]) / l[vb + rr];
        else acc += expf(X[i] * inv_tau - mj) / lj * g[vb + rr];
      }
    }
  }
  red[(wave * 2 + h) * 32 + li] = acc;
  __syncthreads();
  if (tid < 32 && j0 + tid < HW) {
    float s = 0.f;
    for (int k = 0; k < 8; ++k) s += red[k * 32 + tid];
    out[vb + j0 + tid] = s;
  }
}

// BLOCK_IS_P: out = dyt (block rows = yt, stream = yr); else out = dyr (block rows = yr, stream = yt).
// out[j][c] = inv_tau * sum_r ds[r][j] * stream[r][c], ds = S (g[q] - D[p]).
template <int NCT, bool BLOCK_IS_P>
__global__ __launch_bounds__(256) void clm_sim_grad_kernel(const float* __restrict__ blk, int ldk, const float* __restrict__ str, int lds, int HW, int C,
                                                           float inv_tau, const float* __restrict__ m, const float* __restrict__ l,
                                                           const float* __restrict__ g, const float* __restrict__ D, float* __restrict__ out, int ldo) {
  extern __shared__ float sm[];
  const int ldb = ldb_of(C);
  const int b = blockIdx.y, j0 = blockIdx.x * 32, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  load_block(sm, blk + (size_t)b * HW * ldk, ldk, j0, HW, C, ldb, tid);
  __syncthreads();
  const size_t vb = (size_t)b * HW;
  const bool jok = j0 + li < HW;
  float mj = 0.f, lj = 1.f, Dj = 0.f, gj = 0.f;
  if (jok) {
    if (BLOCK_IS_P) { mj = m[vb + j0 + li]; lj = l[vb + j0 + li]; Dj = D[vb + j0 + li]; }
    else gj = g[vb + j0 + li];
  }
  f32x16 acc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
  const int ntiles = (HW + 31) >> 5;
  for (int t = wave; t < ntiles; t += 4) {
    const int r = min(t * 32 + li, HW - 1);
    const f32x16 X = s_tile(str + (vb + r) * lds, sm + li * ldb, C, h);
    float ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int rr = t * 32 + row_of(i, h);
      float v = 0.f;
      if (rr < HW) {
        if (BLOCK_IS_P) v = expf(X[i] * inv_tau - mj) / lj * (g[vb + rr] - Dj);
        else v = expf(X[i] * inv_tau - m[vb + rr]) / l[vb + rr] * (gj - D[vb + rr]);
      }
      ds[i] = v;
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      if (ct * 32 < C) {   // block-uniform
        const int cc = ct * 32 + li;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int rr = min(t * 32 + row_of(i, h), HW - 1);   // (rows past HW: ds = 0, any finite operand serves)
          const float bv = cc < C ? str[(vb + rr) * lds + cc] : 0.f;
          acc[ct] = MFMA(ds[i], bv, acc[ct]);
        }
      }
    }
  }
  __syncthreads();   // every wave is done with the block image: the cross-wave sum reuses its LDS
  float* scr = sm;   // [4][32][33]
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    if (ct * 32 < C) {
#pragma unroll
      for (int i = 0; i < 16; ++i) scr[(wave * 32 + row_of(i, h)) * 33 + li] = acc[ct][i];
      __syncthreads();
      for (int e = tid; e < 1024; e += 256) {
        const int row = e >> 5, col = e & 31;
        const float s = ((scr[row * 33 + col] + scr[(32 + row) * 33 + col]) + scr[(64 + row) * 33 + col]) + scr[(96 + row) * 33 + col];
        if (j0 + row < HW && ct * 32 + col < C) out[(vb + j0 + row) * ldo + ct * 32 + col] = s * inv_tau;
      }
      __syncthreads();
    }
  }
}

inline size_t sim_lds_bytes(int C, bool grad) {
  const size_t img = (size_t)32 * (((C + 7) & ~7) + 4);
  const size_t a = img + 512, g = 4 * 32 * 33;
  return sizeof(float) * (grad ? (img > g ? img : g) : a);
}

// ------------------------------------------------------------------------------------------------------------ streaming backward kernels

__global__ void clm_sigmoid_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo, long rows, int C) {
  const long total = rows * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    out[r * ldo + c] = 1.f / (1.f + expf(-x[r * ldx + c]));
  }
}

// one wave per row: dw[r] = sum_c d[r][c] x[r][c];  dx[r][c] += w[r] d[r][c]
__global__ __launch_bounds__(256) void clm_scale_rows_bwd_kernel(const float* __restrict__ d, int ldd, const float* __restrict__ x, int ldx,
                                                                 const float* __restrict__ w, float* __restrict__ dw, float* __restrict__ dx, int lddx,
                                                                 long rows, int C) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const float wr = w[r];
  float s = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float dv = d[r * ldd + c];
    s += dv * x[r * ldx + c];
    if (dx) dx[r * lddx + c] += wr * dv;
  }
  s = wave_sum(s);
  if (dw && lane == 0) dw[r] = s;
}

struct Tap { bool valid; int h0, w0, h1, w1; float lh, lw; };

__device__ __forceinline__ Tap tap_of(const float* __restrict__ off, long pix, int ldo, int k, int h, int w, int H, int W) {
  Tap t;
  const float oh = (float)h + off[pix * ldo + 2 * k], ow = (float)w + off[pix * ldo + 2 * k + 1];
  t.valid = oh >= 0.f && oh <= (float)(H - 1) && ow >= 0.f && ow <= (float)(W - 1);
  t.h0 = t.valid ? (int)oh : 0; t.w0 = t.valid ? (int)ow : 0;
  t.h1 = min(t.h0 + 1, H - 1); t.w1 = min(t.w0 + 1, W - 1);
  t.lh = oh - (float)t.h0; t.lw = ow - (float)t.w0;
  return t;
}

// one wave per pixel, lanes over channels: d_off[p][2k + {0,1}], d_logit[p][k] = d_mod * m (1 - m)
__global__ __launch_bounds__(256) void clm_deform_bwd_param_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ off, int ldo,
                                                                   const float* __restrict__ mod, int ldm, const float* __restrict__ da, int lda,
                                                                   float* __restrict__ doff, int lddo, float* __restrict__ dlogit, int lddl, int B, int H,
                                                                   int W, int C) {
  const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= (long)B * H * W) return;
  const int lane = threadIdx.x & 63;
  const int w = (int)(pix % W), h = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
  const float* xb = x + (size_t)b * H * W * ldx;
  float acc[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const Tap t = tap_of(off, pix, ldo, k, h, w, H, W);
    if (!t.valid) continue;   // wave-uniform
    const float* p00 = xb + (size_t)(t.h0 * W + t.w0) * ldx;
    const float* p10 = xb + (size_t)(t.h1 * W + t.w0) * ldx;
    const float* p01 = xb + (size_t)(t.h0 * W + t.w1) * ldx;
    const float* p11 = xb + (size_t)(t.h1 * W + t.w1) * ldx;
    for (int c = lane; c < C; c += 64) {
      const float a = da[pix * lda + c];
      const float v00 = p00[c], v10 = p10[c], v01 = p01[c], v11 = p11[c];
      acc[3 * k] += a * ((1.f - t.lh) * (1.f - t.lw) * v00 + t.lh * (1.f - t.lw) * v10 + (1.f - t.lh) * t.lw * v01 + t.lh * t.lw * v11);
      acc[3 * k + 1] += a * ((1.f - t.lw) * (v10 - v00) + t.lw * (v11 - v01));
      acc[3 * k + 2] += a * ((1.f - t.lh) * (v01 - v00) + t.lh * (v11 - v10));
    }
  }
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = wave_sum(acc[i]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float mk = mod[pix * ldm + k];
      dlogit[pix * lddl + k] = acc[3 * k] * mk * (1.f - mk);
      doff[pix * lddo + 2 * k] = mk * acc[3 * k + 1];
      doff[pix * lddo + 2 * k + 1] = mk * acc[3 * k + 2];
    }
    for (int k = 9; k < lddl; ++k) dlogit[pix * lddl + k] = 0.f;
    for (int k = 18; k < lddo; ++k) doff[pix * lddo + k] = 0.f;
  }
}

// The input gradient: dx[d][c] = sum over entries (source pixel p, tap k, corner j) that land on d of coef * da[p][c].
// pass 0 counts entries per destination, pass 1 deals each entry a slot in its destination's bucket (integer atomics: the SET of
// entries in a bucket is fixed, their order is not — the sort below fixes it).
template <int PASS>
__global__ void clm_deform_bucket_kernel(const float* __restrict__ off, int ldo, const float* __restrict__ mod, int ldm, int B, int H, int W,
                                         int* __restrict__ cnt, const int* __restrict__ start, int* __restrict__ ids, float* __restrict__ coef) {
  const long total = (long)B * H * W * 9;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i % 9);
    const long pix = i / 9;
    const int w = (int)(pix % W), h = (int)((pix / W) % H);
    const long base = pix - ((long)h * W + w);   // b * H * W
    const Tap t = tap_of(off, pix, ldo, k, h, w, H, W);
    if (!t.valid) continue;
    const float mk = PASS ? mod[pix * ldm + k] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int hj = (j & 1) ? t.h1 : t.h0, wj = (j & 2) ? t.w1 : t.w0;
      const long d = base + (long)hj * W + wj;
      const int pos = atomicAdd(&cnt[d], 1);
      if (PASS) {
        const float cf = ((j & 1) ? t.lh : 1.f - t.lh) * ((j & 2) ? t.lw : 1.f - t.lw);
        ids[start[d] + pos] = (int)(i * 4 + j);
        coef[start[d] + pos] = cf * mk;
      }
    }
  }
}

// exclusive scan of n counters into start[0..n] (one workgroup; thread t owns a contiguous chunk)
__global__ __launch_bounds__(1024) void clm_scan_kernel(const int* __restrict__ cnt, int* __restrict__ start, long n) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const long per = (n + 1023) / 1024, lo = min((long)tid * per, n), hi = min(lo + per, n);
  int s = 0;
  for (long i = lo; i < hi; ++i) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (long i = lo; i < hi; ++i) { start[i] = run; run += cnt[i]; }
  if (tid == 1023) start[n] = part[1023];
}

// one wave per destination: rank sort of its bucket by entry id (ids are unique) -> source-index order
__global__ __launch_bounds__(256) void clm_bucket_sort_kernel(const int* __restrict__ start, const int* __restrict__ ids, const float* __restrict__ coef,
                                                              int* __restrict__ ids_s, float* __restrict__ coef_s, long n) {
  const long d = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= n) return;
  const int lane = threadIdx.x & 63, s0 = start[d], cnt = start[d + 1] - s0;
  for (int i = lane; i < cnt; i += 64) {
    const int id = ids[s0 + i];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += ids[s0 + j] < id;
    ids_s[s0 + rank] = id;
    coef_s[s0 + rank] = coef[s0 + i];
  }
}

// one wave per destination pixel, lanes over channels, entries in source-index order
__global__ __launch_bounds__(256) void clm_deform_gather_kernel(const int* __restrict__ start, const int* __restrict__ ids, const float* __restrict__ coef,
                                                                const float* __restrict__ da, int lda, float* __restrict__ dx, int lddx, long n, int C) {
  const long d = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= n) return;
  const int lane = threadIdx.x & 63, s0 = start[d], s1 = start[d + 1];
  for (int c = lane; c < C; c += 64) {
    float acc = 0.f;
    for (int e = s0; e < s1; ++e) acc = fmaf(coef[e], da[(size_t)(ids[e] / 36) * lda + c], acc);
    dx[d * lddx + c] = acc;
  }
}

struct FuseBwdPtrs { const float* feat[8]; const float* att[8]; float* dfeat[8]; float* datt[8]; };

// one wave per row (see clc_hip.h for the formulas)
__global__ __launch_bounds__(256) void clm_fuse_bwd_kernel(FuseBwdPtrs P, int M, int ldf, int lda, const float* __restrict__ dout, int lddo, int lddf,
                                                           int ldda, long rows, int C, int gate) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float a[8], wt[8], sg[8], t[8], mx = -INFINITY, l = 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    a[m] = m < M ? P.att[m][r * lda] : -INFINITY;
    mx = fmaxf(mx, a[m]);
  }
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    wt[m] = m < M ? expf(a[m] - mx) : 0.f;
    l += wt[m];
    sg[m] = (gate && m < M) ? 1.f / (1.f + expf(-a[m])) : 1.f;
    t[m] = 0.f;
  }
  for (int c = lane; c < C; c += 64) {
    const float dv = dout[r * lddo + c];
#pragma unroll
    for (int m = 0; m < 8; ++m)
      if (m < M) t[m] += dv * P.feat[m][r * ldf + c];
  }
  float tbar = 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    wt[m] /= l;
    if (m < M) t[m] = wave_sum(t[m]) * sg[m];   // sum_c dout[c] F_m[c], F_m the feature as fused
    tbar += wt[m] * t[m];
  }
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if (m < M) {
      if (lane == 0) {
        float dv = wt[m] * (t[m] - tbar);
        if (gate) dv += wt[m] * (1.f - sg[m]) * t[m];   // sum_c dF_m[c] feat_m[c] sigma'(att_m)
        P.datt[m][r * ldda] = dv;
        for (int k = 1; k < ldda; ++k) P.datt[m][r * ldda + k] = 0.f;
      }
      const float f = wt[m] * sg[m];
      for (int c = lane; c < C; c += 64) P.dfeat[m][r * lddf + c] = f * dout[r * lddo + c];
    }
  }
}

inline int grid_for(long n) { long b = (n + 1023) / 1024; return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b)); }

int sim_args_ok(const char* who, const float* yt, int ldy, const float* yr, int ldr, int B, int HW, int C, float temperature) {
  CLC_CHECK(yt && yr && B > 0 && HW > 0 && C > 0 && temperature > 0.f, "%s: bad args", who);
  CLC_CHECK(HW <= kMaxHW, "%s: HW=%d exceeds %d", who, HW, kMaxHW);
  CLC_CHECK(C % 4 == 0 && C <= kMaxC, "%s: C=%d must be a multiple of 4 and at most %d", who, C, kMaxC);
  CLC_CHECK(ldy >= C && ldr >= C && ldy % 4 == 0 && ldr % 4 == 0 && aligned16(yt) && aligned16(yr), "%s: rows must be 16-byte aligned (ld=%d/%d)", who, ldy, ldr);
  return 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int clc_clm_sim_colsum_train(const float* yt, int ldy, const float* yrt, int ldr, int B, int HW, int C, float temperature, float* colsum,
                                        float* m, float* l, clc_stream_t stream) {
  if (sim_args_ok("clc_clm_sim_colsum_train", yt, ldy, yrt, ldr, B, HW, C, temperature) < 0) return -1;
  CLC_CHECK(colsum && m && l, "clc_clm_sim_colsum_train: bad args");
  const dim3 grid((HW + 31) / 32, B);
  const float it = 1.f / temperature;
  hipLaunchKernelGGL(clm_stats_kernel, grid, dim3(256), sim_lds_bytes(C, false), ST, yt, ldy, yrt, ldr, HW, C, it, m, l);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(clm_rowsum_kernel<0>, grid, dim3(256), sim_lds_bytes(C, false), ST, yrt, ldr, yt, ldy, HW, C, it, (const float*)m, (const float*)l,
                     (const float*)nullptr, colsum);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t clc_clm_sim_colsum_bwd_workspace_bytes(int B, int HW) { return (size_t)B * HW * sizeof(float); }

template <bool BLOCK_IS_P>
static int launch_sim_grad(const float* blk, int ldk, const float* str, int lds, int B, int HW, int C, float it, const float* m, const float* l,
                           const float* g, const float* D, float* out, int ldo, hipStream_t st) {
  const dim3 grid((HW + 31) / 32, B);
  const size_t sh = sim_lds_bytes(C, true);
  if (C <= 128) hipLaunchKernelGGL((clm_sim_grad_kernel<4, BLOCK_IS_P>), grid, dim3(256), sh, st, blk, ldk, str, lds, HW, C, it, m, l, g, D, out, ldo);
  else if (C <= 256) hipLaunchKernelGGL((clm_sim_grad_kernel<8, BLOCK_IS_P>), grid, dim3(256), sh, st, blk, ldk, str, lds, HW, C, it, m, l, g, D, out, ldo);
  else hipLaunchKernelGGL((clm_sim_grad_kernel<12, BLOCK_IS_P>), grid, dim3(256), sh, st, blk, ldk, str, lds, HW, C, it, m, l, g, D, out, ldo);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_clm_sim_colsum_bwd(const float* yt, int ldy, const float* yrt, int ldr, const float* m, const float* l, const float* g, int B,
                                      int HW, int C, float temperature, float* dyt, int lddyt, float* dyr, int lddyr, void* ws, size_t ws_bytes,
                                      clc_stream_t stream) {
  if (sim_args_ok("clc_clm_sim_colsum_bwd", yt, ldy, yrt, ldr, B, HW, C, temperature) < 0) return -1;
  CLC_CHECK(m && l && g && (!dyt || lddyt >= C) && (!dyr || lddyr >= C), "clc_clm_sim_colsum_bwd: bad args");
  CLC_CHECK(ws && ws_bytes >= clc_clm_sim_colsum_bwd_workspace_bytes(B, HW), "clc_clm_sim_colsum_bwd: workspace too small");
  if (!dyt && !dyr) return 0;
  float* D = (float*)ws;
  const float it = 1.f / temperature;
  hipLaunchKernelGGL(clm_rowsum_kernel<1>, dim3((HW + 31) / 32, B), dim3(256), sim_lds_bytes(C, false), ST, yt, ldy, yrt, ldr, HW, C, it, m, l, g, D);
  CLC_LAUNCH_CHECK();
  if (dyt && launch_sim_grad<true>(yt, ldy, yrt, ldr, B, HW, C, it, m, l, g, D, dyt, lddyt, ST) < 0) return -2;
  if (dyr && launch_sim_grad<false>(yrt, ldr, yt, ldy, B, HW, C, it, m, l, g, D, dyr, lddyr, ST) < 0) return -2;
  return 0;
}

extern "C" int clc_clm_sigmoid(const float* x, int ldx, float* out, int ldo, long rows, int C, clc_stream_t stream) {
  CLC_CHECK(x && out && rows > 0 && C > 0 && ldx >= C && ldo >= C, "clc_clm_sigmoid: bad args");
  hipLaunchKernelGGL(clm_sigmoid_kernel, dim3(grid_for(rows * C)), dim3(256), 0, ST, x, ldx, out, ldo, rows, C);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_clm_scale_rows_bwd(const float* d, int ldd, const float* x, int ldx, const float* w, float* dw, float* dx, int lddx, long rows, int C,
                                      clc_stream_t stream) {
  CLC_CHECK(d && x && w && rows > 0 && C > 0 && (dw || dx), "clc_clm_scale_rows_bwd: bad args");
  hipLaunchKernelGGL(clm_scale_rows_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ST, d, ldd, x, ldx, w, dw, dx, lddx, rows, C);
  CLC_LAUNCH_CHECK();
  return 0;
}

// counters [2n] | start [n + 1, padded to 4] | ids [36n] x 2 | coefficients [36n] x 2
extern "C" size_t clc_clm_deform_bwd_workspace_bytes(int B, int H, int W) {
  const size_t n = (size_t)B * H * W;
  return (2 * n + ((n + 1 + 3) & ~(size_t)3) + 4 * 36 * n) * 4;
}

extern "C" int clc_clm_deform_bwd(const float* x, int ldx, const float* offset, int ldo, const float* modulation, int ldm, const float* da, int lda,
                                  float* doff, int lddo, float* dlogit, int lddl, float* dx, int lddx, int B, int H, int W, int C, void* ws,
                                  size_t ws_bytes, clc_stream_t stream) {
  CLC_CHECK(x && offset && modulation && da && B > 0 && H > 0 && W > 0 && C > 0, "clc_clm_deform_bwd: bad args");
  CLC_CHECK(ldo >= 18 && ldm >= 9 && (!doff || lddo >= 18) && (!dlogit || lddl >= 9) && (!doff == !dlogit), "clc_clm_deform_bwd: offset needs 18 and modulation 9 channels");
  const long n = (long)B * H * W;
  CLC_CHECK(n * 36 < (1l << 31), "clc_clm_deform_bwd: B*H*W=%ld too large", n);
  if (doff) {
    hipLaunchKernelGGL(clm_deform_bwd_param_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ST, x, ldx, offset, ldo, modulation, ldm, da, lda, doff,
                       lddo, dlogit, lddl, B, H, W, C);
    CLC_LAUNCH_CHECK();
  }
  if (dx) {
    CLC_CHECK(ws && ws_bytes >= clc_clm_deform_bwd_workspace_bytes(B, H, W), "clc_clm_deform_bwd: workspace too small");
    int* cnt = (int*)ws;
    int* cur = cnt + n;
    int* start = cur + n;
    int* ids = start + ((n + 1 + 3) & ~3l);
    int* ids_s = ids + 36 * n;
    float* coef = (float*)(ids_s + 36 * n);
    float* coef_s = coef + 36 * n;
    if (hipMemsetAsync(cnt, 0, (size_t)2 * n * sizeof(int), ST) != hipSuccess) { clc_set_error("clc_clm_deform_bwd: memset failed"); return -2; }
    hipLaunchKernelGGL(clm_deform_bucket_kernel<0>, dim3(grid_for(n * 9)), dim3(256), 0, ST, offset, ldo, modulation, ldm, B, H, W, cnt, (const int*)nullptr,
                       (int*)nullptr, (float*)nullptr);
    CLC_LAUNCH_CHECK();
    hipLaunchKernelGGL(clm_scan_kernel, dim3(1), dim3(1024), 0, ST, (const int*)cnt, start, n);
    CLC_LAUNCH_CHECK();
    hipLaunchKernelGGL(clm_deform_bucket_kernel<1>, dim3(grid_for(n * 9)), dim3(256), 0, ST, offset, ldo, modulation, ldm, B, H, W, cur, (const int*)start,
                       ids, coef);
    CLC_LAUNCH_CHECK();
    hipLaunchKernelGGL(clm_bucket_sort_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ST, (const int*)start, (const int*)ids, (const float*)coef, ids_s,
                       coef_s, n);
    CLC_LAUNCH_CHECK();
    hipLaunchKernelGGL(clm_deform_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ST, (const int*)start, (const int*)ids_s, (const float*)coef_s,
                       da, lda, dx, lddx, n, C);
    CLC_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int clc_clm_fuse_bwd(const float* const* feats, const float* const* atts, int M, int ldf, int lda, const float* dout, int lddo,
                                float* const* dfeats, int lddf, float* const* datts, int ldda, long rows, int C, int gate, clc_stream_t stream) {
  CLC_CHECK(feats && atts && dout && dfeats && datts && M > 0 && M <= 8 && rows > 0 && C > 0 && ldda >= 1, "clc_clm_fuse_bwd: bad args (M must be 1..8)");
  FuseBwdPtrs P;
  for (int m = 0; m < 8; ++m) {
    P.feat[m] = m < M ? feats[m] : nullptr; P.att[m] = m < M ? atts[m] : nullptr;
    P.dfeat[m] = m < M ? dfeats[m] : nullptr; P.datt[m] = m < M ? datts[m] : nullptr;
  }
  hipLaunchKernelGGL(clm_fuse_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ST, P, M, ldf, lda, dout, lddo, lddf, ldda, rows, C, gate);
  CLC_LAUNCH_CHECK();
  return 0;
}
