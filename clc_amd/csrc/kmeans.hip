// kmeans.hip — full-batch Lloyd k-means on gfx950: the clustering that thins the reference-retrieval dictionary (clc_amd/kmeans.py,
// ReferenceIndex.cluster_features(method="device")).  x = [N][D] f32 rows (leading dimension ldx), c = [K][D] centres.
//
//   kmeans_assign_kernel    label[i] = argmin_k (|c_k|^2 - 2 x_i.c_k), score[i] = that minimum.  A blocked GEMM on
//                           v_mfma_f32_32x32x2_f32: a workgroup owns 128 points and walks the centre tiles (128 centres each); both
//                           operands go through [rows][32 + 4] LDS images in D-chunks of 32 (two stages: the global loads of chunk
//                           s + 1 are in registers while chunk s multiplies).  CENTRES are the A operand and POINTS the B operand, so
//                           a result tile has its point on the lane and its 16 centres in the accumulator registers: the running
//                           (min, index) of a point is a per-LANE fold over registers and centre tiles in ascending centre order
//                           (strict <: the lowest index keeps a tie).  The four partial minima of a point (2 centre halves of the
//                           tile x 2 lane halves) are merged at the end under (score, index) lexicographic order, which does not
//                           depend on the merge order.  The [N][K] matrix is never written; no atomics.
//   kmeans_bounds / scan    the inverted index from a STABLE ordering of the labels (order[] = row indices sorted by label, rows of one
//                           label ascending): start[k] = first position of cluster k, by run boundaries, every entry written once.
//   kmeans_partial_kernel   member lists are cut into chunks of 512 rows; one wave per chunk sums its rows in list order, lanes over
//                           columns -> partial[chunk][D].
//   kmeans_finalize_kernel  one wave per cluster adds its partials in chunk order and divides by the count; an empty cluster copies
//                           its previous centre.
//   kmeans_rep_kernel       one wave per cluster: sum_d (x - c)^2 of each member in list order, strict < keeps the first minimum.
// Every floating-point sum has an order fixed by (labels, N, K, D) alone: the same bits on every run.
#include "common.h"

namespace {

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int kPT = 128;                          // points per workgroup
constexpr int kCT = 128;                          // centres per tile
constexpr int kKC = 32;                           // D-chunk
constexpr int kPitch = kKC + 4;                   // LDS row pitch: 16-lane b128 reads of 16 rows hit 64 different banks
constexpr int kStage = (kPT + kCT) * kPitch;      // floats per stage
constexpr int kAssignLds = 2 * kStage * 4;        // 73 728 B: two workgroups per CU
constexpr int kChunkRows = 512;                   // members per partial sum

__device__ __forceinline__ int row_of(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }   // C/D layout of the 32x32 MFMAs

// two waves per SIMD (two workgroups per CU): without the bound the compiler takes 260 registers and halves the occupancy
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void kmeans_assign_kernel(
    const float* __restrict__ x, int ldx, int N, int D, const float* __restrict__ c, int ldc, int K, const float* __restrict__ csq,
    int* __restrict__ label, float* __restrict__ score) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  const int wp = wave & 1, wc = wave >> 1;        // the wave's 64-point / 64-centre half of the 128 x 128 tile
  const int p0 = blockIdx.x * kPT;
  const int lrow = tid >> 3, lcol = (tid & 7) << 2;   // loader role: rows lrow + 32 i, columns lcol .. lcol + 3 of the chunk
  const int nchunk = (D + kKC - 1) / kKC, nct = (K + kCT - 1) / kCT;
  const long total = (long)nct * nchunk;

  f32x4 px[4], pc[4];
  // rows past N / K are clamped to the last valid row (they are masked in the epilogue / never stored); columns past D are zero
  auto load = [&](int ct, int kc) {
    const int k = kc * kKC + lcol;
#pragma unroll
    for (int i = 0; i < 4; ++i) px[i] = pc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (k < D) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rp = min(p0 + lrow + 32 * i, N - 1), rc = min(ct * kCT + lrow + 32 * i, K - 1);
        px[i] = *reinterpret_cast<const f32x4*>(x + (size_t)rp * ldx + k);
        pc[i] = *reinterpret_cast<const f32x4*>(c + (size_t)rc * ldc + k);
      }
    }
  };
  auto store = [&](int buf) {
    float* P = sm + buf * kStage;
    float* C = P + kPT * kPitch;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4*>(P + (lrow + 32 * i) * kPitch + lcol) = px[i];
      *reinterpret_cast<f32x4*>(C + (lrow + 32 * i) * kPitch + lcol) = pc[i];
    }
  };

  f32x16 acc[2][2];   // [centre tile of the wave][point tile of the wave]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
  float best[2] = {INFINITY, INFINITY};
  int bidx[2] = {0, 0};

  load(0, 0);
  store(0);
  __syncthreads();
  int ct = 0, kc = 0;
  for (long s = 0; s < total; ++s) {
    const int cur = (int)(s & 1);
    int nct_ = ct, nkc = kc + 1;
    if (nkc == nchunk) { nkc = 0; ++nct_; }
    const bool more = s + 1 < total;   // block-uniform
    if (more) load(nct_, nkc);
    const float* P = sm + cur * kStage + (wp * 64 + li) * kPitch + 4 * h;
    const float* C = sm + cur * kStage + (kPT + wc * 64 + li) * kPitch + 4 * h;
#pragma unroll
    for (int ks = 0; ks < kKC / 8; ++ks) {
      // lane half h takes k = 8 ks + 4 h + {0..3}: any k order serves as long as both operands use the same one
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(C + 8 * ks), a1 = *reinterpret_cast<const f32x4*>(C + 32 * kPitch + 8 * ks);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(P + 8 * ks), b1 = *reinterpret_cast<const f32x4*>(P + 32 * kPitch + 8 * ks);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0][0] = MFMA(a0[e], b0[e], acc[0][0]);
        acc[0][1] = MFMA(a0[e], b1[e], acc[0][1]);
        acc[1][0] = MFMA(a1[e], b0[e], acc[1][0]);
        acc[1][1] = MFMA(a1[e], b1[e], acc[1][1]);
      }
    }
    if (kc == nchunk - 1) {   // the centre tile is complete: fold it into the running minimum, ascending centre index
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int kb = ct * kCT + wc * 64 + a * 32;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int k = kb + row_of(i, h);
          const float cs = k < K ? csq[k] : INFINITY;   // centres past K cannot win
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const float v = cs - 2.f * acc[a][b][i];
            if (v < best[b]) { best[b] = v; bidx[b] = k; }
            acc[a][b][i] = 0.f;
          }
        }
      }
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    ct = nct_;
    kc = nkc;
  }
  // merge the 2 centre halves x 2 lane halves of every point (the stages are free after the last barrier)
  float* rs = sm;
  int* ri = reinterpret_cast<int*>(sm + 4 * kPT);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int p = wp * 64 + b * 32 + li;
    rs[(wc * 2 + h) * kPT + p] = best[b];
    ri[(wc * 2 + h) * kPT + p] = bidx[b];
  }
  __syncthreads();
  if (tid < kPT && p0 + tid < N) {   // rows past N are not stored
    float bs = rs[tid];
    int bi = ri[tid];
    for (int q = 1; q < 4; ++q) {
      const float v = rs[q * kPT + tid];
      const int i = ri[q * kPT + tid];
      if (v < bs || (v == bs && i < bi)) { bs = v; bi = i; }
    }
    label[p0 + tid] = bi;
    score[p0 + tid] = bs;
  }
}

// label of the member at position i of the ordering; anything out of range sorts as K (a bucket nobody reads)
__device__ __forceinline__ int sorted_label(const int* __restrict__ label, const int* __restrict__ order, int i, int N, int K) {
  const int r = order[i];
  if ((unsigned)r >= (unsigned)N) return K;
  const int l = label[r];
  return (unsigned)l >= (unsigned)K ? K : l;
}

// start[k] = first position whose label is >= k (k = 0..K): each entry is written by the one position that opens its run
__global__ void kmeans_bounds_kernel(const int* __restrict__ label, const int* __restrict__ order, int N, int K, int* __restrict__ start) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
    const int lab = sorted_label(label, order, (int)i, N, K);
    const int prev = i ? sorted_label(label, order, (int)i - 1, N, K) : -1;
    for (int k = prev + 1; k <= lab; ++k) start[k] = (int)i;
    if (i == N - 1)
      for (int k = lab + 1; k <= K; ++k) start[k] = N;
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// counts[k] = start[k + 1] - start[k]; cstart[0..K] = exclusive scan of the clusters' chunk counts (one workgroup; thread t owns a
// contiguous range, as clm_scan_kernel)
__global__ __launch_bounds__(1024) void kmeans_scan_kernel(const int* __restrict__ start, int N, int K, int* __restrict__ counts,
                                                           int* __restrict__ cstart) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const int per = (K + 1023) / 1024, lo = min(tid * per, K), hi = min(lo + per, K);
  int s = 0;
  for (int k = lo; k < hi; ++k) {
    const int a = clampi(start[k], 0, N), n = clampi(start[k + 1], a, N) - a;
    counts[k] = n;
    s += (n + kChunkRows - 1) / kChunkRows;
  }
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int k = lo; k < hi; ++k) {
    cstart[k] = run;
    run += (counts[k] + kChunkRows - 1) / kChunkRows;
  }
  if (tid == 1023) cstart[K] = part[1023];
}

// one wave per chunk of at most 512 members: rows in list order, lanes over columns
__global__ __launch_bounds__(256) void kmeans_partial_kernel(const float* __restrict__ x, int ldx, int N, int D, const int* __restrict__ order,
                                                             const int* __restrict__ start, const int* __restrict__ cstart, int K, int nslots,
                                                             float* __restrict__ partial) {
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (slot >= nslots || slot >= cstart[K]) return;
  int lo = 0, hi = K;   // the cluster k with cstart[k] <= slot < cstart[k + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cstart[mid] <= slot) lo = mid; else hi = mid;
  }
  const int k = lo;
  const int s0 = clampi(start[k], 0, N), s1 = clampi(start[k + 1], s0, N);
  const int r0 = min(s0 + (slot - cstart[k]) * kChunkRows, s1), r1 = min(r0 + kChunkRows, s1);
  for (int col = lane << 2; col < D; col += 256) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
      const int row = order[r];
      if ((unsigned)row < (unsigned)N) acc += *reinterpret_cast<const f32x4*>(x + (size_t)row * ldx + col);
    }
    *reinterpret_cast<f32x4*>(partial + (size_t)slot * D + col) = acc;
  }
}

// one wave per cluster: partials in chunk order, then the mean; an empty cluster keeps its previous centre
__global__ __launch_bounds__(256) void kmeans_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ counts,
                                                              const int* __restrict__ cstart, const float* __restrict__ prev, int ldp, float* __restrict__ out,
                                                              int ldo, int K, int D, int nslots) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  const int c0 = clampi(cstart[k], 0, nslots), c1 = clampi(cstart[k + 1], c0, nslots);   // (an order[] that is not sorted cannot lead outside)
  const int n = c1 > c0 ? counts[k] : 0;
  for (int col = lane << 2; col < D; col += 256) {
    f32x4 v;
    if (n == 0) {
      v = *reinterpret_cast<const f32x4*>(prev + (size_t)k * ldp + col);
    } else {
      v = *reinterpret_cast<const f32x4*>(partial + (size_t)c0 * D + col);
      for (int j = c0 + 1; j < c1; ++j) v += *reinterpret_cast<const f32x4*>(partial + (size_t)j * D + col);
      const float fn = (float)n;
      v = (f32x4){v[0] / fn, v[1] / fn, v[2] / fn, v[3] / fn};
    }
    *reinterpret_cast<f32x4*>(out + (size_t)k * ldo + col) = v;
  }
}

// one wave per cluster: the member closest to the centre, the first one in list (= row) order on a tie; -1 for an empty cluster
__global__ __launch_bounds__(256) void kmeans_rep_kernel(const float* __restrict__ x, int ldx, int N, int D, const int* __restrict__ order,
                                                         const int* __restrict__ start, const float* __restrict__ c, int ldc, int K,
                                                         int* __restrict__ rep) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  const int s0 = clampi(start[k], 0, N), s1 = clampi(start[k + 1], s0, N);
  float best = INFINITY;
  int bi = -1;
  for (int r = s0; r < s1; ++r) {
    const int row = order[r];
    if ((unsigned)row >= (unsigned)N) continue;   // wave-uniform
    float d = 0.f;
    for (int col = lane << 2; col < D; col += 256) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)row * ldx + col);
      const f32x4 cv = *reinterpret_cast<const f32x4*>(c + (size_t)k * ldc + col);
      const f32x4 t = xv - cv;
      d = fmaf(t[0], t[0], d);
      d = fmaf(t[1], t[1], d);
      d = fmaf(t[2], t[2], d);
      d = fmaf(t[3], t[3], d);
    }
    d = wave_sum(d);   // xor butterfly: every lane holds the same bits
    if (d < best || bi < 0) { best = d; bi = row; }
  }
  if (lane == 0) rep[k] = bi;
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline long max_slots(int N, int K) { return (long)K + N / kChunkRows; }   // >= sum_k ceil(n_k / 512): one per non-empty cluster + N / 512
inline bool rows_ok(const float* p, int ld, int D) { return p && aligned16(p) && ld >= D && ld % 4 == 0; }
inline int grid_for(long n) { long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int clc_kmeans_assign(const float* x, int ldx, int N, int D, const float* c, int ldc, int K, const float* c_sqnorm, int32_t* label,
                                 float* score, clc_stream_t stream) {
  CLC_CHECK(N >= 1 && D >= 4 && D % 4 == 0, "clc_kmeans_assign: N=%d D=%d (N >= 1, D >= 4 and a multiple of 4)", N, D);
  CLC_CHECK(K >= 1, "clc_kmeans_assign: K=%d must be >= 1", K);
  CLC_CHECK(rows_ok(x, ldx, D) && rows_ok(c, ldc, D), "clc_kmeans_assign: rows must be 16-byte aligned with ld >= D, ld %% 4 == 0");
  CLC_CHECK(c_sqnorm && label && score, "clc_kmeans_assign: null pointer");
  static PerDeviceOnce once;
  if (once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_assign_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kAssignLds);
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((N + kPT - 1) / kPT), dim3(256), kAssignLds, ST, x, ldx, N, D, c, ldc, K, c_sqnorm, label, score);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t clc_kmeans_update_workspace_bytes(int N, int D, int K) {
  if (N < 1 || D < 4 || K < 1 || K > N) return 0;
  return 2 * align16((size_t)(K + 1) * sizeof(int)) + (size_t)max_slots(N, K) * D * sizeof(float);
}

extern "C" int clc_kmeans_update(const float* x, int ldx, int N, int D, const int32_t* label, const int32_t* order, int K, const float* prev_c,
                                 int ldp, float* c_out, int ldc, int32_t* counts, void* ws, size_t ws_bytes, clc_stream_t stream) {
  CLC_CHECK(N >= 1 && D >= 4 && D % 4 == 0, "clc_kmeans_update: N=%d D=%d (N >= 1, D >= 4 and a multiple of 4)", N, D);
  CLC_CHECK(K >= 1 && K <= N, "clc_kmeans_update: K=%d must be in 1..N=%d", K, N);
  CLC_CHECK(rows_ok(x, ldx, D) && rows_ok(prev_c, ldp, D) && rows_ok(c_out, ldc, D),
            "clc_kmeans_update: rows must be 16-byte aligned with ld >= D, ld %% 4 == 0");
  CLC_CHECK(label && order && counts, "clc_kmeans_update: null pointer");
  CLC_CHECK(ws && aligned16(ws) && ws_bytes >= clc_kmeans_update_workspace_bytes(N, D, K), "clc_kmeans_update: workspace too small or unaligned");
  int* start = (int*)ws;
  int* cstart = (int*)((char*)ws + align16((size_t)(K + 1) * sizeof(int)));
  float* partial = (float*)((char*)ws + 2 * align16((size_t)(K + 1) * sizeof(int)));
  const long slots = max_slots(N, K);
  hipLaunchKernelGGL(kmeans_bounds_kernel, dim3(grid_for(N)), dim3(256), 0, ST, label, order, N, K, start);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_scan_kernel, dim3(1), dim3(1024), 0, ST, (const int*)start, N, K, counts, cstart);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)((slots + 3) / 4)), dim3(256), 0, ST, x, ldx, N, D, order, (const int*)start,
                     (const int*)cstart, K, (int)slots, partial);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_finalize_kernel, dim3((K + 3) / 4), dim3(256), 0, ST, (const float*)partial, (const int*)counts, (const int*)cstart, prev_c,
                     ldp, c_out, ldc, K, D, (int)slots);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t clc_kmeans_representatives_workspace_bytes(int K) { return K < 1 ? 0 : align16((size_t)(K + 1) * sizeof(int)); }

extern "C" int clc_kmeans_representatives(const float* x, int ldx, int N, int D, const int32_t* label, const int32_t* order, const float* c, int ldc,
                                          int K, int32_t* rep, void* ws, size_t ws_bytes, clc_stream_t stream) {
  CLC_CHECK(N >= 1 && D >= 4 && D % 4 == 0, "clc_kmeans_representatives: N=%d D=%d (N >= 1, D >= 4 and a multiple of 4)", N, D);
  CLC_CHECK(K >= 1 && K <= N, "clc_kmeans_representatives: K=%d must be in 1..N=%d", K, N);
  CLC_CHECK(rows_ok(x, ldx, D) && rows_ok(c, ldc, D), "clc_kmeans_representatives: rows must be 16-byte aligned with ld >= D, ld %% 4 == 0");
  CLC_CHECK(label && order && rep, "clc_kmeans_representatives: null pointer");
  CLC_CHECK(ws && aligned16(ws) && ws_bytes >= clc_kmeans_representatives_workspace_bytes(K), "clc_kmeans_representatives: workspace too small or unaligned");
  int* start = (int*)ws;
  hipLaunchKernelGGL(kmeans_bounds_kernel, dim3(grid_for(N)), dim3(256), 0, ST, label, order, N, K, start);
  CLC_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_rep_kernel, dim3((K + 3) / 4), dim3(256), 0, ST, x, ldx, N, D, order, (const int*)start, c, ldc, K, rep);
  CLC_LAUNCH_CHECK();
  return 0;
}
