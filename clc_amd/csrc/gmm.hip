// gmm.hip — the discretised Gaussian-mixture entropy model of cheng2020 (Cheng et al., CVPR 2020; models.Cheng2020Anchor / Cheng2020Attention
// with K > 1) on gfx950: the likelihood with its gradients for training, and the table-free coder's per-symbol integer CDF rows.
//
// Every latent element has its own K weights, means and scales, so none of the coders' 64-row scale table applies: the likelihood is
//   lik = max(sum_k softmax(w)_k [Phi((1/2 - |v - mu_k|) / s_k) - Phi((-1/2 - |v - mu_k|) / s_k)], 1e-9),   s_k = max(scale_k, 0.11)
// (per component the expression of gauss_lik_fwd_kernel, entropy.hip), and the coder builds, per element, the integer CDF row of
// include/clc_hip.h ("THE ROW RULE") on the device.  Encoder and decoder run the SAME scan (gmm_finish_kernel, one loop for both modes)
// on the same parameter floats, so their rows are equal bit for bit.
//
// Parameter layout: three groups (scales, means, weight logits), each K blocks of C channels (block k of a group at channel k * C), given
// as three base pointers and ONE leading dimension — channel ranges of the single map entropy_parameters writes are read in place, and
// the backward writes the three gradient groups into ranges of one gradient map.
//
// The likelihood kernels stream each map once (HBM-bound; 2 K erfc per element forward); one thread owns 4 consecutive channels of a
// pixel (16-byte loads and stores) when C % 4 == 0 and everything is aligned, else one channel.  The coder kernels own one element per
// thread and scan its row with scalars, storing as they go: no per-thread array indexed at run time, no scratch.  All stream-ordered,
// allocation- and sync-free, graph-capturable; no LDS, no barrier, nothing waits on another workgroup.
#include "coder_device.h"

namespace {
using namespace coder;

constexpr float kLikBound = 1e-9f;
constexpr int kR = CLC_GMM_R, kL = 2 * CLC_GMM_R + 1, kStride = CLC_GMM_ROW_STRIDE;
constexpr float kS = (float)(65535 - kL);
constexpr float kCtrBound = 1048576.f;    // 2^20: centre - R + j - 1/2 stays exact in f32, and every int32 expression stays far from overflow
constexpr float kSymBound = 16777216.f;   // 2^24: the escape payload 2 |sym - offset| stays below 2^27 (8 nibbles carry 32 bits)

template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&o)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
  } else {
    o[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&o)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<f32x4*>(p) = (f32x4){o[0], o[1], o[2], o[3]};
  } else {
    p[0] = o[0];
  }
}

template <int K>
__device__ __forceinline__ void softmax(const float (&lg)[K], float (&pi)[K]) {
  float mx = lg[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, lg[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) { pi[k] = expf(lg[k] - mx); sum += pi[k]; }
#pragma unroll
  for (int k = 0; k < K; ++k) pi[k] = pi[k] / sum;
}

struct GmmLikArgs {
  const float* y; int ldy;
  const float* noise; int ldn;
  const float *sc, *mu, *wt; int ldp;
  float* lik; int ldl;
  const float* dlik; int lddl;
  float* dy; int lddy;
  float *dsc, *dmu, *dwt; int lddp;
  long rows; int C, mode;
};

// mode 0: v = y + noise (training); mode 1: v = round(y) (eval).  BWD: the gradients instead of the likelihood.
template <int K, int V, bool BWD>
__global__ __launch_bounds__(256) void gmm_lik_kernel(const GmmLikArgs a) {
  const int cv = a.C / V;
  const long total = a.rows * cv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / cv;
    const int c = (int)(i - r * cv) * V;
    float v[V], t[V], sc[K][V], mu[K][V], lg[K][V];
    ldv<V>(a.y + r * a.ldy + c, v);
    if (a.mode == 0) {
      ldv<V>(a.noise + r * a.ldn + c, t);
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] += t[e];
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = rintf(v[e]);   // torch.round: half to even
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ldv<V>(a.sc + r * a.ldp + k * a.C + c, sc[k]);
      ldv<V>(a.mu + r * a.ldp + k * a.C + c, mu[k]);
      ldv<V>(a.wt + r * a.ldp + k * a.C + c, lg[k]);
    }
    float g[V], out[V], dsc[K][V], dmu[K][V], dwt[K][V];
    if constexpr (BWD) ldv<V>(a.dlik + r * a.lddl + c, g);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float lge[K], pi[K], lk[K], av[K], bv[K], sg[K], d[K];
#pragma unroll
      for (int k = 0; k < K; ++k) lge[k] = lg[k][e];
      softmax<K>(lge, pi);
      float l = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        sg[k] = fmaxf(sc[k][e], kScaleBound);
        d[k] = v[e] - mu[k][e];
        const float ad = fabsf(d[k]);
        av[k] = (0.5f - ad) / sg[k];
        bv[k] = (-0.5f - ad) / sg[k];
        lk[k] = std_cum(av[k]) - std_cum(bv[k]);
        l += pi[k] * lk[k];
      }
      if constexpr (!BWD) {
        out[e] = fmaxf(l, kLikBound);
      } else {
        float ge = g[e];
        if (!(l >= kLikBound || ge < 0.f)) ge = 0.f;   // LowerBound(lik, 1e-9): pass if lik >= bound or grad < 0
        float gy = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float pa = kInvSqrt2Pi * expf(-0.5f * av[k] * av[k]), pb = kInvSqrt2Pi * expf(-0.5f * bv[k] * bv[k]);
          const float gp = ge * pi[k];
          float gs = gp * ((pb * bv[k] - pa * av[k]) / sg[k]);   // d/dsg [Phi(a) - Phi(b)], da/dsg = -a/sg
          if (!(sc[k][e] >= kScaleBound || gs < 0.f)) gs = 0.f;  // LowerBound(scale, 0.11)
          dsc[k][e] = gs;
          const float sgn = d[k] > 0.f ? 1.f : (d[k] < 0.f ? -1.f : 0.f);
          const float gv = gp * ((pb - pa) / sg[k]) * sgn;
          dmu[k][e] = -gv;
          gy += gv;
          dwt[k][e] = gp * (lk[k] - l);   // softmax: d lik / d logit_k = pi_k (l_k - lik)
        }
        out[e] = gy;
      }
    }
    if constexpr (!BWD) {
      stv<V>(a.lik + r * a.ldl + c, out);
    } else {
      if (a.dy) stv<V>(a.dy + r * a.lddy + c, out);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        stv<V>(a.dsc + r * a.lddp + k * a.C + c, dsc[k]);
        stv<V>(a.dmu + r * a.lddp + k * a.C + c, dmu[k]);
        stv<V>(a.dwt + r * a.lddp + k * a.C + c, dwt[k]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the coder
// The mixture CDF at x, sent into [0, 1] by comparisons that put a NaN at 0.
template <int K>
__device__ __forceinline__ float gmm_cdf(float x, const float (&pi)[K], const float (&mu)[K], const float (&sg)[K]) {
  float f = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) f += pi[k] * std_cum((x - mu[k]) / sg[k]);
  f = (f >= 0.f) ? f : 0.f;
  return (f <= 1.f) ? f : 1.f;
}

__device__ __forceinline__ float clamp_fixed(float v, float bound) {   // NaN -> -bound
  v = (v >= -bound) ? v : -bound;
  return (v <= bound) ? v : bound;
}

// The parameters of one element's row, from its 3 K floats at g (stride N between a group's blocks): the mixture and -> offset = ctr - R.
// The encoder's scan and the device decoder both call this, so their rows start from the same bits.
template <int K>
__device__ __forceinline__ int gmm_row_params(const float* g, int N, float (&pi)[K], float (&mu)[K], float (&sg)[K]) {
  float lg[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sg[k] = fmaxf(g[k * N], kScaleBound);
    mu[k] = g[(K + k) * N];
    lg[k] = g[(2 * K + k) * N];
  }
  softmax<K>(lg, pi);
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) m += pi[k] * mu[k];
  const int ctr = (int)clamp_fixed(rintf(m), kCtrBound);
  return ctr - kR;
}

struct GmmFinArgs {
  const float* gp; int ldg;
  int N;
  const int32_t* pix; int P, H, W;
  const float* y; int ldy;
  float* y_hat; int ldh;
  int32_t* triples;   // encode
  int32_t* cdf_rows;  // decode
  int32_t* offsets;   // decode
  int mode;
  long rows;
};

template <int K>
__global__ __launch_bounds__(256) void gmm_finish_kernel(const GmmFinArgs a) {
  const long total = a.rows * a.N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / a.N;
    const int c = (int)(i - r * a.N);
    const float* g = a.gp + r * a.ldg + c;
    float pi[K], mu[K], sg[K];
    const int offset = gmm_row_params<K>(g, a.N, pi, mu, sg);
    int value = 0;   // encode: the symbol's place in the row; < 0 or >= kL: escaped
    if (a.mode == CLC_AR_ENCODE) {
      const int b = (int)(r / a.P), p = (int)(r - (long)b * a.P);
      const long px = pixel_of(a.pix, p, b, a.H, a.W);
      if (px < 0) continue;   // a pixel outside the map is neither read nor written
      const int sym = (int)clamp_fixed(rintf(a.y[px * a.ldy + c]), kSymBound);
      a.y_hat[px * a.ldh + c] = (float)sym;
      value = sym - offset;
    } else {
      a.offsets[i] = offset;
    }
    // THE ROW RULE: one scan for both modes.  G is the running maximum of the sanitised mixture CDF at the edges offset + j - 1/2.
    int32_t* row = a.mode == CLC_AR_ENCODE ? nullptr : a.cdf_rows + i * kStride;
    const float g0 = gmm_cdf<K>((float)offset - 0.5f, pi, mu, sg);
    float gmax = g0;
    int lo = 0, hi = 0, cdf_j = 0;   // lo = cdf[value], hi = cdf[value + 1] of a symbol inside the row
    if (row) row[0] = 0;
#pragma unroll 1
    for (int j = 1; j <= kL; ++j) {
      const float f = gmm_cdf<K>((float)(offset + j) - 0.5f, pi, mu, sg);
      gmax = (f > gmax) ? f : gmax;
      cdf_j = j + (int)floorf((gmax - g0) * kS);
      if (row) row[j] = cdf_j;
      lo = (j == value) ? cdf_j : lo;
      hi = (j == value + 1) ? cdf_j : hi;
    }
    if (row) {
      row[kL + 1] = 65536;
      continue;
    }
    int start, freq, esc = -1;
    if (value < 0) {
      esc = -2 * value - 1;
      start = cdf_j; freq = 65536 - cdf_j;   // (cdf_j is cdf[kL] here: the tail symbol)
    } else if (value >= kL) {
      esc = 2 * (value - kL);
      start = cdf_j; freq = 65536 - cdf_j;
    } else {
      start = lo; freq = hi - lo;   // (value == 0: lo stays cdf[0] = 0)
    }
    a.triples[3 * i] = start;
    a.triples[3 * i + 1] = freq;
    a.triples[3 * i + 2] = esc;
  }
}

__global__ __launch_bounds__(256) void gmm_commit_kernel(const int32_t* __restrict__ symbols, int N, const int32_t* __restrict__ pix, int P, int H, int W,
                                                       float* __restrict__ y_hat, int ldh, long rows) {
  const long total = rows * N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / N;
    const int c = (int)(i - r * N);
    const int b = (int)(r / P), p = (int)(r - (long)b * P);
    const long px = pixel_of(pix, p, b, H, W);
    if (px < 0) continue;
    y_hat[px * ldh + c] = (float)symbols[i];
  }
}

// ---------------------------------------------------------------------------------------------------- the split stream's device decoder
// One wave per (image, sub-stream): the rANS state and every branch are wave-uniform, the 64 lanes share the work of ONE symbol's row
// (lane l owns edge j = l; the edges 64 and 65 are evaluated beside them and kept by every lane), and the symbol is found by a ballot.
// No row is written anywhere, nothing is read back by the host: see include/clc_hip.h (clc_gmm_decode_step) for the procedure.
struct GmmDecArgs {
  const float* gp; int ldg;
  int N;
  const int32_t* pix; int P, B, H, W;
  const uint32_t* words;
  const int32_t* spans;
  uint32_t* state;   // per (b, s): x low, x high, pos, pad
  int S;
  float* y_hat; int ldh;
};

struct SubStream {
  WordSpan span;   // the sub-stream's words
  uint32_t pos;
  uint64_t x;
  __device__ __forceinline__ void renorm() {   // rans_host.cpp: one word when x < 2^31, zeros at or past the end
    if (x < (1ull << 31)) {
      const uint32_t v = span.word(pos);
      ++pos;
      x = (x << 32) | v;
    }
  }
  __device__ __forceinline__ uint32_t get_bits() {
    const uint32_t v = (uint32_t)x & 15u;
    x >>= 4;
    renorm();
    return v;
  }
};

template <int K>
__global__ __launch_bounds__(256) void gmm_decode_kernel(const GmmDecArgs a) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);   // (b, s); the last workgroup's spare waves leave
  if (wid >= a.B * a.S) return;
  const int b = wid / a.S, s = wid - b * a.S;
  uint32_t* st = a.state + 4 * (long)wid;
  SubStream d;
  d.span.open(a.words, a.spans, wid);
  d.x = (uint64_t)st[0] | ((uint64_t)st[1] << 32);
  d.pos = st[2];
#pragma unroll 1
  for (int p = 0; p < a.P; ++p) {
    const long px = pixel_of(a.pix, p, b, a.H, a.W);
    if (px < 0) continue;   // neither read nor written, consumes nothing
    const float* grow = a.gp + ((long)b * a.P + p) * a.ldg;
    float* out = a.y_hat + px * a.ldh;
#pragma unroll 1
    for (int c = s; c < a.N; c += a.S) {
      float pi[K], mu[K], sg[K];
      const int offset = gmm_row_params<K>(grow + c, a.N, pi, mu, sg);
      // the 66 edges: j = lane, and j = 64 + (lane & 1), of which lanes 0 and 1 hold the two that count
      const float f = gmm_cdf<K>((float)(offset + lane) - 0.5f, pi, mu, sg);
      const float fx = gmm_cdf<K>((float)(offset + 64 + (lane & 1)) - 0.5f, pi, mu, sg);
      float g = f;   // -> G_lane, the inclusive running maximum
#pragma unroll
      for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const float t = __shfl_up(g, dlt);
        g = (lane >= dlt && t > g) ? t : g;
      }
      const float g0 = __shfl(g, 0), f64 = __shfl(fx, 0), f65 = __shfl(fx, 1);
      float gt = __shfl(g, 63);
      gt = (f64 > gt) ? f64 : gt;
      const int cdf64 = 64 + (int)floorf((gt - g0) * kS);
      gt = (f65 > gt) ? f65 : gt;
      const int cdf65 = 65 + (int)floorf((gt - g0) * kS);   // (kL == 65)
      const int cdf_l = lane + (int)floorf((g - g0) * kS);
      // the symbol
      const uint32_t cf = (uint32_t)d.x & 0xFFFFu;
      const unsigned long long below = __ballot(lane >= 1 && (uint32_t)cdf_l <= cf);
      const int v = __popcll(below) + ((uint32_t)cdf64 <= cf ? 1 : 0) + ((uint32_t)cdf65 <= cf ? 1 : 0);   // 0 .. kL
      const int lo_l = __shfl(cdf_l, v & 63), hi_l = __shfl(cdf_l, (v + 1) & 63);
      const int start = v < 64 ? lo_l : (v == 64 ? cdf64 : cdf65);
      const int end = v < 63 ? hi_l : (v == 63 ? cdf64 : (v == 64 ? cdf65 : 65536));
      d.x = (uint64_t)(uint32_t)(end - start) * (d.x >> 16) + cf - (uint32_t)start;
      d.renorm();
      uint32_t value = (uint32_t)v;
      if (v == kL) {   // the tail: the bypass escape of clc_rans_decoder_decode, every loop bounded
        uint32_t nb = d.get_bits();
        if (nb == 15u) nb += d.get_bits();
        nb = nb < 16u ? nb : 16u;
        uint32_t raw = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < nb; ++j) {
          const uint32_t bits = d.get_bits();
          if (j < 8) raw |= bits << (4 * j);
        }
        value = raw >> 1;
        value = (raw & 1u) ? ~value : value + (uint32_t)kL;   // (-value - 1 == ~value)
      }
      if (lane == 0) out[c] = (float)(int32_t)(value + (uint32_t)offset);
    }
  }
  if (lane == 0) {
    st[0] = (uint32_t)d.x;
    st[1] = (uint32_t)(d.x >> 32);
    st[2] = d.pos;
  }
}

int grid_of(long total) { return (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

template <int V, bool BWD>
void launch_lik(const GmmLikArgs& a, int K, hipStream_t st) {
  const dim3 grid(grid_of(a.rows * (a.C / V))), block(256);
  switch (K) {
    case 1: hipLaunchKernelGGL((gmm_lik_kernel<1, V, BWD>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((gmm_lik_kernel<2, V, BWD>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((gmm_lik_kernel<3, V, BWD>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((gmm_lik_kernel<4, V, BWD>), grid, block, 0, st, a); break;
  }
}

bool vec_ok(const GmmLikArgs& a, bool bwd) {
  bool ok = a.C % 4 == 0 && a.ldy % 4 == 0 && a.ldp % 4 == 0 && aligned16(a.y) && aligned16(a.sc) && aligned16(a.mu) && aligned16(a.wt);
  if (a.noise) ok = ok && a.ldn % 4 == 0 && aligned16(a.noise);
  if (!bwd) return ok && a.ldl % 4 == 0 && aligned16(a.lik);
  ok = ok && a.lddl % 4 == 0 && aligned16(a.dlik) && a.lddp % 4 == 0 && aligned16(a.dsc) && aligned16(a.dmu) && aligned16(a.dwt);
  if (a.dy) ok = ok && a.lddy % 4 == 0 && aligned16(a.dy);
  return ok;
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int clc_gmm_half_width(void) { return kR; }

extern "C" int clc_gmm_likelihood_fwd(const float* y, int ldy, const float* noise, int ldn, const float* scales, const float* means, const float* weights,
                                      int ldp, float* lik, int ldl, long rows, int C, int K, int mode, clc_stream_t stream) {
  CLC_CHECK(y && scales && means && weights && lik, "clc_gmm_likelihood_fwd: null pointer");
  CLC_CHECK(K >= 1 && K <= 4, "clc_gmm_likelihood_fwd: K must be between 1 and 4 (got %d)", K);
  CLC_CHECK(rows > 0 && C > 0, "clc_gmm_likelihood_fwd: rows and C must be positive");
  CLC_CHECK(mode == 0 || mode == 1, "clc_gmm_likelihood_fwd: mode must be 0 (noise) or 1 (round) (got %d)", mode);
  CLC_CHECK(mode == 1 || noise, "clc_gmm_likelihood_fwd: mode 0 needs the noise map");
  CLC_CHECK(ldy >= C && ldl >= C && (mode == 1 || ldn >= C), "clc_gmm_likelihood_fwd: ldy, ldn or ldl < C");
  CLC_CHECK(ldp >= K * C, "clc_gmm_likelihood_fwd: ldp < K C (a parameter group is K blocks of C channels)");
  GmmLikArgs a = {};
  a.y = y; a.ldy = ldy; a.noise = mode == 0 ? noise : nullptr; a.ldn = ldn; a.sc = scales; a.mu = means; a.wt = weights; a.ldp = ldp;
  a.lik = lik; a.ldl = ldl; a.rows = rows; a.C = C; a.mode = mode;
  if (vec_ok(a, false)) launch_lik<4, false>(a, K, ST); else launch_lik<1, false>(a, K, ST);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_gmm_likelihood_bwd(const float* dlik, int lddl, const float* y, int ldy, const float* noise, int ldn, const float* scales,
                                      const float* means, const float* weights, int ldp, float* dy, int lddy, float* dscales, float* dmeans,
                                      float* dweights, int lddp, long rows, int C, int K, int mode, clc_stream_t stream) {
  CLC_CHECK(dlik && y && scales && means && weights && dscales && dmeans && dweights, "clc_gmm_likelihood_bwd: null pointer");
  CLC_CHECK(K >= 1 && K <= 4, "clc_gmm_likelihood_bwd: K must be between 1 and 4 (got %d)", K);
  CLC_CHECK(rows > 0 && C > 0, "clc_gmm_likelihood_bwd: rows and C must be positive");
  CLC_CHECK(mode == 0 || mode == 1, "clc_gmm_likelihood_bwd: mode must be 0 (noise) or 1 (round) (got %d)", mode);
  CLC_CHECK(mode == 1 || noise, "clc_gmm_likelihood_bwd: mode 0 needs the noise map");
  CLC_CHECK(mode == 0 || !dy, "clc_gmm_likelihood_bwd: mode 1 has no gradient of y (v = round(y)); pass dy = NULL");
  CLC_CHECK(ldy >= C && lddl >= C && (mode == 1 || ldn >= C) && (!dy || lddy >= C), "clc_gmm_likelihood_bwd: ldy, ldn, lddl or lddy < C");
  CLC_CHECK(ldp >= K * C && lddp >= K * C, "clc_gmm_likelihood_bwd: ldp or lddp < K C (a parameter group is K blocks of C channels)");
  GmmLikArgs a = {};
  a.y = y; a.ldy = ldy; a.noise = mode == 0 ? noise : nullptr; a.ldn = ldn; a.sc = scales; a.mu = means; a.wt = weights; a.ldp = ldp;
  a.dlik = dlik; a.lddl = lddl; a.dy = dy; a.lddy = lddy; a.dsc = dscales; a.dmu = dmeans; a.dwt = dweights; a.lddp = lddp;
  a.rows = rows; a.C = C; a.mode = mode;
  if (vec_ok(a, true)) launch_lik<4, true>(a, K, ST); else launch_lik<1, true>(a, K, ST);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_gmm_finish(const float* gp, int ldg, int N, int K, const int32_t* pix, int P, int B, int H, int W, const float* y, int ldy, float* y_hat,
                              int ldh, int32_t* triples, int32_t* cdf_rows, int32_t* offsets, int mode, clc_stream_t stream) {
  CLC_CHECK(gp && pix, "clc_gmm_finish: null pointer");
  CLC_CHECK(mode == CLC_AR_ENCODE || mode == CLC_AR_DECODE, "clc_gmm_finish: mode must be CLC_AR_ENCODE or CLC_AR_DECODE (got %d)", mode);
  CLC_CHECK(K >= 1 && K <= 4, "clc_gmm_finish: K must be between 1 and 4 (got %d)", K);
  CLC_CHECK(P > 0 && B > 0 && H > 0 && W > 0 && N > 0, "clc_gmm_finish: P, B, H, W and N must be positive");
  CLC_CHECK((long)ldg >= 3l * K * N, "clc_gmm_finish: ldg < 3 K N (scales, means, weight logits: K blocks of N channels each)");
  CLC_CHECK((long)B * H * W < (1l << 31), "clc_gmm_finish: B * H * W must be below 2^31");
  if (mode == CLC_AR_ENCODE)
    CLC_CHECK(y && y_hat && triples && ldy >= N && ldh >= N, "clc_gmm_finish: encode mode needs y, y_hat, triples and ldy, ldh >= N");
  else
    CLC_CHECK(cdf_rows && offsets, "clc_gmm_finish: decode mode needs cdf_rows and offsets");
  GmmFinArgs a = {};
  a.gp = gp; a.ldg = ldg; a.N = N; a.pix = pix; a.P = P; a.H = H; a.W = W; a.y = y; a.ldy = ldy; a.y_hat = y_hat; a.ldh = ldh;
  a.triples = triples; a.cdf_rows = cdf_rows; a.offsets = offsets; a.mode = mode; a.rows = (long)B * P;
  const dim3 grid(grid_of(a.rows * N)), block(256);
  switch (K) {
    case 1: hipLaunchKernelGGL(gmm_finish_kernel<1>, grid, block, 0, ST, a); break;
    case 2: hipLaunchKernelGGL(gmm_finish_kernel<2>, grid, block, 0, ST, a); break;
    case 3: hipLaunchKernelGGL(gmm_finish_kernel<3>, grid, block, 0, ST, a); break;
    default: hipLaunchKernelGGL(gmm_finish_kernel<4>, grid, block, 0, ST, a); break;
  }
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_gmm_commit(const int32_t* symbols, int N, const int32_t* pix, int P, int B, int H, int W, float* y_hat, int ldh, clc_stream_t stream) {
  CLC_CHECK(symbols && pix && y_hat, "clc_gmm_commit: null pointer");
  CLC_CHECK(P > 0 && B > 0 && H > 0 && W > 0 && N > 0, "clc_gmm_commit: P, B, H, W and N must be positive");
  CLC_CHECK(ldh >= N, "clc_gmm_commit: ldh < N");
  CLC_CHECK((long)B * H * W < (1l << 31), "clc_gmm_commit: B * H * W must be below 2^31");
  const long rows = (long)B * P;
  hipLaunchKernelGGL(gmm_commit_kernel, dim3(grid_of(rows * N)), dim3(256), 0, ST, symbols, N, pix, P, H, W, y_hat, ldh, rows);
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_gmm_decode_step(const float* gp, int ldg, int N, int K, const int32_t* pix, int P, int B, int H, int W, const uint32_t* words,
                                   const int32_t* spans, clc_gmm_substream_state* state, int S, float* y_hat, int ldh, clc_stream_t stream) {
  static_assert(kL == 65 && sizeof(clc_gmm_substream_state) == 16, "gmm_decode_kernel: 64 lanes and two extra edges; a 16-byte state");
  CLC_CHECK(gp && pix && words && spans && state && y_hat, "clc_gmm_decode_step: null pointer");
  CLC_CHECK(K >= 1 && K <= 4, "clc_gmm_decode_step: K must be between 1 and 4 (got %d)", K);
  CLC_CHECK(P > 0 && B > 0 && H > 0 && W > 0 && N > 0, "clc_gmm_decode_step: P, B, H, W and N must be positive");
  CLC_CHECK(S >= 1 && S <= 64, "clc_gmm_decode_step: S must be between 1 and 64 sub-streams (got %d)", S);
  CLC_CHECK(S <= N, "clc_gmm_decode_step: S > N (%d sub-streams for %d channels: channel c belongs to sub-stream c mod S)", S, N);
  CLC_CHECK((long)ldg >= 3l * K * N, "clc_gmm_decode_step: ldg < 3 K N (scales, means, weight logits: K blocks of N channels each)");
  CLC_CHECK(ldh >= N, "clc_gmm_decode_step: ldh < N");
  CLC_CHECK((long)B * H * W < (1l << 31), "clc_gmm_decode_step: B * H * W must be below 2^31");
  CLC_CHECK((long)B * S < (1l << 24), "clc_gmm_decode_step: B * S must be below 2^24");
  GmmDecArgs a = {};
  a.gp = gp; a.ldg = ldg; a.N = N; a.pix = pix; a.P = P; a.B = B; a.H = H; a.W = W; a.words = words; a.spans = spans;
  a.state = reinterpret_cast<uint32_t*>(state); a.S = S; a.y_hat = y_hat; a.ldh = ldh;
  const dim3 grid((B * S + 3) / 4), block(256);
  switch (K) {
    case 1: hipLaunchKernelGGL(gmm_decode_kernel<1>, grid, block, 0, ST, a); break;
    case 2: hipLaunchKernelGGL(gmm_decode_kernel<2>, grid, block, 0, ST, a); break;
    case 3: hipLaunchKernelGGL(gmm_decode_kernel<3>, grid, block, 0, ST, a); break;
    default: hipLaunchKernelGGL(gmm_decode_kernel<4>, grid, block, 0, ST, a); break;
  }
  CLC_LAUNCH_CHECK();
  return 0;
}
