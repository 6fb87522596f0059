// Integer context model: the pixel-list int8 GEMM with a tap gather — the integer sibling of clc_ar_linear's contract on the
// gfx950 i8 matrix cores, requantising epilogue fused (include/clc_hip.h: "integer context model" states the arithmetic;
// tests/intctx_ref.py is its reference).
//
// Rows are r = b * P + p over a device pixel list; the K axis is one or two ranges, each an NHWC int8 map read at the row's pixel
// ("pixel"), a dense int8 [rows][C] buffer ("dense"), or an NHWC int8 map gathered at up to 25 (dh, dw) offsets around the pixel, zero
// off the map ("taps": K = ntaps * C, tap-major).  The structure is int_conv_kernel's (int_conv.hip): ONE WAVE per 32 rows x 32 output
// channels, no LDS, no barrier; v_mfma_i32_32x32x32_i8 with A = the packed filter image [Cout / 32][K / 32][2][32][16] (a wave's
// fragment is one coalesced 1 KB load) and B = 16 consecutive channels of the row's source, one aligned 16-byte load, zero for a dead
// row and an off-map tap.  Every range's C is a multiple of 32, so a 32-wide K chunk never straddles a tap or a range.  Both operands
// are read in the same (h, j) order, so which k the hardware assigns to a lane's bytes does not matter: the sum is exact and order-free.
// C/D: column (row of the call) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 h, as in int_conv.hip.
#include "common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

namespace {

struct IntRowsSrc {
  const int8_t* p;
  int ld, kcs, kind;   // kcs = C / 32
};

struct IntRowsParams {
  IntRowsSrc src[2];
  const int32_t* pix;
  const int8_t* wp;
  const int32_t *bias, *mpos, *mneg, *shift;
  void* y;
  long rows;   // B * P
  int nsrc, P, H, W, ntaps, kcs_total, ldy;
  float out_scale;
  int taps[CLC_INT_ROWS_MAX_TAPS];   // (dh & 0xffff) | (dw << 16)
};

// r = (a * m + 2^(s - 1)) >> s with m chosen by the sign of a: 64-bit, arithmetic shift, round half up
__device__ __forceinline__ long requant(int acc, int bias, int mp, int mn, int s) {
  const int a = acc + bias;
  const long m = a >= 0 ? mp : mn;
  return ((long)a * m + (1L << (s - 1))) >> s;
}

template <bool F32OUT>
__global__ __launch_bounds__(64) void int_rows_kernel(IntRowsParams p) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int ct = blockIdx.y;
  const long row = (long)blockIdx.x * 32 + r;       // this lane's row (the B column and the D column)
  const bool live = row < p.rows;
  const long rr = live ? row : 0;
  const int b = (int)(rr / p.P), pi = (int)(rr - (long)b * p.P);
  const int ph = p.pix[2 * pi], pw = p.pix[2 * pi + 1];
  const bool inmap = live && ph >= 0 && ph < p.H && pw >= 0 && pw < p.W;   // (a listed pixel off the map reads zeros, never memory)
  const i32x4* wt = reinterpret_cast<const i32x4*>(p.wp) + (long)ct * p.kcs_total * 64 + lane;

  i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s >= p.nsrc) break;
    const IntRowsSrc S = p.src[s];
    const int npos = S.kind == CLC_INT_SRC_TAPS ? p.ntaps : 1;
    for (int t = 0; t < npos; ++t) {
      bool on;
      long at;   // the source row of this lane: a pixel of the map or a row of the dense buffer
      if (S.kind == CLC_INT_SRC_DENSE) {
        on = live;
        at = rr;
      } else {
        int ih = ph, iw = pw;
        if (S.kind == CLC_INT_SRC_TAPS) {
          const int o = p.taps[t];
          ih += (int)(short)(o & 0xffff);
          iw += o >> 16;
        }
        on = inmap && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        at = ((long)b * p.H + ih) * p.W + iw;
      }
      const int8_t* xp = S.p + at * S.ld + 16 * h;
      for (int kc = 0; kc < S.kcs; ++kc) {
        i32x4 bv = {0, 0, 0, 0};
        if (on) bv = *reinterpret_cast<const i32x4*>(xp + 32 * kc);
        const i32x4 av = *wt;
        wt += 64;
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int co = 32 * ct + 8 * g + 4 * h;
    const i32x4 bi = *reinterpret_cast<const i32x4*>(p.bias + co), mp = *reinterpret_cast<const i32x4*>(p.mpos + co);
    const i32x4 mn = *reinterpret_cast<const i32x4*>(p.mneg + co), sh = *reinterpret_cast<const i32x4*>(p.shift + co);
    long v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = requant(acc[4 * g + e], bi[e], mp[e], mn[e], sh[e]);
    if (F32OUT) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (float)(int)(v[e] < -32768 ? -32768 : (v[e] > 32767 ? 32767 : v[e])) * p.out_scale;
      *reinterpret_cast<f32x4*>(static_cast<float*>(p.y) + row * p.ldy + co) = o;
    } else {
      unsigned o = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) o |= ((unsigned)(int)(v[e] < -128 ? -128 : (v[e] > 127 ? 127 : v[e])) & 0xffu) << (8 * e);
      *reinterpret_cast<unsigned*>(static_cast<int8_t*>(p.y) + row * p.ldy + co) = o;
    }
  }
}

}  // namespace

extern "C" int clc_int_rows(const clc_int_rows_desc* d, clc_stream_t stream) {
  CLC_CHECK(d, "clc_int_rows: descriptor is NULL");
  CLC_CHECK(d->nsrc >= 1 && d->nsrc <= 2, "clc_int_rows: one or two K ranges (got nsrc=%d)", d->nsrc);
  CLC_CHECK(d->pix && d->w_packed && d->bias && d->mult_pos && d->mult_neg && d->shift && d->y,
            "clc_int_rows: pix, w_packed, bias, mult_pos, mult_neg, shift or y is NULL");
  CLC_CHECK(d->P > 0 && d->B > 0 && d->H > 0 && d->W > 0, "clc_int_rows: P, B, H and W must be positive (got P=%d B=%d H=%d W=%d)", d->P, d->B,
            d->H, d->W);
  CLC_CHECK(d->Cout > 0 && d->Cout % 32 == 0, "clc_int_rows: Cout must be a positive multiple of 32 (got %d)", d->Cout);
  CLC_CHECK(d->out_kind == CLC_INT_OUT_I8 || d->out_kind == CLC_INT_OUT_F32, "clc_int_rows: out_kind must be CLC_INT_OUT_I8 or CLC_INT_OUT_F32 (got %d)",
            d->out_kind);
  CLC_CHECK(d->out_kind != CLC_INT_OUT_F32 || (d->f_out >= 0 && d->f_out <= 30), "clc_int_rows: f_out must be 0 .. 30 (got %d)", d->f_out);
  bool any_taps = false;
  long K = 0;
  for (int s = 0; s < d->nsrc; ++s) {
    const clc_int_src& S = d->src[s];
    CLC_CHECK(S.p, "clc_int_rows: range %d: p is NULL", s);
    CLC_CHECK(S.kind == CLC_INT_SRC_PIXEL || S.kind == CLC_INT_SRC_DENSE || S.kind == CLC_INT_SRC_TAPS,
              "clc_int_rows: range %d: kind must be CLC_INT_SRC_PIXEL, CLC_INT_SRC_DENSE or CLC_INT_SRC_TAPS (got %d)", s, S.kind);
    CLC_CHECK(S.C > 0 && S.C % 32 == 0, "clc_int_rows: range %d: C must be a positive multiple of 32 (got %d)", s, S.C);
    CLC_CHECK(S.ld >= S.C && S.ld % 16 == 0, "clc_int_rows: range %d: ld must be >= C and a multiple of 16 (got ld=%d C=%d)", s, S.ld, S.C);
    CLC_CHECK(aligned16(S.p), "clc_int_rows: range %d: p must be 16-byte aligned", s);
    any_taps |= S.kind == CLC_INT_SRC_TAPS;
    K += S.kind == CLC_INT_SRC_TAPS ? (long)(d->ntaps > 0 ? d->ntaps : 0) * S.C : S.C;
  }
  if (any_taps) {
    CLC_CHECK(d->ntaps >= 1 && d->ntaps <= CLC_INT_ROWS_MAX_TAPS, "clc_int_rows: a taps range takes 1 .. %d taps (got ntaps=%d)", CLC_INT_ROWS_MAX_TAPS,
              d->ntaps);
    CLC_CHECK(d->taps, "clc_int_rows: taps is NULL");
    for (int t = 0; t < d->ntaps; ++t)
      CLC_CHECK(d->taps[2 * t] >= -127 && d->taps[2 * t] <= 127 && d->taps[2 * t + 1] >= -127 && d->taps[2 * t + 1] <= 127,
                "clc_int_rows: tap %d: offsets must be within +-127 (got dh=%d dw=%d)", t, d->taps[2 * t], d->taps[2 * t + 1]);
  }
  CLC_CHECK(K <= 65536, "clc_int_rows: K = %ld is above 65536: the int32 sum could overflow (|acc| <= K * 128 * 127)", K);
  CLC_CHECK(d->ldy >= d->Cout && d->ldy % 4 == 0, "clc_int_rows: ldy must be >= Cout and a multiple of 4 (got ldy=%d Cout=%d)", d->ldy, d->Cout);
  CLC_CHECK(aligned16(d->w_packed) && aligned16(d->bias) && aligned16(d->mult_pos) && aligned16(d->mult_neg) && aligned16(d->shift),
            "clc_int_rows: w_packed, bias, mult_pos, mult_neg and shift must be 16-byte aligned");
  CLC_CHECK((reinterpret_cast<uintptr_t>(d->pix) & 3) == 0, "clc_int_rows: pix must be 4-byte aligned");
  CLC_CHECK(d->out_kind == CLC_INT_OUT_F32 ? aligned16(d->y) : (reinterpret_cast<uintptr_t>(d->y) & 3) == 0,
            "clc_int_rows: y must be 16-byte aligned for f32 output, 4-byte aligned for int8 output");
  const long rows = (long)d->B * d->P, tiles = (rows + 31) / 32;
  CLC_CHECK(tiles <= 0x7fffffffL && d->Cout / 32 <= 65535 && (long)d->B * d->H * d->W < (1L << 31), "clc_int_rows: the call is too large (B P = %ld)", rows);
  IntRowsParams p;
  for (int s = 0; s < 2; ++s) {
    const clc_int_src& S = d->src[s < d->nsrc ? s : 0];
    p.src[s].p = S.p; p.src[s].ld = S.ld; p.src[s].kcs = S.C / 32; p.src[s].kind = S.kind;
  }
  p.pix = d->pix; p.wp = d->w_packed; p.bias = d->bias; p.mpos = d->mult_pos; p.mneg = d->mult_neg; p.shift = d->shift; p.y = d->y;
  p.rows = rows; p.nsrc = d->nsrc; p.P = d->P; p.H = d->H; p.W = d->W; p.ntaps = any_taps ? d->ntaps : 0; p.kcs_total = (int)(K / 32); p.ldy = d->ldy;
  p.out_scale = ldexpf(1.f, -d->f_out);
  for (int t = 0; t < CLC_INT_ROWS_MAX_TAPS; ++t)
    p.taps[t] = any_taps && t < d->ntaps ? (int)(((unsigned)d->taps[2 * t] & 0xffffu) | ((unsigned)d->taps[2 * t + 1] << 16)) : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles, (unsigned)(d->Cout / 32), 1);
  if (d->out_kind == CLC_INT_OUT_F32) int_rows_kernel<true><<<grid, 64, 0, st>>>(p);
  else int_rows_kernel<false><<<grid, 64, 0, st>>>(p);
  CLC_LAUNCH_CHECK();
  return 0;
}
