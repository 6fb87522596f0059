// Integer hyper-synthesis: int8 convolutions on the gfx950 i8 matrix cores with the requantising epilogue fused, so that the
// entropy parameters of a hyperprior model are the same bits under every kernel state and every build (include/clc_hip.h: "integer
// hyper-synthesis" states the arithmetic; tests/intnet_ref.py is its reference).
//
// The maps are tiny (z is H/64 x W/64), so the kernel is built for many small independent tiles: ONE WAVE per 32 output pixels x 32
// output channels, no LDS, no barrier.  v_mfma_i32_32x32x32_i8 with swapped roles: A = the filter (row = output channel), B = the
// activations (column = output pixel).  Lane (r = lane & 31, h = lane >> 5) supplies 16 bytes of each operand per MFMA: input channels
// 32 kc + 16 h + j, j = 0 .. 15, of filter row r and of pixel r.  The sum over k is exact and order-free, so WHICH k the hardware assigns
// to (h, j) does not matter as long as both operands share it — and they do, both being read in the same (h, j) order.
//   A: from the packed filter image [Cout / 32][T][Cin / 32][64 lanes][16 B] — a wave's fragment is one coalesced 1 KB load.
//   B: 16 consecutive input channels of one pixel and tap straight from the NHWC int8 map, one aligned 16-byte load; zero for a tap off
//      the map and for a pixel row beyond B H W (never read).
//   C/D: the documented dtype-independent map: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 h — a lane's
//      registers 4 g .. 4 g + 3 are four consecutive output channels 8 g + 4 h .., so four int8 results pack into one dword store.
// The transposed 5x5 / stride-2 layer visits only the live taps of each of the four output parity classes (as conv5.hip does for the
// float deconv): a tile holds 32 pixels of ONE class, so a wave's tap set is uniform; a class has exactly B H W pixels.
#include "common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

namespace {

struct IntConvParams {
  const int8_t* x;
  const int8_t* wp;
  const int32_t *bias, *mpos, *mneg, *shift;
  void* y;
  int B, H, W, Cin, ldx, Cout, ldy;
  long total;   // B * H * W: output pixels (3x3) or pixels of one parity class (transposed)
  float out_scale;
};

// r = (a * m + 2^(s - 1)) >> s with m chosen by the sign of a: 64-bit, arithmetic shift, round half up
__device__ __forceinline__ long requant(int acc, int bias, int mp, int mn, int s) {
  const int a = acc + bias;
  const long m = a >= 0 ? mp : mn;
  return ((long)a * m + (1L << (s - 1))) >> s;
}

template <bool TRANSPOSED, bool F32OUT>
__global__ __launch_bounds__(64) void int_conv_kernel(IntConvParams p) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int ct = blockIdx.y;
  const int kcs = p.Cin >> 5;
  constexpr int T = TRANSPOSED ? 25 : 9;
  const long q = (long)blockIdx.x * 32 + r;        // this lane's pixel (the B column and the D column)
  const bool live = q < p.total;
  const long hw = (long)p.H * p.W;
  const long qq = live ? q : 0;
  const int b = (int)(qq / hw);
  const int rem = (int)(qq - (long)b * hw);
  const int i = rem / p.W, j = rem - i * p.W;
  int ph = 0, pw = 0;
  if (TRANSPOSED) { ph = blockIdx.z >> 1; pw = blockIdx.z & 1; }
  const int8_t* xb = p.x + (long)b * hw * p.ldx + 16 * h;
  const i32x4* wt = reinterpret_cast<const i32x4*>(p.wp) + (long)ct * T * kcs * 64 + lane;

  i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // the taps: 3x3 — all nine, input (i + kh - 1, j + kw - 1); transposed — kh of the row parity, input row (oh + 2 - kh) / 2
  const int nkh = TRANSPOSED ? (ph ? 2 : 3) : 3, nkw = TRANSPOSED ? (pw ? 2 : 3) : 3;
  for (int a = 0; a < nkh; ++a) {
    const int kh = TRANSPOSED ? 2 * a + ph : a;
    const int ih = TRANSPOSED ? i + 1 - a : i + a - 1;          // (2 i + ph + 2 - (2 a + ph)) / 2
    for (int c = 0; c < nkw; ++c) {
      const int kw = TRANSPOSED ? 2 * c + pw : c;
      const int iw = TRANSPOSED ? j + 1 - c : j + c - 1;
      const bool on = live && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
      const int8_t* xp = xb + ((long)ih * p.W + iw) * p.ldx;
      const i32x4* wk = wt + (long)(kh * (TRANSPOSED ? 5 : 3) + kw) * kcs * 64;
      for (int kc = 0; kc < kcs; ++kc) {
        i32x4 bv = {0, 0, 0, 0};
        if (on) bv = *reinterpret_cast<const i32x4*>(xp + 32 * kc);
        const i32x4 av = wk[(long)kc * 64];
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
      }
    }
  }
  if (!live) return;
  long row;   // the output pixel's row in the NHWC output
  if (TRANSPOSED) row = ((long)b * 2 * p.H + (2 * i + ph)) * (2L * p.W) + (2 * j + pw);
  else row = q;
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

// x0 = clamp(rint(z * 2^f0), -128, 127): the multiply by a power of two and rintf (half to even) are IEEE-exact
__global__ __launch_bounds__(256) void int_quantize_kernel(const float* __restrict__ z, long n4, float mul, int8_t* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n4) return;
  const f32x4 v = reinterpret_cast<const f32x4*>(z)[t];
  unsigned o = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float c = fminf(fmaxf(rintf(v[e] * mul), -128.f), 127.f);   // (a NaN becomes -128 through fmaxf / fminf)
    o |= ((unsigned)(int)c & 0xffu) << (8 * e);
  }
  reinterpret_cast<unsigned*>(out)[t] = o;
}

}  // namespace

extern "C" int clc_int_conv(const clc_int_conv_desc* d, clc_stream_t stream) {
  CLC_CHECK(d, "clc_int_conv: descriptor is NULL");
  CLC_CHECK(d->x && d->w_packed && d->bias && d->mult_pos && d->mult_neg && d->shift && d->y,
            "clc_int_conv: x, w_packed, bias, mult_pos, mult_neg, shift or y is NULL");
  CLC_CHECK(d->B > 0 && d->H > 0 && d->W > 0, "clc_int_conv: B, H and W must be positive (got B=%d H=%d W=%d)", d->B, d->H, d->W);
  CLC_CHECK(d->Cin > 0 && d->Cin % 32 == 0 && d->Cout > 0 && d->Cout % 32 == 0,
            "clc_int_conv: Cin and Cout must be positive multiples of 32 (got Cin=%d Cout=%d)", d->Cin, d->Cout);
  CLC_CHECK(d->transposed == 0 || d->transposed == 1, "clc_int_conv: transposed must be 0 (3x3, stride 1) or 1 (5x5, stride 2) (got %d)", d->transposed);
  CLC_CHECK(d->out_kind == CLC_INT_OUT_I8 || d->out_kind == CLC_INT_OUT_F32, "clc_int_conv: out_kind must be CLC_INT_OUT_I8 or CLC_INT_OUT_F32 (got %d)",
            d->out_kind);
  CLC_CHECK(d->ldx >= d->Cin && d->ldx % 16 == 0, "clc_int_conv: ldx must be >= Cin and a multiple of 16 (got ldx=%d Cin=%d)", d->ldx, d->Cin);
  CLC_CHECK(d->ldy >= d->Cout && d->ldy % 4 == 0, "clc_int_conv: ldy must be >= Cout and a multiple of 4 (got ldy=%d Cout=%d)", d->ldy, d->Cout);
  CLC_CHECK(aligned16(d->x) && aligned16(d->w_packed) && aligned16(d->bias) && aligned16(d->mult_pos) && aligned16(d->mult_neg) && aligned16(d->shift),
            "clc_int_conv: x, w_packed, bias, mult_pos, mult_neg and shift must be 16-byte aligned");
  CLC_CHECK(d->out_kind == CLC_INT_OUT_F32 ? aligned16(d->y) : (reinterpret_cast<uintptr_t>(d->y) & 3) == 0,
            "clc_int_conv: y must be 16-byte aligned for f32 output, 4-byte aligned for int8 output");
  CLC_CHECK(d->out_kind != CLC_INT_OUT_F32 || (d->f_out >= 0 && d->f_out <= 30), "clc_int_conv: f_out must be 0 .. 30 (got %d)", d->f_out);
  const long total = (long)d->B * d->H * d->W;
  const long tiles = (total + 31) / 32;
  CLC_CHECK(total * 4 * (d->ldy > d->ldx ? d->ldy : d->ldx) < (1L << 40) && tiles <= 0x7fffffffL && d->Cout / 32 <= 65535,
            "clc_int_conv: the map is too large (B H W = %ld)", total);
  IntConvParams p;
  p.x = d->x; p.wp = d->w_packed; p.bias = d->bias; p.mpos = d->mult_pos; p.mneg = d->mult_neg; p.shift = d->shift; p.y = d->y;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.ldx = d->ldx; p.Cout = d->Cout; p.ldy = d->ldy; p.total = total;
  p.out_scale = ldexpf(1.f, -d->f_out);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles, (unsigned)(d->Cout / 32), d->transposed ? 4 : 1);
  if (d->transposed) {
    if (d->out_kind == CLC_INT_OUT_F32) int_conv_kernel<true, true><<<grid, 64, 0, st>>>(p);
    else int_conv_kernel<true, false><<<grid, 64, 0, st>>>(p);
  } else {
    if (d->out_kind == CLC_INT_OUT_F32) int_conv_kernel<false, true><<<grid, 64, 0, st>>>(p);
    else int_conv_kernel<false, false><<<grid, 64, 0, st>>>(p);
  }
  CLC_LAUNCH_CHECK();
  return 0;
}

extern "C" int clc_int_quantize(const float* z, long n, int f0, int8_t* x0, clc_stream_t stream) {
  CLC_CHECK(z && x0, "clc_int_quantize: z or x0 is NULL");
  CLC_CHECK(n > 0 && n % 4 == 0, "clc_int_quantize: n must be a positive multiple of 4 (got %ld)", n);
  CLC_CHECK(f0 >= 0 && f0 <= 16, "clc_int_quantize: f0 must be 0 .. 16 (got %d)", f0);
  CLC_CHECK(aligned16(z) && (reinterpret_cast<uintptr_t>(x0) & 3) == 0, "clc_int_quantize: z must be 16-byte aligned, x0 4-byte aligned");
  const long n4 = n / 4, blocks = (n4 + 255) / 256;
  CLC_CHECK(blocks <= 0x7fffffffL, "clc_int_quantize: n = %ld is too large", n);
  int_quantize_kernel<<<(unsigned)blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(z, n4, ldexpf(1.f, f0), x0);
  CLC_LAUNCH_CHECK();
  return 0;
}
