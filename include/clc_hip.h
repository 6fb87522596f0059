/* clc_hip.h — C ABI of libclc_hip.so, the MI355X (gfx950) engine behind the CLC hot path.
 *
 * The reference (ydchen0806/CLC) has no FFI of its own: its callers import Python
 * nn.Modules (`from models import TCM, CLC`, /root/reference/train_CLC.py:25,
 * eval_CLC.py:4) whose arithmetic is executed by cuDNN / cuBLAS / ATen and by the
 * CompressAI C++ extensions.  This header is therefore the boundary a maintainer would
 * bind INSTEAD of those native back-ends (INTEGRATION.md shows the ctypes stub); each
 * entry point cites the reference call site whose native work it replaces.
 *
 * Conventions
 *  - Plain pointers and sizes only; no torch types.  Device pointers unless marked HOST.
 *  - All activations are NHWC fp32 ("pixel-major"): element (n,h,w,c) of a tensor lives
 *    at base[((n*H+h)*W+w)*ld + c]; `ld` (floats) lets a call read or write a channel
 *    slice of a wider buffer, so torch.cat / split / chunk never materialise.
 *  - Conv weights are [Cout][KH][KW][Cin] (PyTorch OIHW tensor in channels_last memory format).
 *  - Every function enqueues work on `stream` and returns immediately: no allocation,
 *    no synchronisation, no host read-back -> capturable in a hipGraph.  The caller owns
 *    every buffer including workspaces (sizes from the *_workspace_bytes helpers).
 *  - Return value: >= 0 = ok (clc_conv2d / clc_conv2d_wgrad return the id BM*1000+BN of the
 *    tile variant they launched, 1 = small-Cin kernel), negative = error; clc_last_error()
 *    gives the message (thread-local).  No C++ exception crosses the ABI.
 *  - Results are run-to-run deterministic (no floating-point atomics anywhere) and do not
 *    depend on the batch size for a given image (per-output accumulation order is fixed),
 *    which the encoder/decoder agreement of compress()/decompress() relies on.
 */
#ifndef CLC_HIP_H
#define CLC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* clc_stream_t; /* hipStream_t */

const char* clc_last_error(void);
int clc_version(void);
/* A/B switch between kernel variants (key 1: stream-K filter gradients, 0 or 1; the keys are listed in clc_amd/csrc/common.h);
 * returns the previous value, or -1 for an unknown key.  Keys 0, 2, 3, 12 and 19 are retired: they read as their last defaults
 * (2, 1, 0, 0, 1), and setting one to any other value returns -1 (clc_last_error says why).  Benchmark tooling only. */
int clc_set_tuning(int key, int value);
int clc_get_tuning(int key);
/* The codec container's kernel-configuration tag (clc_amd/codec.py): which generation of context-model summation orders this build,
 * in its CURRENT tuning state, runs.  1..127 = default tuning of that generation; 128..255 = a hash of the order-affecting keys
 * when any is off its default.  A stream decodes only under the tag it was encoded with (the slice loop is autoregressive through
 * the arithmetic decoder: CLC_run.py:738-814 has the same property across devices and records nothing). */
int clc_kernel_config_tag(void);
/* ... and the full 32-bit hash of the same state (generation + order-affecting keys): containers written under a NON-default state (tag >= 128,
 * 7 hash bits) carry it too, so that two such states cannot be mistaken for each other (clc_amd/codec.py, header version 2). */
unsigned clc_kernel_config_hash(void);

/* ---- activation / epilogue codes ---------------------------------------------------- */
enum { CLC_ACT_NONE = 0, CLC_ACT_LRELU = 1, CLC_ACT_RELU = 2, CLC_ACT_GELU = 3, CLC_ACT_HALFTANH = 4 /* 0.5*tanh(v), LRP head */,
       CLC_ACT_SIGMOID = 5 /* forward only (CLM modulation) */,
       CLC_ACT_SAVED_DERIV = 6 /* backward only: the saved tensor IS act'(pre-activation) (see pre_deriv) */ };
/* input prologue applied to the gathered activations */
enum { CLC_IN_NONE = 0, CLC_IN_SQUARE = 1 };
/* norm modes of the epilogue: out = mul * rsqrt(v) (GDN) or mul * sqrt(v) (inverse GDN) */
enum { CLC_NORM_NONE = 0, CLC_NORM_GDN = 1, CLC_NORM_IGDN = 2,
       CLC_NORM_MUL2 = 3 /* out = 2 * mul * v: the chain-rule factor d(x^2)/dx of GDN's backward, fused into the 1x1 data-gradient conv */ };

/* ---- convolution as implicit GEMM on v_mfma_f32_32x32x2_f32 ------------------------- *
 * Replaces cuDNN conv fwd / bwd-data / bwd-weight behind every nn.Conv2d and nn.Linear
 * of the path: /root/reference/models/CLC_run.py:120,123,185-187,207-208,232-233,
 * 273-277,335-354,371-396,412-481 and the CompressAI layers of SURVEY.md A.1.
 *
 * y[n,oh,ow,co] = epi( sum_{kh,kw,ci} in_op(x[n, oh*s-pad+kh, ow*s-pad+kw, ci]) * w[co,kh,kw,ci] )
 * epi(v): v += bias[co]; (y_pre <- v); v = norm(v, mul); v = act(v); v += res_scale*res
 *         (res_first = 1: the residual is added BEFORE the activation: v = act(v + res_scale*res), y_pre includes it)
 * transposed = 1 computes the data gradient of that conv instead: "x" is dY
 * [N,H,W,Cin=Cout_fwd], "y" is dX [N,OH,OW,Cout=Cin_fwd] and w must be the transposed
 * filter [Cin_fwd][KH][KW][Cout_fwd] (clc_filter_transpose).
 * shuffle = 1 fuses PixelShuffle(2) into the store: y has 2*OH x 2*OW pixels of Cout/4 ch.
 */
typedef struct {
  const float* x; int N, H, W, Cin, ldx;
  const float* w;            /* [Cout][ks][ks][Cin] */
  const float* bias;         /* [Cout] or NULL */
  float* y; int OH, OW, Cout, ldy;
  int ks, stride, pad;       /* ks = 1 | 3 (pad = ks / 2 in every caller), or 5 with pad = 2: the 5x5 kernels of csrc/conv5.hip — forward and
                              * transposed, stride 1 or 2, on the aligned path only (Cin % 4 == 0, ldx % 4 == 0, 16-byte aligned x / w; any Cout),
                              * with bias, act = none / ReLU / LeakyReLU, ldx / ldy; every other optional field below is refused by name.
                              * The K order of an output element depends on (Cin, map size) alone, as for the other kernels; no workspace;
                              * f32 in the bf16 precision mode too. */
  int transposed;
  int in_op;
  int act;
  int norm; const float* mul; int ldm;
  const float* res; int ldr; float res_scale;
  float* y_pre; int ldp;     /* optional pre-activation copy (training) */
  int shuffle;
  int res_first;
  /* optional fused activation backward on the gathered operand: x <- x * act'(xs) with xs the saved
   * pre-activation (xs_pre = 1) or activation output of the layer whose gradient x is (same geometry as x) */
  const float* xs; int ldxs; int xs_act; int xs_pre;
  /* optional second filter set: images [N/2, N) of the batch are convolved with w2 / bias2 (same geometry as w / bias),
   * images [0, N/2) with w / bias.  Two same-shaped layers that run side by side on different data (the mean- and the
   * scale-parameter nets of a slice, CLC_run.py:560-566) become ONE launch with twice the rows — the 16x16-map layers
   * are latency-bound, so the second one is nearly free.  NULL = ordinary convolution; N must be even. */
  const float* w2; const float* bias2;
  /* pre_deriv = 1: y_pre receives act'(v) instead of v, so the backward of an expensive activation (GELU: erf + exp) is
   * one multiply in the gradient kernels' loaders (xs_act / dys_act = CLC_ACT_SAVED_DERIV) — no elementwise pass */
  int pre_deriv;
  /* optional gate on the residual term: v += res_scale * res * act'(res_gate) (res_gate_pre as xs_pre).  Lets a data-gradient
   * kernel add the gradient of a residual branch that passed through an activation (ResidualUnit: relu(conv(..) + x)) without a
   * separate activation-backward pass */
  const float* res_gate; int ldg; int res_gate_act; int res_gate_pre;
  /* optional gate on the whole result: y *= act'(out_gate) — a data-gradient kernel hands the PRODUCING layer its gradient
   * already multiplied by that layer's activation derivative (out_gate = the producer's activated output, i.e. this layer's
   * forward input, for LeakyReLU / ReLU; the stored derivative for GELU), so the producer's own gradient kernels need no
   * operand prologue (and run on the LDS-DMA path). */
  const float* out_gate; int ldog; int out_gate_act; int out_gate_pre;
  /* optional third and fourth filter set (both or neither, with w2): quarter k of the batch, images [k N/4, (k+1) N/4), is convolved
   * with set k of (w, w2, w3, w4).  The ResidualUnits of an attention block's two branches — conv_a on the block input, conv_b on the
   * Swin output (CLC_run.py:235-244) — of the mean- AND the scale-parameter net are four same-shaped layers on different data: one
   * launch instead of four.  N must be a multiple of 4. */
  const float* w3; const float* bias3; const float* w4; const float* bias4;
  /* optional scratch (clc_conv2d_workspace_bytes(d) bytes, caller-owned, 16-B aligned): lets a DATA-GRADIENT launch whose grid would
   * leave most CUs with one 4-wave workgroup (3x3 layers on 32x32 / 16x16 maps with few output channels) split K over 2-4
   * workgroups per tile — partial tiles to the scratch, a fixed-order finish launch adds them and applies the epilogue.  Without it
   * (NULL) the launch is not split.  Forward launches are not split unless batch_variant_ok is set: an image's bits must not depend on
   * the batch size in the codec. */
  void* workspace; size_t workspace_bytes;
  /* nonzero: this launch's result may depend (in summation order only) on the batch size — set by training forward passes, never by the
   * codec path.  Lets the long-K forward layers of the slice-parameter nets (3x3, 384..704 -> 224 on 16x16 maps) run on 128x128 LDS tiles
   * with a K split sized to the grid (needs `workspace`). */
  int batch_variant_ok;
  /* optional: the same filter in the fragment order of conv_halo3x3_kernel (clc_filter_pack_halo; for transposed = 1: of the transposed
   * filter).  With it, 3x3 / stride-1 / pad-1 layers with 128 (64) input channels and a multiple of 128 (64) output channels on maps whose
   * height is a multiple of 8 and width of 16 run on the halo-resident kernel (csrc/conv_halo.hip) — same bits as the tiled kernels.  NULL: tiled. */
  const float* w_packed;
  /* optional: the filter's Winograd F(2x2, 3x3) transform in fragment order (clc_filter_wino; for transposed = 1: of the transposed filter, taps
   * flipped).  With it, 3x3 / stride-1 / pad-1 layers with 64 k input and 64 k output channels on maps whose height is a multiple of 8 and
   * width of 16 run on conv_wino_kernel / conv_wino64_kernel (csrc/conv_wino.hip): 2.25x fewer multiplications, ANOTHER summation order than the direct kernels
   * (fp32 error of a few ulp of the operands; measured 4..9e-7 of the largest output against fp64, the direct kernels 1.3e-6).  Takes precedence
   * over w_packed.  For TRAINING launches (forward of a recorded pass, data gradients): a launch whose result feeds the entropy coder or a parity
   * measurement leaves it NULL (direct kernels) — the codec's kernel_config tag does not cover this kernel. */
  const float* w_wino;
} clc_conv_desc;

int clc_conv2d(const clc_conv_desc* d, clc_stream_t stream);
/* [N][3][3][K] filter rows, K = 128 or 64, N a multiple of K (the forward filter [Cout][kh][kw][Cin = K], or the transposed filter
 * [Cin][kh][kw][Cout = K] of a K -> K layer) -> `out` (same number of floats) in the fragment order clc_conv_desc.w_packed expects. */
int clc_filter_pack_halo(const float* w, float* out, int N, int K, clc_stream_t stream);
/* ... for every such filter of a model in ONE launch: device table of entries; block_begin = running sum of ceil(N * 9 * K / 4 / 256) (blocks of 256
 * 16-B elements) over the preceding entries, total_blocks = the grand total */
typedef struct { const float* w; float* out; int N, K, block_begin; } clc_halo_pack_entry;
int clc_filter_pack_halo_batched(const clc_halo_pack_entry* table_dev, int n_entries, int total_blocks, clc_stream_t stream);
/* [N][3][3][K] filter rows (N, K multiples of 64) -> `out` (ceil(N / 128) * 128 * 16 * K floats): U = G g G^T per (row, channel) in the fragment order
 * clc_conv_desc.w_wino expects; flip = 1 reverses the taps (data gradients: pass the transposed filter).  The batched form: device table,
 * block_begin = running sum of ceil(N * K / 4 / 256). */
int clc_filter_wino(const float* w, float* out, int N, int K, int flip, clc_stream_t stream);
typedef struct { const float* w; float* out; int N, K, flip, block_begin; } clc_wino_entry;
int clc_filter_wino_batched(const clc_wino_entry* table_dev, int n_entries, int total_blocks, clc_stream_t stream);
/* scratch bytes with which clc_conv2d would split this launch's K range (0: it would not split) */
size_t clc_conv2d_workspace_bytes(const clc_conv_desc* d);

/* Weight gradient: dw[co,kh,kw,ci] = sum_{n,oh,ow} dy[n,oh,ow,co] * in_op(x[n,oh*s-pad+kh,ow*s-pad+kw,ci]).
 * Deterministic split-K: partial slabs in `workspace`, summed in a fixed order.
 * dbias (optional) = column sums of dy. accumulate=1 adds into dw/dbias. */
typedef struct {
  const float* x; int N, H, W, Cin, ldx;
  const float* dy; int OH, OW, Cout, lddy;
  float* dw; float* dbias;
  int ks, stride, pad;       /* ks = 5 (pad 2): one single-pass launch per problem (csrc/conv5.hip), in clc_conv2d_wgrad only — the grouped
                              * entry points refuse it, clc_conv2d_wgrad_variant returns 5; no dys / in_op; Cin % 4 == 0; workspace for dbias only */
  int in_op;
  int accumulate;
  void* workspace; size_t workspace_bytes;
  /* optional fused activation backward on dy: dy <- dy * act'(dys) (same geometry as dy) */
  const float* dys; int lddys; int dys_act; int dys_pre;
} clc_wgrad_desc;

size_t clc_conv2d_wgrad_workspace_bytes(const clc_wgrad_desc* d);
int clc_conv2d_wgrad(const clc_wgrad_desc* d, clc_stream_t stream);
/* `count` independent filter-gradient problems (each with its own workspace): same results, bit for bit, as `count`
 * calls of clc_conv2d_wgrad in order, but problems of one tile shape share a grid and all slab sets share one
 * fixed-order reduce launch (the 16x16-map layers of the slice loop are launch-bound one by one).  Problems that write
 * the same dw / dbias (a filter applied twice, e.g. the reference encoder over several reference frames) are kept in
 * separate launches, in order. */
int clc_conv2d_wgrad_batched(const clc_wgrad_desc* descs, int count, clc_stream_t stream);
/* Stream-K form of the grouped launch: ONE grid of <= 512 workgroups per tile shape walks the K-units of all problems laid end
 * to end; a workgroup accumulates in registers while it stays inside an output tile and leaves at most two partial tile
 * images in `group_workspace` (clc_conv2d_wgrad_group_workspace_bytes(), caller-owned, reusable across calls on one stream),
 * which a fix-up launch adds in workgroup order.  Same results as clc_conv2d_wgrad_batched up to summation order; run-to-run
 * reproducible (the ranges depend only on the group's shapes). */
size_t clc_conv2d_wgrad_group_workspace_bytes(void);
/* per-problem workspace a problem needs INSIDE clc_conv2d_wgrad_batched_sk: 0 for every plan whose partial tiles live in the
 * group workspace (d->workspace may then be NULL), clc_conv2d_wgrad_workspace_bytes(d) for the small-Cin split path. */
size_t clc_conv2d_wgrad_sk_workspace_bytes(const clc_wgrad_desc* d);
/* kernel family a problem is planned on: 1 = small-Cin VALU kernel, 64900 + TW = all-taps 3x3 kernel (TW = 32 | 16 | 8),
 * BM * 1000 + BN = tap-per-workgroup kernel (same ids clc_conv2d_wgrad returns).  Benchmark tooling: FLOP accounting per kernel. */
int clc_conv2d_wgrad_variant(const clc_wgrad_desc* d);
int clc_conv2d_wgrad_batched_sk(const clc_wgrad_desc* descs, int count, void* group_workspace, size_t group_workspace_bytes,
                                clc_stream_t stream);

/* [Cout][T][Cin] -> [Cin][T][Cout]  (T = ks*ks) */
int clc_filter_transpose(const float* w, float* wt, int Cout, int T, int Cin, clc_stream_t stream);
/* all filters of a model in ONE launch: device table of entries; tile_begin = running sum of
 * T*ceil(Cout/32)*ceil(Cin/32) over the preceding entries, total_tiles = the grand total */
typedef struct { const float* w; float* wt; int Cout, T, Cin, tile_begin; } clc_transpose_entry;
int clc_filter_transpose_batched(const clc_transpose_entry* table_dev, int n_entries, int total_tiles, clc_stream_t stream);

/* ---- elementwise / normalisation ------------------------------------------------------ */
/* dz = dy * act'(saved); saved = pre-activation (use_pre=1) or the activation output */
int clc_act_bwd(const float* dy, int lddy, const float* saved, int lds, int use_pre, int act, float* dz, int lddz,
                long rows, int C, clc_stream_t stream);
/* column sums: out[c] (+)= sum_r x[r*ld + c]; workspace >= clc_colsum_workspace_bytes */
size_t clc_colsum_workspace_bytes(long rows, int C);
int clc_colsum(const float* x, int ld, long rows, int C, float* out, int accumulate, void* ws, size_t ws_bytes,
               clc_stream_t stream);

/* Deferred parameter-gradient reductions: out[i] (+)= sum_{b < nblocks} partial[b*n + i], i < n; columns i < split go to
 * out0[i], the rest to out1[i - split] (LayerNorm: n = 2C, split = C, out0 = dgamma, out1 = dbeta; relative-position bias:
 * split = n).  clc_layernorm_bwd with dgamma = dbeta = NULL and clc_winattn_bwd with drelbias = NULL leave their partial
 * rows in the workspace (nblocks = workspace_bytes / (n * 4)); one call here sums up to 64 of them per launch, in a fixed
 * order.  `entries` is a HOST array (copied into the kernel arguments). */
typedef struct { const float* partial; int nblocks; int n; float* out0; float* out1; int split; int accumulate; } clc_reduce_entry;
int clc_partial_reduce_batched(const clc_reduce_entry* entries, int count, clc_stream_t stream);

/* LayerNorm over the channel dim of [rows, C] tokens (nn.LayerNorm, CLC_run.py:180,183), eps = 1e-5.
 * fwd saves mean/rstd per row when non-NULL. */
int clc_layernorm_fwd(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* mean,
                      float* rstd, long rows, int C, clc_stream_t stream);
/* dx (+ dx_add when non-NULL: the gradient of the residual branch x + f(LN(x)), CLC_run.py:190-191, folded into the same
 * pass); dgamma/dbeta partial sums go through ws (deterministic two-stage) */
size_t clc_layernorm_bwd_workspace_bytes(long rows, int C);
/* number of partial rows ([2][C] each) the backward leaves in the workspace (paired: the first half of them belongs to the
 * first module, the second half to the second) */
int clc_layernorm_bwd_blocks(long rows, int paired);
int clc_layernorm_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* mean,
                      const float* rstd, float* dx, int lddx, const float* dx_add, int ld_add, float* dgamma, float* dbeta,
                      int accumulate, long rows, int C, void* ws, size_t ws_bytes, clc_stream_t stream);

/* Paired modules (the mean- and scale-parameter nets of a slice run as ONE stacked batch, see clc_conv_desc.w2): rows
 * [0, half_rows) use gamma / beta, rows [half_rows, rows) use gamma2 / beta2.  C must be 64, 128 or 256. */
int clc_layernorm_fwd_pair(const float* x, int ldx, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                           long half_rows, float* y, int ldy, float* mean, float* rstd, long rows, int C, clc_stream_t stream);
int clc_layernorm_bwd_pair(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* gamma2, long half_rows,
                           const float* mean, const float* rstd, float* dx, int lddx, const float* dx_add, int ld_add,
                           float* dgamma, float* dbeta, float* dgamma2, float* dbeta2, int accumulate, long rows, int C, void* ws,
                           size_t ws_bytes, clc_stream_t stream);

/* GDN backward pieces (CompressAI GDN inside ResidualBlockWithStride / ResidualBlockUpsample):
 * given dy, x, norm v = beta + gamma.x^2 :  dx_direct = dy * f(v);  dv = dy * x * f'(v)
 * with f = rsqrt (inverse=0) or sqrt (inverse=1).  */
int clc_gdn_bwd_elem(const float* dy, const float* x, const float* v, float* dx_direct, float* dv, long n, int inverse,
                     clc_stream_t stream);
/* dx = dx_direct + 2*x*t  (t = gamma^T . dv from clc_conv2d) */
int clc_gdn_bwd_combine(const float* dx_direct, const float* x, const float* t, float* dx, long n, clc_stream_t stream);
/* CompressAI NonNegativeParametrizer (GDN beta / gamma): y = max(x, bound)^2 - pedestal for gamma [C,C] and
 * beta [C] in one launch (gamma_eff also written transposed for the data-gradient conv); backward with the LowerBound
 * gradient rule (pass where x >= bound or the gradient pushes x up), optionally accumulating into dgamma / dbeta. */
int clc_gdn_reparam_fwd(const float* gamma, const float* beta, int C, float gamma_bound, float beta_bound, float pedestal,
                        float* gamma_eff, float* gamma_eff_t, float* beta_eff, clc_stream_t stream);
/* The forward re-parametrisation of MANY GDN modules in one launch: `table_dev` = n_entries device-resident entries, entry e owning the
 * blocks [first_block, first_block + ceil((C*C + C) / 256)) of a grid of total_blocks workgroups of 256 threads. */
typedef struct {
  const float* gamma; const float* beta;
  float* gamma_eff; float* gamma_eff_t; float* beta_eff;
  int C, first_block;
  float gamma_bound, beta_bound, pedestal;
} clc_gdn_entry;
int clc_gdn_reparam_fwd_batched(const clc_gdn_entry* table_dev, int n_entries, int total_blocks, clc_stream_t stream);
int clc_gdn_reparam_bwd(const float* gamma, const float* beta, int C, float gamma_bound, float beta_bound, const float* dgamma_eff,
                        const float* dbeta_eff, float* dgamma, float* dbeta, int accumulate, clc_stream_t stream);
/* backward of PixelShuffle(2) fused with the activation backward of the conv that was stored shuffled:
 * dz[n,h,w,4q+r] = dy[n,2h+(r>>1),2w+(r&1),q] * act'(saved[same]); dy/saved [N,C/4,2H,2W] pixel-major, dz [N,C,H,W] dense.
 * saved may be NULL (no activation). */
int clc_unshuffle_act_bwd(const float* dy, int lddy, const float* saved, int lds, int use_pre, int act, float* dz, int N, int H,
                          int W, int C, clc_stream_t stream);

/* out = a * sigmoid(b) + idn  (SWAtten gate, CLC_run.py:241-242) and its backward */
int clc_gate_fwd(const float* a, const float* b, const float* idn, float* out, long n, clc_stream_t stream);
int clc_gate_bwd(const float* dout, const float* a, const float* b, float* da, float* db, long n, clc_stream_t stream);

/* generic fused adds: out = alpha*a + beta*b */
/* dst = ((src0 + src1) + src2) + ...: up to 12 pixel-major [rows][C] sources (HOST arrays of device pointers / leading dimensions), fixed
 * order — the gradient of a tensor with several consumers in one launch (ops.fanout) instead of autograd's chain of pairwise adds. */
int clc_sum_n(const float* const* srcs, const int* lds, int n, float* dst, int lddst, long rows, int C, clc_stream_t stream);
int clc_axpby(const float* a, float alpha, const float* b, float beta, float* out, long n, clc_stream_t stream);
/* RGB-head filters (3x3 / stride 2 [co][3][3][cin] and its 1x1 skip [co][cin], 9 cin <= 32) as the 32-column matrices of the patch-row
 * formulation (clc_im2col_small): w1[o][k] = w3[o][k] (k < 9 cin), ws[o][4 cin + c] = w1x1[o][c], zero elsewhere; and the reverse, ADDING the
 * two matrices' gradients into the parameters' gradient buffers. */
int clc_stem_pack(const float* w3, const float* w1x1, float* w1, float* ws, int co, int cin, clc_stream_t stream);
int clc_stem_unpack_add(const float* dw1, const float* dws, float* g3, float* g1x1, int co, int cin, clc_stream_t stream);
/* strided copy of a channel slice: dst[r*ldd + c] = src[r*lds + c] (c < C) */
int clc_copy2d(const float* src, int lds, float* dst, int ldd, long rows, int C, clc_stream_t stream);
/* Patch rows of a few-channel image (the RGB heads, Cin = 3: g_a.0 / ref_encoder.encoder.0 of CLC_run.py:274,335):
 * col[m][(kh*ks+kw)*C + c] = x[n, oh*s-pad+kh, ow*s-pad+kw, c], zeros outside the image and in columns ks*ks*C..ldc-1.
 * The 3x3/s2 conv AND the 1x1/s2 skip conv of ResidualBlockWithStride (its input is the centre tap) then run as
 * 1x1 convolutions over `col` on the MFMA kernel. */
int clc_im2col_small(const float* x, int ldx, int N, int H, int W, int C, int ks, int stride, int pad, float* col, int ldc,
                     int OH, int OW, clc_stream_t stream);

/* ---- window attention (WMSA core, CLC_run.py:142-164) --------------------------------- *
 * qkv: [B,H,W,3C] tokens, channel = which*C + head*hd + c ; out: [B,H,W,C].
 * One workgroup per (window, head): softmax(q k^T * hd^-1/2 + relbias[head] (+ shift mask)) v.
 * shift=1 -> cyclic shift by ws/2 folded into the addressing (torch.roll never materialises).
 * relbias: [heads][2ws-1][2ws-1] (the parameter itself; the index gather is done in-kernel). */
/* lse (optional, training): [B*H*W][heads] log-sum-exp of every softmax row, consumed by the backward */
int clc_winattn_fwd(const float* qkv, int ldq, const float* relbias, float* out, int ldo, float* lse, int B, int H, int W,
                    int C, int heads, int ws, int shift, clc_stream_t stream);
/* backward: rebuilds probabilities from qkv + lse, uses the forward output for D = dO.O;
 * drelbias partials via ws (deterministic) */
size_t clc_winattn_bwd_workspace_bytes(int B, int H, int W, int heads, int ws);
int clc_winattn_bwd(const float* dout, int lddo, const float* qkv, int ldq, const float* relbias, const float* out,
                    int ldo, const float* lse, float* dqkv, int lddq, float* drelbias, int accumulate, int B, int H, int W,
                    int C, int heads, int ws, int shift, void* wsb, size_t ws_bytes, clc_stream_t stream);
/* Paired modules: images [B/2, B) use relbias2 (clc_conv_desc.w2 explains the pairing); B even.  The backward's partial
 * rows: the first half of clc_winattn_bwd_blocks(..., 1) belongs to the first module. */
int clc_winattn_bwd_blocks(int B, int H, int W, int heads, int ws, int paired);
int clc_winattn_fwd_pair(const float* qkv, int ldq, const float* relbias, const float* relbias2, float* out, int ldo, float* lse,
                         int B, int H, int W, int C, int heads, int ws, int shift, clc_stream_t stream);
int clc_winattn_bwd_pair(const float* dout, int lddo, const float* qkv, int ldq, const float* relbias, const float* relbias2,
                         const float* out, int ldo, const float* lse, float* dqkv, int lddq, float* drelbias, float* drelbias2,
                         int accumulate, int B, int H, int W, int C, int heads, int ws, int shift, void* wsb, size_t ws_bytes,
                         clc_stream_t stream);

/* ---- entropy-model kernels ------------------------------------------------------------ *
 * GaussianConditional likelihood + rate (CLC_run.py:569-571, train_CLC.py:48-51)
 *   mode 0 (train): y_in = y + noise ; mode 1 (eval): y_in = round(y-mu)+mu
 *   sigma = max(scale, 0.11); lik = max(Phi((.5-|y_in-mu|)/sigma) - Phi((-.5-|..|)/sigma), 1e-9)
 * Writes lik, y_hat = round(y-mu)+mu (STE value) and adds sum(log2 lik) of this call into
 * bits_partial[blockIdx] (two-stage deterministic reduction; finish with clc_sum_partials).
 * Both bounds are torch.max's: a NaN scale or a NaN likelihood stays NaN (in lik, in its block's partial and in every gradient of
 * that element).  An upstream gradient dlik that is NaN or infinite makes dy, dmu, dscale (and dstep's term) of that element NaN,
 * blocked by the LowerBound rule or not: autograd's g phi(a) - g phi(b) gives NaN or an infinity there by the signs of its halves, and
 * an infinity must not reach an optimizer that zeroes only NaN.  In eval mode dmu is gv - gv (mu enters y_in - mu twice): zero, or NaN
 * where the element's gradient is.  Finite operands give the bits they gave before.
 * clc_gauss_lik_fwd, clc_gauss_lik_bwd and clc_quantize_build_indexes refuse, by name in clc_last_error and before any launch, a mode
 * other than 0 or 1 and a leading dimension below C of any operand they are given (noise counts in mode 0 only). */
int clc_gauss_lik_fwd(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc,
                      const float* noise, int ldn, float* lik, int ldl, float* y_hat, int ldh, long rows, int C,
                      int mode, float* bits_partial, int n_partials, clc_stream_t stream);
/* grads wrt y, mu, scale given dlik (gradient wrt lik) — includes both LowerBound rules.  dy_add (optional, leading dimension ldadd):
 * added to dy in the same pass — the straight-through gradient arriving through y_hat = ste_round(y - mu) + mu (CLC_run.py:571). */
int clc_gauss_lik_bwd(const float* dlik, int lddl, const float* y, int ldy, const float* mu, int ldmu,
                      const float* scale, int ldsc, const float* noise, int ldn, float* dy, int lddy, float* dmu,
                      int lddmu, float* dscale, int lddsc, long rows, int C, int mode, const float* dy_add, int ldadd,
                      clc_stream_t stream);

/* number of workgroup partials clc_gauss_lik_fwd writes for (rows, C) */
int clc_gauss_lik_partials(long rows, int C);

/* EntropyBottleneck factorised density (CLC_run.py:526-530). z/lik: [rows, C] NHWC slices;
 * matrices/biases/factors: HOST arrays of 5/5/4 device pointers to _matrix{k} [C,f(k+1),f(k)],
 * _bias{k} [C,f(k+1),1], _factor{k} [C,f(k+1),1]; quantiles [C,1,3].
 * mode 0 (train): v = z + noise; mode 1 (eval): v = round(z - median) + median. z_hat = round(z-med)+med. */
int clc_eb_lik_fwd(const float* z, int ldz, const float* noise, int ldn, const float* quantiles,
                   const float* const* matrices, const float* const* biases, const float* const* factors, float* lik,
                   int ldl, float* z_hat, int ldh, long rows, int C, int mode, clc_stream_t stream);
/* parameter gradients are written (not accumulated); dz may be NULL */
int clc_eb_lik_bwd(const float* dlik, int lddl, const float* z, int ldz, const float* noise, int ldn,
                   const float* quantiles, const float* const* matrices, const float* const* biases,
                   const float* const* factors, float* const* dmatrices, float* const* dbiases, float* const* dfactors,
                   float* dz, int lddz, long rows, int C, int mode, clc_stream_t stream);
/* aux loss (EntropyBottleneck.loss(), train_CLC.py:181): loss_partial[c] = sum_q |logits(quantiles[c,q]) - target[q]|,
 * dquantiles[c,q] = d loss / d quantiles (parameters are detached, as in the reference) */
int clc_eb_aux(const float* quantiles, const float* const* matrices, const float* const* biases,
               const float* const* factors, const float* target, float* loss_partial, float* dquantiles, int C,
               clc_stream_t stream);

/* quantize("symbols") + build_indexes (CLC_run.py:689-690): INT path, bit-exact */
int clc_quantize_build_indexes(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc,
                               const float* scale_table, int n_scales, int32_t* symbols, int32_t* indexes,
                               float* y_hat, int ldh, long rows, int C, clc_stream_t stream);

/* ---- the quantisation step: variable-rate coding on the Gaussian-conditional kernels (csrc/qstep.hip) ----
 * step[C] > 0: one quantisation step per channel, a contiguous device f32 vector shared by all rows.
 *   sigma = max(scale, 0.11);  t = (y - mu) / step[c] (true division);  q = rintf(t)
 *   y_hat = q * step[c] + mu — a rounded multiply followed by a rounded add, never an fmaf (the library is built with contraction off);
 *           as a differentiable value step * ste_round(t) + mu: d y_hat/dy = 1, d y_hat/dmu = 0, d y_hat/dstep = q - t
 *   y_in  = y + step[c] * noise (mode 0, training) | y_hat (mode 1, eval);  v = |y_in - mu|
 *   lik   = max(Phi((step[c] / 2 - v) / sigma) - Phi((-step[c] / 2 - v) / sigma), 1e-9), both LowerBound gradient rules as in clc_gauss_lik_bwd
 *   INT path: symbol = (int) q;  index = the row of max(scale, 0.11) / step[c] in the scale table (a quotient below table[0] takes row 0,
 *           one above the last entry or a NaN quotient the last row; fmaxf drops a NaN SCALE, which is coded as 0.11) — a symbol
 *           round((y - mu) / step) under N(0, sigma^2) is a unit-step symbol under sigma / step, so the unit-step tables serve.  The
 *           likelihood uses sigma / step as it is; the coder's table clamps it to its first row: the one place the two part company.
 * With step == 1.0f everywhere every output equals the unit-step entry's, bit for bit.  Every entry is stream-ordered, allocates
 * nothing, uses no float atomics and can be captured; a refused argument is named in clc_last_error before any launch.
 *
 * clc_gauss_lik_step_fwd: clc_gauss_lik_fwd with the step (same outputs, same partials: clc_gauss_lik_partials).
 * clc_gauss_lik_step_bwd: dy, dmu, dscale as clc_gauss_lik_bwd, and dstep[C] = the sum over all rows of
 *           g (pa + pb) / (2 sigma)  +  g dlik/dv sign(y_in - mu) w  +  g_hat (q - t),   w = noise (mode 0) | q (mode 1),
 *   the half width, y_in and y_hat paths (g: dlik after the likelihood bound's rule; g_hat, optional: the upstream gradient of y_hat,
 *   also added to dy).  dy, dmu may be NULL.  Two fixed stages — per (row block, channel) partials in ws, then four ascending quarter sums added in order — so
 *   dstep is the same bits run to run.  ws: clc_gauss_lik_step_bwd_workspace_bytes(rows, C) bytes (0 and clc_last_error on bad sizes).
 * clc_quantize_build_indexes_step: clc_quantize_build_indexes with the INT path above.
 * clc_gauss_rate_sweep: the estimate of the coded bits of B images under K candidate step vectors in one launch pair:
 *   bits[b][k] = - sum over image b's rows_per_image rows and C channels of log2 lik (mode 1) under steps[k][C], 1 <= K <= 16.
 *   y, mu, scale: [B rows_per_image][ld] pixel-major.  The partition and the order of every sum depend on (rows_per_image, C) alone:
 *   column k of a K-wide call equals the K = 1 call with that candidate, and image b alone equals image b of the batch, bit for bit. */
int clc_gauss_lik_step_fwd(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc, const float* noise, int ldn,
                           const float* step, float* lik, int ldl, float* y_hat, int ldh, long rows, int C, int mode, float* bits_partial,
                           int n_partials, clc_stream_t stream);
size_t clc_gauss_lik_step_bwd_workspace_bytes(long rows, int C);
int clc_gauss_lik_step_bwd(const float* dlik, int lddl, const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc,
                           const float* noise, int ldn, const float* step, float* dy, int lddy, float* dmu, int lddmu, float* dscale, int lddsc,
                           float* dstep, long rows, int C, int mode, const float* g_hat, int ldg, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_quantize_build_indexes_step(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc, const float* step,
                                    const float* scale_table, int n_scales, int32_t* symbols, int32_t* indexes, float* y_hat, int ldh,
                                    long rows, int C, clc_stream_t stream);
size_t clc_gauss_rate_sweep_workspace_bytes(int B, long rows_per_image, int C, int K);
int clc_gauss_rate_sweep(const float* y, int ldy, const float* mu, int ldmu, const float* scale, int ldsc, const float* steps, int K, int B,
                         long rows_per_image, int C, float* bits /* [B][K] */, void* ws, size_t ws_bytes, clc_stream_t stream);

/* rate / distortion reductions and their gradients (train_CLC.py:43-57). g_dev points at the upstream
 * gradient of the loss (a device scalar), so the backward never reads back to the host. */
int clc_log2_sum_partials(const float* x, int ld, long rows, int C, float* partials, int n_partials, clc_stream_t stream);
int clc_scaled_recip(const float* x, int ld, long rows, int C, const float* g_dev, float coef, float* out, int ldo,
                     clc_stream_t stream);                       /* out = g*coef / x   */
int clc_scaled_diff(const float* a, const float* b, long n, const float* g_dev, float coef, float* out,
                    clc_stream_t stream);                        /* out = g*coef*(a-b) */
/* sum of n floats (fixed order) -> out[0] (+)= scale * sum */
int clc_sum_partials(const float* partials, int n, float scale, float* out, int accumulate, clc_stream_t stream);
/* the scalar tail of RateDistortionLoss (train_CLC.py:43-59, MSE form) in one launch: the three fixed-order sums of the partials of
 * sum log2(lik_y), sum log2(lik_z), sum (x_hat - x)^2 and  bpp = (s_y + s_z) / neg_num_pixels, mse = sq / numel, loss = c * mse + bpp
 * (c = float(lmbda * 255^2)), each rounded as the reference's tensor expressions round; and the device scalars its backward hands to
 * clc_scaled_recip / clc_scaled_diff (g_* NULL: no gradient for that output). */
int clc_rd_combine(const float* py, int ny, const float* pz, int nz, const float* psq, int nsq, float neg_num_pixels, float numel, float c,
                   float* bpp, float* mse, float* loss, clc_stream_t stream);
int clc_rd_grad_scalars(const float* g_bpp, const float* g_mse, const float* g_loss, float neg_num_pixels, float numel, float c, float* g_logsum,
                        float* g_sq, clc_stream_t stream);
/* sum((a-b)^2) partials */
int clc_sqdiff_partials(const float* a, const float* b, long n, float* partials, int n_partials, clc_stream_t stream);

/* ---- Conditional Latent Matching ops (standalone module /root/reference/models/CLM.py) ---- *
 * All tensors NHWC fp32.  The first four are the inference forward; the recorded forward and the backward follow below.
 * clc_clm_sim_colsum: colsum[b][q] = sum_p softmax_q( yt[b,p,:].yrt[b,q,:] / temperature )   (CLM.py:107-109,14-20)
 * clc_clm_scale_rows: out[r][c] = w[r] * x[r][c]                                             (CLM.py:16-22)
 * clc_clm_deform:     9-tap modulated bilinear sampling, zero outside the map               (CLM.py:35-60)
 * clc_clm_fuse:       out = sum_m softmax_m(att_m[r]) * feat_m[r][c] (* sigmoid(att_m[r]) if gate) + y[r][c]
 *                                                                                            (CLM.py:118-125, SimpleCLM :166-179) */
size_t clc_clm_sim_colsum_workspace_bytes(int B, int HW);
int clc_clm_sim_colsum(const float* yt, int ldy, const float* yrt, int ldr, int B, int HW, int C, float temperature,
                       float* colsum, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_clm_scale_rows(const float* x, int ldx, const float* w, float* out, int ldo, long rows, int C, clc_stream_t stream);
int clc_clm_deform(const float* x, int ldx, const float* offset, int ldo, const float* modulation, int ldm, float* out,
                   int ldy, int B, int H, int W, int C, clc_stream_t stream);
int clc_clm_fuse(const float* const* feats, const float* const* atts, int M, int ldf, int lda, const float* y, int ldy,
                 float* out, int ldo, long rows, int C, int gate, clc_stream_t stream);

/* Recorded forward and backward of the CLM ops (csrc/clm_train.hip).  Stream-ordered, no allocation, no synchronisation, no
 * floating-point atomics: the same bits on every run.  s[p][q] = yt[p].yrt[q] / temperature, S = softmax_q(s).
 * clc_clm_sim_colsum_train: colsum as clc_clm_sim_colsum, on v_mfma_f32_32x32x2_f32, plus the row statistics the backward
 *                           recomputes S from: m[b][p] = max_q s, l[b][p] = sum_q exp(s - m)                (CLM.py:107-109,14-20)
 *                           Needs C % 4 == 0, C <= 384, HW <= 4096, 16-byte aligned rows.
 * clc_clm_sim_colsum_bwd:   g = d/d colsum;  D[p] = sum_q S[p][q] g[q],  ds = S (g[q] - D[p]),
 *                           dyt[p][:] = 1/temperature sum_q ds[p][q] yrt[q][:],  dyrt[q][:] = 1/temperature sum_p ds[p][q] yt[p][:]
 *                           (differentiates CLM.py:107-109 and the sum of :16-20).  dyt / dyrt NULL: that sweep does not run.
 * clc_clm_sigmoid:          out = sigmoid(x), the modulation of CLM.py:29 kept for the backward
 * clc_clm_scale_rows_bwd:   dw[r] = sum_c d[r][c] x[r][c];  dx[r][c] += w[r] d[r][c]  (CLM.py:16-22; dw / dx NULL: not wanted)
 * clc_clm_deform_bwd:       of out[p][c] = sum_k mod[p][k] valid[p][k] bilinear(x, p + off[p][k])[c]  (CLM.py:35-60), da = d/d out:
 *                           doff[p][2k+{0,1}] (slope of the bilinear weights inside the cell, cell index constant), dlogit[p][k] =
 *                           d_mod[p][k] mod (1 - mod) (gradient of the modulation's PRE-sigmoid value; channels 18.. / 9.. of a padded
 *                           row are zeroed), dx = the scatter, bucketed by destination pixel and summed in source order.
 *                           doff + dlogit NULL or dx NULL: that part does not run.
 * clc_clm_fuse_bwd:         of clc_clm_fuse (CLM.py:118-125, SimpleCLM :166-179): wts = softmax_m(att), F_m = feat_m (* sigmoid(att_m)),
 *                           t_m = sum_c dout[c] F_m[c]:  dfeat_m = wts_m dout (* sigmoid(att_m)),
 *                           datt_m = wts_m (t_m - sum_m' wts_m' t_m') (+ wts_m (1 - sigmoid(att_m)) t_m);  dy = dout.
 *                           Columns 1.. of a padded datt row are zeroed. */
int clc_clm_sim_colsum_train(const float* yt, int ldy, const float* yrt, int ldr, int B, int HW, int C, float temperature,
                             float* colsum, float* m, float* l, clc_stream_t stream);
size_t clc_clm_sim_colsum_bwd_workspace_bytes(int B, int HW);
int clc_clm_sim_colsum_bwd(const float* yt, int ldy, const float* yrt, int ldr, const float* m, const float* l, const float* g,
                           int B, int HW, int C, float temperature, float* dyt, int lddyt, float* dyrt, int lddyr, void* ws,
                           size_t ws_bytes, clc_stream_t stream);
int clc_clm_sigmoid(const float* x, int ldx, float* out, int ldo, long rows, int C, clc_stream_t stream);
int clc_clm_scale_rows_bwd(const float* d, int ldd, const float* x, int ldx, const float* w, float* dw, float* dx, int lddx,
                           long rows, int C, clc_stream_t stream);
size_t clc_clm_deform_bwd_workspace_bytes(int B, int H, int W);
int clc_clm_deform_bwd(const float* x, int ldx, const float* offset, int ldo, const float* modulation, int ldm, const float* da,
                       int lda, float* doff, int lddo, float* dlogit, int lddl, float* dx, int lddx, int B, int H, int W, int C,
                       void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_clm_fuse_bwd(const float* const* feats, const float* const* atts, int M, int ldf, int lda, const float* dout, int lddo,
                     float* const* dfeats, int lddf, float* const* datts, int ldda, long rows, int C, int gate, clc_stream_t stream);

/* ---- patch-matching side information (numeric core of /root/reference/models/Patch_Matching.py) ---- *
 * Planar NCHW fp32 (3-channel images), forward only.
 * clc_pm_prep:       rgb_transform(reduce_mean_and_std_normalize_images(x * in_scale))             (:913-934)
 * clc_pm_gauss_mask: create_gaussian_masks(img_h, img_w, ph, pw) -> [P, H-ph+1, W-pw+1]            (:779-807)
 * clc_pm_pearson:    L2_or_pearson_corr(q [P,C,ph,pw], y [C,H,W]) (* mask) -> [P, H-ph+1, W-pw+1]   (:854-910)
 * clc_pm_topk:       top-k positions per patch (values, flat indices), ties -> lowest index       (:105, :225)
 *                    Ordering (torch.topk / torch.argmax): NaN ranks above +inf, +inf above every finite value; equal entries
 *                    (all NaNs count as equal) -> lowest index first.  1 <= k <= min(8, npos): every index written is in
 *                    [0, npos) and no index repeats within a row, whatever the floats hold.
 * clc_pm_gather:     SI_Wraper / SI_Finder patch gather + re-tiling; temperature < 0: plain argmax copy (k = 1)
 *                    PRECONDITION (not checked on the device): every idx is a flat position of the (H-ph+1) x (W-pw+1) map of
 *                    this y, 0 <= idx < (H-ph+1)*(W-pw+1); an index outside it reads outside y. */
int clc_pm_prep(const float* x, float* out, int n_img, int H, int W, float in_scale, clc_stream_t stream);
int clc_pm_gauss_mask(float* out, int img_h, int img_w, int ph, int pw, clc_stream_t stream);
size_t clc_pm_pearson_workspace_bytes(int P, int C, int H, int W, int ph, int pw);
int clc_pm_pearson(const float* q, int P, const float* y, int C, int H, int W, int ph, int pw, const float* mask,
                   float* out, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_pm_topk(const float* corr, int P, int npos, int k, float* val, int32_t* idx, clc_stream_t stream);
int clc_pm_gather(const float* y, int C, int H, int W, int ph, int pw, const float* val, const int32_t* idx, int k,
                  float temperature, float* out, clc_stream_t stream);

/* ---- MS-SSIM distortion (pytorch_msssim.ms_ssim semantics; train_CLC.py:33-34,55-57) ---- *
 * NHWC fp32. One scale at a time: means[bc][0] = mean(cs map), means[bc][1] = mean(ssim map) over the valid 11x11
 * Gaussian (sigma 1.5) windows; bwd: dx = d(sum_bc g_means[bc][0]*mean_cs + g_means[bc][1]*mean_ssim)/dx
 * + 0.25 * dnext upsampled 2x (gradient arriving through the 2x2 average pool from the next coarser scale, or NULL).
 * clc_ssim_init() uploads the window once (call outside graph capture). */
int clc_ssim_init(void);
size_t clc_ssim_workspace_bytes(int B, int H, int W, int C);
int clc_ssim_scale_fwd(const float* x, int ldx, const float* y, int ldy, int B, int H, int W, int C, float data_range,
                       float* means, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_ssim_scale_bwd(const float* x, int ldx, const float* y, int ldy, int B, int H, int W, int C, float data_range,
                       const float* g_means, const float* dnext, float* dx, int lddx, void* ws, size_t ws_bytes,
                       clc_stream_t stream);
int clc_avgpool2(const float* x, int ldx, float* out, int B, int H, int W, int C, clc_stream_t stream);

/* ---- SSIM / MS-SSIM, descriptor form (pytorch_msssim.ssim / ms_ssim on any image size, window and input gradient) ---- *
 * The window travels by value in the descriptor (no init call, no __constant__ upload: capturable as it stands).
 * One scale at a time, same means layout as clc_ssim_scale_fwd: means[bc][0] = mean cs, means[bc][1] = mean ssim over the
 * (H - win_size + 1) x (W - win_size + 1) valid windows.  bwd writes dx and / or dy (a NULL output is not computed):
 * d(sum_bc g_means[bc][0]*mean_cs + g_means[bc][1]*mean_ssim)/d{x,y} + 0.25 * the gradient arriving through the 2x2 average pool
 * from the next coarser scale (dnext_x / dnext_y, or NULL): input row i reads coarse row (i + pad_h) / 2, columns likewise.
 * With the 11-tap sigma-1.5 window of clc_ssim_window, C1 / C2 as clc_ssim_scale_fwd forms them, and dy == NULL, the results
 * equal clc_ssim_scale_fwd / clc_ssim_scale_bwd bit for bit.
 * clc_avgpool2_pad: F.avg_pool2d(x, 2, padding=(pad_h, pad_w)) with zero padding counted (divisor 4); out is dense
 * [B, (H + pad_h) / 2, (W + pad_w) / 2, C].  pad_h / pad_w must be H % 2 / W % 2 (pytorch_msssim's padding) here and in the descriptor.
 * clc_ssim_window (HOST, no GPU): pytorch_msssim's _fspecial_gauss_1d(win_size, sigma) in fp32. */
#define CLC_SSIM_MAX_WIN 15
typedef struct {
  const float* x; int ldx;
  const float* y; int ldy;
  int B, H, W, C;
  int win_size;                  /* odd, 3 .. CLC_SSIM_MAX_WIN */
  float win[CLC_SSIM_MAX_WIN];   /* taps [0, win_size), applied along both axes */
  float C1, C2;                  /* (K1 * data_range)^2, (K2 * data_range)^2 */
  int pad_h, pad_w;              /* pooling pads toward the next coarser scale */
  float* dx; int lddx;           /* bwd outputs (NULL: not wanted; at least one is set) */
  float* dy; int lddy;
  const float* dnext_x;          /* bwd: dense [B, (H + pad_h) / 2, (W + pad_w) / 2, C] or NULL */
  const float* dnext_y;
} clc_ssim_desc;
int clc_ssim_window(int win_size, float sigma, float* taps);
size_t clc_ssim_desc_workspace_bytes(const clc_ssim_desc* d);
int clc_ssim_desc_fwd(const clc_ssim_desc* d, float* means, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_ssim_desc_bwd(const clc_ssim_desc* d, const float* g_means, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_avgpool2_pad(const float* x, int ldx, float* out, int B, int H, int W, int C, int pad_h, int pad_w, clc_stream_t stream);

/* ---- optimizer ------------------------------------------------------------------------ *
 * Multi-tensor AdamW + grad-norm clip + nan_to_num (train_CLC.py:164-179) over a flat
 * table of (param, grad, m, v, numel) entries resident on the device. */
typedef struct { float* p; float* g; float* m; float* v; long n; } clc_param_entry;
/* chunks_dev: n_chunks pairs (entry index, element offset); one workgroup per chunk of
 * clc_optim_chunk_elems() elements.  partials: n_chunks floats (sum (grad_scale * g)^2 per chunk).
 * grad_scale: 1 on one GPU; 1 / world after a SUMMED gradient all-reduce (the rank mean of run_ddp.sh:1-7 / DDP, folded into
 * the two passes that read the gradients anyway instead of a pass of its own over the arena). */
int clc_optim_chunk_elems(void);
int clc_grad_sqnorm_partials(const clc_param_entry* table_dev, const int32_t* chunks_dev, int n_chunks, float* partials,
                             float grad_scale, clc_stream_t stream);
/* state_dev[3] = {t, 1 - beta1^t, sqrt(1 - beta2^t)}: t += 1 and the two bias corrections of torch.optim.AdamW, evaluated in
 * double on the device (one thread) so the optimizer step stays graph-replayable. */
int clc_adam_tick(float* state_dev, double beta1, double beta2, clc_stream_t stream);
/* g <- nan_to_num(g * grad_scale * min(1, max_norm/(sqrt(*total_sqnorm_dev)+1e-6))) ; AdamW update with the step state
 * read from step_dev[3] (clc_adam_tick) and the learning rate from *lr_dev (device float) so a
 * captured launch is graph-replayable AND follows the MultiStepLR schedule (train_CLC.py:453,497). */
int clc_adamw_step(const clc_param_entry* table_dev, const int32_t* chunks_dev, int n_chunks, const float* total_sqnorm_dev,
                   float max_norm, const float* lr_dev, double beta1, double beta2, float eps, float weight_decay,
                   const float* step_dev, float grad_scale, clc_stream_t stream);
int clc_scalar_add(float* x_dev, float v, clc_stream_t stream);

/* ---- entropy coder (HOST, bit-exact) --------------------------------------------------- *
 * Replaces compressai.ans.BufferedRansEncoder/RansDecoder (CLC_run.py:658,712-713,762-763,793),
 * RansEncoder/RansDecoder.{encode,decode}_with_indexes behind EntropyBottleneck.compress/decompress
 * (CLC_run.py:643-644,749) and compressai._CXX.pmf_to_quantized_cdf (via update(), CLC_run.py:486-491). */
long clc_rans_encode_bound(long n_symbols);
long clc_rans_encode(const int32_t* symbols, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                     const int32_t* cdf_sizes, const int32_t* offsets, uint8_t* out, long out_cap); /* HOST */
/* The same stream from per-symbol (start, freq, esc) int32 triples (n of them, 3 n values) that the caller read from each symbol's own CDF
 * row: esc < 0 for a symbol inside its row, start = cdf[v], freq = cdf[v + 1] - cdf[v]; else esc is the escape payload `raw` of
 * clc_rans_encode (below the row's window -2 v - 1, at or above max_value 2 (v - max_value)) and (start, freq) are those of the row's
 * tail symbol.  The bytes equal clc_rans_encode's for the same symbols coded through their full rows.  Needs 0 <= start, 0 < freq < 2^16,
 * start + freq <= 2^16; anything else is refused by name.  out_cap as for clc_rans_encode (clc_rans_encode_bound). */
long clc_rans_encode_direct(const int32_t* triples, long n, uint8_t* out, long out_cap);           /* HOST */
typedef struct clc_rans_decoder clc_rans_decoder;
clc_rans_decoder* clc_rans_decoder_create(const uint8_t* stream, long nbytes);                    /* HOST, copies */
long clc_rans_decoder_decode(clc_rans_decoder* d, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                             const int32_t* cdf_sizes, const int32_t* offsets, int32_t* out);      /* HOST */
void clc_rans_decoder_destroy(clc_rans_decoder* d);
int clc_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf_out /* n+1 */);  /* HOST */

/* ---- fused ResidualUnit (forward), round 3 ----
 * One launch for CompressAI's AttentionBlock.ResidualUnit as SWAtten uses it (/root/reference/models/CLC_run.py:222-244):
 *   y = relu(x + conv1x1(W3, relu(conv3x3(W2, relu(conv1x1(W1, x) + b1)) + b2)) + b3),  C -> C/2 -> C/2 -> C, on 16x16 maps, C = 128.
 * x [N,16,16,C] pixel-major (leading dimension ldx); t1, t2 [N,16,16,C/2] and y [N,16,16,C] dense outputs — t1 / t2 are the activated
 * outputs of the first two layers, which the ordinary gradient kernels (clc_conv2d transposed / clc_conv2d_wgrad) take as saved
 * activations, so the backward pass of the three layers is unchanged.  sets = 1, 2 or 4 filter sets on equal parts of the batch
 * (images [k N/sets, (k+1) N/sets) use set k), filters in clc_conv2d's layout ([Cout][kh][kw][Cin]).  A result depends on its own
 * image only (one workgroup per 8x4-pixel tile, fixed summation order). */
typedef struct {
  const float* x; int ldx;
  float* t1; float* t2; float* y;
  int N, H, W, C, sets;
  const float* w1[4]; const float* b1[4];
  const float* w2[4]; const float* b2[4];
  const float* w3[4]; const float* b3[4];
  const float* saved_y; const float* saved_t2; const float* saved_t1;   /* clc_residual_unit_dgrad only */
} clc_ru_desc;
int clc_residual_unit_fwd(const clc_ru_desc* d, clc_stream_t stream);
/* The unit's data gradient, one launch: with x = dy (leading dimension ldx), w1 / w2 / w3 = the TRANSPOSED filters of layers 3 / 2 / 1
 * (clc_filter_transpose: [64][128], [64][9][64], [128][64]; biases unused) and the forward pass's saved_y / saved_t2 / saved_t1 (dense),
 * writes  t1 <- g2 = d(layer-2 pre-activation),  t2 <- g1 = d(layer-1 pre-activation)  (the dy operands of those layers' filter
 * gradients; layer 3's is dy gated by saved_y, which clc_conv2d_wgrad applies itself) and  y <- dx  (including the identity branch). */
int clc_residual_unit_dgrad(const clc_ru_desc* d, clc_stream_t stream);

/* ---- fused Swin-block MLP, round 4 ----
 * `x + mlp(ln2(x))` of Block (/root/reference/models/CLC_run.py:185-187, 190-192) for the ConvTransBlocks' Swin blocks (trans_dim 64):
 *   clc_mlp_fwd   y = res + W2 . gelu(W1 . x + b1) + b2     x [M][64] (leading dimension ldx) -> y [M][64] (ldy), res optional (ldr);
 *                 w1 [256][64], w2 [64][256] (nn.Linear layout = clc_conv2d's 1x1 filter layout).  The 256-channel hidden tensor is
 *                 never written: it goes from the first GEMM's accumulator registers straight into the second GEMM's operands.
 *   clc_mlp_bwd   the block's whole DATA gradient from (x, dy) with the hidden tensor RECOMPUTED (fc1 again from the saved input):
 *                 dh [M][256] = (W2^T dy) . gelu'(h)  and  g [M][256] = gelu(h)  (dense; the dy / x operands of fc1's / fc2's
 *                 filter gradients, which stay on clc_conv2d_wgrad*), dx [M][64] (lddx) = W1^T dh.  w2t = clc_filter_transpose(w2)
 *                 ([256][64]).
 * Same summation order per output element and same epilogue expressions as the clc_conv2d launches they replace (fc1 + GELU with the
 * stored derivative, fc2 + residual; their transposed / out_gate forms backward): THE SAME BITS, so either path may serve the codec.
 * M = pixels (N * H * W of a pixel-major tensor), a multiple of 32.  Persistent workgroups, filters resident in LDS (129 KB). */
typedef struct {
  const float* x; int ldx;
  const float* w1; const float* b1;
  const float* w2; const float* b2;
  const float* res; int ldr;
  float* y; int ldy;
  long M; int Cin, Chid, Cout;          /* 64, 256, 64 */
  /* clc_mlp_bwd only */
  const float* dy; int lddy;
  const float* w2t;
  float* dx; int lddx;
  float* dh; float* g;
  /* optional, both directions: h [M][256] dense = the fc1 PRE-activation (W1 x + b1).  clc_mlp_fwd writes it when non-NULL (training,
   * "save" mode); clc_mlp_bwd then reads it instead of recomputing it (256 of a tile's 768 MFMAs for 134 MB of traffic per 8x128x128). */
  float* h;
  /* optional, both directions: the LayerNorm in front (Block.ln2, CLC_run.py:183,192).  ln_gamma / ln_beta [64] non-NULL: x is the block's RAW
   * input and the kernels compute  y = x + mlp(LN(x))  (res must be NULL — the residual is x; h must be NULL).  clc_mlp_fwd also writes LN(x)
   * to ln_out [M][64] dense when that is non-NULL (training).  clc_mlp_bwd reads it back (fc1's operand again; it is also the x operand of
   * fc1's filter gradient), needs a dense x, returns in dx the gradient of the whole expression (clc_layernorm_bwd's result with dy folded in
   * as dx_add) and leaves clc_mlp_blocks(M) partial rows [2][64] (dgamma, dbeta) in ln_ws for clc_partial_reduce_batched.  LN(x), y and dx
   * carry the bits of clc_layernorm_fwd / clc_layernorm_bwd around the plain form. */
  const float* ln_gamma; const float* ln_beta;
  float* ln_out; float* ln_ws;
} clc_mlp_desc;
int clc_mlp_fwd(const clc_mlp_desc* d, clc_stream_t stream);
int clc_mlp_bwd(const clc_mlp_desc* d, clc_stream_t stream);
int clc_mlp_blocks(long M);   /* workgroups (= partial rows in ln_ws) of a clc_mlp_bwd / clc_lnlin_bwd launch over M pixels */

/* ---- LayerNorm + Linear: ln1 and the window attention's embedding, round 4 ----
 * `self.embedding_layer(self.ln1(x))` of Block / WMSA (/root/reference/models/CLC_run.py:120, 141, 180, 191; nn.LayerNorm(64), nn.Linear(64, 192)):
 *   clc_lnlin_fwd   y [M][192] dense = W . LN(x) + b, x [M][64] (ldx: may be a channel range of a wider buffer); writes LN(x) to ln_out [M][64]
 *                   dense when non-NULL (training: the x operand of the Linear's filter gradient, which stays clc_conv2d_wgrad*).
 *   clc_lnlin_bwd   dx [M][64] (lddx) = LayerNorm gradient of (W^T dy) + dadd (the block's residual gradient, ldadd; optional), from dy [M][192]
 *                   dense, wt = clc_filter_transpose(w) ([64][192]) and the raw x; clc_mlp_blocks(M) partial rows [2][64] (dgamma, dbeta) in ln_ws
 *                   for clc_partial_reduce_batched.
 * y and dx carry the bits of clc_layernorm_fwd + clc_conv2d (1x1) / clc_conv2d (transposed) + clc_layernorm_bwd.  M a multiple of 32. */
typedef struct {
  const float* x; int ldx;
  const float* ln_gamma; const float* ln_beta;
  const float* w; const float* b;
  float* y; float* ln_out;
  long M; int Cin, Cout;                /* 64, 192 */
  /* clc_lnlin_bwd only */
  const float* dy; const float* wt;
  float* dx; int lddx;
  const float* dadd; int ldadd;
  float* ln_ws;
} clc_lnlin_desc;
int clc_lnlin_fwd(const clc_lnlin_desc* d, clc_stream_t stream);
int clc_lnlin_bwd(const clc_lnlin_desc* d, clc_stream_t stream);

/* ---- GDN / IGDN data gradient in one launch, round 4 ----
 * CompressAI GDN (y = x * (beta + gamma . x^2)^-1/2, inverse: ^+1/2; g_a / g_s, /root/reference/models/CLC_run.py:296-318, 337-353) on a dense
 * 128-channel map with >= 32 768 pixels: from dy, x and the saved norm v (clc_conv2d's y_pre) -> dv [M][128] = d(loss)/d(v) (the dy operand of
 * gamma's filter gradient) and dx [M][128] = dy * v^-+1/2 + 2 x (gamma_eff^T dv).  Replaces clc_gdn_bwd_elem + the transposed 1x1 clc_conv2d with
 * norm = CLC_NORM_MUL2 (their bits), without the dx_direct tensor.  gamma_eff_t = the [Cin][Cout] image clc_gdn_reparam_fwd writes. */
int clc_gdn_bwd_fused(const float* dy, const float* x, const float* v, const float* gamma_eff_t, float* dv, float* dx, long M, int C, int inverse,
                      clc_stream_t stream);

/* ---- reference-retrieval feature extractor: the pooling layers of torchvision's ResNet50 as the reference uses it ----
 * clc_maxpool2d        nn.MaxPool2d(ks, stride, pad) of resnet50.maxpool (/root/reference/dataloader_ref_cluster.py:41-44, dataloader_CLC.py:275),
 *                      pixel-major in / out, C and the leading dimensions multiples of 4.
 * clc_adaptive_pool2d  F.adaptive_avg_pool2d(x, (1, 1)) (resnet50.avgpool) and the spatial-pyramid levels
 *                      F.adaptive_max_pool2d(x, (L, L)), L = 1, 2, 4 (/root/reference/dataloader_CLC.py:250-256, 282-286); out = [N][C][L][L]
 *                      floats in NCHW order (the order h.view(N, -1) flattens). */
int clc_maxpool2d(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int ks, int stride, int pad, int OH, int OW, clc_stream_t stream);
int clc_adaptive_pool2d(const float* x, int ldx, float* out, int N, int H, int W, int C, int L, int is_max, clc_stream_t stream);

/* ---- reference bank of the codec (clc_amd/refbank.py; the reference prepares its references in eval_CLC.py:246-257, 306-315) ---- *
 * clc_ref_prepare: N reference images, table[n] = {planar NCHW fp32 [3, h_n, w_n] in [0, 1], h_n, w_n} (the TABLE lives in device memory)
 *   -> out channels_last [N, 3, H, W] = pad(F.interpolate(r, (h, w), mode="bilinear", align_corners=False), 128), H / W = h / w rounded up
 *   to 128, the image centred (clc_amd.eval.pad).  ATen's source-index rule; index, weights and blend in double, rounded once to fp32; an
 *   image that already has size (h, w) is copied exactly.  One launch for every image of the table.  Its bits feed the reference encoder,
 *   i.e. the context model: a change to its arithmetic needs a new kernel generation (clc_kernel_config_tag).
 * clc_gather_slots: channels_last latents, one slot = slot_elems floats (a multiple of 4, 16-byte aligned):
 *   out[r*B + b] = arena[idx[b*R + r]] (reference-major, the layout ref_encoder(cat(refs)) returns).  idx [B, R] lives in device memory,
 *   so a captured graph replays the gather with new slots after one small host-to-device copy; an index outside [0, n_slots) yields NaN.
 * clc_fingerprint: out[0] = sum over every 32-bit word of every buffer of mix((global word index << 32) | word) mod 2^64 (a tail of 1-3
 *   bytes zero-extended; word_offset = the buffer's first global word index).  Independent of the grid; partials = n_partials words of
 *   caller scratch (1..4096). */
typedef struct {
  const float* src; int h; int w;
} clc_ref_src;
typedef struct {
  const void* ptr; uint64_t nbytes; int64_t word_offset;
} clc_fp_entry;
int clc_ref_prepare(const clc_ref_src* table, int N, int h, int w, float* out, clc_stream_t stream);
int clc_gather_slots(const float* arena, long slot_elems, int n_slots, const int32_t* idx, int B, int R, float* out, clc_stream_t stream);
int clc_fingerprint(const clc_fp_entry* table, int n, uint64_t* partials, int n_partials, uint64_t* out, clc_stream_t stream);

/* ---- full-batch Lloyd k-means for the reference-retrieval dictionary (clc_amd/kmeans.py, kmeans.hip) ----
 * x [N][D] f32 rows (ldx), c [K][D] centres (ldc): rows 16-byte aligned, ld >= D and a multiple of 4, D >= 4 a multiple of 4 (no upper
 * bound: the D loop is chunked), 1 <= K <= N (clc_kmeans_assign: any K >= 1).  Stream-ordered, allocation-free, sync-free; every sum has a fixed order (same bits on every run).
 * clc_kmeans_assign           label[i] = argmin_k (c_sqnorm[k] - 2 x_i.c_k) on v_mfma_f32_32x32x2_f32, equal scores -> lowest k (the tie rule of
 *                             clc_pm_topk); score[i] = that minimum, so |x_i - c_label|^2 = |x_i|^2 + score[i].  [N][K] is never written.
 * clc_kmeans_update           c_out[k] = mean of the rows with label k, counts[k] = their number; an empty cluster copies prev_c[k] bit for bit.
 *                             order [N] = the row indices sorted by label, rows of one label ascending (a stable sort of label); lists longer than
 *                             512 rows are summed in 512-row chunks by separate waves, the partials added in chunk order.  Labels must lie
 *                             in [0, K) (anything else: unspecified centres, but no access outside the buffers).  ws: clc_kmeans_update_workspace_bytes(N, D, K), 16-byte aligned.
 * clc_kmeans_representatives  rep[k] = the row with label k that minimises sum_d (x - c_k)^2 (f32, lanes over columns), the lowest row on a tie;
 *                             -1 for an empty cluster.  ws: clc_kmeans_representatives_workspace_bytes(K). */
int clc_kmeans_assign(const float* x, int ldx, int N, int D, const float* c, int ldc, int K, const float* c_sqnorm, int32_t* label, float* score,
                      clc_stream_t stream);
size_t clc_kmeans_update_workspace_bytes(int N, int D, int K);
int clc_kmeans_update(const float* x, int ldx, int N, int D, const int32_t* label, const int32_t* order, int K, const float* prev_c, int ldp,
                      float* c_out, int ldc, int32_t* counts, void* ws, size_t ws_bytes, clc_stream_t stream);
size_t clc_kmeans_representatives_workspace_bytes(int K);
int clc_kmeans_representatives(const float* x, int ldx, int N, int D, const int32_t* label, const int32_t* order, const float* c, int ldc, int K,
                               int32_t* rep, void* ws, size_t ws_bytes, clc_stream_t stream);

/* ---- the sequential part of the autoregressive context model (mbt2018, JointAutoregressiveHierarchicalPriors; ar_context.hip) ----
 * What they replace: the per-pixel body of CompressAI's `_compress_ar` / `_decompress_ar` loops — F.conv2d of a 5x5 crop with the
 * masked filter, the three 1x1 layers of `entropy_parameters` on cat((params pixel, context)), `build_indexes`, `quantize(.., "symbols",
 * means)` and the write-back `y_hat[h, w] = symbols + means` — which the published coder runs on the CPU, one pixel at a time.
 *
 * Rows of a call are r = b * P + p for image b < B and entry p of a PIXEL LIST: P pairs (h, w) of int32 in device memory (a whole
 * schedule is uploaded once, a step is an offset into it).  A pair outside the H x W map is neither read nor written.
 *
 * clc_ar_linear   out[r][n] = act(bias[n] + sum_k in(r, k) * w[n][k]), out a dense [rows][ldo] workspace, act CLC_ACT_NONE or
 *                 CLC_ACT_LRELU, w [N][K] row-major, N arbitrary.  The K axis is one or two consecutive ranges (clc_ar_src):
 *                   CLC_AR_SRC_DENSE  row r of a dense [rows][ld] buffer, K = C;
 *                   CLC_AR_SRC_PIXEL  the C channels of the row's own pixel of an NHWC [B][H][W][ld] map, K = C;
 *                   CLC_AR_SRC_TAPS   the 12 live taps of mask A of an NHWC map in (kh, kw) ascending order — (0,0..4), (1,0..4), (2,0),
 *                                     (2,1) of the 5x5 window centred on the pixel — C channels each, K = 12 C; taps outside the map are zeros.
 *                 ORDER RULE: every output element is summed in an order fixed by the K of each range alone (lane l of a wave takes the
 *                 16-byte chunks l, l + 64, ... of each range in turn into one accumulator, then the 64 lanes are added by an xor
 *                 butterfly): not by P, B, the row's place in the list, the pixel's place in the map or the grid.  An encoder step of many
 *                 rows and a decoder step of one therefore give the same bits.  Any row count.  Requires C % 4 == 0, ld % 4 == 0,
 *                 16-byte aligned bases.
 * clc_ar_finish   gp is a dense [rows][ldg] buffer, scales in columns [0, M), means in [M, 2M) (chunk(2, 1)).
 *                   CLC_AR_ENCODE  sym = round(y - mean), y_hat = sym + mean, idx = build_indexes(scale): the arithmetic of
 *                                  clc_quantize_build_indexes, bit for bit.  y_hat goes into the NHWC map (which may be y itself),
 *                                  sym and idx to int32 [B][H*W][M] at the pixel's raster place.
 *                   CLC_AR_DECODE  idx to a dense [rows][M] int32 buffer; gp keeps the means for clc_ar_commit.
 * clc_ar_commit   y_hat[pixel] = symbols[r] + mean from decoded symbols (dense [rows][M] int32): the expression of CLC_AR_ENCODE.
 * All three: stream-ordered, graph-capturable, allocation- and sync-free, no workgroup waits on another. */
enum { CLC_AR_SRC_DENSE = 0, CLC_AR_SRC_PIXEL = 1, CLC_AR_SRC_TAPS = 2 };
enum { CLC_AR_ENCODE = 0, CLC_AR_DECODE = 1 };
typedef struct { const float* p; int ld; int C; int kind; } clc_ar_src;
int clc_ar_linear(const clc_ar_src* srcs /* HOST */, int nsrc, const int32_t* pix, int P, int B, int H, int W, const float* w, const float* bias,
                  int N, int act, float* out, int ldo, clc_stream_t stream);
int clc_ar_finish(const float* gp, int ldg, int M, const int32_t* pix, int P, int B, int H, int W, const float* scale_table, int n_scales,
                  const float* y, int ldy, float* y_hat, int ldh, int32_t* symbols, int32_t* indexes, int mode, clc_stream_t stream);
int clc_ar_commit(const int32_t* symbols, const float* gp, int ldg, int M, const int32_t* pix, int P, int B, int H, int W, float* y_hat,
                  int ldh, clc_stream_t stream);

/* ---- the checkerboard context layer (He et al., CVPR 2021; JointCheckerboardHierarchicalPriors; ckbd_context.hip) ----
 * What they replace: the dense masked layer — layers.MaskedConv2d -> conv5_kernel on the 25-tap filter with 13 taps multiplied by zero,
 * then zeroing the anchors of the result — which spends 25 * 2 / 12 = 4.2 times the multiplications the layer needs.
 *
 * PARITY: a pixel (h, w) of the NHWC [B][H][W][ld] map is an ANCHOR iff (h + w) is odd, a NON-ANCHOR iff (h + w) is even; (0, 0) is a
 * non-anchor.  TAPS: (kh, kw) of the 5x5 / pad-2 window is live iff (kh + kw) is odd: 12 taps, in (kh, kw) ascending order
 *   (0,1) (0,3) (1,0) (1,2) (1,4) (2,1) (2,3) (3,0) (3,2) (3,4) (4,1) (4,3)
 * — the centre is not one of them, a live tap of a non-anchor lands on an anchor or outside the map, and the set is symmetric under
 * (kh, kw) -> (4 - kh, 4 - kw).  Filters are [Cout][12][Cin] in that tap order.
 *
 * clc_ckbd_conv   transposed = 0: y[non-anchor p][co] = act(bias[co] + sum_t sum_ci x[p + offset_t][ci] w[co][t][ci]), y[anchor] = 0.0f
 *                 exactly (no bias); act CLC_ACT_NONE or CLC_ACT_LRELU.  transposed = 1 (the data gradient; x is dy with Cin = the
 *                 layer's output channels, w the [Cin][12][Cout] image clc_filter_transpose(w, Cout, 12, Cin) makes of the layer's
 *                 filter): y[anchor p] = sum_t x[p - offset_t] w[.][t][.], y[non-anchor] = 0.0f; p - offset_t is a non-anchor, an
 *                 anchor's x is never read.  ONE launch writes every element of the output map (no memset needed), no workspace.
 *                 ORDER RULE: taps outside the map contribute exact zeros and are never skipped; every output element is summed in
 *                 the order (tap ascending, 32-channel chunks ascending, inside a chunk by MFMA and lane half) — a function of Cin
 *                 alone, not of B, the image's place in the batch, H, W or the tile the pixel lands in.  A stream written from a batch
 *                 of 8 therefore decodes one image at a time.
 * clc_ckbd_wgrad  dw[co][t][ci] (+)= sum over the non-anchor pixels p of all images of dy[p][co] x[p + offset_t][ci]; an anchor's dy is
 *                 never read.  A single pass: every dw element is written once by one lane (read-modified-written with accumulate);
 *                 no atomics, no workspace.  The bias gradient is the column sum of dy over the non-anchor pixels (clc_colsum of a
 *                 masked dy).
 * Both: Cin % 4 == 0, ldx % 4 == 0, 16-byte aligned x (and w), any Cout (16-byte stores when Cout % 4 == 0, ldy % 4 == 0 and y is
 * aligned, scalar otherwise), any H, W >= 1, B * H * W < 2^31; anything else is refused by name.  Stream-ordered, graph-capturable,
 * allocation- and sync-free, no workgroup waits on another. */
typedef struct {
  const float* x; int B, H, W, Cin, ldx;   /* NHWC input map (transposed: dy) */
  const float* w;                          /* [Cout][12][Cin] */
  const float* bias;                       /* [Cout] or NULL */
  float* y; int Cout, ldy;                 /* NHWC output map, written whole */
  int transposed;                          /* 0 forward (non-anchors), 1 data gradient (anchors) */
  int act;                                 /* CLC_ACT_NONE or CLC_ACT_LRELU */
} clc_ckbd_desc;
typedef struct {
  const float* x; int B, H, W, Cin, ldx;   /* the layer's input map */
  const float* dy; int Cout, lddy;         /* gradient of the layer's output map (read at non-anchors only) */
  float* dw;                               /* [Cout][12][Cin] */
  int accumulate;                          /* 0: dw = ..., 1: dw += ... */
} clc_ckbd_wgrad_desc;
int clc_ckbd_conv(const clc_ckbd_desc* d, clc_stream_t stream);
int clc_ckbd_wgrad(const clc_ckbd_wgrad_desc* d, clc_stream_t stream);

/* ---- the batch-invariant row GEMM of the space-channel context model (ELIC, He et al., CVPR 2022; models.Elic2022; row_gemm.hip) ----
 * What it replaces: the 1x1 "parameter aggregation" layers of the per-group checkerboard passes on clc_ar_linear — one wave per (output
 * channel, 8 rows) on the plain VALU, every wave re-reading its rows and its filter row — at the 768 .. 6 144 rows and 704 .. 1 408 ->
 * 640 -> 512 channels such a pass has.
 *
 * clc_row_gemm    the contract of clc_ar_linear: rows r = b * P + p over a pixel list, w [N][K] row-major with K = sum of C_s,
 *                 out[r][n] = act(bias[n] + sum_k in(r, k) * w[n][k]) into a dense [rows][ldo] buffer.  nsrc is 1 to 4 consecutive K
 *                 ranges, each CLC_AR_SRC_DENSE or CLC_AR_SRC_PIXEL (CLC_AR_SRC_TAPS is refused by name: the gather stays with
 *                 clc_ar_linear); act is CLC_ACT_NONE, CLC_ACT_LRELU or CLC_ACT_RELU.  f32 on v_mfma_f32_32x32x2_f32: a workgroup of
 *                 four waves owns 128 rows x 64 output channels, a K-step is 32 channels of one range, both operands go through
 *                 [rows][32 + 4] LDS images, two stages, one barrier per step.  A row whose pixel lies outside the H x W map is
 *                 zero-filled on load and never stored.
 *                 ORDER RULE: every output element sums its ranges in order, within a range the 32-channel chunks ascending — the last
 *                 chunk of a range zero-filled on both operands, never skipped — and inside a chunk by MFMA and lane half (lane half h
 *                 takes k = 8 ks + 4 h + {0..3}, ks = 0..3); then bias + sum, then the activation.  A function of (C_1, ..., C_nsrc)
 *                 alone: not of P, B, the row's place in the list, the tile it lands in or the grid.  This is NOT the order of
 *                 clc_ar_linear: the two are not interchangeable inside one stream.
 * Requires per range C % 4 == 0, ld % 4 == 0, ld >= C and a 16-byte aligned base, a 16-byte aligned w, ldo >= N; any N >= 1 (16-byte
 * stores when N % 4 == 0, ldo % 4 == 0 and out is aligned, scalar otherwise), any row count with B * P < 2^31, B * H * W < 2^31;
 * anything else is refused by name.  Stream-ordered, graph-capturable, allocation- and sync-free, no workspace, no workgroup waits on
 * another. */
int clc_row_gemm(const clc_ar_src* srcs /* HOST */, int nsrc, const int32_t* pix, int P, int B, int H, int W, const float* w, const float* bias,
                 int N, int act, float* out, int ldo, clc_stream_t stream);

/* ---- the Gaussian-mixture entropy model of cheng2020 (Cheng et al., CVPR 2020; models.Cheng2020Anchor / Cheng2020Attention, K > 1; gmm.hip) ----
 * Every latent element has K weight logits, means and scales of its own, so the 64-row scale table of the other coders does not apply.
 *
 * Parameter groups.  scales, means and weights are three base pointers with ONE leading dimension ldp; a group is K blocks of C channels,
 * component k of channel c at [row * ldp + k * C + c] — channel ranges of the one map entropy_parameters writes are read in place.
 *
 * clc_gmm_likelihood_fwd   lik = max(sum_k softmax_k(weights) [Phi((1/2 - |v - mu_k|) / s_k) - Phi((-1/2 - |v - mu_k|) / s_k)], 1e-9) with
 *                          s_k = max(scale_k, 0.11), Phi(x) = erfc(-x / sqrt 2) / 2, v = y + noise (mode 0) or round(y) (mode 1).
 * clc_gmm_likelihood_bwd   from dlik: dy (mode 0 only; pass NULL in mode 1, where v does not depend on y), and dscales / dmeans / dweights
 *                          as three base pointers with one leading dimension lddp, laid out like the parameters.  Both LowerBounds
 *                          pass the gradient where the input is at or above the bound or the gradient is negative.
 * NHWC f32 [rows][ld] maps, one pass.  Any C >= 1, K in 1 .. 4; 16-byte accesses when C % 4 == 0 and every base and leading dimension is
 * 16-byte aligned, scalar ones otherwise.
 *
 * THE ROW RULE of the coder — per element (row r, channel c), from the 3 K parameters gp[r][part * K * N + k * N + c] (part 0 scales,
 * 1 means, 2 weight logits), everything in f32:
 *   pi = softmax(logits) (max subtracted), s_k = max(scale_k, 0.11), ctr = round(sum_k pi_k mu_k) clamped to [-2^20, 2^20] (NaN: -2^20);
 *   R = CLC_GMM_R, L = 2 R + 1 regular symbols j = 0 .. L - 1 for the values offset + j, offset = ctr - R, and one tail symbol j = L
 *   that carries everything outside through the bypass escape: a GaussianConditional table row with size = L + 2, max_value = L;
 *   F_j = sum_k pi_k Phi((offset + j - 1/2 - mu_k) / s_k) for j = 0 .. L, summed k ascending, then sent into [0, 1] by comparisons that
 *   put a NaN at 0;  G_0 = F_0, G_j = max(G_{j-1}, F_j);
 *   cdf[j] = j + floor((G_j - G_0) * S), S = 65535 - L, for j = 0 .. L;  cdf[L + 1] = 65536.
 * So every regular frequency is >= 1, the tail's is >= 1 and the total is 2^16, for ANY float parameters (NaN and +-Inf included).
 * The symbol is round(y) clamped to [-2^24, 2^24] (NaN: -2^24).
 *
 * clc_gmm_finish   rows r = b * P + p over a pixel list like clc_ar_finish; gp a dense [rows][ldg] buffer, ldg >= 3 K N.
 *                    CLC_AR_ENCODE  sym = round(y[pixel]); y_hat[pixel] = (float)sym; triples[(r * N + c) * 3 ..] = (start, freq, esc) for
 *                                   clc_rans_encode_direct (a pixel outside the map is neither read nor written).
 *                    CLC_AR_DECODE  cdf_rows[(r * N + c) * CLC_GMM_ROW_STRIDE ..] = the row, offsets[r * N + c] = offset.
 *                  Both modes run the same scan, so an encoder's (start, freq) are the decoder's row entries bit for bit.
 * clc_gmm_commit   y_hat[pixel][c] = (float)symbols[r * N + c] from decoded symbols (dense [rows][N] int32).
 *
 * clc_gmm_decode_step   the decoder of the SPLIT stream (clc_amd/ans.py: split_pack), on the device: one step of the wavefront for the
 *                  whole batch with no copy to the host.  An image's y symbols are dealt to S independent rANS sub-streams, channel c
 *                  to sub-stream c mod S; sub-stream s of image b is the 32-bit words words[first .. first + count) with
 *                  (first, count) = spans[(b * S + s) * 2 ..], and its decoder's state is state[b * S + s] (x, pos: the words consumed
 *                  so far; a fresh decoder has x = word 0 | word 1 << 32, pos = 2), carried in device memory from call to call.
 *                  One wave per (b, s), four waves per workgroup.  The wave walks the list's pixels p = 0 .. P - 1 in list order and
 *                  per pixel its channels c = s, s + S, ... < N; a pixel outside the map is neither read nor written and consumes
 *                  nothing.  PER SYMBOL, from the parameter row gp[(b * P + p) * ldg ..] at channel c:
 *                    pi, s_k, ctr, offset as THE ROW RULE has them (the code of clc_gmm_finish);
 *                    lane l evaluates F_l, lanes 0 and 1 also F_64 and F_65 (L = 65: the 66 edges j = 0 .. L); G_j is the running
 *                    maximum in j order (an inclusive max-scan over the lanes, continued into the two extra edges; max is exact, so
 *                    the scan's shape changes no bit); cdf[j] = j + floor((G_j - G_0) * S'), S' = 65535 - L, cdf[L + 1] = 65536: the
 *                    row of clc_gmm_finish bit for bit, never written to memory;
 *                    cf = x & 0xFFFF; the symbol's place v = #{j in 1 .. L : cdf[j] <= cf} (a ballot and a popcount);
 *                    x = (cdf[v + 1] - cdf[v]) * (x >> 16) + cf - cdf[v]; then, as after every nibble below, while-free renorm:
 *                    if x < 2^31: x = x << 32 | word[pos] (zero at or past count), pos += 1;
 *                    v == L, the tail: a nibble n = x & 15, x >>= 4 (and one more, added, if the first was 15 — never more than two),
 *                    then min(n, 16) payload nibbles LSB first, the first 8 of them kept as raw; value = raw >> 1, and
 *                    v = -value - 1 if raw is odd, else value + L: what clc_rans_decoder_decode reads;
 *                    y_hat[pixel][c] = (float)(v + offset).
 *                  When the wave is done, (x, pos) go back to state.  On every stream clc_rans_encode_direct can produce, the symbols
 *                  are those of clc_rans_decoder_decode through the rows of clc_gmm_finish, and a sub-stream decoded to its end
 *                  leaves x == 2^31 and pos == count.  On any other words they are some wrong symbols: every loop is bounded by a
 *                  constant or the symbol count, and no word outside [first, first + count) is read (a negative first or count
 *                  reads nothing).  The caller keeps first + count inside the words buffer.
 *                  Requires K in 1 .. 4, S in 1 .. 64, S <= N, ldg >= 3 K N, ldh >= N, B * H * W < 2^31.
 * All stream-ordered, graph-capturable, allocation- and sync-free; no workspace, no LDS, no barrier; no workgroup (and in
 * clc_gmm_decode_step no wave) waits on another.  Bad arguments are refused by name before any launch. */
#define CLC_GMM_R 32
#define CLC_GMM_ROW_STRIDE (2 * CLC_GMM_R + 3)
int clc_gmm_half_width(void);   /* CLC_GMM_R of the built library */
int clc_gmm_likelihood_fwd(const float* y, int ldy, const float* noise, int ldn, const float* scales, const float* means, const float* weights,
                           int ldp, float* lik, int ldl, long rows, int C, int K, int mode, clc_stream_t stream);
int clc_gmm_likelihood_bwd(const float* dlik, int lddl, const float* y, int ldy, const float* noise, int ldn, const float* scales,
                           const float* means, const float* weights, int ldp, float* dy, int lddy, float* dscales, float* dmeans,
                           float* dweights, int lddp, long rows, int C, int K, int mode, clc_stream_t stream);
int clc_gmm_finish(const float* gp, int ldg, int N, int K, const int32_t* pix, int P, int B, int H, int W, const float* y, int ldy, float* y_hat,
                   int ldh, int32_t* triples, int32_t* cdf_rows, int32_t* offsets, int mode, clc_stream_t stream);
int clc_gmm_commit(const int32_t* symbols, int N, const int32_t* pix, int P, int B, int H, int W, float* y_hat, int ldh, clc_stream_t stream);
typedef struct { uint64_t x; uint32_t pos; uint32_t pad; } clc_gmm_substream_state;   /* 16 bytes, DEVICE memory */
int clc_gmm_decode_step(const float* gp, int ldg, int N, int K, const int32_t* pix, int P, int B, int H, int W, const uint32_t* words,
                        const int32_t* spans /* [B][S][2]: first word, word count */, clc_gmm_substream_state* state /* [B][S] */, int S,
                        float* y_hat, int ldh, clc_stream_t stream);

/* ---- the lane-interleaved ("lanes") rANS stream: host coder (csrc/rans_host.cpp) and device coder (csrc/rans_lanes.hip) ----
 * A table-coded stream (clc_rans_encode's tables: cdfs [n_rows][cdf_stride], cdf_sizes, offsets) re-cut so that one GPU wave codes 64
 * symbols per step.  An image's symbols are P SEGMENTS of n_p symbols (a model's parallel passes: inside a segment every index is known
 * before the first symbol is decoded), coded by W WAVE STREAMS, 1 <= W <= 16, of 64 rANS LANES each.
 *   Placement.  Symbol j of a segment lies in chunk q = j / 64 and lane l = j % 64; chunk q belongs to wave q % W.  A wave takes its
 *   chunks of a segment in ascending q, one chunk per ROUND, and its rounds run on across the segments.  In a segment's last chunk the
 *   lanes with j >= n_p are idle: no state change, no word.  A segment with n_p = 0 contributes nothing.
 *   Per lane the arithmetic is clc_rans_encode's / clc_rans_decoder_decode's: 64-bit state, L = 2^31, 32-bit words, 16-bit precision;
 *   a symbol outside its row is the row's tail symbol followed by the 4-bit bypass escape — here always ONE count nibble nb <= 8 and
 *   then the nb payload nibbles of raw, LSB first (raw = -2 v - 1 below the row, 2 (v - max_value) at or above it).
 *   A wave stream is an array of 32-bit words DEFINED BY THE DECODER'S READS.  It starts with the 64 lane states, 128 words: lane l's low
 *   word at 2 l, its high word at 2 l + 1; pos starts at 128.  Per round the wave runs SUB-STEPS t = 0, 1, 2, ...; in sub-step t every
 *   active lane that has a t-th operation performs it:
 *     operation 0   cf = x & 0xFFFF; s = the largest s <= max_value with cdf[s] <= cf; x = (cdf[s + 1] - cdf[s]) * (x >> 16) + cf - cdf[s];
 *     operations 1 ..   only for a lane with s == max_value (the tail): a count nibble (v = x & 15, x >>= 4; a second one, added, if the
 *                   first was 15 — an encoder never writes one), then min(count, 16) payload nibbles, the first 8 of them kept as raw;
 *                   the symbol is -(raw >> 1) - 1 if raw is odd, else (raw >> 1) + max_value;
 *     every operation ends with the renorm: if x < 2^31, x = x << 32 | word[pos'] (zero at or past the stream's end).
 *   WITHIN A SUB-STEP THE LANES THAT RENORMALISE TAKE THE NEXT WORDS IN ASCENDING LANE ORDER (lane l reads word pos + #{renormalising
 *   lanes below l}; then pos += their number).  The round ends when no lane has an operation left — at most 1 + 2 + 16 sub-steps.
 *   The decoded symbol is the value + offsets[index].
 *   The encoder is the exact reverse: every lane starts at x = 2^31; rounds descending, sub-steps descending, lanes descending, words
 *   written backward (enc_put / enc_put_bits: at most one word per operation, at most 10 operations per symbol); then the 64 states.
 *   So a wave stream of n_w symbols never exceeds 128 + 10 n_w words (clc_rans_lanes_bound, in bytes), and a stream decoded to its end
 *   leaves every lane at x == 2^31 and pos == the word count.  (Overhead against the one stream of clc_rans_encode: 512 W bytes of
 *   states, plus the container's header — clc_amd/ans.py: lanes_pack.)
 *
 * HOST (rans_host.cpp), the oracle and the fallback:
 * clc_rans_lanes_encode_host  one image: symbols / indexes in stream order (the segments back to back), seg_len[P] -> the W wave streams
 *                    back to back in out, lengths[w] = bytes of stream w; returns the total bytes.  out_cap >= the sum over the waves of
 *                    clc_rans_lanes_bound(n_w).  Refused by name: W outside 1 .. 16, a negative segment length, an index outside the
 *                    table, a bad cdf size (below 2 or above cdf_stride), a zero-frequency symbol, a buffer too small.
 * clc_rans_lanes_decoder_create  from the W wave streams back to back (lengths[w] bytes each; copied).  Refused by name: W outside
 *                    1 .. 16, a stream shorter than 512 bytes or not a multiple of 4.
 * clc_rans_lanes_decoder_decode  the NEXT SEGMENT of n symbols -> out[n]; returns n.  The rows are checked (index outside the table, bad
 *                    cdf size: refused by name) before any state changes.  On a truncated stream the decoder feeds zeros and never reads
 *                    outside the stream; every loop is bounded.
 * clc_rans_lanes_decoder_state   wave w's 64 lane states and pos (words consumed so far).
 *
 * DEVICE (rans_lanes.hip): one wave per (image, wave stream), lane l of the wave is lane l of the stream; who takes / writes the next
 * words of a sub-step is a __ballot of the renormalising lanes and a prefix popcount.
 * clc_rans_lanes_decode_step  ONE segment for the whole batch: indexes[b * ld_idx + j], j < n -> symbols[b * ld_sym + j] (offset added:
 *                    what clc_ar_commit takes).  Wave stream (b, w) is words[first .. first + count) with (first, count) =
 *                    spans[(b * W + w) * 2 ..]; state[b * W + w] (the 64 x and pos) is read, advanced and written back, so a stream's
 *                    segments are decoded by consecutive calls.  A fresh state has x[l] = word 2 l | word 2 l + 1 << 32 and pos = 128.
 *                    An index outside the table is clamped into it and a cdf size into 2 .. cdf_stride; no word outside
 *                    [first, first + count) is read (a negative first or count reads nothing) and a word at or past the count is zero;
 *                    every loop is bounded (the search by the row, the escape by 2 count and 16 payload nibbles).  On every stream the
 *                    encoders produce, symbols and final states are the host decoder's; other words give wrong symbols and nothing
 *                    worse.  The caller keeps first + count inside the words buffer.  n == 0 launches nothing.
 * clc_rans_lanes_encode  a whole batch in one launch: symbols / indexes [b * ld + i] in stream order, the segment lengths by value
 *                    (P <= 32).  Wave (b, w) writes backward into the region out[first .. first + capacity) with (first, capacity) =
 *                    regions[(b * W + w) * 2 ..] (128 + 10 n_w words hold every stream) and leaves result[(b * W + w) * 2 ..] =
 *                    (first word of its stream, word count) — or (CLC_RANS_LANES_ZERO_FREQ, 0) / (CLC_RANS_LANES_OVERFLOW, 0).  Nothing
 *                    is ever written outside the region; an index outside the table is clamped.  The words are the host encoder's.
 *
 * THE LANES STREAM OF THE SLICE MODELS (CLC, TCM; CodecEngine / model.compress(..., lanes=W)): the y string of an image is the same
 * container (clc_amd/ans.py: lanes_pack, magic CLN1) with P = num_slices segments in slice order; segment i holds the slice's
 * n = h w (M / num_slices) symbols in the order they lie in memory, pixels in raster order with channels inner (NHWC) — the order
 * clc_quantize_build_indexes writes its int32 buffers in, NOT the NCHW order of the default one-stream format.  The z string stays the
 * default stream.
 * clc_rans_lanes_decode_gauss  clc_rans_lanes_decode_step for a Gaussian-conditional slice, fused with what surrounds it: ONE segment for
 *                    the whole batch from the slice's scale and mu maps, float [rows = B n / C][C] with leading dimensions ldsc, ldmu >= C.
 *                    Symbol j of image b is row b (n / C) + j / C, channel j % C; its index is clc_quantize_build_indexes's, bit for bit
 *                    (sg = max(scale, 0.11); n_scales - 1 - #{k < n_scales - 1: sg <= scale_table[k]}, found by a search: scale_table
 *                    must be non-decreasing, 2 <= n_scales <= 256), formed ahead of the coder's dependent chain (four rounds at a time); it writes
 *                    y_hat[r ldh + c] = (float)symbol + mu[r ldmu + c] and, when symbols is not null, symbols[b ld_sym + j].  Words,
 *                    spans, state, the clamps, the bounds of every loop and what is never read are clc_rans_lanes_decode_step's.
 *                    n must be whole rows (n % C == 0) and below 2^30; n == 0 launches nothing.  The scale table lies in LDS (1 KiB, one barrier).
 * clc_rans_lanes_pack  the encoder's wave streams back to back: reads result [B][W][2] of clc_rans_lanes_encode and copies stream (b, w),
 *                    words[first .. first + count), to packed at the sum of the counts before it, in (b, w) order; header[b W + w] = its
 *                    count, or its negative code as it is (a code copies nothing and counts as 0), header[B W] = the total.  Each wave
 *                    forms its own prefix over the counts, so no wave depends on another's output.  No word is stored at or past
 *                    `capacity` and none is read at or past n_words: a total beyond the capacity is reported and the copy stops there.
 *
 * THE LANES STREAM OF mbt2018 AND mbt2018-checkerboard (model.compress(..., lanes=W); clc_amd/models/hyperprior.py): the same container,
 * cut by the DEPENDENT STEPS of the context model instead of by raster pixels.  mbt2018: the segments are the non-empty steps of the
 * wavefront schedule in ascending t = w + 3 h (W + 3 (H - 1) steps at most, against H W raster pixels); inside a segment the step's
 * pixels in ascending h, channels inner, n = pixels of the step x M.  mbt2018-checkerboard: two segments, the anchors ((h + w) odd) and
 * then the non-anchors, each in raster order with channels inner: the symbol order of its default stream.  z stays the default stream.
 * clc_ar_lanes_decode  ONE step of such a schedule for the whole batch, what clc_ar_finish(CLC_AR_DECODE), clc_rans_lanes_decode_step
 *                    and clc_ar_commit do in three launches: clc_rans_lanes_decode_gauss with scale = gp, mu = gp + M, C = M, and a
 *                    scatter through the step's pixel list in place of the dense row.  gp: dense [B P][ldg], ldg >= 2 M, scales in
 *                    [0, M) and means in [M, 2 M) (clc_ar_linear's output); pix: the step's P (h, w) pairs, device memory.  Symbol
 *                    j < n = P M of image b is row b P + j / M, channel j % M; its index is clc_quantize_build_indexes's, bit for bit;
 *                    it writes y_hat[((b H + h) W + w) ldh + c] = (float)symbol + mean with (h, w) = pix[j / M] (clc_ar_commit's
 *                    expression; y_hat NHWC, ldh >= M) and, when symbols is not null, symbols[b ld_sym + j].  A pair outside the map
 *                    is decoded — it occupies its place in the stream — and not written.  Scale table, words, spans, state, the
 *                    clamps, the bounds of every loop and what is never read are clc_rans_lanes_decode_gauss's.  n < 2^30; n == 0
 *                    launches nothing.  A wave with no round in the step (w >= ceil(n / 64)) leaves its state as it was.
 * clc_rans_lanes_encode_list  clc_rans_lanes_encode with the P segment lengths read from DEVICE memory, seg_len[P], any P >= 0 (a 16 x 16
 *                    latent of mbt2018 has 61 segments, a 32 x 48 one 141).  Regions, result codes and words are clc_rans_lanes_encode's.
 *                    The lengths cannot be checked before the launch: a negative one counts as 0, and THE CALLER keeps their sum
 *                    within ld (no symbol at or past ld may be named); ld < 2^27.
 * All kernels: stream-ordered, graph-capturable, allocation- and sync-free; no atomics, no wave waits on another; no LDS and no barrier
 * but for the scale table of clc_rans_lanes_decode_gauss / clc_ar_lanes_decode.  Bad arguments are refused by name before any launch. */
#define CLC_RANS_LANES_MAX_W 16
#define CLC_RANS_LANES_MAX_SEGMENTS 32
#define CLC_RANS_LANES_ZERO_FREQ (-1)
#define CLC_RANS_LANES_OVERFLOW (-2)
typedef struct { uint64_t x[64]; uint32_t pos; uint32_t pad; } clc_rans_lanes_state;   /* 520 bytes, DEVICE memory */
typedef struct { int P; int n[CLC_RANS_LANES_MAX_SEGMENTS]; } clc_rans_lanes_segments;
long clc_rans_lanes_bound(long n_w);   /* bytes */
long clc_rans_lanes_encode_host(const int32_t* symbols, const int32_t* indexes, const int32_t* seg_len, int P, int W, const int32_t* cdfs,
                                int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets, uint8_t* out, long out_cap,
                                int32_t* lengths /* [W] bytes */);                                  /* HOST */
typedef struct clc_rans_lanes_decoder clc_rans_lanes_decoder;
clc_rans_lanes_decoder* clc_rans_lanes_decoder_create(const uint8_t* streams, const int32_t* lengths /* [W] bytes */, int W);   /* HOST, copies */
long clc_rans_lanes_decoder_decode(clc_rans_lanes_decoder* d, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride, int n_rows,
                                   const int32_t* cdf_sizes, const int32_t* offsets, int32_t* out);   /* HOST */
int clc_rans_lanes_decoder_state(const clc_rans_lanes_decoder* d, int w, uint64_t* x /* [64] */, long* pos);
void clc_rans_lanes_decoder_destroy(clc_rans_lanes_decoder* d);
int clc_rans_lanes_decode_step(const int32_t* indexes, long ld_idx, int n, int B, const int32_t* cdfs, int cdf_stride, int n_rows,
                               const int32_t* cdf_sizes, const int32_t* offsets, const uint32_t* words, const int32_t* spans /* [B][W][2] */,
                               clc_rans_lanes_state* state /* [B][W] */, int W, int32_t* symbols, long ld_sym, clc_stream_t stream);
int clc_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, long ld, int B, clc_rans_lanes_segments segs, int W,
                          const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets,
                          uint32_t* out, const int32_t* regions /* [B][W][2] */, int32_t* result /* [B][W][2] */, clc_stream_t stream);
int clc_rans_lanes_decode_gauss(const float* scale, long ldsc, const float* mu, long ldmu, int C, int n, int B, const float* scale_table,
                                int n_scales, const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes,
                                const int32_t* offsets, const uint32_t* words, const int32_t* spans /* [B][W][2] */,
                                clc_rans_lanes_state* state /* [B][W] */, int W, float* y_hat, long ldh, int32_t* symbols /* or NULL */,
                                long ld_sym, clc_stream_t stream);
/* clc_rans_lanes_decode_gauss under a quantisation step per channel (step[C] > 0, device memory; see the quantisation-step entries above):
 * the index is that of max(scale, 0.11) / step[c] and y_hat[r ldh + c] = (float)symbol * step[c] + mu[r ldmu + c], a rounded multiply
 * and a rounded add — clc_quantize_build_indexes_step's expression, bit for bit.  Everything else, argument for argument, is
 * clc_rans_lanes_decode_gauss's; with step == 1.0f so are the outputs. */
int clc_rans_lanes_decode_gauss_step(const float* scale, long ldsc, const float* mu, long ldmu, const float* step, int C, int n, int B,
                                     const float* scale_table, int n_scales, const int32_t* cdfs, int cdf_stride, int n_rows,
                                     const int32_t* cdf_sizes, const int32_t* offsets, const uint32_t* words, const int32_t* spans /* [B][W][2] */,
                                     clc_rans_lanes_state* state /* [B][W] */, int W, float* y_hat, long ldh, int32_t* symbols /* or NULL */,
                                     long ld_sym, clc_stream_t stream);
int clc_rans_lanes_pack(const uint32_t* words, long n_words, const int32_t* result /* [B][W][2] */, int B, int W, uint32_t* packed,
                        long capacity, int32_t* header /* [B W + 1] */, clc_stream_t stream);
int clc_ar_lanes_decode(const float* gp, long ldg, int M, const int32_t* pix /* [P][2] */, int P, int B, int H, int W_map,
                        const float* scale_table, int n_scales, const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes,
                        const int32_t* offsets, const uint32_t* words, const int32_t* spans /* [B][W][2] */,
                        clc_rans_lanes_state* state /* [B][W] */, int W, float* y_hat, long ldh, int32_t* symbols /* or NULL */,
                        long ld_sym, clc_stream_t stream);
int clc_rans_lanes_encode_list(const int32_t* symbols, const int32_t* indexes, long ld, int B, const int32_t* seg_len /* [P], DEVICE */, int P,
                               int W, const int32_t* cdfs, int cdf_stride, int n_rows, const int32_t* cdf_sizes, const int32_t* offsets,
                               uint32_t* out, const int32_t* regions /* [B][W][2] */, int32_t* result /* [B][W][2] */, clc_stream_t stream);

/* ---- scale-space flow (ssf2020): the scale-space volume of a frame and the trilinear warp through it (csrc/scale_space.hip) ---- *
 * Frames x / dx / y / dy are pixel-major [N, H, W] with 3 channels at a leading dimension (>= 3); flow [N, H, W] x 2 (channel 0
 * along the width, 1 along the height, normalised coordinates) and scale [N, H, W] x 1 (the normalised depth coordinate) likewise,
 * so both may be channel slices of one 3-channel map.  THE VOLUME is [N][H][W][D][4] f32, D = levels + 1: depth and channel
 * innermost, three channels padded to a 16-byte voxel (lane 3 is written 0); 16-byte aligned.
 * Volume: V0 = x; V1 = blur(x); per further level a 2x2 average pool, a blur, and i bilinear x2 upsamplings (align_corners=False)
 * back to H x W.  blur = the separable filter `taps` with replicate padding.  H and W must be divisible by 2^(levels - 1).
 * clc_ss_volume_bwd is the adjoint, dvol -> dx, in gather form (one owner per element, fixed order).
 * Warp: F.grid_sample(volume, identity grid + flow | scale, padding_mode="border", align_corners=False) and its three gradients;
 * a NULL gradient output is not computed.  dvol is a deterministic scatter (no float atomics; bit-identical run to run and for an
 * image alone or in a batch): one stable radix sort of (lower-corner voxel, pixel id) pairs, then one gathering thread per voxel;
 * total work O(N H W), longest serial chain 8 x the largest bucket.  ws (256-byte aligned) is needed only when dvol is wanted.
 * Stream-ordered launches and one hipMemsetAsync; nothing is allocated. */
#define CLC_SS_MAX_TAPS 33
#define CLC_SS_MAX_LEVELS 12
typedef struct {
  int N, H, W;
  int levels;                    /* L >= 1; D = L + 1 */
  int ntaps;                     /* odd, 1 .. CLC_SS_MAX_TAPS */
  float taps[CLC_SS_MAX_TAPS];   /* taps [0, ntaps), applied along both axes */
} clc_ss_desc;
size_t clc_ss_volume_workspace_bytes(const clc_ss_desc* d);   /* 0 and clc_last_error on a refused descriptor */
int clc_ss_volume_fwd(const clc_ss_desc* d, const float* x, int ldx, float* vol, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_ss_volume_bwd(const clc_ss_desc* d, const float* dvol, float* dx, int lddx, void* ws, size_t ws_bytes, clc_stream_t stream);
int clc_ss_warp_fwd(const float* vol, int N, int H, int W, int D, const float* flow, int ldf, const float* scale, int lds, float* y, int ldy,
                    clc_stream_t stream);
size_t clc_ss_warp_bwd_workspace_bytes(int N, int H, int W, int D);
int clc_ss_warp_bwd(const float* vol, int N, int H, int W, int D, const float* flow, int ldf, const float* scale, int lds, const float* dy, int lddy,
                    float* dflow /* or NULL */, int lddf, float* dscale /* or NULL */, int ldds, float* dvol /* or NULL */, void* ws, size_t ws_bytes,
                    clc_stream_t stream);

/* ---- video frame I/O: planar YUV 4:2:0 integer samples <-> the model's f32 RGB frames, and plane SSE (csrc/frame_io.hip) ---- *
 * Sample planes: bytes at bit_depth == 8, 16-bit words read as unsigned at 9 <= bit_depth <= 16, samples in [0, max],
 * max = 2^bit_depth - 1; y is [N][H][W], u and v are [N][H/2][W/2], dense; H and W even.  rgb is pixel-major f32 [N][Hp][Wp] with
 * 3 channels at a leading dimension ld >= 3 (in floats); Hp >= H, Wp >= W, both even.
 * Colour: BT.709 full range, Kr, Kg, Kb = 0.2126, 0.7152, 0.0722; constants are the double expressions rounded once to f32.  The f32
 * operation order (nothing else is fused):
 *   sample -> float:  s = (float)sample * (1 / max)
 *   x2 chroma sample a quarter of a step from tap n towards tap a1 (b behind n, a2 after a1; indices clamped; rows first, then along
 *   the row):  CLC_CHROMA_BILINEAR fmaf(1/4, a1, 3/4 * n);  CLC_CHROMA_BICUBIC fmaf(-27/256, b, fmaf(-9/256, a2, fmaf(67/256, a1, 225/256 * n)))
 *   (F.interpolate(scale_factor=2, align_corners=False); bicubic with torch's A = -0.75)
 *   YCbCr -> RGB:  r = fmaf(2 - 2 Kr, cr - 0.5, y);  b = fmaf(2 - 2 Kb, cb - 0.5, y);  g = fmaf(-Kb, b, fmaf(-Kr, r, y)) * (1 / Kg)
 *   RGB -> YCbCr:  r, g, b clamped to [0, 1];  y = fmaf(Kb, b, fmaf(Kg, g, Kr * r));  cb = fmaf(0.5 / (1 - Kb), b - y, 0.5);
 *                  cr = fmaf(0.5 / (1 - Kr), r - y, 0.5);  chroma of a 2x2 block ((c00 + c01) + (c10 + c11)) * 0.25
 *   float -> sample:  rintf(fminf(fmaxf(v, 0), 1) * max), round half to even
 * clc_yuv420_to_rgb writes the UNCLAMPED frame; output pixel (h, w) is the converted pixel (min(h, H - 1), min(w, W - 1)): replicate
 * padding by clamped reads.  clc_rgb_to_yuv420 reads the top-left H x W of the Hp x Wp frame (the crop).  At 8 bits neutral chroma is
 * 127.5, an exact tie: grey lands on 127 or 128 by the last bit of b - y (the definition's property).
 * clc_plane_sse: out[i] = the exact sum over image i's n samples of (a - b)^2, in 64-bit integers (two stages, no atomics: the same
 * whatever the order); ws holds the partial sums.  Stream-ordered launches; nothing is allocated; capturable. */
#define CLC_CHROMA_BILINEAR 0
#define CLC_CHROMA_BICUBIC 1
int clc_yuv420_to_rgb(const void* y, const void* u, const void* v, int bit_depth, int N, int H, int W, int mode, float* rgb, long ld, int Hp, int Wp,
                      clc_stream_t stream);
int clc_rgb_to_yuv420(const float* rgb, long ld, int Hp, int Wp, int N, int H, int W, int bit_depth, void* y, void* u, void* v, clc_stream_t stream);
size_t clc_plane_sse_workspace_bytes(int N, long n);   /* 0 and clc_last_error on refused sizes */
int clc_plane_sse(const void* a, const void* b, int bit_depth, int N, long n /* samples per image */, int64_t* out /* [N] */, void* ws, size_t ws_bytes,
                  clc_stream_t stream);

/* ---- integer hyper-synthesis: int8 convolutions on the i8 matrix cores, requantising epilogue fused (csrc/int_conv.hip) ---- *
 * The entropy parameters of a hyperprior model in integer arithmetic (Balle, Johnston, Minnen, ICLR 2019): integer sums are exact and
 * order-free, so the parameters are the same bits under every kernel state, build and machine.  tests/intnet_ref.py is the reference.
 * INPUT (clc_int_quantize): x0 = clamp(rintf(z * 2^f0), -128, 127) as int8, rintf half to even; z dense f32, n elements.
 * LAYER (clc_int_conv): x int8 NHWC [B][H][W] with Cin channels at leading dimension ldx (bytes); two geometries:
 *   transposed = 1: 5x5, stride 2, padding 2, output_padding 1 transposed convolution -> [B][2H][2W],
 *                   out[oh][ow][co] = sum over kh, kw, ci with oh = 2 ih - 2 + kh, ow = 2 iw - 2 + kw of x[ih][iw][ci] * w[ci][co][kh][kw];
 *   transposed = 0: 3x3, stride 1, padding 1 convolution -> [B][H][W], out[oh][ow][co] = sum of x[oh + kh - 1][ow + kw - 1][ci] * w[co][ci][kh][kw].
 *   With acc the int32 sum (|acc| <= 25 * 480 * 128 * 127 < 2^28 for the largest shape served; |bias| <= 2^30, so |a| < 2^31):
 *     a = acc + bias[co];  m = a >= 0 ? mult_pos[co] : mult_neg[co]  (int32, >= 0);
 *     r = ((int64)a * m + (1 << (shift[co] - 1))) >> shift[co]       (arithmetic shift: round half up; 1 <= shift <= 62; |a * m| < 2^62)
 *   CLC_INT_OUT_I8:  y int8 NHWC, clamp(r, -128, 127), written as dwords of four channels (y 4-byte aligned, ldy % 4 == 0, in bytes);
 *   CLC_INT_OUT_F32: y f32 NHWC, (float)clamp(r, -32768, 32767) * 2^-f_out, exact in f32 (y 16-byte aligned, ldy % 4 == 0, in floats).
 *   mult_neg = 0 is ReLU, mult_neg = round(slope * ...) LeakyReLU, mult_neg = mult_pos no activation.
 * THE PACKED FILTER w_packed, int8 [Cout / 32][T][Cin / 32][2][32][16] with T = 25 (tap kh * 5 + kw) or 9 (kh * 3 + kw): entry
 *   [ct][t][kc][h][r][j] is the weight of output channel 32 ct + r, tap t, input channel 32 kc + 16 h + j (built in Python:
 *   clc_amd/intnet.py pack_filter).  Cin and Cout are multiples of 32; bias / mult_pos / mult_neg / shift are int32 [Cout], 16-byte aligned;
 *   x and w_packed 16-byte aligned, ldx % 16 == 0.  shift is read on the device and is the caller's to keep in 1 .. 62.
 * Pixel tiles of 32 may cross image boundaries in a batch; rows beyond B H W are neither read nor written; columns beyond Cout of a row
 * (ldy > Cout) are not written.  One stream-ordered launch each; nothing is allocated; capturable; bad arguments are refused by name. */
#define CLC_INT_OUT_I8 0
#define CLC_INT_OUT_F32 1
typedef struct {
  const int8_t* x; int B, H, W, Cin, ldx;
  const int8_t* w_packed;
  const int32_t *bias, *mult_pos, *mult_neg, *shift;   /* [Cout] each */
  void* y; int Cout, ldy;
  int transposed;                                      /* 1: 5x5 stride-2 transposed; 0: 3x3 stride-1 */
  int out_kind;                                        /* CLC_INT_OUT_I8 / CLC_INT_OUT_F32 */
  int f_out;                                           /* CLC_INT_OUT_F32: fractional bits of the output, 0 .. 30 */
} clc_int_conv_desc;
int clc_int_conv(const clc_int_conv_desc* d, clc_stream_t stream);
int clc_int_quantize(const float* z, long n, int f0 /* 0 .. 16 */, int8_t* x0, clc_stream_t stream);

/* ---- integer context model: the pixel-list int8 GEMM with a tap gather (csrc/int_rows.hip) ---- *
 * The entropy parameters of mbt2018-checkerboard in the integer arithmetic above, so that its streams are build-independent too;
 * tests/intctx_ref.py is the reference.  THE ENTROPY MODEL: psi = h_s_int8(z_hat), the three clc_int_conv layers with the LAST one
 * CLC_INT_OUT_I8 too (a 2M-channel NHWC int8 map at a calibrated scale); then per pass over a pixel list, every layer the requantising
 * expression of clc_int_conv (a = acc + bias; m by the sign of a; r = (a m + 2^(shift - 1)) >> shift; a clamp):
 *   yq  = clamp(rintf(y_hat * 2^f_y), -128, 127): clc_int_quantize over the NHWC map of y_hat = symbol + mean after pass 1;
 *   ctx = int8(requant(sum over the 12 taps (kh + kw odd, (kh, kw) ascending) and M channels of w[co][t][ci] * yq(h + kh - 2, w + kw - 2))),
 *         a tap off the map contributing 0 — non-anchor passes only ((h + w) even); on a 1x1 latent ctx is the requantised bias;
 *   h1  = int8(requant(sum over psi at the pixel (K = 2M) [+ ctx (K = 2M), non-anchor passes only])), LeakyReLU through mult_neg;
 *   h2  = int8(requant(h1: 10M/3 -> 8M/3)), LeakyReLU;   gp = CLC_INT_OUT_F32(requant(h2: 8M/3 -> 2M)), the (scales | means) row.
 * ROWS (clc_int_rows): r = b * P + p over pix, int32 [P][2] of (h, w) on the device; a listed pixel off the map reads zeros.  The K
 * axis is nsrc = 1 or 2 ranges in order, each with C channels (a multiple of 32) at leading dimension ld (bytes, >= C, % 16 == 0):
 *   CLC_INT_SRC_PIXEL: an NHWC int8 map [B][H][W] read at the row's pixel;   CLC_INT_SRC_DENSE: int8 [rows][C], row r;
 *   CLC_INT_SRC_TAPS:  an NHWC int8 map gathered at the ntaps (1 .. 25) offsets taps[t] = (dh, dw) (HOST memory, int [ntaps][2], each
 *                      within +-127; copied into the launch), zero off the map: K = ntaps * C, tap-major.
 * THE PACKED FILTER w_packed, int8 [Cout / 32][K / 32][2][32][16]: entry [ct][kc][h][r][j] is the weight of output channel 32 ct + r and
 * k = 32 kc + 16 h + j of the concatenated K axis (clc_amd/intnet.py pack_rows).  The total K is at most 65536, so that
 * |acc| <= K * 128 * 127 <= 2^30 and, with |bias| <= 2^30, |a| < 2^31.  Output as for clc_int_conv: CLC_INT_OUT_I8 int8 [rows][ldy]
 * (dword stores) or CLC_INT_OUT_F32 f32 [rows][ldy] = clamp(r, +-2^15) * 2^-f_out (16-byte stores); columns beyond Cout and rows beyond
 * B P are never written.  Vector stores only; one stream-ordered launch; nothing is allocated; capturable; bad arguments are refused
 * by name before any launch. */
#define CLC_INT_SRC_PIXEL 0
#define CLC_INT_SRC_DENSE 1
#define CLC_INT_SRC_TAPS 2
#define CLC_INT_ROWS_MAX_TAPS 25
typedef struct { const int8_t* p; int ld, C, kind; } clc_int_src;
typedef struct {
  clc_int_src src[2]; int nsrc;
  const int32_t* pix; int P, B, H, W;
  const int* taps; int ntaps;                          /* host memory; read only when a range is CLC_INT_SRC_TAPS */
  const int8_t* w_packed;
  const int32_t *bias, *mult_pos, *mult_neg, *shift;   /* [Cout] each */
  void* y; int Cout, ldy;
  int out_kind;                                        /* CLC_INT_OUT_I8 / CLC_INT_OUT_F32 */
  int f_out;                                           /* CLC_INT_OUT_F32: fractional bits of the output, 0 .. 30 */
} clc_int_rows_desc;
int clc_int_rows(const clc_int_rows_desc* d, clc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CLC_HIP_H */
