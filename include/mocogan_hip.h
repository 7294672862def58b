/*
 * libmocogan_hip.so -- C ABI of the MI355X (gfx950) MoCoGAN training hot path.
 *
 * The reference (raahii/mocogan-chainer) has no FFI: its hot path sits behind the Python
 * classes of model/net.py and model/updater.py and delegates all arithmetic to Chainer
 * 3.1.0 links/functions.  Each entry point below replaces one family of those Chainer calls
 * (the reference call site is cited on every declaration); the build's own model/net.py and
 * model/updater.py call them through ctypes with raw device pointers.
 *
 * Conventions
 *   - every function returns 0 on success or a negative mcg_status; nothing throws;
 *   - all pointers are caller-owned DEVICE pointers (fp32 unless noted); no hidden allocation:
 *     scratch is passed in explicitly and sized with the *_workspace_bytes queries;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it; the library keeps no mutable
 *     process state (every knob, e.g. the GEMM block tile, travels in the call's arguments), so calls on
 *     different streams / host threads do not interact;
 *   - size limit: the conv kernels address each tensor with 32-bit byte offsets checked by the buffer hardware,
 *     so every x, y and w of a mcg_conv_* call must stay below 2 GiB (MCG_ERR_UNSUPPORTED otherwise).  The largest
 *     tensor of the reference's networks is D_V's first activation, 3.4 MB per clip: at most 630 clips per call,
 *     i.e. a per-GPU batch of 315 (D runs real and fake clips as one call); the reference's default batch is 100;
 *   - activations are channels-last fp32, [N][T][H][W][C] with C padded to a multiple of 4
 *     (2-D tensors have T = 1); padded channels hold zeros;
 *   - conv / deconv weights use ONE layout for every layer: w[Co][kt][kh][kw][Ci] with
 *     kh = kw = 4 and kt in {1,4}, "Co" being the channel count on the small-extent side and
 *     "Ci" (padded to a multiple of 4) the one on the large-extent side.  A Chainer
 *     Convolution weight (Cout,Cin,k..) and a Chainer Deconvolution weight (Cin,Cout,k,k) both
 *     map to it with Co = first axis.
 */
#ifndef MOCOGAN_HIP_H
#define MOCOGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mcg_status {
    MCG_OK = 0,
    MCG_ERR_BAD_ARG = -1,      /* null pointer, non power-of-two extent, unpadded channel count ... */
    MCG_ERR_UNSUPPORTED = -2,  /* geometry outside the k4/s2/p1 family this library implements */
    MCG_ERR_LAUNCH = -3,       /* hipGetLastError() != hipSuccess after the launch */
    MCG_ERR_WORKSPACE = -4     /* workspace too small */
} mcg_status;

enum { MCG_ACT_NONE = 0, MCG_ACT_RELU = 1, MCG_ACT_LRELU = 2, MCG_ACT_TANH = 3 };

/* MFMA operand type of the convolution GEMMs.  Tensors are fp32 in memory either way and products are
 * accumulated in fp32; MCG_PREC_BF16 rounds both operands to bf16 (round-to-nearest-even) inside the
 * kernel and multiplies them on v_mfma_f32_32x32x16_bf16 (BASELINE config "bf16 MFMA tiles"). */
enum { MCG_IO_OUT_BF16 = 1, MCG_IO_Y_BF16 = 2, MCG_IO_G_BF16 = 4,   /* which tensors of an element-wise call are bf16 (see mcg_bn_act_fwd) */
       /* the OUTPUT of mcg_bn_act_fwd / the mcg_bn_act_bwd family is written in the split layout of MCG_PREC_SPLIT (mcg_split_planes
        * with run = 16: 4 * M * C uint16_t) instead of fp32 -- what 'f32x3' networks do when every reader of the tensor is a split
        * launch.  Dense y, every channel valid, C a multiple of 16 (and of the widths the eight-channel kernels take), fp32 y / g_out;
        * MCG_ERR_UNSUPPORTED otherwise. */
       MCG_IO_OUT_SPLIT = 8 };
enum { MCG_PREC_F32 = 0, MCG_PREC_BF16 = 1,
       /* as MCG_PREC_BF16, with the INPUT operands of the call (x and w for fprop, y and w for dgrad, x and y for wgrad)
        * already bf16 in memory (uint16_t, round-to-nearest-even of the fp32 values): they are loaded and staged as they
        * are -- half the operand traffic, no conversion in the K loop.  Outputs stay fp32.  Ci, Co multiples of 8. */
       MCG_PREC_BF16_STORE = 2,
       /* fp32 arithmetic on the bf16 matrix pipe: an fp32 value v is held as the three bf16 terms hi = bf16(v),
        * mid = bf16(v - hi), lo = bf16(v - hi - mid) (v == hi + mid + lo exactly) and a product is the sum of the six bf16
        * products hi.hi + hi.mid + mid.hi + hi.lo + mid.mid + lo.hi, accumulated in fp32: what is dropped is below 2^-24 of
        * |a||b|, i.e. below the rounding of an fp32 accumulation.  The INPUT operands of the call are in the split layout
        * mcg_split_planes writes: along the channel dimension that the GEMM sums over (Ci of x and w for fprop, Co of y and
        * w for dgrad) groups of 16 channels x 4 planes (hi, mid, lo, padding) of bf16, i.e. 4 * C uint16_t per pixel / filter row
        * (for dgrad's w: 16 filters x 4 planes, see mcg_split_planes).
        * Outputs stay fp32.  LDS-DMA kernels only (tile 0, 7, 8 or 10, and 9 in dgrad); channel counts along the sum powers of two >= 16. */
       MCG_PREC_SPLIT = 3,
       /* as MCG_PREC_BF16, with the y-side tensor bf16 IN MEMORY while x and w stay fp32: the clip-side layers of bf16 networks
        * (Ci = 4: D's first layer, G's last), whose 64-channel neighbour tensor -- dc1's output gradient, G's last activation -- is
        * 16x the size of the 4-channel clip.  mcg_conv_wgrad (x fp32, y bf16 -> dw fp32) and mcg_conv_dgrad (y bf16, w fp32 -> x fp32);
        * mcg_conv_fprop treats it as MCG_PREC_BF16 (its INPUTS are x and w; a bf16 y OUTPUT is mcg_conv_epilogue.out_bf16).  Co a multiple of 8. */
       MCG_PREC_BF16_Y16 = 4 };

/* Geometry of one 4x4(x4) stride-(1,2,2) pad-(0,1,1) convolution, i.e. every strided layer of
 * the reference: L.ConvolutionND / L.Convolution2D dc1..dc4 (model/net.py:133-136,174-177) and,
 * read backwards, L.DeconvolutionND dc2..dc5 (model/net.py:45-48).
 * "x" is the large side [N][Ti][Hi][Wi][Ci]; "y" the small side [N][To][Ho][Wo][Co] with
 * To = Ti - kt + 1, Ho = Hi/2, Wo = Wi/2 (Ho, Wo powers of two).  y is always dense.  The
 * start of batch item n of x is x + (n % x_perm_n) * x_stride0 + (n / x_perm_n) * x_stride1
 * elements (x_perm_n = 0 means plain n * x_stride0): this expresses both the frame-t view
 * x[:, :, t] of a clip tensor (model/updater.py:97,107) and the (T,N)->(N,T) transpose of
 * model/updater.py:102 without a copy. */
typedef struct mcg_conv_geom {
    int32_t N, Ti, Hi, Wi, Ci;
    int32_t To, Ho, Wo, Co;
    int32_t kt;
    int32_t x_perm_n;
    int32_t precision;         /* MCG_PREC_* */
    int32_t tile;              /* GEMM block tile for this call: 0 = library heuristic; 1 = 128x128, 2 = 128x64,
                                * 3 = 64x64, 4 = 256x64, 5 = 64x256 (the last two with K-steps of 32 in fp32 mode);
                                * 6 = the patch-in-LDS kernels of the Ci = 4, Co = 64 layers (refused elsewhere; what
                                * tile 0 picks for those layers in fprop / dgrad; in wgrad, fp32 only, by request only);
                                * 7 / 8 = the LDS-DMA kernels of bf16-stored operands (MCG_PREC_BF16_STORE, channel counts
                                * powers of two >= 64; refused elsewhere): 512 threads, operands straight from global
                                * memory into a ring of LDS tile buffers, block tile 256x128 / 256x256 (fprop, dgrad;
                                * dgrad with Ci = 64: 256x64) or 128x256 / 256x256 (wgrad); no K split, no +100 / +200;
                                * 9 = mcg_conv_dgrad only, bf16-stored operands, Ci = 64 and a 16 x 16 small side (D's dc2,
                                * G's dc4): one block per frame computes all four output-parity classes from a y patch held
                                * in LDS (each y pixel is loaded once per temporal tap instead of once per class and tap);
                                * 10 = the LDS-DMA kernels with a 128x128 tile and two tile buffers: TWO blocks per CU (fp32,
                                * bf16-stored or MCG_PREC_SPLIT operands; dgrad: Ci >= 128, or Ci = 64 as a 256x64 tile with two buffers (bf16-stored / split); wgrad: Co >= 128) -- fewer FLOP per LDS byte, but the
                                * epilogue of one block runs under the K loop of the other and small launches divide evenly;
                                * MCG_PREC_SPLIT launches accept 0 / 7 / 8 / 10 (+ 1000 / 2000 in fprop and dgrad) and, in dgrad, 9;
                                * 17 / 20 = MCG_PREC_SPLIT only: tile 7 / 10 with the DENSE LDS form -- the padding plane of the
                                * split layout is not brought into LDS (three K-steps hold the live planes of 64 channels, or of 64
                                * pixels in wgrad: 3/4 of the loads, K-steps and barriers).  Needs 64 | Ci (fprop) / 64 | Co (dgrad),
                                * mcg_conv_dense_split_ok(); MCG_ERR_UNSUPPORTED otherwise, and with any other precision.  Where one
                                * block writes an output tile the result is bit for bit that of the padded form of the same tile;
                                * K splits (+ 1000 / 2000) cover whole triples of K-steps (mcg_conv_dense_split_chunk());
                                * +100 / +200 also fixes the K-step depth to 32 / 64; +1000 / +2000
                                * makes mcg_conv_fprop / mcg_conv_dgrad split the K range over 2 / 4 blocks per tile
                                * (partial tiles are added atomically onto a cleared output; for long-K layers with
                                * few tiles; ignored by dgrad with tanh or a strided, non-accumulating x); for mcg_conv_wgrad, which always
                                * splits over pixels, +1000 / +2000 doubles / halves the number of splits.  A pure
                                * performance knob (the caller may time the candidates once per geometry and
                                * keep the winner, as mocogan-chainer_amd/hiplib.py does); results are the same
                                * up to fp32 summation order. */
    int32_t ci_valid;          /* how many of the Ci channels of x carry data (0 = all): the 3-channel clip is stored with
                                * Ci = 4, its padded channel and that channel's weights are zero, and the kernels written for
                                * that layer skip the products with it (same result, 3/4 of the MFMAs) */
    int64_t x_stride0, x_stride1;
} mcg_conv_geom;

/* ABI revision of this header: a host built against another revision must not call in (argument lists differ).
 * 3 = round 3 (mcg_randint, bf16 tensors in the synchronised-BatchNorm backward; round 2 changed mcg_bn_act_fwd / mcg_bn_act_bwd / mcg_adam_wd / mcg_conv_geom);
 * 6 = round 5 (mcg_split_planes_multi); 7 = round 6 (mcg_pack_clip_u8; nothing else changed);
 * 8 = the sampling path (mcg_bn_fold_deconv, mcg_clip_to_u8, MCG_ACT_RELU in mcg_conv_dgrad / mcg_conv_dgrad_ex; no argument list changed);
 *     still 8 with the averaged generator (mcg_adam_wd_ema, mcg_ema_multi added; no argument list changed)
 *     and with the differentiable augmentation (mcg_augment_* added; no argument list changed)
 *     and with the sliced Wasserstein distance (mcg_swd_*, mcg_sort_* added; no argument list changed)
 *     and with the gradient statistics (mcg_grad_stats*, mcg_adam_wd_ctl added; no argument list changed)
 *     and with the adaptive augmentation (mcg_augment_draw_gated, mcg_ada_update added; no argument list changed)
 *     and with the geometric augmentation (mcg_warp_* added; no argument list changed)
 *     and with the nearest-neighbour metrics (mcg_knn_* added; no argument list changed)
 *     and with the motion and content metrics (mcg_mc_* added; no argument list changed). */
#define MCG_ABI_VERSION 8
int mcg_version(void);

/* ---- implicit-GEMM convolution on the fp32 MFMA (v_mfma_f32_32x32x2_f32) ------------------- */

/* y = conv(x, w) + bias.  Replaces the forward of L.ConvolutionND/L.Convolution2D
 * (model/net.py:149-155,190-196) and the input-gradient of L.DeconvolutionND (autograd of
 * model/net.py:111-114).  bias may be NULL. */
int mcg_conv_fprop(const mcg_conv_geom* g, const float* x, const float* w, const float* bias,
                   float* y, void* stream);

/* x (+)= conv_transpose(y, w) + bias; optional tanh or ReLU.  Replaces the forward of
 * L.DeconvolutionND dc2..dc5 (model/net.py:111-114, tanh at :114) and the input-gradient of
 * the convolutions (loss.backward() in model/updater.py:111-113).  accumulate != 0 adds into x
 * (used to add D_I's frame-t gradient onto D_V's clip gradient).  bias may be NULL.
 * act = MCG_ACT_RELU (ABI 8): x = max(conv_transpose(y, w) + bias, 0) in the store -- with w, bias from mcg_bn_fold_deconv this is
 * F.relu(bn(dc(.))) of model/net.py:111-113 in test mode, one launch.  Every dgrad kernel of the wide layers (Ci > 4) carries it;
 * MCG_ERR_UNSUPPORTED together with a split-K tile code (+1000 / +2000), accumulate, or (mcg_conv_dgrad_ex) a sums / mask epilogue. */
int mcg_conv_dgrad(const mcg_conv_geom* g, const float* y, const float* w, const float* bias,
                   float* x, int act, int accumulate, void* stream);

/* dw += sum over pixels y (x) x.  Weight gradient of both layer kinds (model/updater.py:111-113).
 * dw must have been zeroed (or hold the other pass' gradient): the kernel adds with fp32
 * atomics (split-K over pixels). */
int mcg_conv_wgrad(const mcg_conv_geom* g, const float* x, const float* y, float* dw, void* stream);

/* The dense LDS form of MCG_PREC_SPLIT launches (tile codes 17 / 20), host-side queries that launch nothing.
 * pass: 0 = fprop, 1 = dgrad, 2 = wgrad.  g->tile is read by mcg_conv_dense_split_chunk only (its K-split digit).
 * mcg_conv_dense_split_ok: 1 when the geometry admits the form in that pass, 0 when not (or on a bad argument).
 * mcg_conv_dense_split_chunk: the part of the summed dimension one block of such a launch covers -- split elements (4 per
 * channel: a triple of K-steps is 256) in fprop / dgrad without an epilogue, pixels (a triple is 64) in wgrad; 0 when the form
 * does not apply. */
int mcg_conv_dense_split_ok(const mcg_conv_geom* g, int pass);
int mcg_conv_dense_split_chunk(const mcg_conv_geom* g, int pass);

/* ---- fused epilogues of mcg_conv_fprop / mcg_conv_dgrad ---------------------------------------------------
 * What the reference does as separate Chainer function calls right after (forward) or before (backward) a
 * convolution -- BatchNormalization's statistics, leaky_relu + add_noise behind D's first layer
 * (model/net.py:148-149,189-190), the per-channel sums of BatchNormalization's backward, the leaky_relu mask of the
 * first layer's gradient -- computed on the GEMM's accumulators before they are stored, so the tensors are not read
 * again by a pass of their own.  All sums are per block tile and combined in a fixed order by the *_from_partials
 * entry points below: no float atomics, results are reproducible.
 *
 * "rows" are the rows of the launch's OUTPUT ([pixels][C], C = Co for fprop, Ci for dgrad); with groups == 2 the
 * batch items n < N/2 form statistics group 0 and the others group 1 (D runs the real and the fake clips of an
 * iteration as one batch but Chainer normalises each call on its own, model/updater.py:97-98,107-108).
 * Fused epilogues need the launch to own whole output elements: they are refused (MCG_ERR_UNSUPPORTED) together with
 * a split-K tile code, tanh, accumulate, or a strided / permuted x in dgrad. */
enum { MCG_SUMS_NONE = 0,
       MCG_SUMS_STATS = 1,     /* (sum v, sum v^2) of the stored values          -> mcg_bn_stats_from_partials      */
       MCG_SUMS_BN_BWD = 2,    /* (sum g', sum g' x_hat), g' = v * act'(bn(y))   -> mcg_bn_act_bwd_from_partials   */
       MCG_SUMS_COL = 3 };     /* (sum v, -)                                     -> mcg_colsum_from_partials       */
typedef struct mcg_conv_epilogue {
    int32_t sums;               /* MCG_SUMS_* */
    int32_t groups;             /* 1 or 2 statistics groups (halves of the batch) */
    float* part;                /* [n_slots][groups][2][C] floats, mcg_conv_epilogue_part_bytes() */
    const float* bn_y;          /* MCG_SUMS_BN_BWD: the BatchNorm input saved by the forward pass, laid out like the output */
    const float* bn_stats[2];   /*                  per group: the 4*C floats mcg_bn_stats wrote */
    int32_t bn_act;             /*                  MCG_ACT_RELU / MCG_ACT_LRELU behind that BatchNorm */
    /* fprop only: out = act(conv + bias) + noise, and the sign of the pre-activation as one bit per element */
    int32_t act;                /* MCG_ACT_NONE (nothing of this block applies) or MCG_ACT_LRELU; mcg_conv_dgrad_ex (ABI 8): MCG_ACT_RELU
                                 * = mcg_conv_dgrad's act, so that ReLU and out_bf16 travel together (sums == MCG_SUMS_NONE, no mask) */
    const float* addend[2];     /* per group: pre-scaled noise laid out like the group's output rows, or NULL */
    float sigma;                /* else sigma * N(0,1) from Philox4x32-10 (seed, stream_id[group]) when sigma > 0: one
                                 * counter per (row quad, channel) of the group's output -- element (m, c) is normal
                                 * m & 3 of counter (m >> 2) * C + c (mcg_randn_rowquad draws the same stream) */
    uint64_t seed, stream_id[2];
    uint32_t* mask_out;         /* [rows][(C+31)/32] words, bit c & 31 of word c >> 5 set <=> pre-activation >= 0; or NULL.  When C is
                                 * not a multiple of 32 the bits of a row's last word that belong to columns >= C are unspecified
                                 * (every word is written whole); mask_in never looks at them */
    int32_t out_bf16;           /* the OUTPUT tensor (y of fprop, x of dgrad) is bf16 (uint16_t, round-to-nearest-even) --
                                 * what the next layer's GEMMs (with act) or the element-wise passes (without) of a bf16
                                 * network read.  With the plain store or any epilogue (MCG_SUMS_BN_BWD: LDS-DMA kernels only); never with a
                                 * split-K tile code, an accumulating dgrad, the input gradient of the Ci = 4 layers or MCG_PREC_SPLIT
                                 * operands, and on the LDS-DMA kernels (tile 7 / 8 / 10, which store runs of 8 channels) only when the
                                 * output's channel count is a multiple of 8 (MCG_ERR_UNSUPPORTED).  The
                                 * sums of an epilogue are those of the STORED (rounded) values: BatchNorm then normalises the
                                 * tensor it reads with that tensor's own mean and variance.
                                 * MCG_IO_OUT_SPLIT (ABI 7; mcg_conv_fprop_ex with act, Co a multiple of 16): y is written in the
                                 * MCG_PREC_SPLIT layout [pixel][Co/16][4 planes][16] (uint16_t bf16 terms hi, mid, lo; the
                                 * fourth plane is padding and is not written) -- bit for bit what mcg_split_planes(run 16)
                                 * makes of the fp32 result, for a next layer whose GEMMs all read the split form */
    /* dgrad only: v *= (mask bit ? 1 : 0.2) -- leaky_relu's backward from the bits the forward pass stored */
    const uint32_t* mask_in;
    /* out (host side, valid after the call): */
    int32_t n_slots, slot_stride;   /* part holds n_slots slots, slot_stride floats apart; group i starts i*2*C in */
    /* in (ABI 4): MCG_SUMS_BN_BWD on the LDS-DMA kernels (tile 7 / 8 / 10, bf16-stored or split operands -- the only kernels that take it
     * together with out_bf16): bn_y is bf16 (uint16_t) instead of fp32; the sums are those of the STORED output values */
    int32_t bn_y_bf16;
} mcg_conv_epilogue;
/* upper bound of the bytes `part` needs for this geometry (any tile choice); pass = 0 fprop, 1 dgrad.  It is the need of the
 * smallest block tile (64 rows; dgrad: per output-parity class, four classes): a launch writes n_slots * slot_stride floats,
 * slot_stride == groups * 2 * C, at most that many and fewer with a taller tile; nothing behind them is touched, every float of
 * them is written (MCG_SUMS_COL: the second of each pair holds no defined value).  A refused launch writes nothing at all. */
int64_t mcg_conv_epilogue_part_bytes(const mcg_conv_geom* g, int pass, int groups);
int mcg_conv_fprop_ex(const mcg_conv_geom* g, const float* x, const float* w, const float* bias, float* y,
                      mcg_conv_epilogue* ep, void* stream);
int mcg_conv_dgrad_ex(const mcg_conv_geom* g, const float* y, const float* w, const float* bias, float* x,
                      mcg_conv_epilogue* ep, void* stream);

/* ---- full-window layers: D's dc5 (model/net.py:137,178) and G's dc1 (model/net.py:44) ------ */
/* x is [M][K] (one dense window per row), y is [M][Co], w is [Co][K]. */
int mcg_fc_fprop(int M, int K, int Co, const float* x, const float* w, const float* bias,
                 float* y, void* stream);
/* x = y w (+ bias[k % bias_period]) */
int mcg_fc_dgrad(int M, int K, int Co, const float* y, const float* w, const float* bias,
                 int bias_period, float* x, void* stream);
/* dw += y^T x ; db[co] += sum_m y[m][co] when db != NULL */
int mcg_fc_wgrad(int M, int K, int Co, const float* x, const float* y, float* dw, float* db,
                 void* stream);

/* ---- BatchNormalization (train mode) + activation + add_noise ------------------------------ */
/* L.BatchNormalization (model/net.py:50-53,139-141,180-182; Chainer decay 0.9, eps 2e-5).
 * y is [M][C].  stats is a caller buffer of 4*C floats: mean, inv_std, scale = gamma*inv_std,
 * shift = beta - mean*scale (kept for the backward pass).  avg_mean/avg_var (may be NULL) get
 * Chainer's running update.  workspace: mcg_bn_workspace_bytes(M, C).
 * The column reductions (here, in mcg_bn_act_bwd and mcg_colsum_acc) support C = 4 * 2^k, k <= 8 -- every width
 * a power-of-two n_filters produces; other multiples of 4 return MCG_ERR_UNSUPPORTED. */
int64_t mcg_bn_workspace_bytes(int64_t M, int C);
int mcg_bn_stats(int64_t M, int C, const float* y, const float* gamma, const float* beta,
                 float* stats, float* avg_mean, float* avg_var, float eps, float decay,
                 void* workspace, void* stream);

/* out = act(y * scale + shift) + noise.  scale_shift = stats + 2*C or NULL (identity).
 * noise: `addend` when non-NULL (parity mode: the caller's pre-scaled sigma*randn tensor),
 * else sigma * N(0,1) from Philox4x32-10 keyed by (seed, stream_id) when sigma > 0, else none;
 * generated noise is added to channels < c_valid only (padded channels stay exactly zero).
 * Replaces F.relu/F.leaky_relu(bn(.)) followed by add_noise (model/net.py:10-15,110-113,
 * 148-155,189-196).
 * y may be a batch-strided view: when y_rows_per_item > 0, row r of y starts at
 * y + (r / y_rows_per_item) * y_item_stride + (r % y_rows_per_item) * C  (frame t of a clip). */
int mcg_bn_act_fwd(int64_t M, int C, int c_valid, const float* y, int64_t y_rows_per_item,
                   int64_t y_item_stride, const float* scale_shift, int act,
                   const float* addend, float sigma, uint64_t seed, uint64_t stream_id,
                   void* out, int out_bf16, void* stream);
/* out_bf16 (and gx_bf16 of the backward passes below) is a set of MCG_IO_* flags saying which tensors of the call are bf16
 * (uint16_t, round-to-nearest-even) instead of fp32: bf16 networks keep the tensors that are only read by GEMMs
 * (activations, output gradients: MCG_IO_OUT_BF16) and the GEMM outputs these passes read (pre-BatchNorm values
 * MCG_IO_Y_BF16, input gradients MCG_IO_G_BF16) in bf16.  1 == MCG_IO_OUT_BF16 keeps the meaning of the former boolean. */

/* Test-mode BatchNorm (chainer.config.train = False: the running averages, eps inside the square root) folded into the
 * deconvolution in front of it (model/net.py:110-113) (ABI 8): with s_c = gamma_c / sqrt(avg_var_c + eps),
 *   w_out[r][c] = w[r][c] * s_c        (w [rows][Cp]: a deconvolution's filter in the device layout, whose innermost axis is the
 *                                       deconvolution's OUTPUT channel -- rows = Co * kt * 16 of mcg_conv_geom's dgrad reading)
 *   bias_out[c] = (bias[c] - avg_mean_c) * s_c + beta_c     (bias [Cp] or NULL = 0)
 * so that bn(conv_transpose(y, w) + bias) = conv_transpose(y, w_out) + bias_out.  gamma .. avg_var hold C values; channels
 * C .. Cp are copied.  fp32 only: mcg_split_planes / a bf16 copy make the other operand forms of the folded filter. */
int mcg_bn_fold_deconv(int64_t rows, int C, int Cp, const float* w, const float* bias, const float* gamma, const float* beta,
                       const float* avg_mean, const float* avg_var, float eps, float* w_out, float* bias_out, void* stream);

/* Backward of the line above + BN.  g_out: gradient w.r.t. `out`.  Computes
 * g_bn = g_out * act'(y*scale+shift) (the mask is recomputed from the SAVED scale/shift, i.e.
 * the forward's output sign, as Chainer's retained-output backward does), then
 * gx = gamma*inv_std * (g_bn - (x_hat * ggamma + gbeta) / M) with the CURRENT gamma (quirk Q5).
 * dgamma/dbeta (may be NULL: gradient through D for G's loss) are accumulated (+=).
 * stats == NULL means "no BN": gx = g_out * act'(y).  act == MCG_ACT_TANH uses y as the saved
 * tanh OUTPUT.  in-place (gx == g_out) is allowed.  workspace: mcg_bn_workspace_bytes(M, C). */
int mcg_bn_act_bwd(int64_t M, int C, const float* g_out, const float* y, const float* stats,
                   const float* gamma, int act, void* gx, int gx_bf16, float* dgamma, float* dbeta,
                   void* workspace, void* stream);

/* ---- synchronised BatchNorm (opt-in under data parallelism; the reference is single-device) ---------------
 * Both passes of BatchNorm split at their per-channel reduction: the local sums leave the library as
 * doubles, the caller adds them over the ranks (RCCL all-reduce) and the second half starts from the global
 * sums, so the statistics are those of the global batch.
 *   forward : mcg_bn_sums (sums = [sum x | sum x^2], 2*C doubles)  -> all-reduce ->  mcg_bn_stats_from_sums
 *   backward: mcg_bn_bwd_sums (sums = [sum g' | sum g' x_hat], g' = g_out * act')  -> all-reduce ->
 *             mcg_bn_act_bwd_from_sums: gx from the GLOBAL sums and M_total; dgamma / dbeta += the LOCAL sums
 *             (the gradient exchange averages parameter gradients over the ranks afterwards). */
int mcg_bn_sums(int64_t M, int C, const float* y, double* sums, void* workspace, void* stream);
int mcg_bn_stats_from_sums(int64_t M_total, int C, const double* sums, const float* gamma,
                           const float* beta, float* stats, float* avg_mean, float* avg_var, float eps,
                           float decay, void* stream);
/* (io_bf16 / gx_bf16: MCG_IO_* flags as in mcg_bn_act_bwd -- bf16 networks keep gx, and where the schedule allows y and
 * g_out, in bf16) */
int mcg_bn_bwd_sums(int64_t M, int C, const float* g_out, const float* y, const float* stats, int act, int io_bf16,
                    double* sums, void* workspace, void* stream);
int mcg_bn_act_bwd_from_sums(int64_t M, int64_t M_total, int C, const float* g_out, const float* y,
                             const float* stats, const float* gamma, int act, const double* local_sums,
                             const double* global_sums, void* gx, int gx_bf16, float* dgamma, float* dbeta,
                             void* workspace, void* stream);

/* The second halves of the three passes above, starting from per-tile partial sums written by a fused conv
 * epilogue (part / n_slots / slot_stride as returned in mcg_conv_epilogue; `part` already offset to the group):
 *   mcg_bn_stats_from_partials   == mcg_bn_stats' finalize      (M = rows of the group)
 *   mcg_bn_act_bwd_from_partials == mcg_bn_act_bwd without its reduction pass over g_out and y
 *   mcg_colsum_from_partials     == mcg_colsum_acc without its pass over g
 * workspace: mcg_bn_workspace_bytes(M, C) (large slot counts are first folded into it, in a fixed order).
 * Any n_slots >= 1, any slot_stride >= 2*C (columns outside the group's 2*C are never read) and any C % 4 == 0: these three have no
 * pass over rows, so the C = 4 * 2^k limit of the column reductions above does not apply to them. */
int mcg_bn_stats_from_partials(int64_t M, int C, const float* part, int n_slots, int slot_stride, const float* gamma,
                               const float* beta, float* stats, float* avg_mean, float* avg_var, float eps, float decay,
                               void* workspace, void* stream);
int mcg_bn_act_bwd_from_partials(int64_t M, int C, const float* g_out, const float* y, const float* stats,
                                 const float* gamma, int act, const float* part, int n_slots, int slot_stride, void* gx,
                                 int gx_bf16, float* dgamma, float* dbeta, void* workspace, void* stream);
int mcg_colsum_from_partials(int C, const float* part, int n_slots, int slot_stride, float* db, void* workspace,
                             void* stream);

/* db += column sums of g [M][C] (bias gradient of every conv/deconv). */
int mcg_colsum_acc(int64_t M, int C, const float* g, float* db, void* workspace, void* stream);

/* ---- layout ------------------------------------------------------------------------------- */
/* out[N][T][H][W][Cp] = x[N][C][T][H][W] (+ noise as above); padded channels = 0.  Turns the
 * reference-layout real clip batch (model/updater.py:89-90) into D's first conv input.
 * Element (n,c,t,hw) of x is at x + n*x_stride_n + c*x_stride_c + t*HW + hw, so a single frame
 * x[:, :, t] of a clip batch is expressed with T = 1 and the clip's strides.  MCG_ERR_BAD_ARG (here and in mcg_pack_clip_u8):
 * a null x / out, a non-positive extent, Cp < C, Cp % 4, a negative stride. */
int mcg_pack_clip(int N, int C, int Cp, int T, int HW, const float* x, int64_t x_stride_n,
                  int64_t x_stride_c, const float* addend,
                  float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream);
/* The same from the loader's uint8 clips (reference datasets.py:95,108 decodes frames to (T,H,W,C) uint8 and normalises
 * (v - 128) / 128 on the host; model/updater.py:87-92 stacks and transposes): out[N][T][HW][Cp] = (x[N][T][HW][C] - 128) / 128
 * (+ noise as mcg_pack_clip, same counters), padded channels = 0.  Byte (n,t,hw,c) of x is at
 * x + n*x_stride_n + t*x_stride_t + hw*C + c, so frame t of every clip is T = 1 with x + t*HW*C and the clip's x_stride_n. */
int mcg_pack_clip_u8(int N, int C, int Cp, int T, int HW, const uint8_t* x, int64_t x_stride_n, int64_t x_stride_t,
                     const float* addend, float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream);
/* The way out (ABI 8), the inverse of mcg_pack_clip_u8: in[N][T][HW][Cp] fp32 -> uint8 out[n*stride_n + t*stride_t + hw*C + c], so
 * (N,T,H,W,C) and the reference's frame order (T,N,H,W,C) are one call each.  The byte is generate_samples.py:39's
 * ((x / 2. + 0.5) * 255).astype(np.uint8): three separately rounded fp32 operations and a truncating cast (values outside
 * [0, 255] saturate), bit for bit what NumPy makes of the same x.  act = MCG_ACT_NONE: `in` holds x; act = MCG_ACT_TANH: `in` is
 * the last deconvolution's output before bias and tanh (model/net.py:114) and x = tanh(in + bias[c]) (bias [Cp], may be NULL).
 * Cp = 4 (MCG_ERR_UNSUPPORTED otherwise); strides in bytes, >= HW*C, items and frames must not overlap (MCG_ERR_BAD_ARG). */
int mcg_clip_to_u8(int N, int C, int Cp, int T, int HW, const float* in, const float* bias, int act, uint8_t* out,
                   int64_t stride_n, int64_t stride_t, void* stream);
/* cgan (model/updater.py:65-76, concat_label_video): out[n][p][0..Cq) = x[n][p][0..C), then dl label planes -- +1 at channel
 * C + labels[n], -1 at the others -- then zeros; x is [N][P][Cp], out [N][P][Cq], Cq % 4 == 0, labels int32 [N] in [0, dl).
 * dl == 0 (labels may be NULL): a channel slice into another row width -- the way back, where label planes carry no gradient. */
int mcg_concat_label_planes(int N, int64_t P, int C, int Cp, int dl, int Cq, const float* x, const int32_t* labels, float* out,
                            void* stream);
/* x[N][C][T][HW] = in[N][T][HW][Cp] (first C channels) */
int mcg_unpack_clip(int N, int C, int Cp, int T, int HW, const float* in, float* x, void* stream);
/* g_frames[(t*N+n)][HW][Cp] = g_clip[n][t][HW][Cp] * (1 - x_clip^2): tanh backward fused with the
 * (N,T)->(T,N) transpose back to generator frame order (autograd of model/net.py:114-115,
 * model/updater.py:102). */
int mcg_tanh_bwd_to_frames(int N, int T, int64_t frame_elems, const float* g_clip,
                           const float* x_clip, float* g_frames, void* stream);

/* ---- differentiable augmentation of the discriminators' inputs -------------------------------------------------------------
 * Zhao et al. 2020, "Differentiable Augmentation for Data-Efficient GAN Training", policy color,translation,cutout (no reference
 * counterpart: model/updater.py:97-108 hands the clips to the discriminators as they are).  A clip is x[n][T][H][W][Cp], Cp = 4,
 * with C = 1..3 valid channels; the pad channel is zero and stays zero.  Clip n has ONE parameter set for all its frames:
 *   col[n] = (b, s, c, 0)                  brightness, saturation, contrast
 *   geo[n] = (dx, dy, x0, x1, y0, y1, 0, 0) translation and the cutout rectangle (columns [x0, x1), rows [y0, y1), inside the frame)
 * Forward, in the paper's order colour, translation, cutout (valid channels only):
 *   v = x + b;   v = s v + (1 - s) mean_channels(v);   v = c v + (1 - c) m,   m = mean of x over the clip's T H W C elements + b
 *   out(t, y, x) = v(t, y - dy, x - dx) if that source lies inside the frame and (y, x) outside the rectangle, else 0
 * (b = 0, s = 1, c = 1, no shift, empty rectangle: out == x bit for bit).  The map is affine in x; mcg_augment_bwd is the adjoint of
 * its linear part:
 *   g1(t, sy, sx) = g_out(t, sy + dy, sx + dx) if that position lies inside the frame and outside the rectangle, else 0
 *   g2 = c g1 + (1 - c) mean_clip(g1);   g_in = s g2 + (1 - s) mean_channels(g2)
 * Each call is two launches: per-clip partial sums into `workspace` (mcg_augment_workspace_bytes(N) bytes, 8-byte aligned), then an
 * apply pass that adds a clip's partial sums in a fixed order -- no float atomics, results are bit-reproducible run to run.
 * The gather never forms an address outside the clip it reads.  MCG_ERR_BAD_ARG: a null pointer, C outside 1..3, a non-positive
 * extent, in == out (a gather cannot run in place); MCG_ERR_UNSUPPORTED: Cp != 4 (or T*H*W > 2^28, N > 65535). */
enum { MCG_AUG_COLOR = 1, MCG_AUG_TRANSLATION = 2, MCG_AUG_CUTOUT = 4 };
int64_t mcg_augment_workspace_bytes(int N);
int mcg_augment_fwd(int N, int C, int Cp, int T, int H, int W, const float* in, const int32_t* geo, const float* col,
                    void* workspace, float* out, void* stream);
int mcg_augment_bwd(int N, int C, int Cp, int T, int H, int W, const float* g_out, const int32_t* geo, const float* col,
                    void* workspace, float* g_in, void* stream);
/* The parameters of N clips from Philox4x32-10 keyed by (seed, stream_id) like every other draw: clip i takes the counters 2i and
 * 2i + 1, i.e. the words w0..w7; with u(w) = (w >> 9) * 2^-23 (exact in fp32):
 *   b = u(w0) - 0.5, s = 2 u(w1), c = u(w2) + 0.5;   dx = w3 % (2 (W/8) + 1) - W/8, dy likewise from w4 and H;
 *   a W/2 x H/2 rectangle centred at cx = w5 % (W + 1), cy = w6 % (H + 1): columns [cx - W/4, cx - W/4 + W/2) clipped to [0, W),
 *   rows likewise; w7 is not used.
 * policy: a set of MCG_AUG_* flags; a component that is off gets its identity values (b = 0, s = c = 1; no shift; the empty
 * rectangle 0, 0, 0, 0) but its words are consumed, so switching one component never changes another's draw.
 * geo [N][8] int32, col [N][4] float as above. */
int mcg_augment_draw(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, int32_t* geo, float* col, void* stream);

/* ---- adaptive augmentation: the draw gated by a probability that the discriminators' overfitting sets -------------------------
 * Karras et al. 2020, "Training Generative Adversarial Networks with Limited Data", sections 2.2 and 3 (no reference counterpart).
 * The state is a block of eight doubles in device memory that the caller allocates and initialises; mcg_ada_update writes it,
 * mcg_augment_draw_gated reads it, the host never waits for it:
 *   ada[0] = p, the probability with which each component of the policy is applied to a clip
 *   ada[1], ada[2] = sum of sign over the VideoDiscriminator's / the ImageDiscriminator's real logits since the last adjustment
 *   ada[3] = logits counted per discriminator, ada[4] = calls since the last adjustment
 *   ada[5], ada[6] = r_t = E[sign(D(real))] of the VideoDiscriminator / the ImageDiscriminator at the last adjustment
 *   ada[7] = adjustments so far
 *
 * mcg_augment_draw_gated: the parameters mcg_augment_draw(N, H, W, policy, seed, stream_id) writes, each component kept with
 * probability p = ada[0].  Clip i also takes Philox counter i of (seed, gate_stream_id), words g0..g3, and with the draw's own u:
 * colour is kept iff (double)u(g0) < p, translation iff (double)u(g1) < p, cutout iff (double)u(g2) < p; g3 is not used.  A
 * component that fails its gate gets its identity values (as if the policy left it out).  geo[6] holds the MCG_AUG_* flags of the
 * components that are in the policy and passed, geo[7] = 0 (mcg_augment_fwd / mcg_augment_bwd read geo[0..5] only).  So p = 0
 * gives identity parameters for every clip, p >= 1 mcg_augment_draw's bits everywhere except geo[6].  One launch; ada is not written.
 * MCG_ERR_BAD_ARG: what mcg_augment_draw refuses, a null ada, gate_stream_id == stream_id. */
int mcg_augment_draw_gated(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, uint64_t gate_stream_id,
                           const double* ada, int32_t* geo, float* col, void* stream);
/* One step of the controller on the real clips' logits y_video, y_image [N][C] (column 0 is read: y[n * C]).  With
 * s(y) = +1 for y > 0, -1 for y < 0, 0 for +-0 and NaN:  ada[1] += sum s(y_video), ada[2] += sum s(y_image), ada[3] += N,
 * ada[4] += 1 (the sign sums are formed as integers: exact, no order enters).  When ada[4] >= interval the adjustment runs:
 *   r_v = ada[1] / ada[3], r_i = ada[2] / ada[3], r = max(r_v, r_i)   (both discriminators see the same augmented clips: the one
 *   that overfits more sets the strength);   d = (r > target) - (r < target);   ada[0] = min(1, max(0, ada[0] + d step));
 *   ada[5] = r_v, ada[6] = r_i, ada[7] += 1, ada[1..4] = 0
 * all in double.  One launch of one workgroup, any N >= 1.  MCG_ERR_BAD_ARG: a null pointer, N or C or interval <= 0, step
 * negative or NaN, target NaN or outside (-1, 1). */
int mcg_ada_update(int N, int C, const float* y_video, const float* y_image, double target, double step, int interval, double* ada,
                   void* stream);

/* ---- geometric augmentation: a per-clip affine warp with bilinear taps --------------------------------------------------------
 * Karras et al. 2020, section 2.3 and figure 4: x-flip, quarter turns, isotropic scaling and arbitrary rotation (no reference
 * counterpart).  A clip is x[n][T][H][W][Cp], Cp = 4, as mcg_augment_fwd takes it; all four lanes are warped alike, so a zero pad
 * channel stays exactly +0.0.  Clip n has ONE matrix for all its frames (motion is untouched):
 *   mat[n] = (m00, m01, m02, m10, m11, m12, flags, 0)      float; it maps an OUTPUT position to its SOURCE
 * flags is the float value of the MCG_WARP_* components that were applied (the draws below write it; mcg_warp_fwd / mcg_warp_bwd
 * read words 0..5 only).  With cx = (W-1)/2, cy = (H-1)/2, xc = x - cx, yc = y - cy, every operation rounded to fp32 on its own
 * (never contracted into an FMA, so that a NumPy float32 statement gives the same bits):
 *   sx = ((m00*xc) + (m01*yc)) + (cx + m02)        sy = ((m10*xc) + (m11*yc)) + (cy + m12)
 * sx and sy are clamped to [-2, W + 1] and [-2, H + 1] before anything is converted to an integer (a NaN becomes -2; a clamped
 * source has no tap inside the frame, as it had none before), then x0 = floor(sx), fx = sx - x0 (exact), likewise y0 and fy.
 *   out(t, y, x) = sum over the four taps (y0 + j, x0 + i), i, j in {0, 1}, of w_i(fx) w_j(fy) in(t, y0 + j, x0 + i),
 *   w_0(f) = 1 - f, w_1(f) = f; a tap outside the frame contributes 0 (zero padding, as the translation of mcg_augment_fwd has it),
 *   and a tap of weight 0 is not read.
 * Reflection padding and the wavelet low-pass filters of the paper's implementation are NOT here: a magnifying warp interpolates,
 * a reducing one aliases, and the border is zero.  Any matrix of finite entries is safe -- all-zero, singular, 1e6-scale: no
 * address outside the clip is formed.  The identity (1, 0, 0, 0, 1, 0) returns the input bit for bit, and a matrix of entries 0
 * and +-1 with zero offsets (a flip; a quarter turn when H == W) returns an exact permutation: fx = fy = 0, weights exactly 1 and 0.
 *
 * mcg_warp_bwd is the exact adjoint, computed as a GATHER: g_in(t, v, u) = sum over the output pixels (y, x) that have (v, u)
 * among their taps of that tap's weight times g_out(t, y, x).  No float atomics, the candidates are visited in row-major order:
 * two runs give the same bits.  The candidates of (v, u) are the output pixels of a bounding box -- the image of the square
 * (u-1, u+1) x (v-1, v+1) under the 2x2 inverse of the linear part, widened by a pixel, clamped to the frame; the whole frame when
 * the determinant is zero, the inverse is not finite or fp32 rounding of sx, sy could matter at that scale -- and for every
 * candidate x0, fx, y0, fy are recomputed by the same code as in the forward pass.  A degenerate matrix is slow, never wrong.
 * One launch each.  MCG_ERR_BAD_ARG: a null pointer, a non-positive extent, C outside 1..Cp, in == out (a gather cannot run in
 * place); MCG_ERR_UNSUPPORTED: Cp != 4 (or T*H*W > 2^28, N > 65535, as mcg_augment_fwd). */
enum { MCG_WARP_FLIP = 1, MCG_WARP_ROT90 = 2, MCG_WARP_SCALE = 4, MCG_WARP_ROTATE = 8 };
int mcg_warp_fwd(int N, int C, int Cp, int T, int H, int W, const float* in, const float* mat, float* out, void* stream);
int mcg_warp_bwd(int N, int C, int Cp, int T, int H, int W, const float* g_out, const float* mat, float* g_in, void* stream);
/* The matrices of N clips from Philox4x32-10 keyed by (seed, stream_id): clip i takes counter i, the words w0..w3, and with
 * u(w) = (w >> 9) * 2^-23 as in mcg_augment_draw, everything in fp32 with separately rounded + - * / and no transcendental:
 *   flip          f = (w0 & 1) ? -1 : 1
 *   quarter turn  k = w1 & 3, Q_k = Q_1^k, Q_1 = [[0, -1], [1, 0]]
 *   scale         a = (2 u(w2) - 1) / 6, s = (1 + a) / (1 - a): s in (5/7, 7/5), symmetric in the logarithm
 *   rotation      t = 2 u(w3) - 1, c = (1 - t t) / (1 + t t), sn = (2 t) / (1 + t t): the angle 2 atan t in [-90, 90) degrees.  With
 *                 the quarter turn it covers the whole circle; t is uniform, so the angle's density falls by half from the centre
 *                 (angle 0) to the ends (+-90 degrees) -- it is NOT uniform in the angle.
 *   L = (1 / s) [[c, sn], [-sn, c]] Q_k diag(f, 1):  r = 1 / s (one division), the four products r c, r sn, -(r sn), r c (one
 *   rounding each), then the column permutation and signs of Q_k and the sign f on column 0 (exact); a -0 is stored as +0.
 *   m00 m01 m10 m11 = L, m02 = m12 = 0, flags = 0, word 7 = 0.
 * policy: a set of MCG_WARP_* flags; a component that is off takes its identity value (f = 1, k = 0, s = 1, c = 1, sn = 0) and its
 * word is consumed all the same.  MCG_ERR_BAD_ARG: a null mat, a non-positive extent, a policy outside 0..15;
 * MCG_ERR_UNSUPPORTED: MCG_WARP_ROT90 with H != W (the turned frame would not cover the frame). */
int mcg_warp_draw(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, float* mat, void* stream);
/* mcg_warp_draw with each component kept with probability p = ada[0] (the state block of mcg_ada_update; read, never written):
 * clip i also takes counter i of (seed, gate_stream_id), words g0..g3, and flip is kept iff (double)u(g0) < p, the quarter turn iff
 * (double)u(g1) < p, scale iff (double)u(g2) < p, rotation iff (double)u(g3) < p.  A component that fails takes its identity value;
 * flags = the components that are in the policy and passed.  p = 0 gives identity matrices, p >= 1 mcg_warp_draw's bits except
 * flags.  MCG_ERR_BAD_ARG: what mcg_warp_draw refuses with it, a null ada, gate_stream_id == stream_id. */
int mcg_warp_draw_gated(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, uint64_t gate_stream_id,
                        const double* ada, float* mat, void* stream);

/* ---- GRU motion-code recurrence (L.StatelessGRU, model/net.py:39-41,61-81) ------------------ */
/* params: the six Linear links packed as [W_r|U_r|W_z|U_z|W|U], each (weights row-major
 * [dim_zm][in], then bias[dim_zm]); in = dim_zl + dim_zm for W_*, dim_zm for U_*.
 * h0 [N][dim_zm]; e [T][N][dim_zm]; labels [N] int32 (ignored when dim_zl == 0); zc [N][dim_zc].
 * z [T*N][dim_zc + dim_zm] = concat(tile(zc), zm)  (model/net.py:102-107).
 * saved: [T][N][4*dim_zm] (r, z, h_bar, h_prev) for the backward pass.
 * Sizes: dim_zm <= 16 and dim_zm + dim_zl <= 32 (one thread per hidden unit, the weights of its row in registers;
 * the reference's default is 10 (+ 6 labels)); up to dim_zm = 64 and dim_zm + dim_zl = 128 the same recurrence with the
 * weights read from memory (~10x the time per step); larger sizes return MCG_ERR_UNSUPPORTED. */
int mcg_gru_seq_fwd(int N, int T, int dim_zm, int dim_zl, int dim_zc, const float* params,
                    const float* h0, const float* e, const int32_t* labels, const float* zc,
                    float* z, float* saved, void* stream);
/* gz [T*N][dim_zc+dim_zm]: gradient w.r.t. z.  dparams += gradient of all GRU parameters. */
int mcg_gru_seq_bwd(int N, int T, int dim_zm, int dim_zl, int dim_zc, const float* params,
                    const float* e, const int32_t* labels, const float* saved, const float* gz,
                    float* dparams, void* stream);

/* ---- losses (model/updater.py:21-63) -------------------------------------------------------- */
/* logits are [N][C] (C = 1, or 1+K for infogan).  loss_out[0] = loss.  with_ce: add the
 * categorical terms (infogan and VideoDiscriminator only, model/updater.py:28-37). */
int mcg_loss_dis(int N, int C, const float* y_real, const float* y_fake, const int32_t* t_real,
                 const int32_t* t_fake, int with_ce, float* loss_out, float* g_real, float* g_fake,
                 void* stream);
int mcg_loss_gen(int N, int C, const float* y_fake_i, const float* y_fake_v, const int32_t* t_fake,
                 int with_ce, float* loss_out, float* g_i, float* g_v, void* stream);

/* ---- optimiser (train.py:93-101: Chainer Adam + WeightDecay hook) --------------------------- */
/* g' = grad_scale*g + wd*p; m += (1-b1)(g'-m); v += (1-b2)(g'*g'-v); p -= lr_t * m / (sqrt(v) + eps), with
 * lr_t = alpha*sqrt(1-b2^t)/(1-b1^t) computed by the caller in double.  grad_scale is 1 on a single device
 * (the reference) and 1/world under data parallelism, where g holds the all-reduced SUM of the ranks' gradients:
 * the mean is formed here instead of in a separate pass over the gradient. */
int mcg_adam_wd(int64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta1,
                double beta2, double eps, double wd, double grad_scale, uint16_t* p_bf16, void* stream);
/* (p_bf16, may be NULL: a bf16 copy of the updated parameters, the weight operand of MCG_PREC_BF16_STORE launches) */

/* mcg_adam_wd plus an exponential moving average of the parameters in the same pass (no reference counterpart: the reference
 * samples the last iterate of train.py:93-101's optimizers): after the update above, ema <- ema + ema_rate * (p - ema) with the
 * parameter just written, as one subtraction and one fma; ema_rate == 1 stores p itself, bit for bit.  p, m, v and p_bf16 come
 * out bit for bit as mcg_adam_wd writes them.  ema_rate = 1 - decay in (0, 1], formed by the caller in double (a warm-up
 * schedule lives there, like lr_t).  ema [n] must not overlap p, g, m or v.  Pointers need 4-byte alignment only (p_bf16: 2);
 * when all are 16-byte aligned (p_bf16: 8) the pass uses 16-byte accesses.  MCG_ERR_BAD_ARG: a null pointer (p_bf16 may be
 * NULL), n <= 0, ema_rate outside (0, 1], ema overlapping p / g / m / v. */
int mcg_adam_wd_ema(int64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta1,
                    double beta2, double eps, double wd, double grad_scale, uint16_t* p_bf16, float* ema,
                    float ema_rate, void* stream);
/* The same average for tensors no optimizer writes -- the generator's BatchNorm running statistics (model/net.py:50-53), so
 * that the averaged generator is a complete test-mode network: dst <- dst + ema_rate * (src - dst) (ema_rate == 1: dst = src)
 * over nseg <= 32 segments of any n >= 1 in ONE launch.  `segs` is a HOST array; 4-byte alignment suffices.
 * MCG_ERR_BAD_ARG: a null pointer, nseg <= 0 or > 32, an n <= 0, ema_rate outside (0, 1]. */
typedef struct mcg_ema_seg { const float* src; float* dst; int64_t n; } mcg_ema_seg;
int mcg_ema_multi(int nseg, const mcg_ema_seg* segs, float ema_rate, void* stream);

/* ---- gradient norms on the device: telemetry, norm clipping (chainer.optimizer.GradientClipping), non-finite skip ----------
 * mcg_grad_stats reduces nseg <= 32 segments [offset, offset + n) (elements) of the flat gradient g and leaves
 *   stats [(nseg + 1)][4] doubles, a row per segment: { sum of g^2, largest |g|, number of non-finite elements, 0 }.  Non-finite
 *         elements are counted and kept out of the sum and the maximum (0 when no element is finite).  Row nseg is the total: the
 *         sums added in segment order, the largest maximum, the counts added;
 *   ctl   [8] floats, from   norm = grad_scale * sqrt(total sum),   rate = min(1, threshold / norm) (1 when norm == 0),
 *         bad = (total count > 0), all three in double:
 *         ctl[0] = (float)(grad_scale * rate), (float)grad_scale when bad     the gradient scale mcg_adam_wd_ctl applies
 *         ctl[1] = bad ? 1 : 0                                                mcg_adam_wd_ctl then writes nothing
 *         ctl[2] = (float)rate     ctl[3] = (float)norm
 *         ctl[4] = max(ctl[4], ctl[3]) when !bad and ctl[3] is finite         a running peak: the reader zeroes it
 *         ctl[5] += bad                                                       skipped updates, exact to 2^24; persists
 *         ctl[6], ctl[7]: not touched.
 * grad_scale is 1 / world under data parallelism (g holds the SUM over the ranks: the norm is the mean gradient's);
 * threshold = +inf never clips and still skips.  `segs` is a HOST array.  g needs 4-byte alignment; a segment that starts on a
 * 16-byte boundary is read with 16-byte loads throughout, any other after a scalar head.
 * Two launches -- per-block partial sums into `workspace` (mcg_grad_stats_workspace_bytes(nseg) = 32 bytes for each of the at
 * most MAX_PART = 512 blocks), then one block that adds them -- no float atomics, no hand-off between workgroups inside a launch.
 * Squares are formed and added in double: per thread, over the block in a fixed tree, over a segment's blocks in block order.
 * Two calls on the same input agree bit for bit.  Blocks: with S = mcg_grad_stats_span() (the elements a block covers per loop
 * trip) and N the sum of all n, segment s gets  min(ceil(n_s / S), 1 + floor((512 - nseg) * n_s / N))  blocks, its trips
 * dealt to them round-robin.
 * MCG_ERR_BAD_ARG: a null pointer, nseg outside [1, 32], an n <= 0, an offset < 0, grad_scale not finite and positive,
 * threshold NaN or <= 0. */
typedef struct mcg_stat_seg { int64_t offset; int64_t n; } mcg_stat_seg;
int64_t mcg_grad_stats_workspace_bytes(int nseg);
int mcg_grad_stats_span(void);
int mcg_grad_stats(int nseg, const mcg_stat_seg* segs, const float* g, double grad_scale, double threshold,
                   double* stats, float* ctl, void* workspace, void* stream);
/* mcg_adam_wd_ema with the gradient scale taken from DEVICE memory: grad_scale = ctl[0], read once per thread, and a launch that
 * finds ctl[1] != 0 writes nothing -- p, m, v, p_bf16 and ema keep their bits (the host's step counter has advanced all the same:
 * nothing here waits for the device).  ema may be NULL (ema_rate is then ignored): mcg_adam_wd.  Same arithmetic, same 16-byte /
 * scalar forms by the same alignment rule: with ctl[1] == 0 the outputs are bit for bit those of mcg_adam_wd / mcg_adam_wd_ema
 * called with grad_scale = ctl[0].  MCG_ERR_BAD_ARG: as mcg_adam_wd_ema (ema NULL allowed), a null ctl. */
int mcg_adam_wd_ctl(int64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta1,
                    double beta2, double eps, double wd, const float* ctl, uint16_t* p_bf16, float* ema,
                    float ema_rate, void* stream);

/* out[i] = sigma * N(0,1), the same Philox stream mcg_bn_act_fwd / mcg_pack_clip draw from. */
int mcg_randn(int64_t n, float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream);
/* out[M][C] = sigma * N(0,1) in the element order of the fused first-layer epilogue (mcg_conv_epilogue.sigma):
 * element (m, c) is normal m & 3 of Philox counter (m >> 2) * C + c.  M % 4 == 0. */
int mcg_randn_rowquad(int64_t M, int C, float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream);
/* The split layout of MCG_PREC_SPLIT.  src is n fp32 values seen as consecutive runs of `run` values (run a multiple of 16,
 * n a multiple of run); dst gets, per run, four runs of bf16: hi, mid, lo (as above) and one of padding that is neither written
 * nor ever fetched by a MCG_PREC_SPLIT launch (it makes a group of 16 channels one 128-byte K-step) -- 4 * n uint16_t in all.
 *   run = 16                 : channels-last tensors [.. pixels][C] -> [.. pixels][C/16][4][16]   (the summed dimension of
 *                              x / y, and of w = [Co][taps][Ci] as fprop reads it);
 *   run = 16 * taps * Ci     : w as dgrad reads it -> [Co/16][4][16][taps][Ci] (the planes of 16 filters, filter by filter). */
int mcg_split_planes(int64_t n, int64_t run, const float* src, void* dst, void* stream);
/* Several mcg_split_planes in ONE launch (ABI 6): segment s splits segs[s].n values at segs[s].src into segs[s].dst with run
 * segs[s].run -- bit for bit what the single call writes.  For the filters of an 'f32x3' network: every (filter, form) pair the
 * network's launches read is refreshed in one launch right after the Adam update instead of one launch per pair on first use
 * (train.py:93-101 is where the reference's optimizer rewrites the parameters).  `segs` is a HOST array of nseg <= 32 entries. */
typedef struct mcg_split_seg { const float* src; void* dst; int64_t n; int64_t run; } mcg_split_seg;
int mcg_split_planes_multi(int nseg, const mcg_split_seg* segs, void* stream);

/* out[i] = word (i & 3) of Philox counter (i >> 2) of the stream, modulo `modulus`: the generator's label draw
 * xp.random.randint(dim_zl, size=batchsize) (model/net.py:91-92) from the same keyed generator as the normals. */
int mcg_randint(int64_t n, int modulus, uint64_t seed, uint64_t stream_id, int32_t* out, void* stream);

/* ---- sliced Wasserstein distance between two sets of clips (csrc/metrics.hip) ----------------------------------------------
 * Karras et al. 2018, "Progressive Growing of GANs", section 5 (no reference counterpart: the reference has no metric; its
 * model/updater.py imports scipy.linalg for a Frechet score it never computes).  Random 7x7(x pt frames) patches of a three-level
 * Laplacian pyramid are normalised per channel, projected on random unit directions, every direction is sorted, and the two sets'
 * sorted projections are compared rank by rank.  The stages are separate entry points; mocogan-chainer_amd/metrics.py composes them.
 * No float atomics anywhere: sums are per-block partials in double, added in a fixed order, so every result is bit-reproducible.
 * One workspace serves every stage: mcg_swd_workspace_bytes(n, D, rows) bytes, 16-byte aligned, for descriptor matrices of n rows
 * and D columns and `rows` sorted rows of length n (0 on a bad argument).
 *
 * mcg_swd_pyramid: uint8 clips [N][T][64][64][C], C = 1..3 (MCG_ERR_UNSUPPORTED for another frame size), bytes taken as fp32
 *   0..255, to the levels l64 [N][T][64][64][4], l32 [N][T][32][32][4], l16 [N][T][16][16][4] (pad channels zero).  With
 *   f = [1,4,6,4,1]/16 and scipy's 'mirror' boundary (d c b | a b c d | c b a): down(x) = (x * f(x)f)[::2, ::2]; up(x) = x at the
 *   even positions of a zero image twice the size, * 4 f(x)f;  l64 = G64 - up(G32), l32 = G32 - up(G16), l16 = G16 (G64 the frame,
 *   G32 = down(G64), G16 = down(G32)).  One workgroup per frame, all levels of a channel in LDS (31 KB), one launch.
 * mcg_swd_gather: `level` is one of the three levels (hw = 64 / 32 / 16) of N clips whose global indices start at first_clip; writes
 *   the N * P descriptor rows of those clips to `desc` (= row first_clip * P of the whole set's matrix), D = pt * 49 * C floats each.
 *   Row j of clip i takes Philox counter g = i * P + j of (seed, stream_id); with its words w0, w1, w2: t0 = w0 % (T - pt + 1),
 *   y0 = w1 % (hw - 6), x0 = w2 % (hw - 6); element ((dt*7 + dy)*7 + dx)*C + c = level[i][t0 + dt][y0 + dy][x0 + dx][c] -- exact
 *   copies, and by the moduli no address outside the clip.  A set gathered in chunks equals the set gathered in one call.
 * mcg_swd_channel_sums: sums [2*C] doubles = [sum over channel c | sum of squares over channel c] of desc [n][D] (element e of a row
 *   belongs to channel e % C), the pattern of mcg_bn_sums.  A pass of its own over the whole matrix, so chunking cannot change it.
 * mcg_swd_normalize: desc <- (desc - mean_c) / std_c (population std) in place, evaluated in double and rounded once.  A channel of
 *   zero variance -- variance not above 1e-12 of the channel's mean square -- becomes zeros (ProGAN's NumPy would write NaN).
 * mcg_swd_unit_columns: every column of dirs [D][K] (mcg_randn of D * K values) scaled to unit L2 norm (norm in double).
 * mcg_swd_project: out[k][i] = sum_d desc[i][d] * dirs[d][k], direction-major [K][n_stride] (n_stride >= n; a direction is a
 *   contiguous row for the sort), on v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulation; any D (the tail is zero-filled).
 * mcg_sort_rows: sorts `rows` independent rows data[r * row_stride .. + n) ascending, in place, keys only, any n >= 1; elements
 *   n .. row_stride of a row are not touched.  Bitonic: steps inside mcg_sort_local_span() elements run in LDS, every wider step is
 *   a launch of its own over the rows padded to a power of two in `workspace` (not needed, may be NULL, for
 *   n <= mcg_sort_local_span()).  No kernel waits on another workgroup.  The order is the total order of the bit patterns that
 *   agrees with < on finite and infinite values: -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN, NaNs by payload.  So the result is
 *   a permutation of the row's bit patterns whatever it holds, and equal to a comparison sort's wherever the values are no NaN
 *   (-0 before +0).  Every access stays inside the row (indices do not depend on values).  rows <= 65535.
 * mcg_swd_distance: out[0] = mean over k < K, i < n of |a[k][i] - b[k][i]| for two sorted sets (differences and sums in double, fixed
 *   order: out(a, b) == out(b, a) bit for bit and out(a, a) == 0).  n_a != n_b is MCG_ERR_BAD_ARG.
 * MCG_ERR_BAD_ARG: a null pointer, a non-positive extent, C outside 1..3, pt > T, a stride below its extent. */
int64_t mcg_swd_workspace_bytes(int64_t n, int D, int rows);
int mcg_swd_pyramid(int N, int C, int T, int H, int W, const uint8_t* clips, float* l64, float* l32, float* l16, void* stream);
int mcg_swd_gather(int N, int C, int T, int hw, const float* level, int64_t first_clip, int P, int pt, uint64_t seed,
                   uint64_t stream_id, float* desc, void* stream);
int mcg_swd_channel_sums(int64_t n, int D, int C, const float* desc, double* sums, void* workspace, void* stream);
int mcg_swd_normalize(int64_t n, int D, int C, float* desc, const double* sums, void* stream);
int mcg_swd_unit_columns(int D, int K, float* dirs, void* stream);
int mcg_swd_project(int64_t n, int D, int K, const float* desc, const float* dirs, float* out, int64_t n_stride, void* stream);
int mcg_sort_local_span(void);
int mcg_sort_rows(int rows, int64_t n, float* data, int64_t row_stride, void* workspace, void* stream);
int mcg_swd_distance(int K, int64_t n_a, int64_t n_b, const float* a, int64_t a_stride, const float* b, int64_t b_stride,
                     double* out, void* workspace, void* stream);

/* ---- nearest-neighbour sample metrics on the int8 matrix pipe (csrc/knn.hip) -------------------------------------------------
 * Improved precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and a data-copying score (after
 * Meehan et al. 2020) all reduce to pairwise squared distances between whole-clip descriptors, the k smallest per row, and counts
 * (no reference counterpart: the reference has no metric).  The descriptors are bytes, so every quantity is an integer; with
 * D <= 32768, |a.b| <= 2^29, |a|^2 <= 2^29 and the largest squared distance 255^2 * 32768 = 2 130 739 200 < 2^31: dots, norms and
 * distances are exact in int32 and equal NumPy's bit for bit.  mocogan-chainer_amd/metrics.py (KnnMetrics) composes the stages.
 * No atomics, no workspace, no address that depends on data; one launch each.
 *
 * mcg_knn_descriptors: uint8 clips [N][T][64][64][C], C = 1..3 (MCG_ERR_UNSUPPORTED for another frame size), pool in {2, 4, 8}.
 *   With s the sum of a pool x pool box of one channel, q = (2 s + pool^2) / (2 pool^2) (integer division: the mean rounded half
 *   up, 0..255); desc holds int8(q - 128), row-major over (T, 64/pool, 64/pool, C): D = T (64/pool)^2 C, always a multiple of
 *   64.  norms[n] = sum of desc[n][:]^2.  D > 32768 is MCG_ERR_UNSUPPORTED.  One workgroup per clip.
 * mcg_knn_sqdist: out[i][j] = na[i] + nb[j] - 2 sum_d a[i][d] b[j][d] for a [M][D], b [N][D] (both K-contiguous rows, 16-byte
 *   aligned), on v_mfma_i32_32x32x32_i8.  Any M, N >= 1; D a multiple of 64 in 64..32768 (another multiple of 64:
 *   MCG_ERR_UNSUPPORTED; no multiple or a misaligned a / b: MCG_ERR_BAD_ARG).  128 x 128 tiles; row indices past M and N are
 *   clamped on load and their results are not stored: nothing outside a, b, na, nb is read, elements N .. ld of a row of out are
 *   not written.  a and b may be the same matrix.  M <= 128 * 65535.
 * mcg_knn_smallest: for every row of dist [M][ld] the k smallest of its first N entries in ascending (value, column) order -- ties
 *   go to the lower column -- as val [M][k], idx [M][k]; 1 <= k <= 16.  With exclude_self, column self_col0 + i of row i is
 *   skipped (a row block starting at row self_col0 of a self-distance matrix leaves out its own diagonal).  Missing neighbours
 *   (fewer than k candidates) are val = INT32_MAX, idx = -1.  One wave per row.
 * mcg_knn_ball_counts: counts[i] = #{j < N : dist[i][j] <= radius[j]}.  One wave per row.
 * MCG_ERR_BAD_ARG, refused on the host before any launch: a null pointer, a non-positive extent, C outside 1..3, another pool,
 *   ld < N, k outside 1..16. */
int mcg_knn_descriptors(int N, int C, int T, int H, int W, int pool, const uint8_t* clips, int8_t* desc, int32_t* norms, void* stream);
int mcg_knn_sqdist(int M, int N, int D, const int8_t* a, const int32_t* na, const int8_t* b, const int32_t* nb, int32_t* out, int64_t ld,
                   void* stream);
int mcg_knn_smallest(int M, int N, const int32_t* dist, int64_t ld, int k, int exclude_self, int64_t self_col0, int32_t* val, int32_t* idx,
                     void* stream);
int mcg_knn_ball_counts(int M, int N, const int32_t* dist, int64_t ld, const int32_t* radius, int32_t* counts, void* stream);

/* ---- motion and content metrics on the int8 matrix pipe (csrc/motion.hip) ------------------------------------------------------
 * Average Content Distance (after Tulyakov et al. 2018, section 5), a temporal lag profile and motion descriptors for the
 * nearest-neighbour metrics all reduce to squared distances between the frames of ONE clip, plus two reductions (no reference
 * counterpart: the reference has no metric).  A row of mcg_knn_descriptors is row-major over (T, 64/pool, 64/pool, C), so desc seen
 * as [N][T][Df], Df = (64/pool)^2 C, holds the per-frame descriptors: Df is a multiple of 64 and at most 3072, and the largest
 * frame distance is 255^2 * 3072 = 199 756 800.  mocogan-chainer_amd/metrics.py (MotionContent) composes the stages.
 * No atomics, no workspace, no address that depends on data; one launch each; indices past an extent are clamped on load and
 * never stored.
 *
 * mcg_mc_frame_sqdist: dist[n][s][t] = sum_d (desc[n][s][d] - desc[n][t][d])^2 for desc [N][T][Df] (16-byte aligned), dist
 *   [N][T][T], exact in int32, on v_mfma_i32_16x16x64_i8 as G[s][s] + G[t][t] - 2 G[s][t] with G the clip's Gram matrix: the norms
 *   are G's diagonal, the diagonal of dist is exactly 0 and dist is exactly symmetric.  2 <= T <= 64 (padded to tiles of 16 in
 *   registers only); Df a multiple of 64 in 64..3072; anything else is MCG_ERR_UNSUPPORTED.  One wave per clip, four clips per
 *   workgroup; every byte of desc is read once.
 * mcg_mc_clip_stats: pair_sum[n] = sum_{s<t} sqrt((double) dist[n][s][t]), added in double in the fixed order s ascending, then t
 *   ascending, one accumulator chain per clip: the same input gives the same bits.  lag_sum[n][l] = sum_{t=0}^{T-1-l}
 *   dist[n][t][t+l] for l = 0..T-1 (lag_sum [N][T]; l = 0 sums the diagonal), exact in int64.  2 <= T <= 64, else
 *   MCG_ERR_UNSUPPORTED.  One wave per clip.
 * mcg_mc_motion_descriptors: mdesc[n][t][d] = (desc[n][t+1][d] - desc[n][t][d]) >> 1 for t = 0..T-2 (arithmetic shift: the floor of
 *   half the difference; -255 -> -128, 255 -> 127, -1 -> -1, 1 -> 0: every value fits int8 with no clamp), mdesc [N][(T-1) Df];
 *   mnorms[n] = the sum of squares of row n (at most 2^14 (T-1) Df).  desc and mdesc 16-byte aligned.  T >= 2, Df a multiple of 64
 *   and (T-1) Df <= 32768 -- the rows are valid operands of mcg_knn_sqdist -- else MCG_ERR_UNSUPPORTED.  One workgroup per clip.
 * MCG_ERR_BAD_ARG, refused on the host before any launch: a null pointer, a non-positive extent, a misaligned desc / mdesc. */
int mcg_mc_frame_sqdist(int N, int T, int Df, const int8_t* desc, int32_t* dist, void* stream);
int mcg_mc_clip_stats(int N, int T, const int32_t* dist, double* pair_sum, int64_t* lag_sum, void* stream);
int mcg_mc_motion_descriptors(int N, int T, int Df, const int8_t* desc, int8_t* mdesc, int32_t* mnorms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOCOGAN_HIP_H */
