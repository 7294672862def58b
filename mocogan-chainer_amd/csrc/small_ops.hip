// HBM-bound and tiny kernels of the MoCoGAN step for gfx950: BatchNorm statistics / apply /
// backward fused with the activations and add_noise, Philox noise, layout packing, the
// full-window (1x1-output) layers, the fused GRU recurrence, the GAN losses and Chainer-Adam.
// Tensors are channels-last with C % 4 == 0, fp32 or (MCG_IO_* flags, bf16 networks) bf16 in memory.  The element-wise passes
// give a thread 4 channels, or 8 where a tensor of the call is bf16 and C % 8 == 0, so a lane's access is 16 bytes (8 for four bf16).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <type_traits>
#include "mocogan_hip.h"
#include "mcg_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int NT = 256;
constexpr int MAX_PART = 512;        // max partial-reduction blocks (workspace sizing)
constexpr float LRELU_SLOPE = 0.2f;  // model/net.py:149-155,190-196

int launch_status() { return hipGetLastError() == hipSuccess ? MCG_OK : MCG_ERR_LAUNCH; }

using mcg::randn4;

// W = 4 or 8 consecutive channels of a thread, as fp32 values (vecf) and as they lie in a bf16 tensor (vecb)
template <int W> using vecf = float __attribute__((ext_vector_type(W)));
template <int W> using vecb = __bf16 __attribute__((ext_vector_type(W)));
template <int W> constexpr int LOG2 = W == 8 ? 3 : 2;
typedef vecf<8> f32x8;
typedef vecb<4> bf16x4_t;
typedef vecb<8> bf16x8_t;

// the W elements starting at ELEMENT offset e (a multiple of W) of a tensor that is fp32 or (in16) bf16 in memory: bf16 networks
// keep the GEMM operands -- activations, output gradients -- and the GEMM outputs the element-wise passes read -- pre-BatchNorm
// activations, input gradients -- in bf16.  W = 8 makes a bf16 access 16 bytes per lane (with groups of four it is 8, and the bf16
// networks' passes ran at half the bytes in flight); fp32 accesses are 16 bytes at either width.
template <int W>
__device__ __forceinline__ vecf<W> loadv(const float* in, long long e, int in16) {
    if (in16) return __builtin_convertvector(*reinterpret_cast<const vecb<W>*>(reinterpret_cast<const __bf16*>(in) + e), vecf<W>);
    if constexpr (W == 4) return *reinterpret_cast<const f32x4*>(in + e);
    else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(in + e), b = *reinterpret_cast<const f32x4*>(in + e + 4);
        return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}
template <int W>
__device__ __forceinline__ vecf<W> cvec(const float* p, int group) { return loadv<W>(p, group * W, 0); }    // per-channel constants of a channel group

// fp32 -> the three bf16 terms of MCG_PREC_SPLIT (include/mocogan_hip.h): hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid);
// the differences are exact in fp32 and v == hi + mid + lo.  One thread: 8 consecutive values of a run -> one 16-byte piece of each
// of the run's three planes (the fourth, padding, is not written).
__device__ __forceinline__ void split3(f32x8 v, bf16x8_t& hi, bf16x8_t& mid, bf16x8_t& lo) {
    hi = __builtin_convertvector(v, bf16x8_t);
    const f32x8 r1 = v - __builtin_convertvector(hi, f32x8);
    mid = __builtin_convertvector(r1, bf16x8_t);
    const f32x8 r2 = r1 - __builtin_convertvector(mid, f32x8);
    lo = __builtin_convertvector(r2, bf16x8_t);
}
__device__ __forceinline__ void store_split8(__bf16* dst, long long e, long long run, f32x8 v) {      // e: index of the first of 8 source values
    bf16x8_t hi, mid, lo;
    split3(v, hi, mid, lo);
    const long long r = e / run, o = e - r * run;
    __bf16* d = dst + r * 4 * run + o;
    *reinterpret_cast<bf16x8_t*>(d) = hi;
    *reinterpret_cast<bf16x8_t*>(d + run) = mid;
    *reinterpret_cast<bf16x8_t*>(d + 2 * run) = lo;        // (the fourth plane only pads a group to 128 bytes: no kernel fetches it)
}
// the store to match loadv; oflags: 0 (fp32), MCG_IO_OUT_BF16 (round-to-nearest-even, v_cvt_pk_bf16_f32) or, W = 8 only, MCG_IO_OUT_SPLIT
template <int W>
__device__ __forceinline__ void storev(float* out, long long e, vecf<W> v, int oflags) {
    if constexpr (W == 8) {
        if (oflags & MCG_IO_OUT_SPLIT) { store_split8(reinterpret_cast<__bf16*>(out), e, 16, v); return; }
    }
    if (oflags) { *reinterpret_cast<vecb<W>*>(reinterpret_cast<__bf16*>(out) + e) = __builtin_convertvector(v, vecb<W>); return; }
    if constexpr (W == 4) *reinterpret_cast<f32x4*>(out + e) = v;
    else {
        *reinterpret_cast<f32x4*>(out + e) = __builtin_shufflevector(v, v, 0, 1, 2, 3);
        *reinterpret_cast<f32x4*>(out + e + 4) = __builtin_shufflevector(v, v, 4, 5, 6, 7);
    }
}

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == MCG_ACT_RELU) return fmaxf(v, 0.f);
    if (act == MCG_ACT_LRELU) return v >= 0.f ? v : v * LRELU_SLOPE;
    if (act == MCG_ACT_TANH) return tanhf(v);
    return v;
}
// derivative factor given the pre-activation value v (Chainer masks on the retained output,
// whose sign equals the pre-activation's sign for relu / leaky_relu)
__device__ __forceinline__ float act_mask(float v, int act) {
    if (act == MCG_ACT_RELU) return v > 0.f ? 1.f : 0.f;
    if (act == MCG_ACT_LRELU) return v < 0.f ? LRELU_SLOPE : 1.f;
    return 1.f;
}

// ------------------------------------------------------------------------------------------
// per-channel partial sums over rows of a [M][C] tensor.
// MODE 0: (sum y, sum y^2)           -> BN statistics
// MODE 1: (sum g_bn, sum g_bn*x_hat) -> BN backward
// MODE 2: (sum g, unused)            -> bias gradient
// Thread layout: CW = C/W columns of W channels, RL = NT/CW row lanes per pass (CW divides NT: unsupported_c, wide_c); the
// block's row lanes are combined through LDS; part[block][2][C].  W = 8 (MODE 1 of bf16 networks) has half the columns and
// twice the row lanes of W = 4, so the two widths add the same addends in different trees.
// ------------------------------------------------------------------------------------------
template <int MODE, int W = 4, int IO = 0>           // IO: MCG_IO_* flags of a (G) and y (Y), compile-time (see bn_act_fwd_kernel)
__global__ __launch_bounds__(NT) void col_partial_kernel(long long M, int C, long long rows_per_block,
                                                         const float* __restrict__ a, const float* __restrict__ y,
                                                         const float* __restrict__ stats, int act,
                                                         float* __restrict__ part) {
    using V = vecf<W>;
    __shared__ V red[2][NT];
    const int CW = C >> LOG2<W>;
    const int c = threadIdx.x % CW, rl = threadIdx.x / CW, RL = NT / CW;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    long long r1 = r0 + rows_per_block; if (r1 > M) r1 = M;
    V s0 = {}, s1 = {}, mean = {}, istd = {}, sc = {}, sh = {};
    // (every launch of MODE 1 has stats; the four-wide kernel keeps its test of the pointer because without it the register
    //  allocation comes out three VGPRs larger, 98, and costs the kernel a wave of occupancy)
    if (MODE == 1 && (W == 8 || stats)) { mean = cvec<W>(stats, c); istd = cvec<W>(stats + C, c); sc = cvec<W>(stats + 2 * C, c); sh = cvec<W>(stats + 3 * C, c); }
    auto row = [&](long long r, V& t0, V& t1) {
        const V v = loadv<W>(a, r * C + c * W, IO & MCG_IO_G_BF16);
        if constexpr (MODE == 0) { t0 = v; t1 = v * v; }
        else if constexpr (MODE == 2) { t0 = v; }
        else {
            const V yy = loadv<W>(y, r * C + c * W, IO & MCG_IO_Y_BF16);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float gb = v[i] * act_mask(fmaf(yy[i], sc[i], sh[i]), act);
                t0[i] = gb; t1[i] = gb * (yy[i] - mean[i]) * istd[i];
            }
        }
    };
    // four rows in flight per thread: with at most MAX_PART blocks on the chip a single dependent load per iteration
    // leaves the pass latency-bound (measured 3.3 TB/s); the sums of a row quad are added in a fixed order
    long long r = r0 + rl;
    for (; r + 3LL * RL < r1; r += 4LL * RL) {
        V a0 = {}, a1 = {}, b0 = {}, b1 = {}, c0 = {}, c1 = {}, d0 = {}, d1 = {};
        row(r, a0, a1); row(r + RL, b0, b1); row(r + 2LL * RL, c0, c1); row(r + 3LL * RL, d0, d1);
        s0 += (a0 + b0) + (c0 + d0); s1 += (a1 + b1) + (c1 + d1);
    }
    for (; r < r1; r += RL) {
        V a0 = {}, a1 = {};
        row(r, a0, a1);
        s0 += a0; s1 += a1;
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1;
    __syncthreads();
    if (threadIdx.x < CW) {
        for (int k = 1; k < RL; ++k) { s0 += red[0][k * CW + c]; s1 += red[1][k * CW + c]; }
        float* p = part + (long long)blockIdx.x * 2 * C;
        storev<W>(p, c * W, s0, 0);
        storev<W>(p + C, c * W, s1, 0);
    }
}

// blocks of col_partial_kernel and the rows each takes: at least 8 rows per thread of the four-wide layout, at most MAX_PART blocks
struct PartPlan { int blocks; long long rows_per_block; };
PartPlan plan_partial(long long M, int C) {
    int RL = NT / (C >> 2);
    long long min_rows = (long long)RL * 8;                   // >= 8 rows per thread
    long long b = (M + min_rows - 1) / min_rows;
    if (b > MAX_PART) b = MAX_PART;
    if (b < 1) b = 1;
    PartPlan p;
    p.rows_per_block = (M + b - 1) / b;
    p.blocks = (int)((M + p.rows_per_block - 1) / p.rows_per_block);
    return p;
}

// Conv epilogues leave one partial per block tile -- thousands for the big layers, far more than a finalize block (8
// channels) can sum at memory latency.  fold_partials_kernel first folds runs of `per` consecutive slots into the
// workspace with fully coalesced row reads (thread = one channel, NT / cw slots in flight per pass), in a fixed order.
__global__ __launch_bounds__(NT) void fold_partials_kernel(int n_slots, long long stride, int C, int per, const float* __restrict__ part,
                                                           float* __restrict__ out) {
    __shared__ double red[2][NT];
    const int cw = C < 64 ? C : 64;                         // channels per block (C = 4 * 2^k: cw divides NT)
    const int c = blockIdx.x * cw + threadIdx.x % cw, rl = threadIdx.x / cw, RL = NT / cw;
    const int s0 = blockIdx.y * per;
    int s1 = s0 + per; if (s1 > n_slots) s1 = n_slots;
    double a = 0, b = 0;
    if (c < C) {
        // eight slots in flight per thread (round 5): with one dependent load per trip this kernel, like the finalize kernels below,
        // ran at memory LATENCY -- 5-8 us for a few hundred KB.  The additions keep their order (bit-identical sums).
        int sl = s0 + rl;
        for (; sl + 7 * RL < s1; sl += 8 * RL) {
            float x[8], y[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { x[u] = part[(long long)(sl + u * RL) * stride + c]; y[u] = part[(long long)(sl + u * RL) * stride + C + c]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { a += x[u]; b += y[u]; }
        }
        for (; sl < s1; sl += RL) { a += part[(long long)sl * stride + c]; b += part[(long long)sl * stride + C + c]; }
    }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
    __syncthreads();
    if (rl == 0 && c < C) {
        for (int k = 1; k < RL; ++k) { a += red[0][k * cw + threadIdx.x]; b += red[1][k * cw + threadIdx.x]; }
        out[(long long)blockIdx.y * 2 * C + c] = (float)a;
        out[(long long)blockIdx.y * 2 * C + C + c] = (float)b;
    }
}

constexpr int FOLD_ABOVE = 96;       // slot counts up to this go straight to the finalize kernels

// Finalize kernels: block = FIN_CH channels x FIN_SL slices of the partial-block list; each thread
// sums its slice in double, slices are combined through LDS in a fixed order (deterministic).
constexpr int FIN_CH = 8, FIN_SL = 32;

__device__ __forceinline__ bool reduce_partials(int nblocks, int C, const float* __restrict__ part, int& c, double& s, double& ss,
                                                long long stride = 0) {
    if (stride == 0) stride = 2LL * C;                        // col_partial_kernel's own layout; fused conv epilogues pass theirs
    __shared__ double red[2][FIN_SL][FIN_CH];
    const int cl = threadIdx.x % FIN_CH, sl = threadIdx.x / FIN_CH;
    c = blockIdx.x * FIN_CH + cl;
    double a = 0, b2 = 0;
    if (c < C) {
        int b = sl;
        for (; b + 7 * FIN_SL < nblocks; b += 8 * FIN_SL) {          // eight partials in flight per thread, added in the old order
            float x[8], y[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { x[u] = part[(long long)(b + u * FIN_SL) * stride + c]; y[u] = part[(long long)(b + u * FIN_SL) * stride + C + c]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { a += x[u]; b2 += y[u]; }
        }
        for (; b < nblocks; b += FIN_SL) { a += part[(long long)b * stride + c]; b2 += part[(long long)b * stride + C + c]; }
    }
    red[0][sl][cl] = a; red[1][sl][cl] = b2;
    __syncthreads();
    if (sl != 0 || c >= C) return false;
    s = 0; ss = 0;
    for (int k = 0; k < FIN_SL; ++k) { s += red[0][k][cl]; ss += red[1][k][cl]; }
    return true;
}

// Channel c's BatchNorm statistics from its sums over M = 1 / inv_m rows: stats[0..4C) = mean, inv_std, scale = gamma * inv_std,
// shift = beta - mean * scale, and the running averages (adjust: bessel_adjust(M)).  The ONE statement of the Chainer-3.1 variance rule.
__device__ __forceinline__ void bn_stats_write(int c, int C, double s, double ss, double inv_m, double adjust, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, float* __restrict__ stats, float* avg_mean, float* avg_var,
                                               float eps, float decay) {
    double mean = s * inv_m;
    double var = ss * inv_m - mean * mean;
    if (var < 0) var = 0;
    var += eps;                                            // Chainer 3.1: var += eps before everything else
    float istd = (float)(1.0 / sqrt(var));
    float scale = gamma[c] * istd;
    stats[c] = (float)mean;
    stats[C + c] = istd;
    stats[2 * C + c] = scale;
    stats[3 * C + c] = fmaf(-(float)mean, scale, beta[c]);
    if (avg_mean) {
        avg_mean[c] = avg_mean[c] * decay + (1.f - decay) * (float)mean;
        avg_var[c] = avg_var[c] * decay + (1.f - decay) * (float)(adjust * var);
    }
}

// Channel c of the backward pass: coef[0..C) = gamma*inv_std, [C..2C) = ggamma/M, [2C..3C) = gbeta/M from the sums (gb, gg) of the
// batch the statistics were taken over; dgamma / dbeta accumulate this rank's own sums (the same numbers unless BatchNorm is synchronised)
__device__ __forceinline__ void bn_bwd_write(int c, int C, double gb, double gg, double inv_m, double gb_local, double gg_local,
                                             const float* __restrict__ stats, const float* __restrict__ gamma, float* __restrict__ coef,
                                             float* dgamma, float* dbeta) {
    coef[c] = gamma[c] * stats[C + c];
    coef[C + c] = (float)(gg * inv_m);
    coef[2 * C + c] = (float)(gb * inv_m);
    if (dgamma) dgamma[c] += (float)gg_local;
    if (dbeta) dbeta[c] += (float)gb_local;
}

__global__ __launch_bounds__(FIN_CH * FIN_SL) void bn_stats_finalize_kernel(int nblocks, int C, double inv_m, double adjust, const float* __restrict__ part,
                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                         float* __restrict__ stats, float* avg_mean, float* avg_var, float eps, float decay, long long stride) {
    int c; double s, ss;
    if (reduce_partials(nblocks, C, part, c, s, ss, stride)) bn_stats_write(c, C, s, ss, inv_m, adjust, gamma, beta, stats, avg_mean, avg_var, eps, decay);
}

__global__ __launch_bounds__(FIN_CH * FIN_SL) void bn_bwd_finalize_kernel(int nblocks, int C, double inv_m, const float* __restrict__ part,
                                       const float* __restrict__ stats, const float* __restrict__ gamma,
                                       float* __restrict__ coef, float* dgamma, float* dbeta, long long stride) {
    int c; double gb, gg;
    if (reduce_partials(nblocks, C, part, c, gb, gg, stride)) bn_bwd_write(c, C, gb, gg, inv_m, gb, gg, stats, gamma, coef, dgamma, dbeta);
}

// ---- synchronised BatchNorm (opt-in, data parallel): the per-channel sums leave the library as doubles, the caller
// all-reduces them over the ranks, and the second half of each pass starts from the global sums ----
__global__ __launch_bounds__(FIN_CH * FIN_SL) void sums_finalize_kernel(int nblocks, int C, const float* __restrict__ part, double* __restrict__ sums) {
    int c; double s, ss;
    if (!reduce_partials(nblocks, C, part, c, s, ss)) return;
    sums[c] = s; sums[C + c] = ss;
}

__global__ void bn_stats_from_sums_kernel(int C, double inv_m, double adjust, const double* __restrict__ sums,
                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                          float* __restrict__ stats, float* avg_mean, float* avg_var, float eps, float decay) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) bn_stats_write(c, C, sums[c], sums[C + c], inv_m, adjust, gamma, beta, stats, avg_mean, avg_var, eps, decay);
}

// coef from the GLOBAL sums; dgamma / dbeta take the LOCAL sums (the gradient exchange averages them over the ranks afterwards)
__global__ void bn_bwd_from_sums_kernel(int C, double inv_m_total, const double* __restrict__ local_sums, const double* __restrict__ global_sums,
                                        const float* __restrict__ stats, const float* __restrict__ gamma, float* __restrict__ coef,
                                        float* dgamma, float* dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) bn_bwd_write(c, C, global_sums[c], global_sums[C + c], inv_m_total, local_sums[c], local_sums[C + c], stats, gamma, coef, dgamma, dbeta);
}

__global__ __launch_bounds__(FIN_CH * FIN_SL) void colsum_finalize_kernel(int nblocks, int C, const float* __restrict__ part, float* db, long long stride) {
    int c; double s, unused;
    if (!reduce_partials(nblocks, C, part, c, s, unused, stride)) return;
    db[c] += (float)s;
}

// The element-wise passes' grid-stride loop over n groups of W channels: two groups per trip, both loaded before either is used
// -- with bf16 tensors a four-wide group is an 8-byte access, and one per thread in flight leaves the pass latency-bound.
template <class Load, class Finish>
__device__ __forceinline__ void for_each_pair(long long n, Load load, Finish finish) {
    const long long stride = (long long)gridDim.x * NT;
    for (long long i0 = (long long)blockIdx.x * NT + threadIdx.x; i0 < n; i0 += 2 * stride) {
        const long long i1 = i0 + stride < n ? i0 + stride : i0;          // (the tail repeats group 0's load, its result is dropped)
        const auto v0 = load(i0);
        const auto v1 = load(i1);
        finish(i0, v0);
        if (i1 != i0) finish(i1, v1);
    }
}
// A thread's channel group is the same on every trip when the grid stride is a multiple of C / W (every power-of-two channel
// count): the per-channel vectors are then loaded once (first_group), not once per group.
__device__ __forceinline__ bool fixed_group(int CW) { return ((long long)gridDim.x * NT) % CW == 0; }
__device__ __forceinline__ int first_group(int CW) { return (int)(((long long)blockIdx.x * NT + threadIdx.x) % CW); }

// out = act(y*scale+shift) + noise over n groups of W channels.  Noise keeps its element order at either width: group i takes the
// Philox counters i * W/4 + q, q < W/4.  W = 4 only: y may be a batch-strided view (frame t of a clip tensor: item = i / item_groups)
// and channels >= c_valid (the clip's pad channel) take no noise; the eight-wide launches have dense y and every channel valid.
template <int W, int IO>   // MCG_IO_* flags as a compile-time constant: a run-time element type puts a branch (and a wait) around every load
__global__ __launch_bounds__(NT) void bn_act_fwd_kernel(long long n, int C, int c_valid, const float* __restrict__ y,
                                                        long long item_groups, long long item_stride,
                                                        const float* __restrict__ ss, int act,
                                                        const float* __restrict__ addend, float sigma,
                                                        uint64_t seed, uint64_t stream_id, float* __restrict__ out) {
    using V = vecf<W>;
    const int CW = C >> LOG2<W>;
    const bool fixed_c = fixed_group(CW);
    V sc = V{} + 1.f, sh = {};
    auto consts = [&](int c) { if (ss) { sc = cvec<W>(ss, c); sh = cvec<W>(ss + C, c); } };
    consts(first_group(CW));
    auto load = [&](long long i) {
        long long e = i * W;
        if constexpr (W == 4) { if (item_groups) e = (i / item_groups) * item_stride + (i % item_groups) * 4; }
        return loadv<W>(y, e, IO & MCG_IO_Y_BF16);
    };
    auto finish = [&](long long i, V v) {
        const int c = (int)(i % CW);
        if (!fixed_c) consts(c);
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = act_fwd(ss ? fmaf(v[k], sc[k], sh[k]) : v[k], act);
        if (addend) v += loadv<W>(addend, i * W, 0);
        else if (sigma > 0.f) {
#pragma unroll
            for (int q = 0; q < W / 4; ++q) {
                const f32x4 z = randn4((uint64_t)(i * (W / 4) + q), seed, stream_id);
#pragma unroll
                for (int k = 0; k < 4; ++k) if (W == 8 || c * 4 + k < c_valid) v[q * 4 + k] = fmaf(sigma, z[k], v[q * 4 + k]);
            }
        }
        storev<W>(out, i * W, v, IO & (MCG_IO_OUT_BF16 | MCG_IO_OUT_SPLIT));
    };
    for_each_pair(n, load, finish);
}

// gx = coef0 * (g*mask - x_hat*coef1 - coef2)    (BN)   or, W = 4 only,   gx = g*mask(y) / g*(1-y^2)  (no BN: stats == nullptr)
// The one fused multiply-add of the BN form is written out (as in adam_wd_elem): left to the compiler, g*mask - x_hat*coef1 stayed
// unfused in the four-wide kernels, became fma(g, mask, -(x_hat*coef1)) in the eight-wide ones with IO 2, 4, 5, 6, 7 and
// fma(-x_hat, coef1, g*mask) in those with IO 1, 3, 8 -- the bf16 output of one set of inputs was then not always the rounded
// fp32 output of the same inputs (tests/test_gpu_sync_bn.py::test_flag_forms: 1 element of 2 150 400).
template <int W, int IO>
__global__ __launch_bounds__(NT) void bn_act_bwd_apply_kernel(long long n, int C, const float* __restrict__ g,
                                                              const float* __restrict__ y, const float* __restrict__ stats,
                                                              const float* __restrict__ coef, int act, float* __restrict__ gx) {
    using V = vecf<W>;
    struct GY { V g, y; };
    const int CW = C >> LOG2<W>;
    const bool bn = W == 8 || stats != nullptr;
    const bool fixed_c = fixed_group(CW);                       // (the seven per-channel vectors once per thread)
    V mean = {}, istd = {}, sc = {}, sh = {}, k0 = {}, k1 = {}, k2 = {};
    auto consts = [&](int c) {
        if (!bn) return;
        mean = cvec<W>(stats, c); istd = cvec<W>(stats + C, c); sc = cvec<W>(stats + 2 * C, c); sh = cvec<W>(stats + 3 * C, c);
        k0 = cvec<W>(coef, c); k1 = cvec<W>(coef + C, c); k2 = cvec<W>(coef + 2 * C, c);
    };
    consts(first_group(CW));
    auto load = [&](long long i) { return GY{loadv<W>(g, i * W, IO & MCG_IO_G_BF16), loadv<W>(y, i * W, IO & MCG_IO_Y_BF16)}; };
    auto finish = [&](long long i, const GY& in) {
        if (!fixed_c) consts((int)(i % CW));
        V o;
        if (bn) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float gb = in.g[k] * act_mask(fmaf(in.y[k], sc[k], sh[k]), act);
                const float xh = (in.y[k] - mean[k]) * istd[k];
                o[k] = k0[k] * (fmaf(-xh, k1[k], gb) - k2[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = act == MCG_ACT_TANH ? in.g[k] * (1.f - in.y[k] * in.y[k]) : in.g[k] * act_mask(in.y[k], act);
        }
        storev<W>(gx, i * W, o, IO & (MCG_IO_OUT_BF16 | MCG_IO_OUT_SPLIT));
    };
    for_each_pair(n, load, finish);
}

constexpr int EW_GRID = 2048;        // max blocks of an element-wise pass (grid-stride loops)
int ew_grid(long long n4) {
    long long b = (n4 + NT - 1) / NT;
    if (b > EW_GRID) b = EW_GRID;
    if (b < 1) b = 1;
    return (int)b;
}

// ------------------------------------------------------------------------------------------
// layout kernels
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void pack_clip_kernel(int N, int C, int Cp, int T, int HW, const float* __restrict__ x,
                                                       long long sn, long long sc,
                                                       const float* __restrict__ addend, float sigma, uint64_t seed,
                                                       uint64_t stream_id, float* __restrict__ out) {
    const long long npix = (long long)N * T * HW;
    const int Cp4 = Cp >> 2;
    for (long long p = (long long)blockIdx.x * NT + threadIdx.x; p < npix; p += (long long)gridDim.x * NT) {
        int hw = (int)(p % HW);
        long long q = p / HW;
        int t = (int)(q % T), n = (int)(q / T);
        const float* src = x + (long long)n * sn + (long long)t * HW + hw;
        for (int c4 = 0; c4 < Cp4; ++c4) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int c = c4 * 4 + k;
                v[k] = c < C ? src[(long long)c * sc] : 0.f;
            }
            long long i4 = p * Cp4 + c4;
            if (addend) v += *reinterpret_cast<const f32x4*>(addend + i4 * 4);
            else if (sigma > 0.f) {
                f32x4 z = randn4((uint64_t)i4, seed, stream_id);
#pragma unroll
                for (int k = 0; k < 4; ++k) if (c4 * 4 + k < C) v[k] = fmaf(sigma, z[k], v[k]);
            }
            *reinterpret_cast<f32x4*>(out + i4 * 4) = v;
        }
    }
}

// The loader's clips as they arrive: uint8 [n][t][hw][C] (datasets.py:95 decodes to (T,H,W,C); the reference normalises and
// transposes on the host, model/updater.py:87-92).  One pass does what five torch passes did on the product path (uint8 -> float,
// - 128, / 128, permute to (N,C,T,H,W), and mcg_pack_clip back to channels-last): (v - 128) / 128 into the device layout
// [n][t][hw][Cp], zero channel pad, + noise drawn exactly as pack_clip_kernel draws it (one Philox counter per 4-channel group).
// sn / st: BYTE strides of the batch item and the frame in x (a single frame per item: T = 1, sn = T_clip * HW * C).
__global__ __launch_bounds__(NT) void pack_clip_u8_kernel(int N, int C, int Cp, int T, int HW, const uint8_t* __restrict__ x,
                                                          long long sn, long long st,
                                                          const float* __restrict__ addend, float sigma, uint64_t seed,
                                                          uint64_t stream_id, float* __restrict__ out) {
    const long long npix = (long long)N * T * HW;
    const int Cp4 = Cp >> 2;
    for (long long p = (long long)blockIdx.x * NT + threadIdx.x; p < npix; p += (long long)gridDim.x * NT) {
        int hw = (int)(p % HW);
        long long q = p / HW;
        int t = (int)(q % T), n = (int)(q / T);
        const uint8_t* src = x + (long long)n * sn + (long long)t * st + (long long)hw * C;
        for (int c4 = 0; c4 < Cp4; ++c4) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int c = c4 * 4 + k;
                v[k] = c < C ? ((float)src[c] - 128.f) / 128.f : 0.f;
            }
            long long i4 = p * Cp4 + c4;
            if (addend) v += *reinterpret_cast<const f32x4*>(addend + i4 * 4);
            else if (sigma > 0.f) {
                f32x4 z = randn4((uint64_t)i4, seed, stream_id);
#pragma unroll
                for (int k = 0; k < 4; ++k) if (c4 * 4 + k < C) v[k] = fmaf(sigma, z[k], v[k]);
            }
            *reinterpret_cast<f32x4*>(out + i4 * 4) = v;
        }
    }
}

// The way out of the generator, the inverse of pack_clip_u8_kernel: in[n][t][hw][4] fp32 (the padded 3-channel clip, 16 bytes per pixel)
// -> uint8 out[n * sn + t * st + hw * C + c].  The byte is the reference's ((x / 2. + 0.5) * 255).astype(np.uint8)
// (generate_samples.py:39): three separately rounded fp32 operations -- x / 2 is exact, so it is x * 0.5 -- and a truncating cast, so
// that the bytes equal NumPy's on the same x.  act == MCG_ACT_TANH: `in` is the last deconvolution's output BEFORE bias and tanh
// (what dgrad_c4_mfma_kernel leaves) and x = tanh(in + bias) is formed here as bn_act_fwd_kernel forms it.
// PACK (C == 3, hw / strides / out multiples of 4): a thread takes 4 consecutive pixels, 64 bytes in, 12 bytes out as three words.
__device__ __forceinline__ unsigned clip_byte(float x) {
    float v = __fmul_rn(__fadd_rn(__fmul_rn(x, 0.5f), 0.5f), 255.f);
    v = fminf(fmaxf(v, 0.f), 255.f);                  // (|x| <= 1 gives 0 .. 255 already; anything else saturates instead of wrapping)
    return (unsigned)(int)v;
}
template <bool PACK>
__global__ __launch_bounds__(NT) void clip_to_u8_kernel(long long nitems, int C, int T, int HW, const float* __restrict__ in,
                                                        const float* __restrict__ bias, int act, uint8_t* __restrict__ out,
                                                        long long sn, long long st) {
    constexpr int PIX = PACK ? 4 : 1;
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (bias) b = *reinterpret_cast<const f32x4*>(bias);
    const int per = HW / PIX;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < nitems; i += (long long)gridDim.x * NT) {
        const int hw = (int)(i % per) * PIX;
        const long long q = i / per;
        const int t = (int)(q % T);
        const long long n = q / T;
        const f32x4* src = reinterpret_cast<const f32x4*>(in) + i * PIX;
        uint8_t* dst = out + n * sn + (long long)t * st + (long long)hw * C;
        unsigned by[PIX][4];
#pragma unroll
        for (int p = 0; p < PIX; ++p) {
            f32x4 v = src[p];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x = v[k];
                if (act == MCG_ACT_TANH) x = tanhf(__fadd_rn(x, b[k]));
                by[p][k] = clip_byte(x);
            }
        }
        if constexpr (PACK) {                          // 4 pixels x 3 channels = 3 words (little endian: byte 0 is the lowest)
            unsigned* d32 = reinterpret_cast<unsigned*>(dst);       // (4-byte aligned: mcg_clip_to_u8 checks out, strides and HW)
            d32[0] = by[0][0] | (by[0][1] << 8) | (by[0][2] << 16) | (by[1][0] << 24);
            d32[1] = by[1][1] | (by[1][2] << 8) | (by[2][0] << 16) | (by[2][1] << 24);
            d32[2] = by[2][2] | (by[3][0] << 8) | (by[3][1] << 16) | (by[3][2] << 24);
        } else {
            for (int c = 0; c < C; ++c) dst[c] = (uint8_t)by[0][c];
        }
    }
}

// Test-mode BatchNorm folded into the deconvolution in front of it (model/net.py:110-113 under chainer.config.train = False):
// bn(conv_transpose(y, W) + b) = conv_transpose(y, W') + b' with s_c = gamma_c / sqrt(avg_var_c + eps),
// W'[..., c] = W[..., c] * s_c and b'_c = (b_c - avg_mean_c) * s_c + beta_c.  The BatchNorm channel is the innermost axis of the
// device-layout filter w[rows][Cp] (the deconvolution runs as the input-gradient GEMM of that array); padded channels are copied.
// One launch: items 0 .. rows * Cp / 4 are the filter, the last Cp / 4 items the bias.
__global__ __launch_bounds__(NT) void bn_fold_deconv_kernel(long long n4, int C, int Cp, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mean,
                                                            const float* __restrict__ var, float eps, float* __restrict__ w_out,
                                                            float* __restrict__ b_out) {
    const int Cp4 = Cp >> 2;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4 + Cp4; i += (long long)gridDim.x * NT) {
        const bool is_w = i < n4;
        const int c0 = (int)((is_w ? i : i - n4) % Cp4) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (is_w) v = reinterpret_cast<const f32x4*>(w)[i];
        else if (bias) v = *reinterpret_cast<const f32x4*>(bias + c0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k;
            if (c >= C) continue;
            const float s = __fdiv_rn(gamma[c], __fsqrt_rn(__fadd_rn(var[c], eps)));
            v[k] = is_w ? __fmul_rn(v[k], s) : fmaf(v[k] - mean[c], s, beta[c]);
        }
        if (is_w) reinterpret_cast<f32x4*>(w_out)[i] = v;
        else *reinterpret_cast<f32x4*>(b_out + c0) = v;
    }
}

// cgan (model/updater.py:65-76): the first C channels of every pixel, then dl label planes (+1 on the item's label, -1 elsewhere),
// then zero padding.  dl == 0: a plain channel slice into another row width (the way back: label planes carry no gradient).
__global__ __launch_bounds__(NT) void concat_label_planes_kernel(long long npix, long long P, int C, int Cp, int dl, int Cq,
                                                                 const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                 float* __restrict__ out) {
    const int Cq4 = Cq >> 2;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < npix * Cq4; i += (long long)gridDim.x * NT) {
        const long long p = i / Cq4;
        const int c0 = (int)(i - p * Cq4) * 4;
        const int lab = dl ? labels[p / P] : 0;
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k;
            v[k] = c < C ? x[p * Cp + c] : (c < C + dl ? (c - C == lab ? 1.f : -1.f) : 0.f);
        }
        *reinterpret_cast<f32x4*>(out + i * 4) = v;
    }
}

__global__ __launch_bounds__(NT) void unpack_clip_kernel(int N, int C, int Cp, int T, int HW, const float* __restrict__ in,
                                                         float* __restrict__ x) {
    const long long npix = (long long)N * T * HW;
    for (long long p = (long long)blockIdx.x * NT + threadIdx.x; p < npix; p += (long long)gridDim.x * NT) {
        int hw = (int)(p % HW);
        long long q = p / HW;
        int t = (int)(q % T), n = (int)(q / T);
        for (int c = 0; c < C; ++c) x[(((long long)n * C + c) * T + t) * HW + hw] = in[p * Cp + c];
    }
}

__global__ __launch_bounds__(NT) void tanh_bwd_to_frames_kernel(int N, int T, long long fe4, const float* __restrict__ g_clip,
                                                                const float* __restrict__ x_clip, float* __restrict__ g_frames) {
    const long long n4 = (long long)N * T * fe4;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        long long e = i % fe4, f = i / fe4;      // f = clip-order frame index n*T + t
        int t = (int)(f % T), n = (int)(f / T);
        f32x4 g = *reinterpret_cast<const f32x4*>(g_clip + i * 4);
        f32x4 xv = *reinterpret_cast<const f32x4*>(x_clip + i * 4);
        f32x4 o = g * (1.f - xv * xv);
        *reinterpret_cast<f32x4*>(g_frames + (((long long)t * N + n) * fe4 + e) * 4) = o;
    }
}

// ------------------------------------------------------------------------------------------
// full-window layers
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void fc_fprop_kernel(int K, int Co, const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y) {
    __shared__ float red[NT / 64];
    const int m = blockIdx.x, co = blockIdx.y;
    const float* xr = x + (long long)m * K;
    const float* wr = w + (long long)co * K;
    float s = 0.f;
    for (int k = threadIdx.x * 4; k < K; k += NT * 4) {
        f32x4 a = *reinterpret_cast<const f32x4*>(xr + k), b = *reinterpret_cast<const f32x4*>(wr + k);
        s += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < NT / 64; ++i) t += red[i];
        y[(long long)m * Co + co] = t + (bias ? bias[co] : 0.f);
    }
}

__global__ __launch_bounds__(NT) void fc_dgrad_kernel(int K, int Co, const float* __restrict__ y, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int bias_period, float* __restrict__ x) {
    const int m = blockIdx.y;
    const int k = (blockIdx.x * NT + threadIdx.x) * 4;
    if (k >= K) return;
    f32x4 s = {0, 0, 0, 0};
    for (int co = 0; co < Co; ++co) {
        float yv = y[(long long)m * Co + co];
        s += yv * *reinterpret_cast<const f32x4*>(w + (long long)co * K + k);
    }
    if (bias) s += *reinterpret_cast<const f32x4*>(bias + (k % bias_period));
    *reinterpret_cast<f32x4*>(x + (long long)m * K + k) = s;
}

// the same for R rows per thread: each filter value is loaded once for R outputs (G's dc1: 512 rows x 60 inputs -> 8192)
template <int R>
__global__ __launch_bounds__(NT) void fc_dgrad_rows_kernel(int K, int Co, const float* __restrict__ y, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int bias_period, float* __restrict__ x) {
    const int m0 = blockIdx.y * R;
    const int k = (blockIdx.x * NT + threadIdx.x) * 4;
    if (k >= K) return;
    f32x4 s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = f32x4{0, 0, 0, 0};
    const float* yr = y + (long long)m0 * Co;
#pragma unroll 4
    for (int co = 0; co < Co; ++co) {                           // (unrolled: four filter loads in flight)
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (long long)co * K + k);
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += yr[r * Co + co] * wv;
    }
    f32x4 b = {0, 0, 0, 0};
    if (bias) b = *reinterpret_cast<const f32x4*>(bias + (k % bias_period));
#pragma unroll
    for (int r = 0; r < R; ++r) *reinterpret_cast<f32x4*>(x + (long long)(m0 + r) * K + k) = s[r] + b;
}

// dw[co][k] += sum_m y[m][co] x[m][k] (the discriminators' last layer: Co = 1 + dim_zl rows of K = 8 k .. 32 k inputs, M = the batch).
// Block = FCW_Q k quads x FCW_S row slices: thread (q, sl) sums rows sl, sl + FCW_S, .. of its quad, the slices are combined through
// LDS in slice order (fixed order, no atomics); block x = 0 also reduces the bias gradient.  (Round 4: the first form gave a thread
// one quad and ALL rows -- 32 blocks for K = 32768, 512 dependent steps each, and db as one thread's serial loop: 154 us per call at
// 512 clips where the 67 MB of x take 17.)
constexpr int FCW_Q = 32, FCW_S = NT / FCW_Q;
__global__ __launch_bounds__(NT) void fc_wgrad_kernel(int M, int K, int Co, const float* __restrict__ x, const float* __restrict__ y,
                                                      float* __restrict__ dw, float* db) {
    __shared__ f32x4 red[FCW_S][FCW_Q];
    __shared__ float redb[NT];
    const int co = blockIdx.y;
    const int q = threadIdx.x % FCW_Q, sl = threadIdx.x / FCW_Q;
    const int k = (blockIdx.x * FCW_Q + q) * 4;
    f32x4 s = {0, 0, 0, 0};
    if (k < K) {
#pragma unroll 4
        for (int m = sl; m < M; m += FCW_S) s += y[(long long)m * Co + co] * *reinterpret_cast<const f32x4*>(x + (long long)m * K + k);
    }
    red[sl][q] = s;
    if (db && blockIdx.x == 0) {
        float t = 0.f;
        for (int m = threadIdx.x; m < M; m += NT) t += y[(long long)m * Co + co];
        redb[threadIdx.x] = t;
    }
    __syncthreads();
    if (sl == 0 && k < K) {
#pragma unroll
        for (int j = 1; j < FCW_S; ++j) s += red[j][q];
        f32x4* d = reinterpret_cast<f32x4*>(dw + (long long)co * K + k);
        *d = *d + s;
    }
    if (db && blockIdx.x == 0 && threadIdx.x == 0) {
        float t = 0.f;
        for (int j = 0; j < NT; ++j) t += redb[j];
        db[co] += t;
    }
}

// ------------------------------------------------------------------------------------------
// GRU (Chainer StatelessGRU): thread = (sample, hidden unit); 16 samples x 16 units per block
// ------------------------------------------------------------------------------------------
constexpr int GRU_S = 16, GRU_U = 16, GRU_MAXIN = 32, GRU_MAXP = 6 * (GRU_U * GRU_MAXIN + GRU_U);

struct GruOff { int w[6]; int b[6]; int in[6]; int total; };
__host__ __device__ inline GruOff gru_offsets(int dim_zm, int dim_zl) {
    GruOff o; int p = 0;
    for (int i = 0; i < 6; ++i) {           // W_r U_r W_z U_z W U
        o.in[i] = (i & 1) ? dim_zm : dim_zm + dim_zl;
        o.w[i] = p; p += dim_zm * o.in[i];
        o.b[i] = p; p += dim_zm;
    }
    o.total = p;
    return o;
}

__device__ __forceinline__ float sigmoidf_(float v) { return 0.5f * tanhf(0.5f * v) + 0.5f; }

// Both kernels keep the weight rows / columns a thread needs in REGISTERS (zero beyond the real sizes, as are the LDS
// vectors they multiply: the padded products add +0 and the loops have compile-time bounds) -- with the weights in LDS and
// run-time loop bounds every step was a chain of ~90 dependent LDS reads (3 us per step, measured).
template <int IN_MAX>
__global__ __launch_bounds__(GRU_S * GRU_U) void gru_fwd_kernel(int N, int T, int dz, int dl, int dc, const float* __restrict__ params,
                                                                const float* __restrict__ h0, const float* __restrict__ e,
                                                                const int32_t* __restrict__ labels, const float* __restrict__ zc,
                                                                float* __restrict__ z, float* __restrict__ saved) {
    __shared__ float xs[GRU_S][IN_MAX + 4], hs[GRU_S][GRU_U + 4], rhs[GRU_S][GRU_U + 4];
    const GruOff o = gru_offsets(dz, dl);
    const int s = threadIdx.x / GRU_U, j = threadIdx.x % GRU_U;
    const int n = blockIdx.x * GRU_S + s;
    const bool live = n < N && j < dz;
    const int in = dz + dl, zw = dc + dz;
    // row j of W_r, W_z, W (x side) and of U_r, U_z, U (h side); biases summed as the reference adds them
    float Wr[IN_MAX], Wz[IN_MAX], Wh[IN_MAX], Ur[GRU_U], Uz[GRU_U], Uh[GRU_U];
#pragma unroll
    for (int c = 0; c < IN_MAX; ++c) {
        const bool ok = j < dz && c < in;
        Wr[c] = ok ? params[o.w[0] + j * in + c] : 0.f;
        Wz[c] = ok ? params[o.w[2] + j * in + c] : 0.f;
        Wh[c] = ok ? params[o.w[4] + j * in + c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < GRU_U; ++c) {
        const bool ok = j < dz && c < dz;
        Ur[c] = ok ? params[o.w[1] + j * dz + c] : 0.f;
        Uz[c] = ok ? params[o.w[3] + j * dz + c] : 0.f;
        Uh[c] = ok ? params[o.w[5] + j * dz + c] : 0.f;
    }
    const float b_r = j < dz ? params[o.b[0] + j] + params[o.b[1] + j] : 0.f;
    const float b_z = j < dz ? params[o.b[2] + j] + params[o.b[3] + j] : 0.f;
    const float b_h = j < dz ? params[o.b[4] + j] + params[o.b[5] + j] : 0.f;
    for (int c = j; c < IN_MAX + 4; c += GRU_U) xs[s][c] = 0.f;
    hs[s][j] = 0.f; rhs[s][j] = 0.f;
    if (j < 4) { hs[s][GRU_U + j] = 0.f; rhs[s][GRU_U + j] = 0.f; }
    __syncthreads();
    if (live) hs[s][j] = h0[n * dz + j];
    if (n < N) {
        for (int c = j; c < dl; c += GRU_U) xs[s][c] = (c == labels[n]) ? 1.f : 0.f;
        for (int t = 0; t < T; ++t) for (int c = j; c < dc; c += GRU_U) z[((long long)t * N + n) * zw + c] = zc[n * dc + c];
    }
    // the noise input of step t + 1 is fetched during step t: no memory round trip inside the dependency chain (and the
    // time loop stays rolled: unrolled, its 16 bodies run at instruction-fetch speed)
    float e_next = live ? e[(long long)n * dz + j] : 0.f;
    __syncthreads();
    auto step = [&](int t, float e_t) {
        if (live) xs[s][dl + j] = e_t;
        __syncthreads();
        float ar = b_r, az = b_z, hb = b_h;
#pragma unroll
        for (int c = 0; c < IN_MAX; ++c) {
            const float xv = xs[s][c];
            ar = fmaf(Wr[c], xv, ar);
            az = fmaf(Wz[c], xv, az);
            hb = fmaf(Wh[c], xv, hb);
        }
#pragma unroll
        for (int c = 0; c < GRU_U; ++c) {
            const float hv = hs[s][c];
            ar = fmaf(Ur[c], hv, ar);
            az = fmaf(Uz[c], hv, az);
        }
        const float r = sigmoidf_(ar), zz = sigmoidf_(az), h = hs[s][j];
        if (live) rhs[s][j] = r * h;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < GRU_U; ++c) hb = fmaf(Uh[c], rhs[s][c], hb);
        hb = tanhf(hb);
        const float hn = (1.f - zz) * h + zz * hb;
        if (live) {
            float* sv = saved + ((long long)t * N + n) * 4 * dz;
            sv[j] = r; sv[dz + j] = zz; sv[2 * dz + j] = hb; sv[3 * dz + j] = h;
            z[((long long)t * N + n) * zw + dc + j] = hn;
            hs[s][j] = hn;
        }
        __syncthreads();
    };
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const float e_t = e_next;
        e_next = (live && t + 1 < T) ? e[((long long)(t + 1) * N + n) * dz + j] : 0.f;
        step(t, e_t);
    }
}

template <int IN_MAX>
__global__ __launch_bounds__(GRU_S * GRU_U) void gru_bwd_kernel(int N, int T, int dz, int dl, int dc, const float* __restrict__ params,
                                                                const float* __restrict__ e, const int32_t* __restrict__ labels,
                                                                const float* __restrict__ saved, const float* __restrict__ gz,
                                                                float* __restrict__ dparams) {
    __shared__ float DP[GRU_MAXP];
    __shared__ float xs[GRU_S][IN_MAX + 4], ga_s[GRU_S][GRU_U + 4], gaz_s[GRU_S][GRU_U + 4], gar_s[GRU_S][GRU_U + 4];
    __shared__ float h_s[GRU_S][GRU_U + 4], rh_s[GRU_S][GRU_U + 4];
    const GruOff o = gru_offsets(dz, dl);
    for (int i = threadIdx.x; i < o.total; i += blockDim.x) DP[i] = 0.f;
    const int s = threadIdx.x / GRU_U, j = threadIdx.x % GRU_U;
    const int n = blockIdx.x * GRU_S + s;
    const bool live = n < N && j < dz;
    const int in = dz + dl, zw = dc + dz;
    // column j of U, U_z, U_r (the transposed products of the backward pass)
    float Uhc[GRU_U], Uzc[GRU_U], Urc[GRU_U];
#pragma unroll
    for (int i = 0; i < GRU_U; ++i) {
        const bool ok = j < dz && i < dz;
        Uhc[i] = ok ? params[o.w[5] + i * dz + j] : 0.f;
        Uzc[i] = ok ? params[o.w[3] + i * dz + j] : 0.f;
        Urc[i] = ok ? params[o.w[1] + i * dz + j] : 0.f;
    }
    for (int c = j; c < IN_MAX + 4; c += GRU_U) xs[s][c] = 0.f;
    for (int c = j; c < GRU_U + 4; c += GRU_U) { ga_s[s][c] = 0.f; gaz_s[s][c] = 0.f; gar_s[s][c] = 0.f; h_s[s][c] = 0.f; rh_s[s][c] = 0.f; }
    __syncthreads();
    if (n < N) for (int c = j; c < dl; c += GRU_U) xs[s][c] = (c == labels[n]) ? 1.f : 0.f;
    float gh = 0.f;
    float gW[3][IN_MAX], gU[3][GRU_U], gb[3] = {0.f, 0.f, 0.f};       // d(W, W_z, W_r), d(U, U_z, U_r) rows, biases
#pragma unroll
    for (int c = 0; c < IN_MAX; ++c) { gW[0][c] = 0.f; gW[1][c] = 0.f; gW[2][c] = 0.f; }
#pragma unroll
    for (int c = 0; c < GRU_U; ++c) { gU[0][c] = 0.f; gU[1][c] = 0.f; gU[2][c] = 0.f; }
    struct In { float r, zz, hb, h, e, gz; };
    auto fetch = [&](int t) {
        In v = {0, 0, 0, 0, 0, 0};
        if (live && t >= 0) {
            const float* sv = saved + ((long long)t * N + n) * 4 * dz;
            v.r = sv[j]; v.zz = sv[dz + j]; v.hb = sv[2 * dz + j]; v.h = sv[3 * dz + j];
            v.e = e[((long long)t * N + n) * dz + j];
            v.gz = gz[((long long)t * N + n) * zw + dc + j];
        }
        return v;
    };
    In next = fetch(T - 1);                         // as in gru_fwd_kernel: step t - 1's inputs are fetched during step t
    __syncthreads();
    auto step = [&](int t, const In& v) {
        const float r = v.r, zz = v.zz, hb = v.hb, h = v.h;      // (all zero in the padded threads)
        const float ghn = gh + v.gz;
        const float gzz = ghn * (hb - h), ghb = ghn * zz;
        const float ga = ghb * (1.f - hb * hb);
        const float gaz = gzz * zz * (1.f - zz);
        if (live) {
            xs[s][dl + j] = v.e;
            ga_s[s][j] = ga; gaz_s[s][j] = gaz; h_s[s][j] = h; rh_s[s][j] = r * h;
        }
        __syncthreads();
        float grh = 0.f;
#pragma unroll
        for (int i = 0; i < GRU_U; ++i) grh = fmaf(ga_s[s][i], Uhc[i], grh);
        gh = ghn * (1.f - zz) + grh * r;
        const float gr = grh * h;
        const float gar = gr * r * (1.f - r);
        if (live) gar_s[s][j] = gar;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GRU_U; ++i) {
            gh = fmaf(gaz_s[s][i], Uzc[i], gh);
            gh = fmaf(gar_s[s][i], Urc[i], gh);
        }
        // parameter gradients of row j of each link: accumulated in registers over the 16 steps
#pragma unroll
        for (int c = 0; c < IN_MAX; ++c) {
            const float xv = xs[s][c];
            gW[0][c] = fmaf(ga, xv, gW[0][c]); gW[1][c] = fmaf(gaz, xv, gW[1][c]); gW[2][c] = fmaf(gar, xv, gW[2][c]);
        }
#pragma unroll
        for (int c = 0; c < GRU_U; ++c) {
            gU[0][c] = fmaf(ga, rh_s[s][c], gU[0][c]); gU[1][c] = fmaf(gaz, h_s[s][c], gU[1][c]);
            gU[2][c] = fmaf(gar, h_s[s][c], gU[2][c]);
        }
        gb[0] += ga; gb[1] += gaz; gb[2] += gar;
        __syncthreads();
    };
#pragma unroll 1
    for (int t = T - 1; t >= 0; --t) {
        const In cur = next;
        next = fetch(t - 1);
        step(t, cur);
    }
    if (live) {                                    // one LDS reduction over the block's samples
#pragma unroll
        for (int c = 0; c < IN_MAX; ++c)
            if (c < in) {
                atomicAdd(&DP[o.w[4] + j * in + c], gW[0][c]);
                atomicAdd(&DP[o.w[2] + j * in + c], gW[1][c]);
                atomicAdd(&DP[o.w[0] + j * in + c], gW[2][c]);
            }
#pragma unroll
        for (int c = 0; c < GRU_U; ++c)
            if (c < dz) {
                atomicAdd(&DP[o.w[5] + j * dz + c], gU[0][c]);
                atomicAdd(&DP[o.w[3] + j * dz + c], gU[1][c]);
                atomicAdd(&DP[o.w[1] + j * dz + c], gU[2][c]);
            }
        atomicAdd(&DP[o.b[4] + j], gb[0]); atomicAdd(&DP[o.b[5] + j], gb[0]);
        atomicAdd(&DP[o.b[2] + j], gb[1]); atomicAdd(&DP[o.b[3] + j], gb[1]);
        atomicAdd(&DP[o.b[0] + j], gb[2]); atomicAdd(&DP[o.b[1] + j], gb[2]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < o.total; i += blockDim.x) atomicAdd(dparams + i, DP[i]);
}

// ------------------------------------------------------------------------------------------
// GRU, wide states (16 < dim_zm <= 64, dim_zm + dim_zl <= 128; the reference accepts any --dim_zm, train.py:39): the same
// recurrence with the weights read from memory (L1 / L2: a few hundred KB at most) and run-time loop bounds -- a step is a chain of
// dependent loads, ~10 x the time of the register-resident kernels above, which keep the default sizes.  Thread = (sample, unit):
// GRUW_S samples x 64 units per block.  Backward: every thread adds its row's parameter gradients into the block's copy of the
// gradient in LDS (dynamic: gru_offsets().total floats) step by step; one pass of global atomics at the end, as above.
// ------------------------------------------------------------------------------------------
constexpr int GRUW_S = 4, GRUW_U = 64, GRUW_IN = 128;

__global__ __launch_bounds__(GRUW_S * GRUW_U) void gru_fwd_wide_kernel(int N, int T, int dz, int dl, int dc, const float* __restrict__ params,
                                                                     const float* __restrict__ h0, const float* __restrict__ e,
                                                                     const int32_t* __restrict__ labels, const float* __restrict__ zc,
                                                                     float* __restrict__ z, float* __restrict__ saved) {
    __shared__ float xs[GRUW_S][GRUW_IN], hs[GRUW_S][GRUW_U], rhs[GRUW_S][GRUW_U];
    const GruOff o = gru_offsets(dz, dl);
    const int s = threadIdx.x / GRUW_U, j = threadIdx.x % GRUW_U;
    const int n = blockIdx.x * GRUW_S + s;
    const bool live = n < N && j < dz;
    const int in = dz + dl, zw = dc + dz;
    const float* Wr = params + o.w[0] + j * in; const float* Ur = params + o.w[1] + j * dz;
    const float* Wz = params + o.w[2] + j * in; const float* Uz = params + o.w[3] + j * dz;
    const float* Wh = params + o.w[4] + j * in; const float* Uh = params + o.w[5] + j * dz;
    const float b_r = j < dz ? params[o.b[0] + j] + params[o.b[1] + j] : 0.f;
    const float b_z = j < dz ? params[o.b[2] + j] + params[o.b[3] + j] : 0.f;
    const float b_h = j < dz ? params[o.b[4] + j] + params[o.b[5] + j] : 0.f;
    for (int c = j; c < GRUW_IN; c += GRUW_U) xs[s][c] = 0.f;
    hs[s][j] = 0.f; rhs[s][j] = 0.f;
    __syncthreads();
    if (live) hs[s][j] = h0[n * dz + j];
    if (n < N) {
        for (int c = j; c < dl; c += GRUW_U) xs[s][c] = (c == labels[n]) ? 1.f : 0.f;
        for (int t = 0; t < T; ++t) for (int c = j; c < dc; c += GRUW_U) z[((long long)t * N + n) * zw + c] = zc[n * dc + c];
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        if (live) xs[s][dl + j] = e[((long long)t * N + n) * dz + j];
        __syncthreads();
        float ar = b_r, az = b_z, hb = b_h;
        if (live) {
            for (int c = 0; c < in; ++c) { const float xv = xs[s][c]; ar = fmaf(Wr[c], xv, ar); az = fmaf(Wz[c], xv, az); hb = fmaf(Wh[c], xv, hb); }
            for (int c = 0; c < dz; ++c) { const float hv = hs[s][c]; ar = fmaf(Ur[c], hv, ar); az = fmaf(Uz[c], hv, az); }
        }
        const float r = sigmoidf_(ar), zz = sigmoidf_(az), h = hs[s][j];
        if (live) rhs[s][j] = r * h;
        __syncthreads();
        if (live) {
            for (int c = 0; c < dz; ++c) hb = fmaf(Uh[c], rhs[s][c], hb);
            hb = tanhf(hb);
            const float hn = (1.f - zz) * h + zz * hb;
            float* sv = saved + ((long long)t * N + n) * 4 * dz;
            sv[j] = r; sv[dz + j] = zz; sv[2 * dz + j] = hb; sv[3 * dz + j] = h;
            z[((long long)t * N + n) * zw + dc + j] = hn;
            hs[s][j] = hn;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GRUW_S * GRUW_U) void gru_bwd_wide_kernel(int N, int T, int dz, int dl, int dc, const float* __restrict__ params,
                                                                     const float* __restrict__ e, const int32_t* __restrict__ labels,
                                                                     const float* __restrict__ saved, const float* __restrict__ gz,
                                                                     float* __restrict__ dparams) {
    extern __shared__ float DPw[];                                   // gru_offsets().total floats: the block's share of the gradient
    __shared__ float xs[GRUW_S][GRUW_IN], ga_s[GRUW_S][GRUW_U], gaz_s[GRUW_S][GRUW_U], gar_s[GRUW_S][GRUW_U];
    __shared__ float h_s[GRUW_S][GRUW_U], rh_s[GRUW_S][GRUW_U];
    const GruOff o = gru_offsets(dz, dl);
    for (int i = threadIdx.x; i < o.total; i += blockDim.x) DPw[i] = 0.f;
    const int s = threadIdx.x / GRUW_U, j = threadIdx.x % GRUW_U;
    const int n = blockIdx.x * GRUW_S + s;
    const bool live = n < N && j < dz;
    const int in = dz + dl, zw = dc + dz;
    const float* Uh = params + o.w[5]; const float* Uz = params + o.w[3]; const float* Ur = params + o.w[1];       // column j: [i * dz + j]
    for (int c = j; c < GRUW_IN; c += GRUW_U) xs[s][c] = 0.f;
    ga_s[s][j] = 0.f; gaz_s[s][j] = 0.f; gar_s[s][j] = 0.f; h_s[s][j] = 0.f; rh_s[s][j] = 0.f;
    __syncthreads();
    if (n < N) for (int c = j; c < dl; c += GRUW_U) xs[s][c] = (c == labels[n]) ? 1.f : 0.f;
    float gh = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        float r = 0.f, zz = 0.f, hb = 0.f, h = 0.f, gzv = 0.f;
        if (live) {
            const float* sv = saved + ((long long)t * N + n) * 4 * dz;
            r = sv[j]; zz = sv[dz + j]; hb = sv[2 * dz + j]; h = sv[3 * dz + j];
            gzv = gz[((long long)t * N + n) * zw + dc + j];
        }
        const float ghn = gh + gzv;
        const float gzz = ghn * (hb - h), ghb = ghn * zz;
        const float ga = ghb * (1.f - hb * hb);
        const float gaz = gzz * zz * (1.f - zz);
        if (live) {
            xs[s][dl + j] = e[((long long)t * N + n) * dz + j];
            ga_s[s][j] = ga; gaz_s[s][j] = gaz; h_s[s][j] = h; rh_s[s][j] = r * h;
        }
        __syncthreads();
        float grh = 0.f;
        if (live) for (int i = 0; i < dz; ++i) grh = fmaf(ga_s[s][i], Uh[i * dz + j], grh);
        gh = ghn * (1.f - zz) + grh * r;
        const float gar = grh * h * r * (1.f - r);
        if (live) gar_s[s][j] = gar;
        __syncthreads();
        if (live) {
            for (int i = 0; i < dz; ++i) { gh = fmaf(gaz_s[s][i], Uz[i * dz + j], gh); gh = fmaf(gar_s[s][i], Ur[i * dz + j], gh); }
            for (int c = 0; c < in; ++c) {
                const float xv = xs[s][c];
                atomicAdd(&DPw[o.w[4] + j * in + c], ga * xv); atomicAdd(&DPw[o.w[2] + j * in + c], gaz * xv); atomicAdd(&DPw[o.w[0] + j * in + c], gar * xv);
            }
            for (int c = 0; c < dz; ++c) {
                atomicAdd(&DPw[o.w[5] + j * dz + c], ga * rh_s[s][c]); atomicAdd(&DPw[o.w[3] + j * dz + c], gaz * h_s[s][c]);
                atomicAdd(&DPw[o.w[1] + j * dz + c], gar * h_s[s][c]);
            }
            atomicAdd(&DPw[o.b[4] + j], ga); atomicAdd(&DPw[o.b[5] + j], ga);
            atomicAdd(&DPw[o.b[2] + j], gaz); atomicAdd(&DPw[o.b[3] + j], gaz);
            atomicAdd(&DPw[o.b[0] + j], gar); atomicAdd(&DPw[o.b[1] + j], gar);
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < o.total; i += blockDim.x) atomicAdd(dparams + i, DPw[i]);
}

// ------------------------------------------------------------------------------------------
// losses: one block
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplusf_(float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }

__device__ float block_sum(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}

// softmax cross entropy over classes 1..C-1 of row n; returns loss term, writes grad/N (added)
__device__ float ce_row(const float* yrow, int C, int label, float invn, float* grow) {
    float mx = -INFINITY;
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, yrow[c]);
    float se = 0.f;
    for (int c = 1; c < C; ++c) se += expf(yrow[c] - mx);
    float lse = mx + logf(se);
    for (int c = 1; c < C; ++c) grow[c] += (expf(yrow[c] - lse) - (c - 1 == label ? 1.f : 0.f)) * invn;
    return (lse - yrow[1 + label]) * invn;
}

__global__ __launch_bounds__(NT) void loss_dis_kernel(int N, int C, const float* __restrict__ yr, const float* __restrict__ yf,
                                                      const int32_t* tr, const int32_t* tf, int with_ce, float* loss,
                                                      float* __restrict__ gr, float* __restrict__ gf) {
    __shared__ float red[NT / 64];
    const float invn = 1.f / (float)N;
    float l = 0.f;
    for (int i = threadIdx.x; i < N * C; i += NT) {
        bool first = i < C;                       // sample 0 only (model/updater.py:25-26)
        gr[i] = first ? -sigmoidf_(-yr[i]) * invn : 0.f;
        gf[i] = first ? sigmoidf_(yf[i]) * invn : 0.f;
        if (first) l += (softplusf_(-yr[i]) + softplusf_(yf[i])) * invn;
    }
    __syncthreads();
    if (with_ce) {
        for (int n = threadIdx.x; n < N; n += NT) {
            l += ce_row(yr + n * C, C, tr[n], invn, gr + n * C);
            l += ce_row(yf + n * C, C, tf[n], invn, gf + n * C);
        }
    }
    float t = block_sum(l, red);
    if (threadIdx.x == 0) loss[0] = t;
}

__global__ __launch_bounds__(NT) void loss_gen_kernel(int N, int C, const float* __restrict__ yi, const float* __restrict__ yv,
                                                      const int32_t* tf, int with_ce, float* loss,
                                                      float* __restrict__ gi, float* __restrict__ gv) {
    __shared__ float red[NT / 64];
    const float invn = 1.f / (float)N;
    float l = 0.f;
    for (int i = threadIdx.x; i < N * C; i += NT) {
        bool ch0 = (i % C) == 0;                  // channel 0, full batch (model/updater.py:50-51)
        gi[i] = ch0 ? -sigmoidf_(-yi[i]) * invn : 0.f;
        gv[i] = ch0 ? -sigmoidf_(-yv[i]) * invn : 0.f;
        if (ch0) l += (softplusf_(-yi[i]) + softplusf_(-yv[i])) * invn;
    }
    __syncthreads();
    if (with_ce) {
        for (int n = threadIdx.x; n < N; n += NT) {
            l += ce_row(yi + n * C, C, tf[n], invn, gi + n * C);
            l += ce_row(yv + n * C, C, tf[n], invn, gv + n * C);
        }
    }
    float t = block_sum(l, red);
    if (threadIdx.x == 0) loss[0] = t;
}

// ------------------------------------------------------------------------------------------
// Adam + weight decay, randn
// ------------------------------------------------------------------------------------------
struct AdamK { float lr, b1c, b2c, eps, wd, gscale; };

// One parameter's update: the ONE statement of the arithmetic, with every fused multiply-add written out.  Left to the compiler's
// contraction, g * gscale + wd * p became fma(wd, p, g * gscale) in the scalar form of the kernel below and fma(gscale, g, wd * p)
// in its 16-byte form: one element in some ten thousand then differs in the last bit.  What is spelled here is what the scalar
// kernel has always computed, so the forms (scalar / 16-byte accesses, with / without the average) agree bit for bit.
__device__ __forceinline__ float adam_wd_elem(float pv, float g, float& mv, float& vv, const AdamK& k) {
    const float gg = fmaf(k.wd, pv, g * k.gscale);   // gscale = 1 / world: the all-reduced SUM becomes the mean here (x 1.0f is exact)
    mv = fmaf(k.b1c, gg - mv, mv);
    vv = fmaf(k.b2c, fmaf(gg, gg, -vv), vv);
    return pv - k.lr * mv / (sqrtf(vv) + k.eps);
}

// e <- e + r (x - e): one subtraction, one fma (the form of m and v above: x == e is a fixed point).  r == 1 takes x itself --
// e + (x - e) is not x in floating point -- so a decay of 0 tracks the parameters exactly.
__device__ __forceinline__ float ema_elem(float e, float x, float r, bool take_x) { return take_x ? x : fmaf(r, x - e, e); }

// EMA: the exponential moving average `ema` of the parameters follows in the same pass (the fresh parameter is in a register).
// V = 4: 16-byte accesses, for pointers that are all 16-byte aligned (p16: 8-byte); the n % 4 last elements are done one by one
// by the first threads of block 0.  V = 1: any 4-byte aligned pointers.
// CTL (mcg_adam_wd_ctl): the gradient scale is ctl[0] of device memory, read once per thread -- what mcg_grad_stats' finalize launch
// left there (grad_scale x clipping rate) -- and a non-zero ctl[1] (a non-finite gradient) ends the launch before anything is written.
template <bool EMA, int V, bool CTL = false>
__global__ __launch_bounds__(NT) void adam_wd_kernel(long long n, float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v, AdamK k, __bf16* __restrict__ p16,
                                                     float* __restrict__ ema, float r, const float* __restrict__ ctl = nullptr) {
    if constexpr (CTL) {
        if (ctl[1] != 0.0f) return;               // (uniform over the whole grid: p, m, v, p16 and ema keep their bits)
        k.gscale = ctl[0];
    }
    const bool take_x = r == 1.0f;
    const long long stride = (long long)gridDim.x * NT, first = (long long)blockIdx.x * NT + threadIdx.x;
    auto one = [&](long long i) {
        float mv = m[i], vv = v[i];
        const float pv = adam_wd_elem(p[i], g[i], mv, vv, k);
        m[i] = mv; v[i] = vv;
        p[i] = pv;
        if (p16) p16[i] = (__bf16)pv;             // the GEMMs' bf16 copy of the master weights (MCG_PREC_BF16_STORE)
        if (EMA) ema[i] = ema_elem(ema[i], pv, r, take_x);
    };
    if constexpr (V == 1) {
        for (long long i = first; i < n; i += stride) one(i);
        return;
    }
    const long long n4 = n >> 2;
    for (long long i = first; i < n4; i += stride) {
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i], mv = reinterpret_cast<const f32x4*>(m)[i], vv = reinterpret_cast<const f32x4*>(v)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 ev;
        if (EMA) ev = reinterpret_cast<const f32x4*>(ema)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mj = mv[j], vj = vv[j];
            pv[j] = adam_wd_elem(pv[j], gv[j], mj, vj, k);
            mv[j] = mj; vv[j] = vj;
            if (EMA) ev[j] = ema_elem(ev[j], pv[j], r, take_x);
        }
        reinterpret_cast<f32x4*>(m)[i] = mv; reinterpret_cast<f32x4*>(v)[i] = vv;
        reinterpret_cast<f32x4*>(p)[i] = pv;
        if (p16) reinterpret_cast<bf16x4_t*>(p16)[i] = __builtin_convertvector(pv, bf16x4_t);
        if (EMA) reinterpret_cast<f32x4*>(ema)[i] = ev;
    }
    const long long tail = (n4 << 2) + first;      // (first < 3 in block 0 only)
    if (tail < n) one(tail);
}

// mcg_ema_multi: dst <- dst + r (src - dst) over up to 32 segments of any length in one launch (the generator's eight running
// statistics).  A block belongs to one segment, found as split_planes_multi_kernel below finds it; 4-byte accesses.
constexpr int MAX_EMA_SEGS = 32, EMA_SEG_BLOCKS = 64;
struct EmaSegs { const float* src[MAX_EMA_SEGS]; float* dst[MAX_EMA_SEGS]; long long n[MAX_EMA_SEGS]; int blk_end[MAX_EMA_SEGS]; int nseg; };
__global__ __launch_bounds__(NT) void ema_multi_kernel(EmaSegs sg, float r) {
    int s = 0;
    while (s + 1 < sg.nseg && (int)blockIdx.x >= sg.blk_end[s]) ++s;                    // (block-uniform)
    const int b0 = s ? sg.blk_end[s - 1] : 0, nb = sg.blk_end[s] - b0;
    const float* src = sg.src[s];
    float* dst = sg.dst[s];
    const long long n = sg.n[s];
    const bool take_x = r == 1.0f;
    for (long long i = (long long)((int)blockIdx.x - b0) * NT + threadIdx.x; i < n; i += (long long)nb * NT)
        dst[i] = ema_elem(dst[i], src[i], r, take_x);
}

// ------------------------------------------------------------------------------------------
// mcg_grad_stats: sum of squares, largest |g| and non-finite count of up to 32 segments of a flat gradient, and from the total the
// control block the Adam launch reads (mcg_adam_wd_ctl).  Two launches, no atomics, no hand-off between workgroups inside a launch:
// every sum has ONE order, so two calls on the same input agree bit for bit.
//   partial: a block belongs to one segment (found in the prefix sums of the block counts, as split_planes_multi_kernel finds it) and walks it in trips of STAT_SPAN
//            elements, its trips strided by the segment's block count.  A thread issues its STAT_LOADS 16-byte loads of a trip before it
//            uses the first (the note at col_partial_kernel: with at most MAX_PART blocks on the chip one dependent load per
//            iteration leaves HBM idle).  Squares are formed and added in double (the product of two fp32 values is exact there):
//            per thread, then over the block through LDS in a fixed tree -> workspace[block][4].
//   final:   one block; thread s adds segment s's partials in block order, thread 0 the segments in segment order -> stats, ctl.
// A segment start that is not 16-byte aligned gets a scalar head (up to 3 elements), n % 4 leftovers a scalar tail: both in the
// segment's first block.  Non-finite elements are counted and kept OUT of the sum and the maximum, so the norm stays that of the
// finite part and says how large the rest of the gradient was.
// ------------------------------------------------------------------------------------------
constexpr int MAX_STAT_SEGS = 32, STAT_LOADS = 4, STAT_SPAN = NT * 4 * STAT_LOADS;
struct StatSegs { long long off[MAX_STAT_SEGS]; long long n[MAX_STAT_SEGS]; int blk_end[MAX_STAT_SEGS]; int nseg; };

struct StatAcc {
    double ss; float mx; unsigned int bad;
    __device__ __forceinline__ void add(float x) {
        const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
        const double d = fin ? (double)x : 0.0;
        ss += d * d;
        mx = fmaxf(mx, fin ? fabsf(x) : 0.0f);
        bad += fin ? 0u : 1u;
    }
};

__global__ __launch_bounds__(NT) void grad_stats_partial_kernel(StatSegs sg, const float* __restrict__ g, double* __restrict__ part) {
    int s = 0, hi = sg.nseg - 1;
    while (s < hi) {                                                                    // (block-uniform; by halves: the small tensors come last)
        const int mid = (s + hi) >> 1;
        if ((int)blockIdx.x >= sg.blk_end[mid]) s = mid + 1; else hi = mid;
    }
    const int b0 = s ? sg.blk_end[s - 1] : 0, nb = sg.blk_end[s] - b0, b = (int)blockIdx.x - b0;
    const float* __restrict__ x = g + sg.off[s];
    const long long n = sg.n[s];
    const int tid = threadIdx.x;
    long long head = (long long)((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2;    // elements in front of the first 16-byte boundary
    if (head > n) head = n;
    const long long nq = (n - head) >> 2, tail0 = head + (nq << 2);
    StatAcc a = {0.0, 0.0f, 0u};
    if (b == 0) {
        if (tid < head) a.add(x[tid]);
        if (tid >= 4 && tail0 + (tid - 4) < n) a.add(x[tail0 + (tid - 4)]);             // (threads 4..6)
    }
    const f32x4* __restrict__ xq = reinterpret_cast<const f32x4*>(x + head);
    constexpr long long TRIP = STAT_SPAN / 4;                                           // 16-byte pieces of a trip
    for (long long q0 = (long long)b * TRIP; q0 < nq; q0 += (long long)nb * TRIP) {
        f32x4 v[STAT_LOADS];
#pragma unroll
        for (int j = 0; j < STAT_LOADS; ++j) {
            const long long q = q0 + j * NT + tid;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            v[j] = q < nq ? xq[q] : zero;
        }
#pragma unroll
        for (int j = 0; j < STAT_LOADS; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) a.add(v[j][e]);
    }
    __shared__ double sh_ss[NT];
    __shared__ float sh_mx[NT];
    __shared__ unsigned int sh_bad[NT];
    sh_ss[tid] = a.ss; sh_mx[tid] = a.mx; sh_bad[tid] = a.bad;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {                                              // the fixed tree: t <- t + (t + w)
        if (tid < w) {
            sh_ss[tid] += sh_ss[tid + w];
            sh_mx[tid] = fmaxf(sh_mx[tid], sh_mx[tid + w]);
            sh_bad[tid] += sh_bad[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = part + 4LL * blockIdx.x;
        o[0] = sh_ss[0]; o[1] = (double)sh_mx[0]; o[2] = (double)sh_bad[0]; o[3] = 0.0;
    }
}

__global__ __launch_bounds__(NT) void grad_stats_final_kernel(StatSegs sg, const double* __restrict__ part, double gscale, double threshold,
                                                              double* __restrict__ stats, float* __restrict__ ctl) {
    __shared__ double sh[3][MAX_PART];
    __shared__ double row[MAX_STAT_SEGS][3];
    const int tid = threadIdx.x, nblk = sg.blk_end[sg.nseg - 1];
    for (int i = tid; i < nblk; i += NT) {
        const double* q = part + 4LL * i;
        sh[0][i] = q[0]; sh[1][i] = q[1]; sh[2][i] = q[2];
    }
    __syncthreads();
    // the sums in block order by threads 0.. of the first wave, maxima and counts (any order gives the same) by the second wave beside
    // them; eight LDS reads are in flight before the first is added (one read per dependent add: 20 us for G's 330 partials)
    const int seg = tid & 63, role = tid >> 6;
    if (seg < sg.nseg && role < 2) {
        const int b0 = seg ? sg.blk_end[seg - 1] : 0, b1 = sg.blk_end[seg];
        double* o = stats + 4LL * seg;
        int b = b0;
        if (role == 0) {
            double ss = 0.0;
            for (; b + 8 <= b1; b += 8) {
                double t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = sh[0][b + j];
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += t[j];
            }
            for (; b < b1; ++b) ss += sh[0][b];
            row[seg][0] = ss;
            o[0] = ss; o[3] = 0.0;
        } else {
            double mx = 0.0, bad = 0.0;
            for (; b + 4 <= b1; b += 4) {
                double t[4], c[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { t[j] = sh[1][b + j]; c[j] = sh[2][b + j]; }
#pragma unroll
                for (int j = 0; j < 4; ++j) { mx = fmax(mx, t[j]); bad += c[j]; }
            }
            for (; b < b1; ++b) { mx = fmax(mx, sh[1][b]); bad += sh[2][b]; }
            row[seg][1] = mx; row[seg][2] = bad;
            o[1] = mx; o[2] = bad;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double ss = 0.0, mx = 0.0, cnt = 0.0;
        for (int s = 0; s < sg.nseg; ++s) { ss += row[s][0]; mx = fmax(mx, row[s][1]); cnt += row[s][2]; }       // segment order
        double* o = stats + 4LL * sg.nseg;
        o[0] = ss; o[1] = mx; o[2] = cnt; o[3] = 0.0;
        const bool bad = cnt > 0.0;
        const double norm = gscale * sqrt(ss);
        const double rate = norm == 0.0 ? 1.0 : fmin(1.0, threshold / norm);
        const float fnorm = (float)norm;
        ctl[0] = bad ? (float)gscale : (float)(gscale * rate);
        ctl[1] = bad ? 1.0f : 0.0f;
        ctl[2] = (float)rate;
        ctl[3] = fnorm;
        const bool fin = (__float_as_uint(fnorm) & 0x7f800000u) != 0x7f800000u;
        if (!bad && fin) ctl[4] = fmaxf(ctl[4], fnorm);                                  // peak over the finite norms of clean calls
        if (bad) ctl[5] += 1.0f;                                                        // skipped updates (exact to 2^24)
    }
}

__global__ __launch_bounds__(NT) void randn_kernel(long long n, float sigma, uint64_t seed, uint64_t stream_id, float* __restrict__ out) {
    const long long n4 = (n + 3) / 4;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        f32x4 z = randn4((uint64_t)i, seed, stream_id);
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i * 4 + k < n) out[i * 4 + k] = sigma * z[k];
    }
}

// element (m, c) = normal (m & 3) of Philox counter (m >> 2) * C + c: the order in which the fused first-layer epilogue of
// conv_gemm.hip draws its noise (a lane of the MFMA accumulator holds four consecutive rows of one channel)
__global__ __launch_bounds__(NT) void randn_rowquad_kernel(long long quads, int C, float sigma, uint64_t seed, uint64_t stream_id, float* __restrict__ out) {
    const long long n = quads * C;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const long long mq = i / C; const int c = (int)(i - mq * C);
        f32x4 z = randn4((uint64_t)i, seed, stream_id);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[(mq * 4 + k) * C + c] = sigma * z[k];
    }
}

// element i = word (i & 3) of Philox counter (i >> 2), modulo `modulus` (labels of the generator's draw)
__global__ __launch_bounds__(NT) void randint_kernel(long long n, uint32_t modulus, uint64_t seed, uint64_t stream_id, int32_t* __restrict__ out) {
    const long long n4 = (n + 3) / 4;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        uint32_t r[4];
        mcg::philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i * 4 + k < n) out[i * 4 + k] = (int32_t)(r[k] % modulus);
    }
}

bool bad_c(int C) { return C <= 0 || (C & 3); }

// many conv-epilogue slots -> at most MAX_PART folded partials in `ws` (col_partial_kernel's own layout); returns the
// partial list the finalize kernel should read
struct Folded { const float* part; int n; long long stride; };
Folded fold_slots(const float* part, int n_slots, int slot_stride, int C, float* ws, hipStream_t s) {
    if (n_slots <= FOLD_ABOVE || !ws || (NT % (C < 64 ? C : 64)) != 0) return {part, n_slots, (long long)slot_stride};
    int per = 32;
    if ((n_slots + per - 1) / per > MAX_PART) per = (n_slots + MAX_PART - 1) / MAX_PART;
    const int chunks = (n_slots + per - 1) / per;
    const int cw = C < 64 ? C : 64;
    hipLaunchKernelGGL(fold_partials_kernel, dim3((C + cw - 1) / cw, chunks), dim3(NT), 0, s, n_slots, (long long)slot_stride, C, per, part, ws);
    return {ws, chunks, 2LL * C};
}
// the column-reduction kernels give each thread one channel quad and stride the rows by NT / (C/4):
// C must be 4 * 2^k, k <= 8 (every width the reference can produce from a power-of-two n_filters)
bool unsupported_c(int C) { return (C >> 2) > NT || (NT % (C >> 2)) != 0; }


__global__ __launch_bounds__(NT) void split_planes_kernel(long long n8, long long run, const float* __restrict__ src, __bf16* __restrict__ dst) {
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < n8; i += (long long)gridDim.x * NT)
        store_split8(dst, i * 8, run, loadv<8>(src, i * 8, 0));
}

// mcg_split_planes_multi: up to 32 (source, run, destination) segments in one launch.  A BLOCK belongs to one segment (found in the
// prefix sums of the segments' block counts: a uniform scan, scalar loads of the kernel arguments -- a per-thread segment index would
// put the argument arrays into scratch); its threads write the three planes exactly as split_planes_kernel does.
constexpr int MAX_SPLIT_SEGS = 32;
struct SplitSegs { const float* src[MAX_SPLIT_SEGS]; __bf16* dst[MAX_SPLIT_SEGS]; long long run[MAX_SPLIT_SEGS]; long long n8[MAX_SPLIT_SEGS];
                   int blk_end[MAX_SPLIT_SEGS]; int nseg; };
__global__ __launch_bounds__(NT) void split_planes_multi_kernel(SplitSegs sg) {
    int s = 0;
    while (s + 1 < sg.nseg && (int)blockIdx.x >= sg.blk_end[s]) ++s;                    // (block-uniform)
    const int b0 = s ? sg.blk_end[s - 1] : 0, nb = sg.blk_end[s] - b0;
    const float* __restrict__ src = sg.src[s];
    __bf16* __restrict__ dst = sg.dst[s];
    const long long run = sg.run[s], n8 = sg.n8[s];
    for (long long i = (long long)((int)blockIdx.x - b0) * NT + threadIdx.x; i < n8; i += (long long)nb * NT)
        store_split8(dst, i * 8, run, loadv<8>(src, i * 8, 0));
}

// ---- launches of the BatchNorm / activation kernels for a run-time set of MCG_IO_* flags (compile-time in the kernels) ----
template <int W> using width = std::integral_constant<int, W>;

// f(std::integral_constant<int, IO>) for the IO of the list that equals io; the last of the list takes every other value
template <int IO0, int... IOs, class F>
void with_io(int io, F f) {
    if constexpr (sizeof...(IOs) == 0) f(std::integral_constant<int, IO0>{});
    else if (io == IO0) f(std::integral_constant<int, IO0>{});
    else with_io<IOs...>(io, f);
}

// eight channels per thread: a bf16 (or split) tensor in the call, C % 8 == 0 and a channel-group count the block size divides
bool wide_c(int io, int C) { return (io & 15) != 0 && (C & 7) == 0 && (C >> 3) <= NT && NT % (C >> 3) == 0; }
bool split_out_ok(int io, int C, const float* stats) {      // MCG_IO_OUT_SPLIT: fp32 inputs, BatchNorm behind it, C % 16 == 0
    return io == MCG_IO_OUT_SPLIT && stats && wide_c(io, C) && (C & 15) == 0;
}
// gx_bf16 of the backward entry points: MCG_IO_* flags (OUT = gx, Y = y, G = g_out).  In place only between tensors of one
// element type; the split output never in place
int check_bwd_io(const void* gx, const void* g_out, int io, int C, const float* stats) {
    if (gx == g_out && !(io & MCG_IO_OUT_BF16) != !(io & MCG_IO_G_BF16)) return MCG_ERR_BAD_ARG;
    if ((io & MCG_IO_OUT_SPLIT) && (gx == g_out || !split_out_ok(io, C, stats))) return MCG_ERR_UNSUPPORTED;
    return MCG_OK;
}
double bessel_adjust(long long M) { return (double)M / (M - 1.0 > 1.0 ? M - 1.0 : 1.0); }     // running variance: m / max(m - 1, 1)

void launch_bwd_partial(int io, int blocks, hipStream_t s, long long M, int C, long long rows_per_block, const float* g_out,
                        const float* y, const float* stats, int act, float* part) {
    const int in = io & (MCG_IO_Y_BF16 | MCG_IO_G_BF16);
    auto launch = [&](auto w, auto ioc) {
        hipLaunchKernelGGL((col_partial_kernel<1, decltype(w)::value, decltype(ioc)::value>), dim3(blocks), dim3(NT), 0, s, M, C, rows_per_block,
                           g_out, y, stats, act, part);
    };
    if (stats && in && wide_c(io, C)) with_io<2, 4, 6>(in, [&](auto ioc) { launch(width<8>{}, ioc); });
    else with_io<0, 2, 4, 6>(in, [&](auto ioc) { launch(width<4>{}, ioc); });
}
void launch_bwd_apply(int io, hipStream_t s, long long M, int C, const float* g_out, const float* y, const float* stats,
                      const float* coef, int act, float* gx) {
    auto launch = [&](auto w, auto ioc) {
        constexpr int W = decltype(w)::value;
        const long long n = M * (C >> LOG2<W>);
        hipLaunchKernelGGL((bn_act_bwd_apply_kernel<W, decltype(ioc)::value>), dim3(ew_grid(n)), dim3(NT), 0, s, n, C, g_out, y, stats, coef, act, gx);
    };
    if (io & MCG_IO_OUT_SPLIT) launch(width<8>{}, std::integral_constant<int, MCG_IO_OUT_SPLIT>{});
    else if (stats && wide_c(io, C)) with_io<1, 2, 3, 4, 5, 6, 7>(io & 7, [&](auto ioc) { launch(width<8>{}, ioc); });
    else with_io<0, 1, 2, 3, 4, 5, 6, 7>(io & 7, [&](auto ioc) { launch(width<4>{}, ioc); });
}


// ------------------------------------------------------------------------------------------
// Differentiable augmentation of the discriminators' inputs (Zhao et al. 2020, policy color,translation,cutout; no reference
// counterpart).  A clip is [T][H][W][4] with C <= 3 valid channels; one parameter set per clip: geo[8] = dx, dy, x0, x1, y0, y1, -, -
// and col[4] = b, s, c, -.  The map is affine in x; mcg_augment_bwd is the adjoint of its linear part (include/mocogan_hip.h states
// both).  Each direction is two launches: per-clip partial sums (doubles, one per block, AUG_MAX_BLOCKS slots per clip), then an
// apply pass that folds the clip's slots in slot order -- no float atomics, results are bit-reproducible.
// ------------------------------------------------------------------------------------------
constexpr int AUG_MAX_BLOCKS = 64;           // partial-sum blocks (workspace slots) per clip
constexpr int AUG_MIN_PIX = NT * 4;          // ... each of at least this many pixels

struct AugPlan { int blocks; int pix_per_block; };
AugPlan plan_augment(long long P) {
    long long b = (P + AUG_MIN_PIX - 1) / AUG_MIN_PIX;
    if (b > AUG_MAX_BLOCKS) b = AUG_MAX_BLOCKS;
    AugPlan p;
    p.pix_per_block = (int)((P + b - 1) / b);
    p.blocks = (int)((P + p.pix_per_block - 1) / p.pix_per_block);
    return p;
}

struct AugGeo { int dx, dy, x0, x1, y0, y1; };
__device__ __forceinline__ AugGeo aug_geo(const int32_t* __restrict__ geo, int n) {
    const int32_t* q = geo + 8 * (long long)n;
    AugGeo a = {q[0], q[1], q[2], q[3], q[4], q[5]};
    return a;
}
// the output position (y, x) is written from the clip: inside the frame and outside the cutout rectangle
__device__ __forceinline__ bool aug_kept(const AugGeo& a, int y, int x, int H, int W) {
    return y >= 0 && y < H && x >= 0 && x < W && !(x >= a.x0 && x < a.x1 && y >= a.y0 && y < a.y1);
}
// The gradient that reaches SOURCE pixel p = (t, sy, sx) of a clip: g at (t, sy + dy, sx + dx) where that position is kept, else 0.
// The bounds are tested BEFORE the address is formed: a kept position lies inside the frame t of the same clip.
__device__ __forceinline__ f32x4 aug_gather_bwd(const float* __restrict__ g_clip, const AugGeo& a, int p, int H, int W) {
    const int sx = p % W, q = p / W, sy = q % H, t = q / H;
    const int y = sy + a.dy, x = sx + a.dx;
    f32x4 v = {};
    if (aug_kept(a, y, x, H, W)) v = *reinterpret_cast<const f32x4*>(g_clip + ((long long)(t * H + y) * W + x) * 4);
    return v;
}
__device__ __forceinline__ float aug_sum_valid(f32x4 v, int C) { return C == 3 ? (v[0] + v[1]) + v[2] : C == 2 ? v[0] + v[1] : v[0]; }

// slot (n, block) = sum over the block's pixels and the C valid channels of x (forward) or of the gathered, masked g_out (BWD);
// a thread adds its pixels in index order, the block's threads are combined by a fixed tree
template <bool BWD>
__global__ __launch_bounds__(NT) void augment_partial_kernel(int C, int P, int H, int W, int pix_per_block, const float* __restrict__ in,
                                                             const int32_t* __restrict__ geo, double* __restrict__ part) {
    __shared__ double red[NT];
    const int n = blockIdx.y;
    const float* clip = in + (long long)n * P * 4;
    const AugGeo a = aug_geo(geo, n);
    const int p0 = blockIdx.x * pix_per_block;
    int p1 = p0 + pix_per_block; if (p1 > P) p1 = P;
    double s = 0;
    for (int p = p0 + threadIdx.x; p < p1; p += NT) {
        const f32x4 v = BWD ? aug_gather_bwd(clip, a, p, H, W) : *reinterpret_cast<const f32x4*>(clip + (long long)p * 4);
        s += (double)aug_sum_valid(v, C);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = NT / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)n * AUG_MAX_BLOCKS + blockIdx.x] = red[0];
}

// the clip's mean over its T*H*W*C valid elements from its slots, added in slot order (every thread of the launch the same way)
__device__ __forceinline__ float aug_clip_mean(const double* __restrict__ part, int n, int nslots, double inv_count) {
    double s = 0;
    for (int k = 0; k < nslots; ++k) s += part[(long long)n * AUG_MAX_BLOCKS + k];
    return (float)(s * inv_count);
}

// Every fused multiply-add of the two apply kernels is written out (adam_wd_elem's comment says why): s * v + (1 - s) * mu and
// c * v + (1 - c) * m are fmaf(s, v, (1 - s) * mu) and fmaf(c, v, (1 - c) * m), so that b = 0, s = 1, c = 1 returns v itself.
__global__ __launch_bounds__(NT) void augment_fwd_apply_kernel(int C, int P, int H, int W, int nslots, double inv_count,
                                                               const float* __restrict__ in, const int32_t* __restrict__ geo,
                                                               const float* __restrict__ col, const double* __restrict__ part,
                                                               float* __restrict__ out) {
    const int n = blockIdx.y;
    const float* clip = in + (long long)n * P * 4;
    float* oclip = out + (long long)n * P * 4;
    const AugGeo a = aug_geo(geo, n);
    const float b = col[4 * n], s = col[4 * n + 1], c = col[4 * n + 2];
    const float m = aug_clip_mean(part, n, nslots, inv_count) + b;        // the clip mean after brightness (saturation keeps it)
    const float ms = 1.f - s, cm = (1.f - c) * m, fc = (float)C;
    for (int p = blockIdx.x * NT + threadIdx.x; p < P; p += gridDim.x * NT) {
        const int x = p % W, q = p / W, y = q % H, t = q / H;
        const int sy = y - a.dy, sx = x - a.dx;
        f32x4 o = {};
        // (the source is tested before its address is formed: it then lies in frame t of this clip)
        if (sy >= 0 && sy < H && sx >= 0 && sx < W && aug_kept(a, y, x, H, W)) {
            f32x4 v = *reinterpret_cast<const f32x4*>(clip + ((long long)(t * H + sy) * W + sx) * 4);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = k < C ? v[k] + b : 0.f;
            const float mu = aug_sum_valid(v, C) / fc;
#pragma unroll
            for (int k = 0; k < 3; ++k) if (k < C) o[k] = fmaf(c, fmaf(s, v[k], ms * mu), cm);
        }
        *reinterpret_cast<f32x4*>(oclip + (long long)p * 4) = o;
    }
}

__global__ __launch_bounds__(NT) void augment_bwd_apply_kernel(int C, int P, int H, int W, int nslots, double inv_count,
                                                               const float* __restrict__ g_out, const int32_t* __restrict__ geo,
                                                               const float* __restrict__ col, const double* __restrict__ part,
                                                               float* __restrict__ g_in) {
    const int n = blockIdx.y;
    const float* clip = g_out + (long long)n * P * 4;
    float* oclip = g_in + (long long)n * P * 4;
    const AugGeo a = aug_geo(geo, n);
    const float s = col[4 * n + 1], c = col[4 * n + 2];
    const float ms = 1.f - s, cm = (1.f - c) * aug_clip_mean(part, n, nslots, inv_count), fc = (float)C;
    for (int p = blockIdx.x * NT + threadIdx.x; p < P; p += gridDim.x * NT) {
        f32x4 v = aug_gather_bwd(clip, a, p, H, W);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = k < C ? fmaf(c, v[k], cm) : 0.f;
        const float mu = aug_sum_valid(v, C) / fc;
        f32x4 o = {};
#pragma unroll
        for (int k = 0; k < 3; ++k) if (k < C) o[k] = fmaf(s, v[k], ms * mu);
        *reinterpret_cast<f32x4*>(oclip + (long long)p * 4) = o;
    }
}

// clip i: Philox counters 2i, 2i + 1 of the stream -> words w0..w7 (w7 unused); a component the policy leaves out gets its
// identity values, its words are consumed all the same
struct AugDraw { float b, s, c; int dx, dy, x0, x1, y0, y1; };
__device__ __forceinline__ void aug_philox(uint64_t ctr, uint64_t seed, uint64_t stream_id, uint32_t (&r)[4]) {
    mcg::philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32), (uint32_t)seed,
                       (uint32_t)(seed >> 32), r);
}
__device__ __forceinline__ float aug_unit(uint32_t v) { return (float)(v >> 9) * 1.1920928955078125e-07f; }       // 23 bits x 2^-23: exact in fp32
__device__ __forceinline__ AugDraw aug_draw_clip(int i, int H, int W, int policy, uint64_t seed, uint64_t stream_id) {
    uint32_t w[8], r[4];
    for (int h = 0; h < 2; ++h) {
        aug_philox(2ull * (uint64_t)i + h, seed, stream_id, r);
        for (int k = 0; k < 4; ++k) w[4 * h + k] = r[k];
    }
    AugDraw a = {0.f, 1.f, 1.f, 0, 0, 0, 0, 0, 0};
    if (policy & MCG_AUG_COLOR) { a.b = aug_unit(w[0]) - 0.5f; a.s = 2.f * aug_unit(w[1]); a.c = aug_unit(w[2]) + 0.5f; }
    if (policy & MCG_AUG_TRANSLATION) {
        a.dx = (int)(w[3] % (uint32_t)(2 * (W / 8) + 1)) - W / 8;
        a.dy = (int)(w[4] % (uint32_t)(2 * (H / 8) + 1)) - H / 8;
    }
    if (policy & MCG_AUG_CUTOUT) {
        const int cx = (int)(w[5] % (uint32_t)(W + 1)), cy = (int)(w[6] % (uint32_t)(H + 1));
        int x0 = cx - W / 4, x1 = x0 + W / 2, y0 = cy - H / 4, y1 = y0 + H / 2;
        a.x0 = x0 < 0 ? 0 : x0; a.x1 = x1 > W ? W : x1; a.y0 = y0 < 0 ? 0 : y0; a.y1 = y1 > H ? H : y1;
    }
    return a;
}
// (word 6 of geo: the components that were applied -- 0 from the plain draw, the flags that passed from the gated one)
__device__ __forceinline__ void aug_store(const AugDraw& a, int applied, int i, int32_t* __restrict__ geo, float* __restrict__ col) {
    int32_t* q = geo + 8 * (long long)i;
    q[0] = a.dx; q[1] = a.dy; q[2] = a.x0; q[3] = a.x1; q[4] = a.y0; q[5] = a.y1; q[6] = applied; q[7] = 0;
    float* f = col + 4 * (long long)i;
    f[0] = a.b; f[1] = a.s; f[2] = a.c; f[3] = 0.f;
}

__global__ __launch_bounds__(NT) void augment_draw_kernel(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id,
                                                          int32_t* __restrict__ geo, float* __restrict__ col) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    aug_store(aug_draw_clip(i, H, W, policy, seed, stream_id), 0, i, geo, col);
}

// The gated draw (Karras et al. 2020, section 2.2: an augmentation applied with probability p < 1 does not leak into the generated
// clips).  Clip i also takes counter i of the gate stream, words g0..g3: colour passes iff u(g0) < p, translation iff u(g1) < p,
// cutout iff u(g2) < p, p = ada[0] read from device memory (mcg_ada_update writes it; the host never sees it).  A component that
// fails is drawn as if the policy left it out.
__global__ __launch_bounds__(NT) void augment_draw_gated_kernel(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id,
                                                                uint64_t gate_stream_id, const double* __restrict__ ada,
                                                                int32_t* __restrict__ geo, float* __restrict__ col) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const double p = ada[0];
    uint32_t g[4];
    aug_philox((uint64_t)i, seed, gate_stream_id, g);
    int pass = 0;
    if ((double)aug_unit(g[0]) < p) pass |= MCG_AUG_COLOR;
    if ((double)aug_unit(g[1]) < p) pass |= MCG_AUG_TRANSLATION;
    if ((double)aug_unit(g[2]) < p) pass |= MCG_AUG_CUTOUT;
    const int applied = policy & pass;
    aug_store(aug_draw_clip(i, H, W, applied, seed, stream_id), applied, i, geo, col);
}

// The controller of the gate's probability (Karras et al. 2020, section 3: r_t = E[sign(D(real))] as the overfitting signal).
// ada[8] = p, sign sum of D_V, of D_I, logits counted, calls counted, r_t of D_V, of D_I at the last adjustment, adjustments.
// One workgroup: the signs are summed as integers -- per thread, then over the block in a fixed tree -- so the sums are exact and
// no order enters; thread 0 does the rest in double.
__device__ __forceinline__ int ada_sign(float y) { return (y > 0.f) - (y < 0.f); }                   // (NaN and +-0: 0)
__global__ __launch_bounds__(NT) void ada_update_kernel(int N, int C, const float* __restrict__ y_video, const float* __restrict__ y_image,
                                                        double target, double step, int interval, double* __restrict__ ada) {
    __shared__ int sh_v[NT], sh_i[NT];
    const int tid = threadIdx.x;
    int sv = 0, si = 0;
    for (int n = tid; n < N; n += NT) {
        sv += ada_sign(y_video[(long long)n * C]);
        si += ada_sign(y_image[(long long)n * C]);
    }
    sh_v[tid] = sv; sh_i[tid] = si;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (tid < w) { sh_v[tid] += sh_v[tid + w]; sh_i[tid] += sh_i[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double sum_v = ada[1] + (double)sh_v[0], sum_i = ada[2] + (double)sh_i[0];
        const double count = ada[3] + (double)N, calls = ada[4] + 1.0;
        if (calls >= (double)interval) {
            const double r_v = sum_v / count, r_i = sum_i / count, r = fmax(r_v, r_i);
            const double d = (double)((r > target) - (r < target));
            ada[0] = fmin(1.0, fmax(0.0, ada[0] + d * step));
            ada[1] = 0.0; ada[2] = 0.0; ada[3] = 0.0; ada[4] = 0.0;
            ada[5] = r_v; ada[6] = r_i; ada[7] += 1.0;
        } else {
            ada[1] = sum_v; ada[2] = sum_i; ada[3] = count; ada[4] = calls;
        }
    }
}

int check_augment(int N, int C, int Cp, int T, int H, int W, const void* in, const void* geo, const void* col, const void* ws, const void* out) {
    if (!in || !geo || !col || !ws || !out || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C < 1 || C > 3) return MCG_ERR_BAD_ARG;
    if (in == out) return MCG_ERR_BAD_ARG;                                     // a gather: never in place
    if (Cp != 4) return MCG_ERR_UNSUPPORTED;
    if ((long long)T * H * W > (1LL << 28) || N > 65535) return MCG_ERR_UNSUPPORTED;     // pixel indices of a clip are ints; N is gridDim.y
    return MCG_OK;
}
int augment_apply_blocks(int N, long long P) {
    long long b = (P + NT - 1) / NT, cap = EW_GRID / N;
    if (cap < 1) cap = 1;
    return (int)(b > cap ? cap : b);
}

// ------------------------------------------------------------------------------------------
// Geometric augmentation (Karras et al. 2020, the x-flip / quarter-turn / isotropic-scale / rotation family; no reference
// counterpart): a per-clip affine warp with bilinear taps and zero padding, the same matrix for every frame of a clip.
// mat[8] = m00 m01 m02 m10 m11 m12 flags 0 maps an OUTPUT position to its SOURCE (include/mocogan_hip.h states the arithmetic).
// Forward and backward take the source of an output pixel from ONE function, warp_source, whose operations are rounded one by
// one (no contraction into FMAs): the weights of a tap are then the same floats in both directions, and the backward pass -- a
// gather over a conservative box of output pixels, no atomics, fixed order -- is the exact adjoint.
// ------------------------------------------------------------------------------------------
// One rounding per operation: the compiler contracts a * b + c into an FMA by default, and its __fmul_rn / __fadd_rn are plain
// operators compiled under that default, so they fuse as well once inlined.  These four carry the pragma themselves.
__device__ __forceinline__ float warp_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float warp_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float warp_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float warp_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}
struct WarpMat { float m00, m01, m02, m10, m11, m12, cx, cy, xmax, ymax; };
__device__ __forceinline__ WarpMat warp_mat(const float* __restrict__ mat, int n, int H, int W) {
    const float* q = mat + 8 * (long long)n;
    WarpMat m = {q[0], q[1], q[2], q[3], q[4], q[5], (float)(W - 1) * 0.5f, (float)(H - 1) * 0.5f, (float)(W + 1), (float)(H + 1)};
    return m;
}
// (x0, y0) = floor of the source of output pixel (y, x), (fx, fy) = its fraction -- exact.  The source is clamped to [-2, extent + 1]
// BEFORE the conversion (fmaxf drops a NaN): a clamped source has no tap inside the frame, as the unclamped one had none.
struct WarpSrc { int x0, y0; float fx, fy; };
__device__ __forceinline__ WarpSrc warp_source(const WarpMat& m, int y, int x) {
    const float xc = warp_sub((float)x, m.cx), yc = warp_sub((float)y, m.cy);
    float sx = warp_add(warp_add(warp_mul(m.m00, xc), warp_mul(m.m01, yc)), warp_add(m.cx, m.m02));
    float sy = warp_add(warp_add(warp_mul(m.m10, xc), warp_mul(m.m11, yc)), warp_add(m.cy, m.m12));
    sx = fminf(fmaxf(sx, -2.f), m.xmax);
    sy = fminf(fmaxf(sy, -2.f), m.ymax);
    const float flx = floorf(sx), fly = floorf(sy);
    WarpSrc s = {(int)flx, (int)fly, warp_sub(sx, flx), warp_sub(sy, fly)};
    return s;
}
// the weight of tap (y0 + iy, x0 + ix), ix, iy in {0, 1}
__device__ __forceinline__ float warp_weight(const WarpSrc& s, int iy, int ix) {
    return warp_mul(ix ? s.fx : warp_sub(1.f, s.fx), iy ? s.fy : warp_sub(1.f, s.fy));
}

__global__ __launch_bounds__(NT) void warp_fwd_kernel(int P, int H, int W, const float* __restrict__ in, const float* __restrict__ mat,
                                                      float* __restrict__ out) {
    const int n = blockIdx.y;
    const float* clip = in + (long long)n * P * 4;
    float* oclip = out + (long long)n * P * 4;
    const WarpMat m = warp_mat(mat, n, H, W);
    for (int p = blockIdx.x * NT + threadIdx.x; p < P; p += gridDim.x * NT) {
        const int x = p % W, q = p / W, y = q % H, t = q / H;
        const WarpSrc s = warp_source(m, y, x);
        f32x4 o = {};
#pragma unroll
        for (int iy = 0; iy < 2; ++iy)
#pragma unroll
            for (int ix = 0; ix < 2; ++ix) {
                const int yy = s.y0 + iy, xx = s.x0 + ix;
                const float w = warp_weight(s, iy, ix);
                // (the tap is tested before its address is formed: it then lies in frame t of this clip; a tap of weight 0 is not read)
                if (w != 0.f && yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(clip + ((long long)(t * H + yy) * W + xx) * 4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = fmaf(w, v[k], o[k]);
                }
            }
        *reinterpret_cast<f32x4*>(oclip + (long long)p * 4) = o;
    }
}

// The output pixels whose source can touch source pixel (v, u): the image of the open square (u - 1, u + 1) x (v - 1, v + 1) under
// the inverse of the linear part, widened by a pixel, clamped to the frame.  The inverse is formed in double (the products of two
// floats are exact there).  The whole frame is taken when the determinant is zero, the inverse is not finite, or the rounding of
// warp_source (bounded by 2^-21 of the magnitudes it adds) could move a source by half a pixel of the OUTPUT once mapped back.
struct WarpInv { double i00, i01, i10, i11, ex, ey, ox, oy; bool whole; };
__device__ __forceinline__ WarpInv warp_inverse(const WarpMat& m, int H, int W) {
    const double a = m.m00, b = m.m01, c = m.m10, d = m.m11;
    const double det = a * d - b * c, r = 1.0 / det;
    WarpInv v;
    v.i00 = d * r; v.i01 = -b * r; v.i10 = -c * r; v.i11 = a * r;
    v.ex = fabs(v.i00) + fabs(v.i01); v.ey = fabs(v.i10) + fabs(v.i11);
    v.ox = (double)m.cx + (double)m.m02; v.oy = (double)m.cy + (double)m.m12;
    const double mag = (fabs(a) + fabs(b) + fabs(c) + fabs(d)) * (double)(H + W) + fabs(v.ox) + fabs(v.oy);
    const double slack = (v.ex + v.ey) * mag * 4.76837158203125e-07;           // 2^-21
    v.whole = !(fabs(det) > 0.0) || !(slack < 0.5);                            // (a NaN or an infinity fails the second test)
    return v;
}
struct WarpBox { int x_lo, x_hi, y_lo, y_hi; };
__device__ __forceinline__ WarpBox warp_box(const WarpMat& m, const WarpInv& v, int vy, int ux, int H, int W) {
    WarpBox bx = {0, W - 1, 0, H - 1};
    if (!v.whole) {
        const double du = (double)ux - v.ox, dv = (double)vy - v.oy;
        const double xo = (double)m.cx + (v.i00 * du + v.i01 * dv), yo = (double)m.cy + (v.i10 * du + v.i11 * dv);
        // (clamped as doubles, then converted: the values are inside the frame; an empty box has lo > hi)
        bx.x_lo = (int)fmin(fmax(floor(xo - v.ex - 1.0), 0.0), (double)W);
        bx.x_hi = (int)fmin(fmax(ceil(xo + v.ex + 1.0), -1.0), (double)(W - 1));
        bx.y_lo = (int)fmin(fmax(floor(yo - v.ey - 1.0), 0.0), (double)H);
        bx.y_hi = (int)fmin(fmax(ceil(yo + v.ey + 1.0), -1.0), (double)(H - 1));
    }
    return bx;
}

// One thread per source pixel (v, u) and group of WARP_TC frames: the candidates and their weights are those of every frame of the
// clip, so the search is paid once per group.  Candidates in row-major order, frames innermost: the order of the sum is fixed.
// g_out is gathered through L2; a block per (frame, clip) that staged the frame in LDS first measured 2.6 x (32 clips) and
// 1.9 x (256 clips) slower (profiles/warp_notes.md) and is not kept.
constexpr int WARP_TC = 4;
__global__ __launch_bounds__(NT) void warp_bwd_kernel(int T, int H, int W, const float* __restrict__ g_out, const float* __restrict__ mat,
                                                      float* __restrict__ g_in) {
    const int n = blockIdx.y, HW = H * W;
    const long long P = (long long)T * HW;
    const float* clip = g_out + (long long)n * P * 4;
    float* oclip = g_in + (long long)n * P * 4;
    const WarpMat m = warp_mat(mat, n, H, W);
    const WarpInv inv = warp_inverse(m, H, W);
    const int total = HW * ((T + WARP_TC - 1) / WARP_TC);
    for (int q = blockIdx.x * NT + threadIdx.x; q < total; q += gridDim.x * NT) {
        const int pix = q % HW, t0 = (q / HW) * WARP_TC, u = pix % W, v = pix / W;
        const int nt = T - t0 < WARP_TC ? T - t0 : WARP_TC;
        const WarpBox bx = warp_box(m, inv, v, u, H, W);
        f32x4 acc[WARP_TC] = {};
        for (int y = bx.y_lo; y <= bx.y_hi; ++y)
            for (int x = bx.x_lo; x <= bx.x_hi; ++x) {
                const WarpSrc s = warp_source(m, y, x);
                const int ix = u - s.x0, iy = v - s.y0;
                if ((unsigned)ix > 1u || (unsigned)iy > 1u) continue;
                const float w = warp_weight(s, iy, ix);
                if (w == 0.f) continue;
                const float* g = clip + ((long long)(t0 * H + y) * W + x) * 4;           // (y, x) lies in the frame: the box is clamped
#pragma unroll
                for (int k = 0; k < WARP_TC; ++k)
                    if (k < nt) {
                        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (long long)k * HW * 4);
#pragma unroll
                        for (int l = 0; l < 4; ++l) acc[k][l] = fmaf(w, gv[l], acc[k][l]);
                    }
            }
#pragma unroll
        for (int k = 0; k < WARP_TC; ++k)
            if (k < nt) *reinterpret_cast<f32x4*>(oclip + ((long long)(t0 + k) * HW + pix) * 4) = acc[k];
    }
}

// Clip i: Philox counter i of the stream, words w0..w3 -> flip, quarter turn, scale, rotation; a component the policy leaves out
// takes its identity value, its word is consumed all the same.  fp32, every + - * / rounded on its own, no transcendental:
// L = (1 / s) [[c, sn], [-sn, c]] Q_k diag(f, 1) -- one division, four products by 1 / s, then signs and a permutation (exact).
struct WarpDraw { float m00, m01, m10, m11; };
__device__ __forceinline__ float warp_pos_zero(float v) { return v == 0.f ? 0.f : v; }              // (-0 -> +0)
__device__ __forceinline__ WarpDraw warp_draw_clip(int i, int policy, uint64_t seed, uint64_t stream_id) {
    uint32_t w[4];
    aug_philox((uint64_t)i, seed, stream_id, w);
    float f = 1.f, s = 1.f, c = 1.f, sn = 0.f;
    int k = 0;
    if (policy & MCG_WARP_FLIP) f = (w[0] & 1u) ? -1.f : 1.f;
    if (policy & MCG_WARP_ROT90) k = (int)(w[1] & 3u);
    if (policy & MCG_WARP_SCALE) {
        const float a = warp_div(warp_sub(warp_mul(2.f, aug_unit(w[2])), 1.f), 6.f);
        s = warp_div(warp_add(1.f, a), warp_sub(1.f, a));
    }
    if (policy & MCG_WARP_ROTATE) {
        const float t = warp_sub(warp_mul(2.f, aug_unit(w[3])), 1.f), tt = warp_mul(t, t), den = warp_add(1.f, tt);
        c = warp_div(warp_sub(1.f, tt), den);
        sn = warp_div(warp_mul(2.f, t), den);
    }
    const float r = warp_div(1.f, s), rc = warp_mul(r, c), rs = warp_mul(r, sn);
    float a00 = rc, a01 = rs, a10 = -rs, a11 = rc;                       // (1 / s) R
    for (int j = 0; j < k; ++j) {                                        // times Q_1 = [[0, -1], [1, 0]], k times
        const float b00 = a01, b01 = -a00, b10 = a11, b11 = -a10;
        a00 = b00; a01 = b01; a10 = b10; a11 = b11;
    }
    WarpDraw d = {warp_pos_zero(warp_mul(f, a00)), warp_pos_zero(a01), warp_pos_zero(warp_mul(f, a10)), warp_pos_zero(a11)};
    return d;
}
// (word 6: the components that were applied, as a float -- 0 from the plain draw, the flags that passed from the gated one)
__device__ __forceinline__ void warp_store(const WarpDraw& d, int applied, int i, float* __restrict__ mat) {
    float* q = mat + 8 * (long long)i;
    q[0] = d.m00; q[1] = d.m01; q[2] = 0.f; q[3] = d.m10; q[4] = d.m11; q[5] = 0.f; q[6] = (float)applied; q[7] = 0.f;
}
__global__ __launch_bounds__(NT) void warp_draw_kernel(int N, int policy, uint64_t seed, uint64_t stream_id, float* __restrict__ mat) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    warp_store(warp_draw_clip(i, policy, seed, stream_id), 0, i, mat);
}
// the gates of augment_draw_gated_kernel: flip, quarter turn, scale, rotation pass iff u(g0), u(g1), u(g2), u(g3) < p = ada[0]
__global__ __launch_bounds__(NT) void warp_draw_gated_kernel(int N, int policy, uint64_t seed, uint64_t stream_id, uint64_t gate_stream_id,
                                                             const double* __restrict__ ada, float* __restrict__ mat) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const double p = ada[0];
    uint32_t g[4];
    aug_philox((uint64_t)i, seed, gate_stream_id, g);
    int pass = 0;
    if ((double)aug_unit(g[0]) < p) pass |= MCG_WARP_FLIP;
    if ((double)aug_unit(g[1]) < p) pass |= MCG_WARP_ROT90;
    if ((double)aug_unit(g[2]) < p) pass |= MCG_WARP_SCALE;
    if ((double)aug_unit(g[3]) < p) pass |= MCG_WARP_ROTATE;
    const int applied = policy & pass;
    warp_store(warp_draw_clip(i, applied, seed, stream_id), applied, i, mat);
}

int check_warp(int N, int C, int Cp, int T, int H, int W, const void* in, const void* mat, const void* out) {
    if (!in || !mat || !out || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C < 1 || C > Cp) return MCG_ERR_BAD_ARG;
    if (in == out) return MCG_ERR_BAD_ARG;                                     // a gather: never in place
    if (Cp != 4) return MCG_ERR_UNSUPPORTED;
    if ((long long)T * H * W > (1LL << 28) || N > 65535) return MCG_ERR_UNSUPPORTED;     // mcg_augment_fwd's extents
    return MCG_OK;
}
int check_warp_draw(int N, int H, int W, int policy, const void* mat) {
    if (!mat || N <= 0 || H <= 0 || W <= 0 || policy < 0 || policy > 15) return MCG_ERR_BAD_ARG;
    if ((policy & MCG_WARP_ROT90) && H != W) return MCG_ERR_UNSUPPORTED;       // a quarter turn maps the frame onto itself only when square
    return MCG_OK;
}

}  // namespace

extern "C" int mcg_version(void) { return MCG_ABI_VERSION; }

extern "C" int64_t mcg_bn_workspace_bytes(int64_t /*M*/, int C) {
    return (int64_t)(MAX_PART * 2 * C + 3 * C) * (int64_t)sizeof(float);
}

extern "C" int mcg_bn_stats(int64_t M, int C, const float* y, const float* gamma, const float* beta, float* stats,
                            float* avg_mean, float* avg_var, float eps, float decay, void* workspace, void* stream) {
    if (!y || !gamma || !beta || !stats || !workspace || M <= 0 || bad_c(C)) return MCG_ERR_BAD_ARG;
    if ((avg_mean == nullptr) != (avg_var == nullptr)) return MCG_ERR_BAD_ARG;
    if (unsupported_c(C)) return MCG_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    PartPlan pl = plan_partial(M, C);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(col_partial_kernel<0>, dim3(pl.blocks), dim3(NT), 0, s, (long long)M, C, pl.rows_per_block, y, nullptr, nullptr, 0, part);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, s, pl.blocks, C, 1.0 / (double)M, bessel_adjust(M),
                       part, gamma, beta, stats, avg_mean, avg_var, eps, decay, 0LL);
    return launch_status();
}

extern "C" int mcg_bn_stats_from_partials(int64_t M, int C, const float* part, int n_slots, int slot_stride, const float* gamma, const float* beta,
                                          float* stats, float* avg_mean, float* avg_var, float eps, float decay, void* workspace, void* stream) {
    if (!part || !gamma || !beta || !stats || M <= 0 || bad_c(C) || n_slots <= 0 || slot_stride < 2 * C) return MCG_ERR_BAD_ARG;
    if ((avg_mean == nullptr) != (avg_var == nullptr)) return MCG_ERR_BAD_ARG;
    const Folded f = fold_slots(part, n_slots, slot_stride, C, (float*)workspace, (hipStream_t)stream);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, (hipStream_t)stream, f.n, C, 1.0 / (double)M,
                       bessel_adjust(M), f.part, gamma, beta, stats, avg_mean, avg_var, eps, decay, f.stride);
    return launch_status();
}

extern "C" int mcg_bn_act_fwd(int64_t M, int C, int c_valid, const float* y, int64_t y_rows_per_item, int64_t y_item_stride,
                              const float* scale_shift, int act, const float* addend,
                              float sigma, uint64_t seed, uint64_t stream_id, void* out, int out_bf16, void* stream) {
    if (!y || !out || M <= 0 || bad_c(C)) return MCG_ERR_BAD_ARG;
    if (y_rows_per_item < 0 || (y_rows_per_item > 0 && (M % y_rows_per_item || (y_item_stride & 3)))) return MCG_ERR_BAD_ARG;
    if (out_bf16 & ~(MCG_IO_OUT_BF16 | MCG_IO_Y_BF16 | MCG_IO_OUT_SPLIT)) return MCG_ERR_BAD_ARG;
    if ((out_bf16 & MCG_IO_OUT_SPLIT) && out_bf16 != MCG_IO_OUT_SPLIT) return MCG_ERR_BAD_ARG;
    // the eight-wide kernel takes dense y with every channel valid; the split output exists there only (a 16-byte piece of each plane per thread)
    const bool wide = wide_c(out_bf16, C) && y_rows_per_item == 0 && c_valid == C;
    if (out_bf16 == MCG_IO_OUT_SPLIT && (!wide || (C & 15))) return MCG_ERR_UNSUPPORTED;
    auto launch = [&](auto w, auto ioc) {
        constexpr int W = decltype(w)::value;
        const long long n = (long long)M * (C >> LOG2<W>);
        hipLaunchKernelGGL((bn_act_fwd_kernel<W, decltype(ioc)::value>), dim3(ew_grid(n)), dim3(NT), 0, (hipStream_t)stream, n, C, c_valid, y,
                           (long long)y_rows_per_item * (C >> LOG2<W>), (long long)y_item_stride, scale_shift, act, addend, sigma, seed, stream_id,
                           (float*)out);
    };
    if (wide) with_io<1, 2, 8, 3>(out_bf16, [&](auto ioc) { launch(width<8>{}, ioc); });
    else with_io<0, 1, 2, 3>(out_bf16, [&](auto ioc) { launch(width<4>{}, ioc); });
    return launch_status();
}

extern "C" int mcg_bn_act_bwd(int64_t M, int C, const float* g_out, const float* y, const float* stats, const float* gamma, int act,
                              void* gx, int gx_bf16, float* dgamma, float* dbeta, void* workspace, void* stream) {
    if (!g_out || !y || !gx || M <= 0 || bad_c(C)) return MCG_ERR_BAD_ARG;
    if (const int bad = check_bwd_io(gx, g_out, gx_bf16, C, stats)) return bad;
    hipStream_t s = (hipStream_t)stream;
    float* coef = nullptr;
    if (stats) {
        if (!gamma || !workspace) return MCG_ERR_BAD_ARG;
        if (unsupported_c(C)) return MCG_ERR_UNSUPPORTED;
        PartPlan pl = plan_partial(M, C);
        float* part = (float*)workspace;
        coef = part + (long long)MAX_PART * 2 * C;
        launch_bwd_partial(gx_bf16, pl.blocks, s, (long long)M, C, pl.rows_per_block, g_out, y, stats, act, part);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, s, pl.blocks, C, 1.0 / (double)M, part, stats, gamma,
                           coef, dgamma, dbeta, 0LL);
    }
    launch_bwd_apply(gx_bf16, s, (long long)M, C, g_out, y, stats, coef, act, (float*)gx);
    return launch_status();
}

extern "C" int mcg_bn_act_bwd_from_partials(int64_t M, int C, const float* g_out, const float* y, const float* stats, const float* gamma, int act,
                                            const float* part, int n_slots, int slot_stride, void* gx, int gx_bf16, float* dgamma, float* dbeta,
                                            void* workspace, void* stream) {
    if (!g_out || !y || !gx || !stats || !gamma || !part || !workspace || M <= 0 || bad_c(C) || n_slots <= 0 || slot_stride < 2 * C) return MCG_ERR_BAD_ARG;
    if (const int bad = check_bwd_io(gx, g_out, gx_bf16, C, stats)) return bad;
    hipStream_t s = (hipStream_t)stream;
    float* coef = (float*)workspace + (long long)MAX_PART * 2 * C;
    const Folded f = fold_slots(part, n_slots, slot_stride, C, (float*)workspace, s);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, s, f.n, C, 1.0 / (double)M, f.part, stats, gamma,
                       coef, dgamma, dbeta, f.stride);
    launch_bwd_apply(gx_bf16, s, (long long)M, C, g_out, y, stats, coef, act, (float*)gx);
    return launch_status();
}

extern "C" int mcg_colsum_from_partials(int C, const float* part, int n_slots, int slot_stride, float* db, void* workspace, void* stream) {
    if (!part || !db || bad_c(C) || n_slots <= 0 || slot_stride < 2 * C) return MCG_ERR_BAD_ARG;
    const Folded f = fold_slots(part, n_slots, slot_stride, C, (float*)workspace, (hipStream_t)stream);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, (hipStream_t)stream, f.n, C, f.part, db, f.stride);
    return launch_status();
}

extern "C" int mcg_bn_sums(int64_t M, int C, const float* y, double* sums, void* workspace, void* stream) {
    if (!y || !sums || !workspace || M <= 0 || bad_c(C)) return MCG_ERR_BAD_ARG;
    if (unsupported_c(C)) return MCG_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    PartPlan pl = plan_partial(M, C);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(col_partial_kernel<0>, dim3(pl.blocks), dim3(NT), 0, s, (long long)M, C, pl.rows_per_block, y, nullptr, nullptr, 0, part);
    hipLaunchKernelGGL(sums_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, s, pl.blocks, C, part, sums);
    return launch_status();
}

extern "C" int mcg_bn_stats_from_sums(int64_t M_total, int C, const double* sums, const float* gamma, const float* beta, float* stats,
                                      float* avg_mean, float* avg_var, float eps, float decay, void* stream) {
    if (!sums || !gamma || !beta || !stats || M_total <= 0 || C <= 0) return MCG_ERR_BAD_ARG;
    if ((avg_mean == nullptr) != (avg_var == nullptr)) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(bn_stats_from_sums_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, C, 1.0 / (double)M_total, bessel_adjust(M_total), sums,
                       gamma, beta, stats, avg_mean, avg_var, eps, decay);
    return launch_status();
}

extern "C" int mcg_bn_bwd_sums(int64_t M, int C, const float* g_out, const float* y, const float* stats, int act, int io_bf16, double* sums,
                               void* workspace, void* stream) {
    if (!g_out || !y || !stats || !sums || !workspace || M <= 0 || bad_c(C)) return MCG_ERR_BAD_ARG;
    if (io_bf16 & ~(MCG_IO_Y_BF16 | MCG_IO_G_BF16)) return MCG_ERR_BAD_ARG;
    if (unsupported_c(C)) return MCG_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    PartPlan pl = plan_partial(M, C);
    float* part = (float*)workspace;
    launch_bwd_partial(io_bf16, pl.blocks, s, (long long)M, C, pl.rows_per_block, g_out, y, stats, act, part);
    hipLaunchKernelGGL(sums_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, s, pl.blocks, C, part, sums);
    return launch_status();
}

extern "C" int mcg_bn_act_bwd_from_sums(int64_t M, int64_t M_total, int C, const float* g_out, const float* y, const float* stats,
                                        const float* gamma, int act, const double* local_sums, const double* global_sums, void* gx,
                                        int gx_bf16, float* dgamma, float* dbeta, void* workspace, void* stream) {
    if (!g_out || !y || !gx || !stats || !gamma || !local_sums || !global_sums || !workspace || M <= 0 || M_total < M || bad_c(C)) return MCG_ERR_BAD_ARG;
    if (gx_bf16 & ~7) return MCG_ERR_BAD_ARG;
    if (const int bad = check_bwd_io(gx, g_out, gx_bf16, C, stats)) return bad;
    hipStream_t s = (hipStream_t)stream;
    float* coef = (float*)workspace + (long long)MAX_PART * 2 * C;
    hipLaunchKernelGGL(bn_bwd_from_sums_kernel, dim3((C + 63) / 64), dim3(64), 0, s, C, 1.0 / (double)M_total, local_sums, global_sums, stats, gamma,
                       coef, dgamma, dbeta);
    launch_bwd_apply(gx_bf16, s, (long long)M, C, g_out, y, stats, coef, act, (float*)gx);
    return launch_status();
}

extern "C" int mcg_colsum_acc(int64_t M, int C, const float* g, float* db, void* workspace, void* stream) {
    if (!g || !db || !workspace || M <= 0 || bad_c(C)) return MCG_ERR_BAD_ARG;
    if (unsupported_c(C)) return MCG_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    PartPlan pl = plan_partial(M, C);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(col_partial_kernel<2>, dim3(pl.blocks), dim3(NT), 0, s, (long long)M, C, pl.rows_per_block, g, nullptr, nullptr, 0, part);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_SL), 0, s, pl.blocks, C, part, db, 0LL);
    return launch_status();
}

extern "C" int mcg_pack_clip(int N, int C, int Cp, int T, int HW, const float* x, int64_t x_stride_n, int64_t x_stride_c,
                             const float* addend, float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream) {
    if (!x || !out || N <= 0 || C <= 0 || Cp < C || (Cp & 3) || T <= 0 || HW <= 0 || x_stride_n < 0 || x_stride_c < 0) return MCG_ERR_BAD_ARG;
    long long npix = (long long)N * T * HW;
    hipLaunchKernelGGL(pack_clip_kernel, dim3(ew_grid(npix)), dim3(NT), 0, (hipStream_t)stream, N, C, Cp, T, HW, x,
                       (long long)x_stride_n, (long long)x_stride_c, addend, sigma, seed, stream_id, out);
    return launch_status();
}

extern "C" int mcg_pack_clip_u8(int N, int C, int Cp, int T, int HW, const uint8_t* x, int64_t x_stride_n, int64_t x_stride_t,
                                const float* addend, float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream) {
    if (!x || !out || N <= 0 || C <= 0 || Cp < C || (Cp & 3) || T <= 0 || HW <= 0 || x_stride_n < 0 || x_stride_t < 0) return MCG_ERR_BAD_ARG;
    long long npix = (long long)N * T * HW;
    hipLaunchKernelGGL(pack_clip_u8_kernel, dim3(ew_grid(npix)), dim3(NT), 0, (hipStream_t)stream, N, C, Cp, T, HW, x,
                       (long long)x_stride_n, (long long)x_stride_t, addend, sigma, seed, stream_id, out);
    return launch_status();
}

extern "C" int mcg_clip_to_u8(int N, int C, int Cp, int T, int HW, const float* in, const float* bias, int act, uint8_t* out,
                              int64_t stride_n, int64_t stride_t, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || Cp < C || (Cp & 3) || T <= 0 || HW <= 0) return MCG_ERR_BAD_ARG;
    // a frame is HW * C dense bytes; items and frames must not overlap: (N,T,...) or (T,N,...) order, padded or not
    const long long frame = (long long)HW * C;
    if (stride_n < frame || stride_t < frame || !(stride_n >= (long long)T * stride_t || stride_t >= (long long)N * stride_n)) return MCG_ERR_BAD_ARG;
    if (act != MCG_ACT_NONE && act != MCG_ACT_TANH) return MCG_ERR_BAD_ARG;
    if (Cp != 4) return MCG_ERR_UNSUPPORTED;           // the clip side: one 16-byte load per pixel
    const long long npix = (long long)N * T * HW;
    const bool pack = C == 3 && (HW & 3) == 0 && (stride_n & 3) == 0 && (stride_t & 3) == 0 && ((uintptr_t)out & 3) == 0;
    if (pack) hipLaunchKernelGGL(clip_to_u8_kernel<true>, dim3(ew_grid(npix / 4)), dim3(NT), 0, (hipStream_t)stream, npix / 4, C, T, HW, in, bias,
                                 act, out, (long long)stride_n, (long long)stride_t);
    else hipLaunchKernelGGL(clip_to_u8_kernel<false>, dim3(ew_grid(npix)), dim3(NT), 0, (hipStream_t)stream, npix, C, T, HW, in, bias, act, out,
                            (long long)stride_n, (long long)stride_t);
    return launch_status();
}

extern "C" int mcg_bn_fold_deconv(int64_t rows, int C, int Cp, const float* w, const float* bias, const float* gamma, const float* beta,
                                  const float* avg_mean, const float* avg_var, float eps, float* w_out, float* bias_out, void* stream) {
    if (!w || !gamma || !beta || !avg_mean || !avg_var || !w_out || !bias_out || rows <= 0 || C <= 0 || Cp < C || (Cp & 3) || !(eps >= 0.f))
        return MCG_ERR_BAD_ARG;
    const long long n4 = (long long)rows * (Cp >> 2);
    hipLaunchKernelGGL(bn_fold_deconv_kernel, dim3(ew_grid(n4 + (Cp >> 2))), dim3(NT), 0, (hipStream_t)stream, n4, C, Cp, w, bias, gamma, beta,
                       avg_mean, avg_var, eps, w_out, bias_out);
    return launch_status();
}

extern "C" int mcg_concat_label_planes(int N, int64_t P, int C, int Cp, int dl, int Cq, const float* x, const int32_t* labels, float* out,
                                       void* stream) {
    if (!x || !out || N <= 0 || P <= 0 || C <= 0 || Cp < C || dl < 0 || Cq < C + dl || (Cq & 3) || (dl && !labels)) return MCG_ERR_BAD_ARG;
    const long long npix = (long long)N * P;
    hipLaunchKernelGGL(concat_label_planes_kernel, dim3(ew_grid(npix * (Cq >> 2))), dim3(NT), 0, (hipStream_t)stream, npix, (long long)P, C, Cp,
                       dl, Cq, x, labels, out);
    return launch_status();
}

extern "C" int mcg_unpack_clip(int N, int C, int Cp, int T, int HW, const float* in, float* x, void* stream) {
    if (!x || !in || N <= 0 || C <= 0 || Cp < C || T <= 0 || HW <= 0) return MCG_ERR_BAD_ARG;
    long long npix = (long long)N * T * HW;
    hipLaunchKernelGGL(unpack_clip_kernel, dim3(ew_grid(npix)), dim3(NT), 0, (hipStream_t)stream, N, C, Cp, T, HW, in, x);
    return launch_status();
}

extern "C" int mcg_tanh_bwd_to_frames(int N, int T, int64_t frame_elems, const float* g_clip, const float* x_clip, float* g_frames, void* stream) {
    if (!g_clip || !x_clip || !g_frames || N <= 0 || T <= 0 || frame_elems <= 0 || (frame_elems & 3)) return MCG_ERR_BAD_ARG;
    long long n4 = (long long)N * T * (frame_elems >> 2);
    hipLaunchKernelGGL(tanh_bwd_to_frames_kernel, dim3(ew_grid(n4)), dim3(NT), 0, (hipStream_t)stream, N, T, (long long)(frame_elems >> 2), g_clip, x_clip, g_frames);
    return launch_status();
}

// conv_gemm.hip: the fully-connected layers with a real output width run on the MFMA GEMM core
extern "C" __attribute__((visibility("hidden"))) int mcg_detail_fc_fprop_gemm(int M, int K, int N, const float* x, const float* w, const float* bias, float* y, void* stream);
extern "C" __attribute__((visibility("hidden"))) int mcg_detail_fc_wgrad_gemm(int M, int K, int N, const float* x, const float* y, float* dw, void* stream);

extern "C" int mcg_fc_fprop(int M, int K, int Co, const float* x, const float* w, const float* bias, float* y, void* stream) {
    if (!x || !w || !y || M <= 0 || K <= 0 || (K & 3) || Co <= 0) return MCG_ERR_BAD_ARG;
    if (Co >= 16 && M >= 64) {                       // G's dc1 (60 x 8192): a GEMM, not 60 dot products per row
        int st = mcg_detail_fc_fprop_gemm(M, K, Co, x, w, bias, y, stream);
        if (st != MCG_ERR_UNSUPPORTED) return st;
    }
    hipLaunchKernelGGL(fc_fprop_kernel, dim3(M, Co), dim3(NT), 0, (hipStream_t)stream, K, Co, x, w, bias, y);
    return launch_status();
}

extern "C" int mcg_fc_dgrad(int M, int K, int Co, const float* y, const float* w, const float* bias, int bias_period, float* x, void* stream) {
    if (!x || !w || !y || M <= 0 || K <= 0 || (K & 3) || Co <= 0) return MCG_ERR_BAD_ARG;
    if (bias && (bias_period <= 0 || (bias_period & 3) || K % bias_period)) return MCG_ERR_BAD_ARG;
    if (Co >= 8 && M % 8 == 0 && M >= 64)
        hipLaunchKernelGGL(fc_dgrad_rows_kernel<8>, dim3((K / 4 + NT - 1) / NT, M / 8), dim3(NT), 0, (hipStream_t)stream, K, Co, y, w, bias, bias_period, x);
    else
        hipLaunchKernelGGL(fc_dgrad_kernel, dim3((K / 4 + NT - 1) / NT, M), dim3(NT), 0, (hipStream_t)stream, K, Co, y, w, bias, bias_period, x);
    return launch_status();
}

extern "C" int mcg_fc_wgrad(int M, int K, int Co, const float* x, const float* y, float* dw, float* db, void* stream) {
    if (!x || !dw || !y || M <= 0 || K <= 0 || (K & 3) || Co <= 0) return MCG_ERR_BAD_ARG;
    if (Co >= 16 && !(Co & 3) && M >= 64 && !db) {
        int st = mcg_detail_fc_wgrad_gemm(M, K, Co, x, y, dw, stream);
        if (st != MCG_ERR_UNSUPPORTED) return st;
    }
    hipLaunchKernelGGL(fc_wgrad_kernel, dim3((K / 4 + FCW_Q - 1) / FCW_Q, Co), dim3(NT), 0, (hipStream_t)stream, M, K, Co, x, y, dw, db);
    return launch_status();
}

extern "C" int mcg_gru_seq_fwd(int N, int T, int dim_zm, int dim_zl, int dim_zc, const float* params, const float* h0, const float* e,
                               const int32_t* labels, const float* zc, float* z, float* saved, void* stream) {
    if (!params || !h0 || !e || !zc || !z || !saved || N <= 0 || T <= 0) return MCG_ERR_BAD_ARG;
    if (dim_zm <= 0 || dim_zm > GRUW_U || dim_zl < 0 || dim_zm + dim_zl > GRUW_IN || dim_zc < 0) return MCG_ERR_UNSUPPORTED;
    if (dim_zl && !labels) return MCG_ERR_BAD_ARG;
    if (dim_zm > GRU_U || dim_zm + dim_zl > GRU_MAXIN)             // wide states: the weights stay in memory
        hipLaunchKernelGGL(gru_fwd_wide_kernel, dim3((N + GRUW_S - 1) / GRUW_S), dim3(GRUW_S * GRUW_U), 0, (hipStream_t)stream, N, T, dim_zm, dim_zl,
                           dim_zc, params, h0, e, labels, zc, z, saved);
    else if (dim_zm + dim_zl <= 16)
        hipLaunchKernelGGL(gru_fwd_kernel<16>, dim3((N + GRU_S - 1) / GRU_S), dim3(GRU_S * GRU_U), 0, (hipStream_t)stream, N, T, dim_zm, dim_zl, dim_zc,
                           params, h0, e, labels, zc, z, saved);
    else
        hipLaunchKernelGGL(gru_fwd_kernel<GRU_MAXIN>, dim3((N + GRU_S - 1) / GRU_S), dim3(GRU_S * GRU_U), 0, (hipStream_t)stream, N, T, dim_zm, dim_zl, dim_zc,
                           params, h0, e, labels, zc, z, saved);
    return launch_status();
}

extern "C" int mcg_gru_seq_bwd(int N, int T, int dim_zm, int dim_zl, int dim_zc, const float* params, const float* e, const int32_t* labels,
                               const float* saved, const float* gz, float* dparams, void* stream) {
    if (!params || !e || !saved || !gz || !dparams || N <= 0 || T <= 0) return MCG_ERR_BAD_ARG;
    if (dim_zm <= 0 || dim_zm > GRUW_U || dim_zl < 0 || dim_zm + dim_zl > GRUW_IN || dim_zc < 0) return MCG_ERR_UNSUPPORTED;
    if (dim_zl && !labels) return MCG_ERR_BAD_ARG;
    if (dim_zm > GRU_U || dim_zm + dim_zl > GRU_MAXIN) {
        const size_t lds = (size_t)gru_offsets(dim_zm, dim_zl).total * sizeof(float);       // <= 6 * (64 * 128 + 64) floats: 148 KB with the 8 KB of static vectors
        static std::once_flag once;
        static hipError_t attr = hipSuccess;
        std::call_once(once, [&] { attr = hipFuncSetAttribute((const void*)gru_bwd_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); });
        if (attr != hipSuccess) return MCG_ERR_LAUNCH;
        hipLaunchKernelGGL(gru_bwd_wide_kernel, dim3((N + GRUW_S - 1) / GRUW_S), dim3(GRUW_S * GRUW_U), lds, (hipStream_t)stream, N, T, dim_zm, dim_zl,
                           dim_zc, params, e, labels, saved, gz, dparams);
    } else if (dim_zm + dim_zl <= 16)
        hipLaunchKernelGGL(gru_bwd_kernel<16>, dim3((N + GRU_S - 1) / GRU_S), dim3(GRU_S * GRU_U), 0, (hipStream_t)stream, N, T, dim_zm, dim_zl, dim_zc,
                           params, e, labels, saved, gz, dparams);
    else
        hipLaunchKernelGGL(gru_bwd_kernel<GRU_MAXIN>, dim3((N + GRU_S - 1) / GRU_S), dim3(GRU_S * GRU_U), 0, (hipStream_t)stream, N, T, dim_zm, dim_zl, dim_zc,
                           params, e, labels, saved, gz, dparams);
    return launch_status();
}

extern "C" int mcg_loss_dis(int N, int C, const float* y_real, const float* y_fake, const int32_t* t_real, const int32_t* t_fake, int with_ce,
                            float* loss_out, float* g_real, float* g_fake, void* stream) {
    if (!y_real || !y_fake || !loss_out || !g_real || !g_fake || N <= 0 || C <= 0) return MCG_ERR_BAD_ARG;
    if (with_ce && (!t_real || !t_fake || C < 2)) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(loss_dis_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, N, C, y_real, y_fake, t_real, t_fake, with_ce, loss_out, g_real, g_fake);
    return launch_status();
}

extern "C" int mcg_loss_gen(int N, int C, const float* y_fake_i, const float* y_fake_v, const int32_t* t_fake, int with_ce, float* loss_out,
                            float* g_i, float* g_v, void* stream) {
    if (!y_fake_i || !y_fake_v || !loss_out || !g_i || !g_v || N <= 0 || C <= 0) return MCG_ERR_BAD_ARG;
    if (with_ce && (!t_fake || C < 2)) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(loss_gen_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, N, C, y_fake_i, y_fake_v, t_fake, with_ce, loss_out, g_i, g_v);
    return launch_status();
}

namespace {
AdamK adam_consts(double lr_t, double beta1, double beta2, double eps, double wd, double grad_scale) {
    // hyper-parameters arrive as doubles so that (1 - beta) is rounded to fp32 once, like Chainer's python-float arithmetic
    return {(float)lr_t, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)wd, (float)grad_scale};
}
bool ema_rate_ok(float r) { return r > 0.0f && r <= 1.0f; }                              // (false for a NaN)
bool overlaps(const float* a, const float* b, int64_t n) {                               // [a, a + n) and [b, b + n)
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
    return x < y + len && y < x + len;
}
}  // namespace

extern "C" int mcg_adam_wd(int64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta1, double beta2, double eps,
                           double wd, double grad_scale, uint16_t* p_bf16, void* stream) {
    if (!p || !g || !m || !v || n <= 0) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL((adam_wd_kernel<false, 1>), dim3(ew_grid(n)), dim3(NT), 0, (hipStream_t)stream, (long long)n, p, g, m, v,
                       adam_consts(lr_t, beta1, beta2, eps, wd, grad_scale), (__bf16*)p_bf16, (float*)nullptr, 0.0f);
    return launch_status();
}

extern "C" int mcg_adam_wd_ema(int64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta1, double beta2, double eps,
                               double wd, double grad_scale, uint16_t* p_bf16, float* ema, float ema_rate, void* stream) {
    if (!p || !g || !m || !v || !ema || n <= 0 || !ema_rate_ok(ema_rate)) return MCG_ERR_BAD_ARG;
    if (overlaps(ema, p, n) || overlaps(ema, g, n) || overlaps(ema, m, n) || overlaps(ema, v, n)) return MCG_ERR_BAD_ARG;
    const AdamK k = adam_consts(lr_t, beta1, beta2, eps, wd, grad_scale);
    // the ABI promises 4-byte alignment only: the 16-byte form needs every pointer on a 16-byte boundary (the bf16 copy: 8)
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | ((uintptr_t)p_bf16 << 1);
    if ((bits & 15) == 0 && n >= 4)
        hipLaunchKernelGGL((adam_wd_kernel<true, 4>), dim3(ew_grid(n / 4)), dim3(NT), 0, (hipStream_t)stream, (long long)n, p, g, m, v, k,
                           (__bf16*)p_bf16, ema, ema_rate);
    else
        hipLaunchKernelGGL((adam_wd_kernel<true, 1>), dim3(ew_grid(n)), dim3(NT), 0, (hipStream_t)stream, (long long)n, p, g, m, v, k,
                           (__bf16*)p_bf16, ema, ema_rate);
    return launch_status();
}

extern "C" int mcg_ema_multi(int nseg, const mcg_ema_seg* segs, float ema_rate, void* stream) {
    if (!segs || nseg <= 0 || nseg > MAX_EMA_SEGS || !ema_rate_ok(ema_rate)) return MCG_ERR_BAD_ARG;
    EmaSegs sg;
    int blocks = 0;
    for (int s = 0; s < nseg; ++s) {
        const mcg_ema_seg& q = segs[s];
        if (!q.src || !q.dst || q.n <= 0) return MCG_ERR_BAD_ARG;
        long long nb = (q.n + NT - 1) / NT;
        if (nb > EMA_SEG_BLOCKS) nb = EMA_SEG_BLOCKS;                 // (the rest of a long segment is grid-strided)
        blocks += (int)nb;
        sg.src[s] = q.src; sg.dst[s] = q.dst; sg.n[s] = q.n; sg.blk_end[s] = blocks;
    }
    sg.nseg = nseg;
    hipLaunchKernelGGL(ema_multi_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, sg, ema_rate);
    return launch_status();
}

extern "C" int64_t mcg_grad_stats_workspace_bytes(int nseg) {
    return nseg >= 1 && nseg <= MAX_STAT_SEGS ? (int64_t)MAX_PART * 4 * (int64_t)sizeof(double) : 0;
}

extern "C" int mcg_grad_stats_span(void) { return STAT_SPAN; }

extern "C" int mcg_grad_stats(int nseg, const mcg_stat_seg* segs, const float* g, double grad_scale, double threshold, double* stats,
                              float* ctl, void* workspace, void* stream) {
    if (!segs || !g || !stats || !ctl || !workspace || nseg < 1 || nseg > MAX_STAT_SEGS) return MCG_ERR_BAD_ARG;
    if (!(grad_scale > 0.0) || !__builtin_isfinite(grad_scale) || !(threshold > 0.0)) return MCG_ERR_BAD_ARG;      // (NaN fails both; threshold +inf: never clips)
    StatSegs sg;
    unsigned __int128 total = 0;
    for (int s = 0; s < nseg; ++s) {
        if (segs[s].n <= 0 || segs[s].offset < 0) return MCG_ERR_BAD_ARG;
        total += (unsigned __int128)segs[s].n;
    }
    // the apportioning rule (include/mocogan_hip.h): one block per segment, the other MAX_PART - nseg by size, never more than trips
    int blocks = 0;
    for (int s = 0; s < nseg; ++s) {
        const long long trips = (long long)((segs[s].n + STAT_SPAN - 1) / STAT_SPAN);
        long long nb = 1 + (long long)((unsigned __int128)(MAX_PART - nseg) * (unsigned __int128)segs[s].n / total);
        if (nb > trips) nb = trips;
        blocks += (int)nb;
        sg.off[s] = segs[s].offset; sg.n[s] = segs[s].n; sg.blk_end[s] = blocks;
    }
    sg.nseg = nseg;
    hipLaunchKernelGGL(grad_stats_partial_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, sg, g, (double*)workspace);
    hipLaunchKernelGGL(grad_stats_final_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, sg, (const double*)workspace, grad_scale, threshold,
                       stats, ctl);
    return launch_status();
}

extern "C" int mcg_adam_wd_ctl(int64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta1, double beta2, double eps,
                               double wd, const float* ctl, uint16_t* p_bf16, float* ema, float ema_rate, void* stream) {
    if (!p || !g || !m || !v || !ctl || n <= 0) return MCG_ERR_BAD_ARG;
    if (ema && (!ema_rate_ok(ema_rate) || overlaps(ema, p, n) || overlaps(ema, g, n) || overlaps(ema, m, n) || overlaps(ema, v, n))) return MCG_ERR_BAD_ARG;
    const AdamK k = adam_consts(lr_t, beta1, beta2, eps, wd, 1.0);                        // (gscale: ctl[0], read by the kernel)
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | ((uintptr_t)p_bf16 << 1);
    const bool wide = (bits & 15) == 0 && n >= 4;                                        // mcg_adam_wd_ema's rule
    const dim3 grid(ew_grid(wide ? n / 4 : n));
    auto launch = [&](auto kern, float r) {
        hipLaunchKernelGGL(kern, grid, dim3(NT), 0, (hipStream_t)stream, (long long)n, p, g, m, v, k, (__bf16*)p_bf16, ema, r, ctl);
    };
    if (ema) { if (wide) launch(adam_wd_kernel<true, 4, true>, ema_rate); else launch(adam_wd_kernel<true, 1, true>, ema_rate); }
    else     { if (wide) launch(adam_wd_kernel<false, 4, true>, 0.0f);    else launch(adam_wd_kernel<false, 1, true>, 0.0f); }
    return launch_status();
}

extern "C" int mcg_split_planes(int64_t n, int64_t run, const float* src, void* dst, void* stream) {
    if (!src || !dst || n <= 0 || run < 16 || (run & 15) || n % run) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(split_planes_kernel, dim3(ew_grid(n / 8)), dim3(NT), 0, (hipStream_t)stream, (long long)(n / 8), (long long)run, src, (__bf16*)dst);
    return launch_status();
}

extern "C" int mcg_split_planes_multi(int nseg, const mcg_split_seg* segs, void* stream) {
    if (!segs || nseg <= 0 || nseg > MAX_SPLIT_SEGS) return MCG_ERR_BAD_ARG;
    SplitSegs sg;
    int blocks = 0;
    for (int s = 0; s < nseg; ++s) {
        const mcg_split_seg& q = segs[s];
        if (!q.src || !q.dst || q.n <= 0 || q.run < 16 || (q.run & 15) || q.n % q.run) return MCG_ERR_BAD_ARG;
        long long nb = (q.n / 8 + NT - 1) / NT;
        if (nb > 512) nb = 512;                                     // (a few MB per filter: 512 blocks of a segment keep every CU busy)
        blocks += (int)nb;
        sg.src[s] = q.src; sg.dst[s] = (__bf16*)q.dst; sg.run[s] = q.run; sg.n8[s] = q.n / 8; sg.blk_end[s] = blocks;
    }
    sg.nseg = nseg;
    hipLaunchKernelGGL(split_planes_multi_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, sg);
    return launch_status();
}

extern "C" int mcg_randn_rowquad(int64_t M, int C, float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream) {
    if (!out || M <= 0 || (M & 3) || C <= 0) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(randn_rowquad_kernel, dim3(ew_grid((M / 4) * C)), dim3(NT), 0, (hipStream_t)stream, (long long)(M / 4), C, sigma, seed, stream_id, out);
    return launch_status();
}

extern "C" int mcg_randint(int64_t n, int modulus, uint64_t seed, uint64_t stream_id, int32_t* out, void* stream) {
    if (!out || n <= 0 || modulus <= 0) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(randint_kernel, dim3(ew_grid((n + 3) / 4)), dim3(NT), 0, (hipStream_t)stream, (long long)n, (uint32_t)modulus, seed, stream_id, out);
    return launch_status();
}

extern "C" int mcg_randn(int64_t n, float sigma, uint64_t seed, uint64_t stream_id, float* out, void* stream) {
    if (!out || n <= 0) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(randn_kernel, dim3(ew_grid((n + 3) / 4)), dim3(NT), 0, (hipStream_t)stream, (long long)n, sigma, seed, stream_id, out);
    return launch_status();
}

extern "C" int64_t mcg_augment_workspace_bytes(int N) { return N > 0 ? (int64_t)N * AUG_MAX_BLOCKS * (int64_t)sizeof(double) : 0; }

extern "C" int mcg_augment_draw(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, int32_t* geo, float* col, void* stream) {
    if (!geo || !col || N <= 0 || H <= 0 || W <= 0 || policy < 0 || policy > 7) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(augment_draw_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, N, H, W, policy, seed, stream_id, geo, col);
    return launch_status();
}

extern "C" int mcg_augment_draw_gated(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, uint64_t gate_stream_id,
                                      const double* ada, int32_t* geo, float* col, void* stream) {
    if (!geo || !col || !ada || N <= 0 || H <= 0 || W <= 0 || policy < 0 || policy > 7 || gate_stream_id == stream_id) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(augment_draw_gated_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, N, H, W, policy, seed, stream_id,
                       gate_stream_id, ada, geo, col);
    return launch_status();
}

extern "C" int mcg_ada_update(int N, int C, const float* y_video, const float* y_image, double target, double step, int interval, double* ada,
                              void* stream) {
    if (!y_video || !y_image || !ada || N <= 0 || C <= 0 || interval <= 0) return MCG_ERR_BAD_ARG;
    if (!(step >= 0.0) || !(target > -1.0 && target < 1.0)) return MCG_ERR_BAD_ARG;          // (a NaN fails either test)
    hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, N, C, y_video, y_image, target, step, interval, ada);
    return launch_status();
}

extern "C" int mcg_augment_fwd(int N, int C, int Cp, int T, int H, int W, const float* in, const int32_t* geo, const float* col,
                               void* workspace, float* out, void* stream) {
    if (int e = check_augment(N, C, Cp, T, H, W, in, geo, col, workspace, out)) return e;
    const int P = T * H * W;
    const AugPlan pl = plan_augment(P);
    hipLaunchKernelGGL(augment_partial_kernel<false>, dim3(pl.blocks, N), dim3(NT), 0, (hipStream_t)stream, C, P, H, W, pl.pix_per_block, in, geo,
                       (double*)workspace);
    hipLaunchKernelGGL(augment_fwd_apply_kernel, dim3(augment_apply_blocks(N, P), N), dim3(NT), 0, (hipStream_t)stream, C, P, H, W, pl.blocks,
                       1.0 / ((double)P * C), in, geo, col, (const double*)workspace, out);
    return launch_status();
}

extern "C" int mcg_augment_bwd(int N, int C, int Cp, int T, int H, int W, const float* g_out, const int32_t* geo, const float* col,
                               void* workspace, float* g_in, void* stream) {
    if (int e = check_augment(N, C, Cp, T, H, W, g_out, geo, col, workspace, g_in)) return e;
    const int P = T * H * W;
    const AugPlan pl = plan_augment(P);
    hipLaunchKernelGGL(augment_partial_kernel<true>, dim3(pl.blocks, N), dim3(NT), 0, (hipStream_t)stream, C, P, H, W, pl.pix_per_block, g_out, geo,
                       (double*)workspace);
    hipLaunchKernelGGL(augment_bwd_apply_kernel, dim3(augment_apply_blocks(N, P), N), dim3(NT), 0, (hipStream_t)stream, C, P, H, W, pl.blocks,
                       1.0 / ((double)P * C), g_out, geo, col, (const double*)workspace, g_in);
    return launch_status();
}

extern "C" int mcg_warp_fwd(int N, int C, int Cp, int T, int H, int W, const float* in, const float* mat, float* out, void* stream) {
    if (int e = check_warp(N, C, Cp, T, H, W, in, mat, out)) return e;
    const int P = T * H * W;
    hipLaunchKernelGGL(warp_fwd_kernel, dim3(augment_apply_blocks(N, P), N), dim3(NT), 0, (hipStream_t)stream, P, H, W, in, mat, out);
    return launch_status();
}

extern "C" int mcg_warp_bwd(int N, int C, int Cp, int T, int H, int W, const float* g_out, const float* mat, float* g_in, void* stream) {
    if (int e = check_warp(N, C, Cp, T, H, W, g_out, mat, g_in)) return e;
    const long long work = (long long)H * W * ((T + WARP_TC - 1) / WARP_TC);
    hipLaunchKernelGGL(warp_bwd_kernel, dim3(augment_apply_blocks(N, work), N), dim3(NT), 0, (hipStream_t)stream, T, H, W, g_out, mat, g_in);
    return launch_status();
}

extern "C" int mcg_warp_draw(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, float* mat, void* stream) {
    if (int e = check_warp_draw(N, H, W, policy, mat)) return e;
    hipLaunchKernelGGL(warp_draw_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, N, policy, seed, stream_id, mat);
    return launch_status();
}

extern "C" int mcg_warp_draw_gated(int N, int H, int W, int policy, uint64_t seed, uint64_t stream_id, uint64_t gate_stream_id,
                                   const double* ada, float* mat, void* stream) {
    if (!ada || gate_stream_id == stream_id) return MCG_ERR_BAD_ARG;
    if (int e = check_warp_draw(N, H, W, policy, mat)) return e;
    hipLaunchKernelGGL(warp_draw_gated_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, N, policy, seed, stream_id,
                       gate_stream_id, ada, mat);
    return launch_status();
}
