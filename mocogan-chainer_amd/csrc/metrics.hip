// Sliced Wasserstein distance over Laplacian-pyramid patches (Karras et al. 2018, "Progressive Growing of GANs", section 5) for
// gfx950: the pyramid of uint8 clips, the patch gather, per-channel statistics and normalisation, unit random directions, the
// projection on the fp32 MFMA, a bitonic sort of every direction's row and the mean absolute difference of two sorted sets.
// No reference counterpart (the reference has no metric).  No float atomics: every sum is per-block partials added in a fixed
// order, so results are bit-reproducible run to run.  Every pass of the sort is a launch of its own: nothing waits on another
// workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "mocogan_hip.h"
#include "mcg_common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int NT = 256;
constexpr int RED_BLOCKS = 1024;     // max partial-sum blocks of the statistics and distance passes (workspace sizing)

int launch_status() { return hipGetLastError() == hipSuccess ? MCG_OK : MCG_ERR_LAUNCH; }

// ------------------------------------------------------------------------------------------
// Pyramid.  One workgroup per frame; the channels one after the other, every level of the channel in LDS (31 KB).
// f = [1,4,6,4,1]/16, boundary 'mirror' (d c b | a b c d | c b a); down = blur then [::2, ::2]; up = zero-stuff to twice the
// size then blur with 4 f (x) f -- each as two separable passes (2 f per axis for up).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ __forceinline__ float tap_w(int j) { return j == 2 ? 0.375f : ((j == 1 || j == 3) ? 0.25f : 0.0625f); }

// tmp[h][w/2] = horizontal blur of src[h][w] at the even columns
__device__ __forceinline__ void down_h(const float* src, float* tmp, int h, int w) {
    const int wo = w >> 1;
    for (int i = threadIdx.x; i < h * wo; i += NT) {
        const int y = i / wo, x = 2 * (i % wo);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) s += tap_w(j) * src[y * w + mirror(x + j - 2, w)];
        tmp[i] = s;
    }
}
// dst[h/2][wo] = vertical blur of tmp[h][wo] at the even rows
__device__ __forceinline__ void down_v(const float* tmp, float* dst, int h, int wo) {
    for (int i = threadIdx.x; i < (h >> 1) * wo; i += NT) {
        const int y = 2 * (i / wo), x = i % wo;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) s += tap_w(j) * tmp[mirror(y + j - 2, h) * wo + x];
        dst[i] = s;
    }
}
// tmp[h][2w] = horizontal pass of up(src[h][w]): the zero-stuffed row (src at the even positions) blurred with 2 f
__device__ __forceinline__ void up_h(const float* src, float* tmp, int h, int w) {
    const int w2 = 2 * w;
    for (int i = threadIdx.x; i < h * w2; i += NT) {
        const int y = i / w2, x = i % w2;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int e = mirror(x + j - 2, w2);
            if (!(e & 1)) s += tap_w(j) * src[y * w + (e >> 1)];
        }
        tmp[i] = 2.f * s;
    }
}
// value (Y, x) of the vertical pass over tmp[h][w2] (the rows of the zero-stuffed image are tmp's rows at the even positions)
__device__ __forceinline__ float up_v(const float* tmp, int h, int w2, int Y, int x) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int e = mirror(Y + j - 2, 2 * h);
        if (!(e & 1)) s += tap_w(j) * tmp[(e >> 1) * w2 + x];
    }
    return 2.f * s;
}

__global__ __launch_bounds__(NT) void swd_pyramid_kernel(int C, const uint8_t* __restrict__ clips, float* __restrict__ l64,
                                                         float* __restrict__ l32, float* __restrict__ l16) {
    __shared__ float g64[64 * 64], g32[32 * 32], g16[16 * 16], tmp[64 * 32], tmp2[32 * 16];
    const long long f = blockIdx.x;
    const uint8_t* src = clips + f * 4096 * C;
    float* o64 = l64 + f * 4096 * 4;
    float* o32 = l32 + f * 1024 * 4;
    float* o16 = l16 + f * 256 * 4;
    for (int c = 0; c < C; ++c) {
        for (int p = threadIdx.x; p < 4096; p += NT) g64[p] = (float)src[p * C + c];
        __syncthreads();
        down_h(g64, tmp, 64, 64);
        __syncthreads();
        down_v(tmp, g32, 64, 32);
        __syncthreads();
        down_h(g32, tmp2, 32, 32);
        up_h(g32, tmp, 32, 32);
        __syncthreads();
        down_v(tmp2, g16, 32, 16);
        for (int p = threadIdx.x; p < 4096; p += NT) o64[p * 4 + c] = g64[p] - up_v(tmp, 32, 64, p >> 6, p & 63);
        __syncthreads();
        up_h(g16, tmp2, 16, 16);
        if (threadIdx.x < 256) o16[threadIdx.x * 4 + c] = g16[threadIdx.x];
        __syncthreads();
        for (int p = threadIdx.x; p < 1024; p += NT) o32[p * 4 + c] = g32[p] - up_v(tmp2, 16, 32, p >> 5, p & 31);
        __syncthreads();
    }
    for (int c = C; c < 4; ++c) {                       // the pad channels hold zeros
        for (int p = threadIdx.x; p < 4096; p += NT) o64[p * 4 + c] = 0.f;
        for (int p = threadIdx.x; p < 1024; p += NT) o32[p * 4 + c] = 0.f;
        if (threadIdx.x < 256) o16[threadIdx.x * 4 + c] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------
// Gather.  Row r of the call is patch j = r % P of clip r / P; its Philox counter is first * P + r.  The position is reduced
// modulo the number of admissible positions, so every address lies inside the clip's level.
// ------------------------------------------------------------------------------------------
constexpr int GATHER_ROWS = 4;       // descriptor rows per block

__global__ __launch_bounds__(NT) void swd_gather_kernel(long long nrows, int T, int C, int hw, int P, int pt, long long first_row,
                                                        uint64_t seed, uint64_t stream_id, const float* __restrict__ level,
                                                        float* __restrict__ desc) {
    __shared__ long long origin[GATHER_ROWS];             // element offset of the patch's first pixel in `level`
    const long long r0 = (long long)blockIdx.x * GATHER_ROWS;
    if (threadIdx.x < GATHER_ROWS && r0 + threadIdx.x < nrows) {
        const long long r = r0 + threadIdx.x;
        const uint64_t ctr = (uint64_t)(first_row + r);
        uint32_t w[4];
        mcg::philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32), (uint32_t)seed,
                           (uint32_t)(seed >> 32), w);
        const int t0 = (int)(w[0] % (uint32_t)(T - pt + 1)), y0 = (int)(w[1] % (uint32_t)(hw - 6)), x0 = (int)(w[2] % (uint32_t)(hw - 6));
        origin[threadIdx.x] = ((((r / P) * T + t0) * hw + y0) * hw + x0) * 4;
    }
    __syncthreads();
    const int D = pt * 49 * C;
    for (int e = threadIdx.x; e < GATHER_ROWS * D; e += NT) {
        const int lr = e / D, k = e - lr * D;
        if (r0 + lr >= nrows) break;
        const int c = k % C;
        int q = k / C;
        const int dx = q % 7; q /= 7;
        const int dy = q % 7, dt = q / 7;
        desc[(r0 + lr) * D + k] = level[origin[lr] + ((long long)(dt * hw + dy) * hw + dx) * 4 + c];
    }
}

// per-channel (sum, sum of squares) of desc [n][D], D a multiple of C: channel of flat element i is i % C.  A thread adds its
// elements in index order, the block's threads are combined by a fixed tree, the blocks by swd_fold_kernel in a fixed order.
__global__ __launch_bounds__(NT) void swd_sums_partial_kernel(long long total, int C, const float* __restrict__ desc, double* __restrict__ part) {
    __shared__ double red[6][NT];
    double s[3] = {0, 0, 0}, q[3] = {0, 0, 0};
    const long long step = (long long)gridDim.x * NT;
    const long long i0 = (long long)blockIdx.x * NT + threadIdx.x;
    const int cstep = (int)(step % C);
    int c = (int)(i0 % C);                                   // the channel of element i is i % C, advanced without a 64-bit division
    for (long long i = i0; i < total; i += step) {
        const double v = (double)desc[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) if (c == k) { s[k] += v; q[k] += v * v; }
        c += cstep; if (c >= C) c -= C;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = s[k]; red[3 + k][threadIdx.x] = q[k]; }
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int k = 0; k < 6; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 6) part[(long long)blockIdx.x * 6 + threadIdx.x] = red[threadIdx.x][0];
}
// out[j] = scale * sum over blocks of part[b * width + src(j)], j = blockIdx.x: thread t adds the blocks t, t + NT, .. in that
// order, the threads are combined by the fixed tree
__global__ __launch_bounds__(NT) void swd_fold_kernel(int nblocks, int width, int C, double scale, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double red[NT];
    const int j = blockIdx.x;
    const int src = width == 6 ? (j < C ? j : 3 + (j - C)) : j;    // sums are [sum c < C | sum of squares c < C]
    double s = 0;
    for (int b = threadIdx.x; b < nblocks; b += NT) s += part[(long long)b * width + src];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[j] = red[0] * scale;
}

// desc <- (desc - mean_c) / std_c in double, rounded once; a constant channel (variance not above 1e-12 of the mean square) -> 0
__global__ __launch_bounds__(NT) void swd_normalize_kernel(long long total, int C, double inv_count, const double* __restrict__ sums, float* __restrict__ desc) {
    double mean[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
    for (int c = 0; c < C; ++c) {
        const double m = sums[c] * inv_count, ms = sums[C + c] * inv_count, var = ms - m * m;
        mean[c] = m;
        inv[c] = var > 1e-12 * ms ? 1.0 / sqrt(var) : 0.0;
    }
    const long long step = (long long)gridDim.x * NT;
    const long long i0 = (long long)blockIdx.x * NT + threadIdx.x;
    const int cstep = (int)(step % C);
    int c = (int)(i0 % C);
    for (long long i = i0; i < total; i += step) {
        const double m = c == 0 ? mean[0] : c == 1 ? mean[1] : mean[2], s = c == 0 ? inv[0] : c == 1 ? inv[1] : inv[2];
        desc[i] = (float)(((double)desc[i] - m) * s);
        c += cstep; if (c >= C) c -= C;
    }
}

// every column of dirs [D][K] to unit L2 norm (norm in double, each element rounded once)
__global__ __launch_bounds__(NT) void swd_unit_columns_kernel(int D, int K, float* __restrict__ dirs) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= K) return;
    double s = 0;
    for (int d = 0; d < D; ++d) { const double v = (double)dirs[(long long)d * K + j]; s += v * v; }
    const double inv = s > 0 ? 1.0 / sqrt(s) : 0.0;
    for (int d = 0; d < D; ++d) dirs[(long long)d * K + j] = (float)((double)dirs[(long long)d * K + j] * inv);
}

// ------------------------------------------------------------------------------------------
// Projection on v_mfma_f32_32x32x2_f32: out[dir][row] = sum_d dirs[d][dir] * desc[row][d], i.e. the product dirs^T x desc^T, so
// that the accumulator's lane index runs along `row` and a direction's values are stored as contiguous 128-byte runs.
// Block tile 128 directions x 128 rows, four waves of 2 x 2 MFMA tiles, D in chunks of 32 through LDS; rows, directions and the
// D tail outside the matrices are zero-filled on load and never stored.
// ------------------------------------------------------------------------------------------
constexpr int PJ_T = 128, PJ_KC = 32, PJ_LD = PJ_T + 2;

__global__ __launch_bounds__(NT) void swd_project_kernel(long long n, int D, int K, const float* __restrict__ desc,
                                                         const float* __restrict__ dirs, float* __restrict__ out, long long n_stride) {
    __shared__ float sa[PJ_KC][PJ_T];        // sa[k][dir]
    __shared__ float sb[PJ_KC][PJ_LD];       // sb[k][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 31, h = lane >> 5;
    const long long row0 = (long long)blockIdx.x * PJ_T;
    const int dir0 = blockIdx.y * PJ_T;
    const int wd = (wave & 1) * 64, wr = (wave >> 1) * 64;
    f32x16 acc[2][2] = {};
    constexpr int PER = PJ_KC * PJ_T / NT;          // elements of each operand's chunk per thread
    float ra[PER], rb[PER];
    // chunk d0 of both operands into registers: the loads of the next chunk are in flight under the MFMAs of the current one
    auto fetch = [&](int d0) {
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int i = tid + e * NT;
            const int ka = i / PJ_T, j = i % PJ_T, da = d0 + ka, dir = dir0 + j;
            ra[e] = (da < D && dir < K) ? dirs[(long long)da * K + dir] : 0.f;
            const int r = i / PJ_KC, kb = i % PJ_KC, db = d0 + kb;
            const long long row = row0 + r;
            rb[e] = (row < n && db < D) ? desc[row * D + db] : 0.f;
        }
    };
    fetch(0);
    for (int d0 = 0; d0 < D; d0 += PJ_KC) {
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int i = tid + e * NT;
            sa[i / PJ_T][i % PJ_T] = ra[e];
            sb[i % PJ_KC][i / PJ_KC] = rb[e];
        }
        __syncthreads();
        if (d0 + PJ_KC < D) fetch(d0 + PJ_KC);
#pragma unroll 4
        for (int k = 0; k < PJ_KC; k += 2) {
            const float a0 = sa[k + h][wd + l], a1 = sa[k + h][wd + 32 + l];
            const float b0 = sb[k + h][wr + l], b1 = sb[k + h][wr + 32 + l];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const long long row = row0 + wr + 32 * b + l;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dir = dir0 + wd + 32 * a + 8 * (r >> 2) + 4 * h + (r & 3);
                if (dir < K && row < n) out[(long long)dir * n_stride + row] = acc[a][b][r];
            }
        }
}

// ------------------------------------------------------------------------------------------
// Bitonic sort of independent rows.  Values are compared as keys: the bit pattern with the magnitude bits of negative values
// inverted, a signed integer that orders like the value for everything finite or infinite and is a TOTAL order of all bit
// patterns (-NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN).  The row is seen padded to a power of two n2 with the largest key
// (0x7fffffff), so the first n elements of the sorted padded row are the row's own bit patterns whatever they hold (a float
// comparison is false both ways for a NaN: next to +inf padding it put padding into the first n places and elements out of them).
// Steps with a partner distance below SORT_L run on a span of SORT_L elements in LDS (one launch for all of them); the steps with a larger distance are launches of
// their own over the padded rows in the workspace, two steps to a launch where both are that wide.  Element i's partner in step j is i ^ j, its direction in stage k is ascending where
// (i & k) == 0: indices depend on nothing but (i, j, k), so no value (NaN included) can move an access.
// ------------------------------------------------------------------------------------------
constexpr int SORT_L = 8192;

constexpr int SORT_PAD = 0x7fffffff;  // the largest key

// a value's bit pattern -> its key, and back: the map is its own inverse.  The kernels see the rows as ints: no float is formed.
__device__ __forceinline__ int sort_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

__device__ __forceinline__ void cmpx(int& a, int& b, bool asc) {
    if ((a > b) == asc) { const int t = a; a = b; b = t; }
}

// full != 0: sorts each span (stages 2 .. span; span `b` ascending where (b * span & span) == 0 -- the next stage's input);
// full == 0: the steps j = span / 2 .. 1 of stage `stage`.  Reads elements below n_src of src (others the pad key), writes those
// below n_dst.  LDS and the workspace hold keys, the caller's rows values: src_values / dst_values say which of the two src and
// dst are (so a value is converted once on its way in and once on its way out, whatever the number of launches).
__global__ __launch_bounds__(NT) void sort_local_kernel(const int* src, long long src_stride, int n_src, int src_values, int* dst,
                                                        long long dst_stride, int n_dst, int dst_values, int span, int stage, int full) {
    __shared__ int s[SORT_L];
    const int base = blockIdx.x * span;
    const int* in = src + (long long)blockIdx.y * src_stride;
    int* o = dst + (long long)blockIdx.y * dst_stride;
    for (int i = threadIdx.x; i < span; i += NT) {
        int k = SORT_PAD;
        if (base + i < n_src) { k = in[base + i]; if (src_values) k = sort_key(k); }
        s[i] = k;
    }
    __syncthreads();
    auto step = [&](int k, int j) {
        for (int p = threadIdx.x; p < (span >> 1); p += NT) {
            const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
            cmpx(s[i], s[i | j], ((base + i) & k) == 0);
        }
        __syncthreads();
    };
    if (full) {
        for (int k = 2; k <= span; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) step(k, j);
    } else {
        for (int j = span >> 1; j > 0; j >>= 1) step(stage, j);
    }
    for (int i = threadIdx.x; i < span; i += NT) if (base + i < n_dst) o[base + i] = dst_values ? sort_key(s[i]) : s[i];
}

// one step with partner distance j >= SORT_L of stage k over the padded rows' keys ws [rows][n2]; a thread owns 4 consecutive pairs
__global__ __launch_bounds__(NT) void sort_global_kernel(int* __restrict__ ws, int n2, int k, int j) {
    const int p = 4 * (blockIdx.x * NT + threadIdx.x);
    if (p >= (n2 >> 1)) return;
    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
    int* row = ws + (long long)blockIdx.y * n2;
    i32x4 a = *reinterpret_cast<const i32x4*>(row + i), b = *reinterpret_cast<const i32x4*>(row + i + j);
    const bool asc = (i & k) == 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int x = a[e], y = b[e];
        cmpx(x, y, asc);
        a[e] = x; b[e] = y;
    }
    *reinterpret_cast<i32x4*>(row + i) = a;
    *reinterpret_cast<i32x4*>(row + i + j) = b;
}

// the two steps j and j / 2 (both >= SORT_L) of stage k in one pass: the four elements i, i + j/2, i + j, i + 3j/2 (i with zero
// bits at j and j / 2) exchange among themselves only; a thread owns 4 consecutive such quadruples
__global__ __launch_bounds__(NT) void sort_global2_kernel(int* __restrict__ ws, int n2, int k, int j) {
    const int p = 4 * (blockIdx.x * NT + threadIdx.x), h = j >> 1;
    if (p >= (n2 >> 2)) return;
    const int i = ((p & ~(h - 1)) << 2) | (p & (h - 1));
    int* row = ws + (long long)blockIdx.y * n2;
    i32x4 v0 = *reinterpret_cast<const i32x4*>(row + i), v1 = *reinterpret_cast<const i32x4*>(row + i + h);
    i32x4 v2 = *reinterpret_cast<const i32x4*>(row + i + j), v3 = *reinterpret_cast<const i32x4*>(row + i + j + h);
    const bool asc = (i & k) == 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int a = v0[e], b = v1[e], c = v2[e], d = v3[e];
        cmpx(a, c, asc); cmpx(b, d, asc);         // step j
        cmpx(a, b, asc); cmpx(c, d, asc);         // step j / 2
        v0[e] = a; v1[e] = b; v2[e] = c; v3[e] = d;
    }
    *reinterpret_cast<i32x4*>(row + i) = v0;
    *reinterpret_cast<i32x4*>(row + i + h) = v1;
    *reinterpret_cast<i32x4*>(row + i + j) = v2;
    *reinterpret_cast<i32x4*>(row + i + j + h) = v3;
}

int pow2_at_least(long long n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// part[block] = sum of |a - b| over the block's elements (differences and sums in double; thread, tree and block order fixed)
__global__ __launch_bounds__(NT) void swd_distance_partial_kernel(int K, long long n, const float* __restrict__ a, long long a_stride,
                                                                  const float* __restrict__ b, long long b_stride, double* __restrict__ part) {
    __shared__ double red[NT];
    double s = 0;
    const long long step = (long long)gridDim.x * NT;
    for (int k = 0; k < K; ++k) {
        const float* ak = a + k * a_stride;
        const float* bk = b + k * b_stride;
        for (long long r = (long long)blockIdx.x * NT + threadIdx.x; r < n; r += step) s += fabs((double)ak[r] - (double)bk[r]);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

int red_blocks(long long total) {
    const long long b = (total + NT - 1) / NT;
    return (int)(b > RED_BLOCKS ? RED_BLOCKS : b);
}

constexpr long long SWD_MAX_ROWS = 1LL << 30;     // row indices inside the kernels are ints

}  // namespace

extern "C" int mcg_sort_local_span(void) { return SORT_L; }

extern "C" int64_t mcg_swd_workspace_bytes(int64_t n, int D, int rows) {
    if (n < 1 || D < 1 || rows < 1 || n > SWD_MAX_ROWS) return 0;
    int64_t bytes = (int64_t)RED_BLOCKS * 6 * sizeof(double);                 // statistics partials (the distance needs fewer)
    if (n > SORT_L) {
        const int64_t sort = (int64_t)rows * pow2_at_least(n) * (int64_t)sizeof(float);
        if (sort > bytes) bytes = sort;
    }
    return (bytes + 15) / 16 * 16;
}

extern "C" int mcg_swd_pyramid(int N, int C, int T, int H, int W, const uint8_t* clips, float* l64, float* l32, float* l16, void* stream) {
    if (!clips || !l64 || !l32 || !l16 || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C < 1 || C > 3) return MCG_ERR_BAD_ARG;
    if (H != 64 || W != 64) return MCG_ERR_UNSUPPORTED;
    if ((long long)N * T > 0x7fffffffLL) return MCG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(swd_pyramid_kernel, dim3(N * T), dim3(NT), 0, (hipStream_t)stream, C, clips, l64, l32, l16);
    return launch_status();
}

extern "C" int mcg_swd_gather(int N, int C, int T, int hw, const float* level, int64_t first_clip, int P, int pt, uint64_t seed,
                              uint64_t stream_id, float* desc, void* stream) {
    if (!level || !desc || N <= 0 || T <= 0 || C < 1 || C > 3 || P <= 0 || pt <= 0 || first_clip < 0) return MCG_ERR_BAD_ARG;
    if (pt > T) return MCG_ERR_BAD_ARG;
    if (hw != 64 && hw != 32 && hw != 16) return MCG_ERR_UNSUPPORTED;
    const long long nrows = (long long)N * P;
    if (nrows > SWD_MAX_ROWS || (first_clip + N) > (1LL << 40) / P || (long long)pt * 49 * C > 4096) return MCG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(swd_gather_kernel, dim3((unsigned)((nrows + GATHER_ROWS - 1) / GATHER_ROWS)), dim3(NT), 0, (hipStream_t)stream, nrows, T, C,
                       hw, P, pt, (long long)first_clip * P, seed, stream_id, level, desc);
    return launch_status();
}

namespace {
int check_matrix(int64_t n, int D, int C) {
    if (n < 1 || D < 1 || C < 1 || C > 3 || D % C != 0) return MCG_ERR_BAD_ARG;
    if (n > SWD_MAX_ROWS) return MCG_ERR_UNSUPPORTED;
    return MCG_OK;
}
}  // namespace

extern "C" int mcg_swd_channel_sums(int64_t n, int D, int C, const float* desc, double* sums, void* workspace, void* stream) {
    if (!desc || !sums || !workspace) return MCG_ERR_BAD_ARG;
    if (int e = check_matrix(n, D, C)) return e;
    const long long total = (long long)n * D;
    const int blocks = red_blocks(total);
    hipLaunchKernelGGL(swd_sums_partial_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, total, C, desc, (double*)workspace);
    hipLaunchKernelGGL(swd_fold_kernel, dim3(2 * C), dim3(NT), 0, (hipStream_t)stream, blocks, 6, C, 1.0, (const double*)workspace, sums);
    return launch_status();
}

extern "C" int mcg_swd_normalize(int64_t n, int D, int C, float* desc, const double* sums, void* stream) {
    if (!desc || !sums) return MCG_ERR_BAD_ARG;
    if (int e = check_matrix(n, D, C)) return e;
    const long long total = (long long)n * D;
    const long long b = (total + NT - 1) / NT;
    hipLaunchKernelGGL(swd_normalize_kernel, dim3((unsigned)(b > 8192 ? 8192 : b)), dim3(NT), 0, (hipStream_t)stream, total, C,
                       1.0 / ((double)total / C), sums, desc);
    return launch_status();
}

extern "C" int mcg_swd_unit_columns(int D, int K, float* dirs, void* stream) {
    if (!dirs || D < 1 || K < 1) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(swd_unit_columns_kernel, dim3((K + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, D, K, dirs);
    return launch_status();
}

extern "C" int mcg_swd_project(int64_t n, int D, int K, const float* desc, const float* dirs, float* out, int64_t n_stride, void* stream) {
    if (!desc || !dirs || !out || n < 1 || D < 1 || K < 1 || n_stride < n) return MCG_ERR_BAD_ARG;
    if (n > SWD_MAX_ROWS || (K + PJ_T - 1) / PJ_T > 65535) return MCG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(swd_project_kernel, dim3((unsigned)((n + PJ_T - 1) / PJ_T), (K + PJ_T - 1) / PJ_T), dim3(NT), 0, (hipStream_t)stream,
                       (long long)n, D, K, desc, dirs, out, (long long)n_stride);
    return launch_status();
}

extern "C" int mcg_sort_rows(int rows, int64_t n, float* data, int64_t row_stride, void* workspace, void* stream) {
    if (!data || rows < 1 || n < 1 || row_stride < n) return MCG_ERR_BAD_ARG;
    if (rows > 65535 || n > SWD_MAX_ROWS) return MCG_ERR_UNSUPPORTED;
    if (n == 1) return MCG_OK;
    const int n2 = pow2_at_least(n);
    hipStream_t st = (hipStream_t)stream;
    int* rows_bits = reinterpret_cast<int*>(data);
    if (n2 <= SORT_L) {
        hipLaunchKernelGGL(sort_local_kernel, dim3(1, rows), dim3(NT), 0, st, rows_bits, (long long)row_stride, (int)n, 1, rows_bits,
                           (long long)row_stride, (int)n, 1, n2, 0, 1);
        return launch_status();
    }
    if (!workspace || ((uintptr_t)workspace & 15)) return MCG_ERR_BAD_ARG;
    int* ws = (int*)workspace;                                  // the padded rows' keys
    const dim3 lgrid(n2 / SORT_L, rows), ggrid(n2 / 8 / NT, rows), g2grid(n2 / 16 / NT, rows);
    hipLaunchKernelGGL(sort_local_kernel, lgrid, dim3(NT), 0, st, rows_bits, (long long)row_stride, (int)n, 1, ws, (long long)n2, n2, 0,
                       SORT_L, 0, 1);
    for (long long k = 2LL * SORT_L; k <= n2; k <<= 1) {
        for (int j = (int)(k >> 1); j >= SORT_L;) {
            if ((j >> 1) >= SORT_L) {
                hipLaunchKernelGGL(sort_global2_kernel, g2grid, dim3(NT), 0, st, ws, n2, (int)k, j);
                j >>= 2;
            } else {
                hipLaunchKernelGGL(sort_global_kernel, ggrid, dim3(NT), 0, st, ws, n2, (int)k, j);
                j >>= 1;
            }
        }
        const bool last = k == n2;
        hipLaunchKernelGGL(sort_local_kernel, lgrid, dim3(NT), 0, st, ws, (long long)n2, n2, 0, last ? rows_bits : ws,
                           last ? (long long)row_stride : (long long)n2, last ? (int)n : n2, last ? 1 : 0, SORT_L, (int)k, 0);
    }
    return launch_status();
}

extern "C" int mcg_swd_distance(int K, int64_t n_a, int64_t n_b, const float* a, int64_t a_stride, const float* b, int64_t b_stride,
                                double* out, void* workspace, void* stream) {
    if (!a || !b || !out || !workspace || K < 1 || n_a < 1 || n_b < 1 || a_stride < n_a || b_stride < n_b) return MCG_ERR_BAD_ARG;
    if (n_a != n_b) return MCG_ERR_BAD_ARG;                 // the rank-wise comparison needs sets of one size
    if (n_a > SWD_MAX_ROWS) return MCG_ERR_UNSUPPORTED;
    const long long total = (long long)K * n_a;
    const int blocks = red_blocks(n_a);
    hipLaunchKernelGGL(swd_distance_partial_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, K, (long long)n_a, a, (long long)a_stride,
                       b, (long long)b_stride, (double*)workspace);
    hipLaunchKernelGGL(swd_fold_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, blocks, 1, 1, 1.0 / (double)total, (const double*)workspace, out);
    return launch_status();
}
