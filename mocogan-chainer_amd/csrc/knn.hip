// Nearest-neighbour sample metrics (improved precision / recall, density / coverage, a data-copying score) for gfx950: whole-clip
// int8 descriptors of uint8 clips, every pairwise squared distance on the int8 matrix pipe (v_mfma_i32_32x32x32_i8, int32
// accumulation), the k smallest entries of every row and per-row counts inside per-column radii.  Every quantity is an integer
// and every sum fits int32 by the size limit D <= 32768 (255^2 * 32768 < 2^31), so results are exact and equal NumPy's bit for
// bit.  No reference counterpart (the reference has no metric).  No atomics; no address depends on data; rows past the end of a
// matrix are clamped on load and guarded on store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "mocogan_hip.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
constexpr int NT = 256;
constexpr int KNN_MAX_D = 32768;
constexpr int KNN_MAX_K = 16;

int launch_status() { return hipGetLastError() == hipSuccess ? MCG_OK : MCG_ERR_LAUNCH; }

// ------------------------------------------------------------------------------------------
// Descriptors.  One workgroup per clip.  Element ((t * S + y) * S + x) * C + c of a row (S = 64 / pool) is the pool x pool box
// mean of channel c rounded half up, minus 128; the row's sum of squares (at most 2^14 * 32768 = 2^29) is added per thread in
// element order and combined by a fixed tree.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void knn_descriptors_kernel(int C, int T, int pool, const uint8_t* __restrict__ clips,
                                                             int8_t* __restrict__ desc, int32_t* __restrict__ norms) {
    __shared__ int red[NT];
    const int S = 64 / pool, D = T * S * S * C, area = pool * pool;
    const uint8_t* src = clips + (long long)blockIdx.x * T * 4096 * C;
    int8_t* row = desc + (long long)blockIdx.x * D;
    int sq = 0;
    for (int e = threadIdx.x; e < D; e += NT) {
        const int c = e % C;
        int q = e / C;
        const int x = q % S; q /= S;
        const int y = q % S, t = q / S;
        const uint8_t* box = src + ((long long)(t * 64 + y * pool) * 64 + x * pool) * C + c;
        int s = 0;
        for (int dy = 0; dy < pool; ++dy)
            for (int dx = 0; dx < pool; ++dx) s += box[(dy * 64 + dx) * C];
        const int v = (2 * s + area) / (2 * area) - 128;
        row[e] = (int8_t)v;
        sq += v * v;
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) norms[blockIdx.x] = red[0];
}

// ------------------------------------------------------------------------------------------
// Squared distances.  out[i][j] = na[i] + nb[j] - 2 sum_d a[i][d] b[j][d].  A workgroup of four waves owns a 128 x 128 tile of
// out, a wave a 64 x 64 quarter as 2 x 2 MFMA tiles.  Per K-step of 64 bytes the 128 rows of a and of b go through one LDS stage
// (rows of 64 bytes at a pitch of 80, so the 16-byte fragment reads of 16 consecutive rows fall into 16 different bank groups);
// the next step's global loads are issued before the MFMAs of the current one.  Both operands are K-contiguous rows: lane l of
// a 32x32x32 product holds the 16 bytes k = 16 (l >> 5) .. + 15 of row (l & 31) of its a tile and of its b tile, and
// result register r of lane l is out[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] (a row of a, b row on the lane).
// Row indices past M / N are clamped to the last row on load (never an address outside a or b) and their results are not stored.
// ------------------------------------------------------------------------------------------
constexpr int SQ_T = 128;            // tile edge of a workgroup
constexpr int SQ_K = 64;             // bytes of K per step
constexpr int SQ_PITCH = 80;         // LDS row pitch in bytes

__global__ __launch_bounds__(NT) void knn_sqdist_kernel(int M, int N, int D, const int8_t* __restrict__ a, const int32_t* __restrict__ na,
                                                        const int8_t* __restrict__ b, const int32_t* __restrict__ nb,
                                                        int32_t* __restrict__ out, long long ld) {
    __shared__ __attribute__((aligned(16))) int8_t sa[SQ_T * SQ_PITCH], sb[SQ_T * SQ_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.y * SQ_T, col0 = blockIdx.x * SQ_T;
    // global -> LDS: thread t moves 16-byte chunk (t & 3) of tile rows (t >> 2) and (t >> 2) + 64, of a and of b
    const int lr = tid >> 2, lc = (tid & 3) * 16;
    const int8_t* ga[2];
    const int8_t* gb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ra = min(row0 + lr + 64 * h, M - 1), rb = min(col0 + lr + 64 * h, N - 1);
        ga[h] = a + (long long)ra * D + lc;
        gb[h] = b + (long long)rb * D + lc;
    }
    i32x4 pa[2], pb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        pa[h] = *reinterpret_cast<const i32x4*>(ga[h]);
        pb[h] = *reinterpret_cast<const i32x4*>(gb[h]);
    }
    i32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;          // the wave's quarter of the tile
    const int fr = lane & 31, fk = (lane >> 5) * 16;
    for (int k0 = 0; k0 < D; k0 += SQ_K) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<i32x4*>(&sa[(lr + 64 * h) * SQ_PITCH + lc]) = pa[h];
            *reinterpret_cast<i32x4*>(&sb[(lr + 64 * h) * SQ_PITCH + lc]) = pb[h];
        }
        __syncthreads();
        if (k0 + SQ_K < D) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                pa[h] = *reinterpret_cast<const i32x4*>(ga[h] + k0 + SQ_K);
                pb[h] = *reinterpret_cast<const i32x4*>(gb[h] + k0 + SQ_K);
            }
        }
#pragma unroll
        for (int s = 0; s < SQ_K / 32; ++s) {
            i32x4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const i32x4*>(&sa[(wr + 32 * i + fr) * SQ_PITCH + 32 * s + fk]);
                fb[i] = *reinterpret_cast<const i32x4*>(&sb[(wc + 32 * i + fr) * SQ_PITCH + 32 * s + fk]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = col0 + wc + 32 * j + (lane & 31);
        if (col >= N) continue;
        const uint32_t nbj = (uint32_t)nb[col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < M)                                       // (unsigned: the sum fits int32, its parts need not be added in a safe order)
                    out[(long long)row * ld + col] = (int32_t)((uint32_t)na[row] + nbj - 2u * (uint32_t)acc[i][j][r]);
            }
    }
}

// ------------------------------------------------------------------------------------------
// The k smallest of every row in ascending (value, column) order.  One wave per row.  A lane walks the columns lane, lane + 64,
// .. and keeps its KMAX smallest (value, column) pairs sorted in registers (a new pair is carried through the list by
// compare-and-swap, all indices static); as its columns ascend, a strict comparison keeps the lower column first among equal
// values.  Then k rounds: the wave-wide lexicographic minimum of the lanes' heads is the next result, and the lane that held it
// shifts its list.  An empty slot is (INT32_MAX, INT32_MAX): it loses against every real pair, and is reported as (INT32_MAX, -1).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pair_less(int v, int c, int w, int d) { return v < w || (v == w && c < d); }

template <int KMAX>
__global__ __launch_bounds__(NT) void knn_smallest_kernel(int M, int N, const int32_t* __restrict__ dist, long long ld, int k, int exclude_self,
                                                          long long self_col0, int32_t* __restrict__ val, int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= M) return;                                            // (whole waves: no barrier follows)
    const long long self = exclude_self ? self_col0 + row : -1;
    const int32_t* src = dist + (long long)row * ld;
    int v[KMAX], c[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; ++s) { v[s] = INT_MAX; c[s] = INT_MAX; }
    for (int col = lane; col < N; col += 64) {
        if (col == self) continue;
        int nv = src[col], nc = col;
        if (!pair_less(nv, nc, v[KMAX - 1], c[KMAX - 1])) continue;
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            const bool lt = pair_less(nv, nc, v[s], c[s]);
            const int tv = v[s], tc = c[s];
            v[s] = lt ? nv : tv; c[s] = lt ? nc : tc;
            nv = lt ? tv : nv; nc = lt ? tc : nc;
        }
    }
    for (int r = 0; r < k; ++r) {
        int mv = v[0], mc = c[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int ov = __shfl_xor(mv, off, 64), oc = __shfl_xor(mc, off, 64);
            const bool lt = pair_less(ov, oc, mv, mc);
            mv = lt ? ov : mv; mc = lt ? oc : mc;
        }
        if (lane == 0) {
            val[(long long)row * k + r] = mv;
            idx[(long long)row * k + r] = mc == INT_MAX ? -1 : mc;
        }
        if (mv == v[0] && mc == c[0]) {                              // the winner (or, with nothing left, every lane) shifts
#pragma unroll
            for (int s = 0; s + 1 < KMAX; ++s) { v[s] = v[s + 1]; c[s] = c[s + 1]; }
            v[KMAX - 1] = INT_MAX; c[KMAX - 1] = INT_MAX;
        }
    }
}

// counts[i] = #{j < N : dist[i][j] <= radius[j]}: one wave per row, the lanes' counts added by a butterfly
__global__ __launch_bounds__(NT) void knn_ball_counts_kernel(int M, int N, const int32_t* __restrict__ dist, long long ld,
                                                             const int32_t* __restrict__ radius, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= M) return;
    const int32_t* src = dist + (long long)row * ld;
    int n = 0;
    for (int col = lane; col < N; col += 64) n += src[col] <= radius[col] ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) counts[row] = n;
}

}  // namespace

extern "C" int mcg_knn_descriptors(int N, int C, int T, int H, int W, int pool, const uint8_t* clips, int8_t* desc, int32_t* norms, void* stream) {
    if (!clips || !desc || !norms || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C < 1 || C > 3) return MCG_ERR_BAD_ARG;
    if (pool != 2 && pool != 4 && pool != 8) return MCG_ERR_BAD_ARG;
    if (H != 64 || W != 64) return MCG_ERR_UNSUPPORTED;
    const int S = 64 / pool;
    if ((long long)T * S * S * C > KNN_MAX_D) return MCG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(knn_descriptors_kernel, dim3(N), dim3(NT), 0, (hipStream_t)stream, C, T, pool, clips, desc, norms);
    return launch_status();
}

extern "C" int mcg_knn_sqdist(int M, int N, int D, const int8_t* a, const int32_t* na, const int8_t* b, const int32_t* nb, int32_t* out,
                              int64_t ld, void* stream) {
    if (!a || !na || !b || !nb || !out || M <= 0 || N <= 0 || D <= 0 || ld < N) return MCG_ERR_BAD_ARG;
    if (D % 64 != 0 || (((uintptr_t)a | (uintptr_t)b) & 15)) return MCG_ERR_BAD_ARG;      // rows are read as 16-byte fragments
    if (D > KNN_MAX_D) return MCG_ERR_UNSUPPORTED;
    const int gy = (M + SQ_T - 1) / SQ_T;
    if (gy > 65535) return MCG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(knn_sqdist_kernel, dim3((N + SQ_T - 1) / SQ_T, gy), dim3(NT), 0, (hipStream_t)stream, M, N, D, a, na, b, nb, out,
                       (long long)ld);
    return launch_status();
}

extern "C" int mcg_knn_smallest(int M, int N, const int32_t* dist, int64_t ld, int k, int exclude_self, int64_t self_col0, int32_t* val,
                                int32_t* idx, void* stream) {
    if (!dist || !val || !idx || M <= 0 || N <= 0 || ld < N || k < 1 || k > KNN_MAX_K) return MCG_ERR_BAD_ARG;
    const dim3 grid((M + NT / 64 - 1) / (NT / 64));
    if (k <= 8)
        hipLaunchKernelGGL(knn_smallest_kernel<8>, grid, dim3(NT), 0, (hipStream_t)stream, M, N, dist, (long long)ld, k, exclude_self,
                           (long long)self_col0, val, idx);
    else
        hipLaunchKernelGGL(knn_smallest_kernel<KNN_MAX_K>, grid, dim3(NT), 0, (hipStream_t)stream, M, N, dist, (long long)ld, k, exclude_self,
                           (long long)self_col0, val, idx);
    return launch_status();
}

extern "C" int mcg_knn_ball_counts(int M, int N, const int32_t* dist, int64_t ld, const int32_t* radius, int32_t* counts, void* stream) {
    if (!dist || !radius || !counts || M <= 0 || N <= 0 || ld < N) return MCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(knn_ball_counts_kernel, dim3((M + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, (hipStream_t)stream, M, N, dist, (long long)ld,
                       radius, counts);
    return launch_status();
}
