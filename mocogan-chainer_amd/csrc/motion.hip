// Motion and content metrics (Average Content Distance after Tulyakov et al. 2018, a temporal lag profile, motion descriptors for
// the nearest-neighbour metrics) for gfx950.  All of it reduces to squared distances between the frames OF ONE CLIP: the per-frame
// descriptors are the rows of mcg_knn_descriptors seen as [N][T][Df], and a clip's T x T matrix is a batch of tiny Gram matrices
// on the int8 matrix pipe (v_mfma_i32_16x16x64_i8, int32 accumulation; at T = 16 a clip is exactly one MFMA tile).  Every quantity
// but pair_sum is an integer and exact; pair_sum is one chain of double additions in a fixed order.  No reference counterpart (the
// reference has no metric).  No atomics, no workspace; no address depends on data; indices past an extent are clamped on load
// and never stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mocogan_hip.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int NT = 256;
constexpr int MC_WAVES = NT / 64;    // clips per workgroup of the per-wave kernels
constexpr int MC_MAX_T = 64;
constexpr int MC_MAX_DF = 3072;
constexpr int MC_MAX_ROW = 32768;    // KNN_MAX_D of knn.hip: a motion row is an operand of mcg_knn_sqdist
constexpr int MC_UNROLL = 4;         // K-steps whose loads are issued before the first of their MFMAs

int launch_status() { return hipGetLastError() == hipSuccess ? MCG_OK : MCG_ERR_LAUNCH; }

// ------------------------------------------------------------------------------------------
// Frame distances.  One wave per clip, MC_WAVES clips per workgroup, so a short clip leaves no wave idle.  With G = X X^T the Gram
// matrix of the clip's frames X [T][Df], dist[s][t] = G[s][s] + G[t][t] - 2 G[s][t]: the norms are G's diagonal, so they come out
// of the same products and the diagonal of dist is exactly 0.  T is padded to NTL = ceil(T / 16) tiles of 16 rows in registers
// only (a row past T - 1 is a second read of row T - 1); the tiles i <= j are computed and i < j is stored twice, mirrored.
// Fragments come straight from global memory: per K-step of 64 bytes lane l reads the 16 bytes k = 16 (l >> 4) .. + 15 of row
// (l & 15) of every row tile, once, and the same fragment serves as the A operand (rows of the result) and the B operand
// (columns): each byte of desc crosses HBM once, and no LDS stage is needed because nothing is shared between waves.
// Result register r of lane l is G[16 i + 4 (l >> 4) + r][16 j + (l & 15)].  |G| <= 128^2 * 3072 < 2^26.
// ------------------------------------------------------------------------------------------
template <int NTL, int U>
__device__ __forceinline__ void mc_gram_steps(const int8_t* const (&rows)[NTL], int k0, i32x4 (&acc)[NTL][NTL]) {
    i32x4 f[U][NTL];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < NTL; ++i) f[u][i] = *reinterpret_cast<const i32x4*>(rows[i] + k0 + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < NTL; ++i)
#pragma unroll
            for (int j = i; j < NTL; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(f[u][i], f[u][j], acc[i][j], 0, 0, 0);
}

template <int NTL>
__global__ __launch_bounds__(NT) void mc_frame_sqdist_kernel(int N, int T, int Df, const int8_t* __restrict__ desc, int32_t* __restrict__ dist) {
    __shared__ int nrm[MC_WAVES][16 * NTL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long clip = (long long)blockIdx.x * MC_WAVES + wave;
    const bool live = clip < N;
    const int8_t* base = desc + (live ? clip : (long long)N - 1) * T * Df;          // a wave past N reads the last clip, stores nothing
    const int fr = lane & 15, fq = lane >> 4;
    const int8_t* rows[NTL];
#pragma unroll
    for (int i = 0; i < NTL; ++i) rows[i] = base + (long long)min(16 * i + fr, T - 1) * Df + 16 * fq;
    i32x4 acc[NTL][NTL];
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int j = 0; j < NTL; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0;
    int k0 = 0;
    for (; k0 + 64 * MC_UNROLL <= Df; k0 += 64 * MC_UNROLL) mc_gram_steps<NTL, MC_UNROLL>(rows, k0, acc);
    for (; k0 < Df; k0 += 64) mc_gram_steps<NTL, 1>(rows, k0, acc);
    // the norms: element (c, c) of a diagonal tile lies in register c & 3 of lane c + 16 (c >> 2)
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (fr == 4 * fq + r) nrm[wave][16 * i + fr] = acc[i][i][r];
    __syncthreads();
    if (!live) return;                                              // (no barrier follows)
    int32_t* out = dist + clip * T * T;
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int j = i; j < NTL; ++j) {
            const int col = 16 * j + fr;
            const uint32_t ncol = (uint32_t)nrm[wave][col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + 4 * fq + r;
                if (row >= T || col >= T) continue;
                // (unsigned: the sum fits int32, its parts need not be added in a safe order)
                const int32_t d = (int32_t)((uint32_t)nrm[wave][row] + ncol - 2u * (uint32_t)acc[i][j][r]);
                out[row * T + col] = d;
                if (i != j) out[col * T + row] = d;
            }
        }
}

// ------------------------------------------------------------------------------------------
// Clip statistics.  One wave per clip.  pair_sum: per row s the lanes take the square roots of dist[s][0 .. T-1] at once, then
// every lane adds the entries t = s + 1 .. T - 1 to the one accumulator in ascending order (a broadcast per term): one chain per
// clip, the same bits for the same input.  lag_sum: lane l walks the l-th diagonal in int64.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mc_clip_stats_kernel(int N, int T, const int32_t* __restrict__ dist, double* __restrict__ pair_sum,
                                                           int64_t* __restrict__ lag_sum) {
    const int lane = threadIdx.x & 63;
    const long long clip = (long long)blockIdx.x * MC_WAVES + (threadIdx.x >> 6);
    if (clip >= N) return;                                           // (whole waves: no barrier follows)
    const int32_t* src = dist + clip * T * T;
    const int col = min(lane, T - 1);
    double sum = 0.0;
    for (int s = 0; s + 1 < T; ++s) {
        const double root = sqrt((double)src[s * T + col]);
        for (int t = s + 1; t < T; ++t) sum += __shfl(root, t, 64);
    }
    if (lane == 0) pair_sum[clip] = sum;
    if (lane < T) {
        int64_t lag = 0;
        for (int t = 0; t + lane < T; ++t) lag += src[t * T + t + lane];
        lag_sum[clip * T + lane] = lag;
    }
}

// ------------------------------------------------------------------------------------------
// Motion descriptors.  One workgroup per clip; a thread takes 16 bytes of two consecutive frames at a time.  The halved
// difference (d >> 1, arithmetic: floor(d / 2)) of two int8 lies in -128 .. 127.  The row's sum of squares (at most
// 2^14 * 32768 = 2^29) is added per thread in element order and combined by a fixed tree, as in knn_descriptors_kernel.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mc_motion_descriptors_kernel(int T, int Df, const int8_t* __restrict__ desc, int8_t* __restrict__ mdesc,
                                                                   int32_t* __restrict__ mnorms) {
    __shared__ int red[NT];
    union Bytes { i32x4 v; int8_t b[16]; };
    const int L = (T - 1) * Df;
    const int8_t* src = desc + (long long)blockIdx.x * T * Df;
    int8_t* row = mdesc + (long long)blockIdx.x * L;
    int sq = 0;
    for (int e = threadIdx.x * 16; e < L; e += NT * 16) {
        Bytes a, b, m;
        a.v = *reinterpret_cast<const i32x4*>(src + e);
        b.v = *reinterpret_cast<const i32x4*>(src + e + Df);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int v = ((int)b.b[q] - (int)a.b[q]) >> 1;
            m.b[q] = (int8_t)v;
            sq += v * v;
        }
        *reinterpret_cast<i32x4*>(row + e) = m.v;
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) mnorms[blockIdx.x] = red[0];
}

}  // namespace

extern "C" int mcg_mc_frame_sqdist(int N, int T, int Df, const int8_t* desc, int32_t* dist, void* stream) {
    if (!desc || !dist || N <= 0 || T <= 0 || Df <= 0 || ((uintptr_t)desc & 15)) return MCG_ERR_BAD_ARG;    // rows are read as 16-byte fragments
    if (T < 2 || T > MC_MAX_T || Df % 64 != 0 || Df > MC_MAX_DF) return MCG_ERR_UNSUPPORTED;
    const dim3 grid((N + MC_WAVES - 1) / MC_WAVES);
    hipStream_t s = (hipStream_t)stream;
    switch ((T + 15) / 16) {
        case 1: hipLaunchKernelGGL(mc_frame_sqdist_kernel<1>, grid, dim3(NT), 0, s, N, T, Df, desc, dist); break;
        case 2: hipLaunchKernelGGL(mc_frame_sqdist_kernel<2>, grid, dim3(NT), 0, s, N, T, Df, desc, dist); break;
        case 3: hipLaunchKernelGGL(mc_frame_sqdist_kernel<3>, grid, dim3(NT), 0, s, N, T, Df, desc, dist); break;
        default: hipLaunchKernelGGL(mc_frame_sqdist_kernel<4>, grid, dim3(NT), 0, s, N, T, Df, desc, dist); break;
    }
    return launch_status();
}

extern "C" int mcg_mc_clip_stats(int N, int T, const int32_t* dist, double* pair_sum, int64_t* lag_sum, void* stream) {
    if (!dist || !pair_sum || !lag_sum || N <= 0 || T <= 0) return MCG_ERR_BAD_ARG;
    if (T < 2 || T > MC_MAX_T) return MCG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mc_clip_stats_kernel, dim3((N + MC_WAVES - 1) / MC_WAVES), dim3(NT), 0, (hipStream_t)stream, N, T, dist, pair_sum, lag_sum);
    return launch_status();
}

extern "C" int mcg_mc_motion_descriptors(int N, int T, int Df, const int8_t* desc, int8_t* mdesc, int32_t* mnorms, void* stream) {
    if (!desc || !mdesc || !mnorms || N <= 0 || T <= 0 || Df <= 0 || (((uintptr_t)desc | (uintptr_t)mdesc) & 15)) return MCG_ERR_BAD_ARG;
    if (T < 2 || Df % 64 != 0 || (long long)(T - 1) * Df > MC_MAX_ROW) return MCG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mc_motion_descriptors_kernel, dim3(N), dim3(NT), 0, (hipStream_t)stream, T, Df, desc, mdesc, mnorms);
    return launch_status();
}
