// dsvd_kernels.hip -- compression of a simulated dictionary to its SVD subspace: an EXTENSION with no reference counterpart (the reference loads
// dictionaries that are already compressed, main_recon_tsmis_FFT.m:121-130).  Definition: include/qmri.h, DESIGN.md section 18.
//
// F is K x T real, column-major (frame t contiguous over the atoms), fp64 or fp32.
//   k_dsvd_gram         G = F^T F on v_mfma_f64_16x16x4_f64.  A workgroup (4 waves) owns a GB x GB = 64 x 64 tile of G and one chunk of GCH atoms; only
//                       block pairs bi <= bj are computed.  The reduction runs along K, F's contiguous axis, so a lane's A / B element (A[i][k]: frame
//                       i, atom k) sits a whole column away from its neighbour's: GKC atoms of the two 64-frame panels are staged in LDS with 16-byte
//                       loads along K (fp32 input: 8-byte loads, widened on the way) and the fragments are read from LDS.  Row stride GLD = GKC + 4
//                       doubles: the 16 frames x 4 atoms a fragment read touches fall in distinct banks.  The next stage's loads are issued before the
//                       products of the current one.  Each wave keeps a 32 x 32 sub-tile: 2 x 2 accumulators of 4 doubles.
//                       C/D map of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg (NOT the f32 forms' 4 * (lane >> 4) + reg).
//   k_dsvd_gram_reduce  adds the partial tiles in chunk order, writes both triangles of G and its diagonal
//   k_dsvd_gq           Z = G Q for the subspace iteration (one wave per row of G; G is symmetric, so row i is the contiguous column i)
//   k_dsvd_project      Dc = F V, normD, D: one pass over F.  A lane owns two atoms and keeps PS = 4, 8, 12 or 16 >= s accumulators for each (V is
//                       zero-padded to PS columns in LDS, PTC frames at a time), frames ascending.
// No floating-point atomics; the chunking is a constant, every sum has one order: equal inputs give equal bits.
#include <algorithm>
#include <cstdint>
#include <type_traits>
#include "qmri_internal.h"

namespace {
constexpr int NT = 256;          // threads per workgroup
constexpr int GB = 64;           // frames per side of a workgroup's tile of G
constexpr int GKC = 32;          // atoms per LDS stage
constexpr int GLD = GKC + 4;     // LDS row stride in doubles (288 B: 16-byte aligned rows, conflict-free fragment reads)
constexpr int GCH = 2048;        // atoms per split-K chunk
constexpr int PTC = 128;         // frames of V per LDS chunk of the projection (16 KB)
constexpr int QB = 24;           // widest block of the subspace iteration (16 + 8)

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void pair_of(int p, int n, int& i, int& j) {       // p-th entry of the upper triangle, row by row
    i = 0;
    while (p >= n - i) { p -= n - i; ++i; }
    j = i + p;
}

// two consecutive atoms (k, k + 1) of frame t, zero outside the matrix; vec: k + t * K is even and the base is aligned for the wide load
template <typename TF> __device__ __forceinline__ double2 load2(const TF* __restrict__ F, int K, int T, int t, int k, bool vec);
template <> __device__ __forceinline__ double2 load2<double>(const double* __restrict__ F, int K, int T, int t, int k, bool vec) {
    if (t >= T || k >= K) return make_double2(0.0, 0.0);
    const size_t o = (size_t)t * K + k;
    if (vec && k + 1 < K) return *reinterpret_cast<const double2*>(F + o);
    return make_double2(F[o], k + 1 < K ? F[o + 1] : 0.0);
}
template <> __device__ __forceinline__ double2 load2<float>(const float* __restrict__ F, int K, int T, int t, int k, bool vec) {
    if (t >= T || k >= K) return make_double2(0.0, 0.0);
    const size_t o = (size_t)t * K + k;
    if (vec && k + 1 < K) { const float2 v = *reinterpret_cast<const float2*>(F + o); return make_double2((double)v.x, (double)v.y); }
    return make_double2((double)F[o], k + 1 < K ? (double)F[o + 1] : 0.0);
}

// grid: (block pairs of the upper triangle, chunks).  part[(chunk * npairs + pair) * GB * GB + i * GB + j]
template <typename TF>
__global__ void __launch_bounds__(NT) k_dsvd_gram(const TF* __restrict__ F, int K, int T, int nblk, int vec, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double As[GB * GLD];
    __shared__ __attribute__((aligned(16))) double Bs[GB * GLD];
    int bi, bj;
    pair_of(blockIdx.x, nblk, bi, bj);
    const bool diag = bi == bj;
    const int ti0 = bi * GB, tj0 = bj * GB;
    const int kbeg = blockIdx.y * GCH, kend = min(K, kbeg + GCH);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, li = lane & 15, lh = lane >> 4;
    const int lf = tid >> 4, lk = 2 * (tid & 15);             // this thread's frame (+ 16 r) and atom pair of a stage
    const double* Bp = diag ? As : Bs;

    d4 acc[2][2];
    for (int m = 0; m < 2; ++m)
        for (int n = 0; n < 2; ++n) acc[m][n] = (d4){0.0, 0.0, 0.0, 0.0};

    double2 ra[4], rb[4];
    auto fetch = [&](int k0) {
        for (int r = 0; r < 4; ++r) {
            ra[r] = load2<TF>(F, K, T, ti0 + lf + 16 * r, k0 + lk, vec);
            if (!diag) rb[r] = load2<TF>(F, K, T, tj0 + lf + 16 * r, k0 + lk, vec);
        }
    };
    fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += GKC) {
        for (int r = 0; r < 4; ++r) {
            *reinterpret_cast<double2*>(&As[(lf + 16 * r) * GLD + lk]) = ra[r];
            if (!diag) *reinterpret_cast<double2*>(&Bs[(lf + 16 * r) * GLD + lk]) = rb[r];
        }
        __syncthreads();
        if (k0 + GKC < kend) fetch(k0 + GKC);
#pragma unroll
        for (int kk = 0; kk < GKC; kk += 4) {
            const double a0 = As[(wr * 32 + li) * GLD + kk + lh], a1 = As[(wr * 32 + 16 + li) * GLD + kk + lh];
            const double b0 = Bp[(wc * 32 + li) * GLD + kk + lh], b1 = Bp[(wc * 32 + 16 + li) * GLD + kk + lh];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    double* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (GB * GB);
    for (int m = 0; m < 2; ++m)
        for (int n = 0; n < 2; ++n)
            for (int r = 0; r < 4; ++r) {
                const int i = wr * 32 + m * 16 + lh + 4 * r, j = wc * 32 + n * 16 + li;      // the f64 C/D map
                out[i * GB + j] = acc[m][n][r];
            }
}

// grid: (GB * GB / NT, block pairs)
__global__ void __launch_bounds__(NT) k_dsvd_gram_reduce(const double* __restrict__ part, int T, int nblk, int npairs, int nchunks, double* __restrict__ G,
                                                         double* __restrict__ diag) {
    int bi, bj;
    pair_of(blockIdx.y, nblk, bi, bj);
    const int e = blockIdx.x * NT + threadIdx.x, i = e / GB, j = e % GB;
    const int gi = bi * GB + i, gj = bj * GB + j;
    if (gi >= T || gj >= T) return;
    double v = 0.0;
    for (int c = 0; c < nchunks; ++c) v += part[((size_t)c * npairs + blockIdx.y) * (GB * GB) + e];
    G[gi + (size_t)gj * T] = v;
    if (bi != bj) G[gj + (size_t)gi * T] = v;
    if (gi == gj) diag[gi] = v;
}

// Z[i, c] = sum_j G[j, i] Q[j, c]: one wave per row i, lane l takes j = l, l + 64, ...; then a fixed xor tree over the lanes
__global__ void __launch_bounds__(NT) k_dsvd_gq(const double* __restrict__ G, const double* __restrict__ Q, int T, int b, double* __restrict__ Z) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (i >= T) return;
    double acc[QB];
#pragma unroll
    for (int c = 0; c < QB; ++c) acc[c] = 0.0;
    const double* g = G + (size_t)i * T;
    for (int j = lane; j < T; j += 64) {
        const double gv = g[j];
#pragma unroll
        for (int c = 0; c < QB; ++c)
            if (c < b) acc[c] = fma(gv, Q[j + (size_t)c * T], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < QB; ++c) {
        double v = acc[c];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0 && c < b) Z[i + (size_t)c * T] = v;
    }
}

// grid: ceil(K / (2 NT)).  A lane owns atoms k and k + NT of its workgroup's 2 NT.  PS: columns carried (s rounded up to 4, 8, 12 or 16).
template <typename TF, int PS>
__global__ void __launch_bounds__(NT) k_dsvd_project(const TF* __restrict__ F, int K, int T, int s, const double* __restrict__ V, float* __restrict__ D,
                                                     float* __restrict__ normD) {
    __shared__ __attribute__((aligned(16))) double Vs[PTC * PS];       // [frame][column]
    const long long kb = (long long)blockIdx.x * (2 * NT) + threadIdx.x;
    const bool in0 = kb < K, in1 = kb + NT < K;
    const TF* f0 = F + (in0 ? kb : 0);
    const TF* f1 = F + (in1 ? kb + NT : 0);
    double a0[PS], a1[PS];
#pragma unroll
    for (int c = 0; c < PS; ++c) a0[c] = a1[c] = 0.0;
    for (int t0 = 0; t0 < T; t0 += PTC) {
        __syncthreads();
        for (int e = threadIdx.x; e < PTC * PS; e += NT) {
            const int tt = e / PS, c = e % PS;
            Vs[e] = (t0 + tt < T && c < s) ? V[t0 + tt + (size_t)c * T] : 0.0;
        }
        __syncthreads();
        const int nt = min(PTC, T - t0);
#pragma unroll 4
        for (int tt = 0; tt < nt; ++tt) {
            const size_t o = (size_t)(t0 + tt) * K;
            const double x0 = in0 ? (double)f0[o] : 0.0, x1 = in1 ? (double)f1[o] : 0.0;
#pragma unroll
            for (int c = 0; c < PS; ++c) {
                const double v = Vs[tt * PS + c];
                a0[c] = fma(x0, v, a0[c]);
                a1[c] = fma(x1, v, a1[c]);
            }
        }
    }
    for (int h = 0; h < 2; ++h) {
        if (!(h ? in1 : in0)) continue;
        const long long k = kb + (h ? NT : 0);
        double n2 = 0.0;
#pragma unroll
        for (int c = 0; c < PS; ++c) { const double a = h ? a1[c] : a0[c]; n2 = fma(a, a, n2); }       // (columns >= s hold exact zeros)
        const double nrm = sqrt(n2);
        normD[k] = (float)nrm;
#pragma unroll
        for (int c = 0; c < PS; ++c)
            if (c < s) D[k + (size_t)c * K] = nrm > 0.0 ? (float)((h ? a1[c] : a0[c]) / nrm) : 0.0f;
    }
}
}  // namespace

int dsvd_gram_chunk() { return GCH; }

size_t dsvd_gram_scratch(int K, int T) {
    const size_t nblk = (T + GB - 1) / GB, npairs = nblk * (nblk + 1) / 2, nchunks = ((size_t)K + GCH - 1) / GCH;
    return npairs * nchunks * GB * GB;
}

int dsvd_gram_dev(qmri_ctx* ctx, int K, int T, const void* d_F, bool f64, double* d_part, double* d_G, double* d_diag) {
    const int nblk = (T + GB - 1) / GB, npairs = nblk * (nblk + 1) / 2, nchunks = (K + GCH - 1) / GCH;
    const int vec = K % 2 == 0 && (uintptr_t)d_F % (f64 ? 16 : 8) == 0;      // the wide loads need every column to start aligned
    const dim3 grid(npairs, nchunks);
    if (f64) k_dsvd_gram<double><<<grid, NT, 0, ctx->stream>>>((const double*)d_F, K, T, nblk, vec, d_part);
    else k_dsvd_gram<float><<<grid, NT, 0, ctx->stream>>>((const float*)d_F, K, T, nblk, vec, d_part);
    QMRI_HIP(ctx, hipGetLastError());
    k_dsvd_gram_reduce<<<dim3(GB * GB / NT, npairs), NT, 0, ctx->stream>>>(d_part, T, nblk, npairs, nchunks, d_G, d_diag);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int dsvd_gq_dev(qmri_ctx* ctx, int T, int b, const double* d_G, const double* d_Q, double* d_Z) {
    if (b < 1 || b > QB) { qmri_set_error(ctx, "internal: subspace block %d outside 1..%d", b, QB); return QMRI_ERR_INVALID_ARG; }
    k_dsvd_gq<<<(T + NT / 64 - 1) / (NT / 64), NT, 0, ctx->stream>>>(d_G, d_Q, T, b, d_Z);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int dsvd_project_dev(qmri_ctx* ctx, int K, int T, int s, const void* d_F, bool f64, const double* d_V, float* d_D, float* d_normD) {
    const unsigned grid = (unsigned)(((long long)K + 2 * NT - 1) / (2 * NT));
    auto go = [&](auto tf, auto ps) {
        using TF = decltype(tf);
        k_dsvd_project<TF, decltype(ps)::value><<<grid, NT, 0, ctx->stream>>>((const TF*)d_F, K, T, s, d_V, d_D, d_normD);
    };
    auto by_s = [&](auto tf) {
        if (s <= 4) go(tf, std::integral_constant<int, 4>());
        else if (s <= 8) go(tf, std::integral_constant<int, 8>());
        else if (s <= 12) go(tf, std::integral_constant<int, 12>());
        else go(tf, std::integral_constant<int, 16>());
    };
    if (f64) by_s(double()); else by_s(float());
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
