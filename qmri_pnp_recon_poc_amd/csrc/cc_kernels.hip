// cc_kernels.hip -- software coil compression and noise pre-whitening of multi-coil stacks: an EXTENSION with no reference counterpart (the
// reference is single-coil, README.md:63), like mc_kernels.hip whose stacks it feeds.  Definition: DESIGN.md section 13, "Coil compression".
//
// For one slice (or one stack, shared mode) with data y [ncoil][m] and an optional noise covariance Psi = L L^H:
//     K = sum_i  L^-1 y_i (L^-1 y_i)^H,   K = U diag(lambda) U^H (host: cc_eig_host, api_cc.cpp),   W = L^-H U_nv,   y' = W^H y,  maps' = W^H C.
// The whitening is fused, not a pass of its own over y: the covariance pass sums R = sum_i y_i y_i^H of the RAW samples and one workgroup per
// matrix then forms K = L^-1 R L^-H by two triangular solves (ncoil^3 work once instead of ncoil^2 per sample); the projection applies W = L^-H U_nv,
// whose W^H y = U_nv^H L^-1 y is the whitened projection.  All fp64 complex.
//
// Kernels (launch order):
//   k_cc_chol       one workgroup: Psi (lower triangle) -> L, and a not-positive-definite flag in pinned host memory
//   k_cc_cov_part   (block of CH samples, slice): fixed partial of the upper triangle of R per block; y staged in LDS TS samples at a time
//   k_cc_cov_reduce (pair range, matrix): the partials added in one fixed order -- blocks ascending, then (shared mode) slices ascending
//   k_cc_whiten     one workgroup per matrix: K = L^-1 (L^-1 R)^H, one column per thread, forward substitution
//   k_cc_wmat       one workgroup per matrix: W = L^-H U_nv, one column per thread, back substitution
//   k_cc_proj       (sample range, group of LG virtual coils, slice): out_l = sum_j conj(W[j, l]) in_j, j ascending from 0
// No floating-point atomics: CH depends on ncoil only and every sum has one order, so a slice's K, W and outputs are the same bits alone, at any
// position of a stack and with any max_batch.
//
// Projection: vector FMA, not fp64 MFMA.  Per sample it reads ncoil and writes nv complex values (16 B each) for 8 ncoil nv flops, i.e. about
// nv / 2 flop per byte (4 at 32 -> 8 coils), under half the fp64 ridge point (~10 flop / B: 78.6 TF/s over 8 TB/s), so HBM bounds it.  fp64 MFMA
// (v_mfma_f64_16x16x4, cdna_hip_programming.md) would need four real products per complex one and a 16-wide output tile that nv = 4..8 fills a
// quarter to a half of, for no gain on a bandwidth-bound pass.  The covariance pass is ~ (ncoil + 1) / 4 flop per byte (8 at 32 coils) and
// runs from LDS, vector FMA as well.
#include <algorithm>
#include <cmath>
#include <vector>
#include "qmri_internal.h"

namespace {
constexpr int NT = 256;          // threads per workgroup
constexpr int TS = 32;           // samples per LDS tile of the covariance pass (row stride TS + 1: no bank conflicts between rows)
constexpr int LG = 8;            // virtual coils per thread of the projection

// samples per covariance partial: depends on ncoil alone (the partial layout, hence the bits, must not depend on the stack)
int cc_chunk(int ncoil) { return std::max(512, 16 * ncoil); }
int cc_qmax(int npairs) { return npairs <= NT ? 1 : npairs <= 4 * NT ? 4 : npairs <= 16 * NT ? 16 : 33; }

__device__ __forceinline__ void pair_of(int p, int n, int& i, int& j) {       // p-th entry of the upper triangle, row by row
    i = 0;
    while (p >= n - i) { p -= n - i; ++i; }
    j = i + p;
}

__global__ void __launch_bounds__(NT) k_cc_chol(const double2* __restrict__ psi, int n, double2* __restrict__ L, int* bad) {
    __shared__ int fail;
    if (threadIdx.x == 0) fail = 0;
    for (int e = threadIdx.x; e < n * n; e += NT) {
        const int i = e % n, j = e / n;
        L[e] = i >= j ? psi[e] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        const double d = L[k + k * n].x;
        if (!(d > 0.0) || !std::isfinite(d)) { if (threadIdx.x == 0) fail = 1; break; }          // (uniform: every thread reads the same d)
        const double lkk = std::sqrt(d);
        __syncthreads();
        for (int i = k + 1 + threadIdx.x; i < n; i += NT) { double2 v = L[i + k * n]; L[i + k * n] = make_double2(v.x / lkk, v.y / lkk); }
        if (threadIdx.x == 0) L[k + k * n] = make_double2(lkk, 0.0);
        __syncthreads();
        const int r = n - k - 1;
        for (int e = threadIdx.x; e < r * r; e += NT) {                          // L[i, j] -= L[i, k] conj(L[j, k]),  k < j <= i
            const int i = k + 1 + e % r, j = k + 1 + e / r;
            if (j > i) continue;
            const double2 a = L[i + k * n], b = L[j + k * n];
            double2 v = L[i + j * n];
            v.x = fma(-a.x, b.x, fma(-a.y, b.y, v.x));
            v.y = fma(-a.y, b.x, fma(a.x, b.y, v.y));
            L[i + j * n] = v;
        }
        __syncthreads();
    }
    __syncthreads();
    if (threadIdx.x == 0) *bad = fail;
}

// R partials: part[(b * nblk + blk) * npairs + p] = sum over the block's samples s of y_i(s) conj(y_j(s)), samples ascending
template <int QMAX>
__global__ void __launch_bounds__(NT) k_cc_cov_part(const double2* __restrict__ y, int m, int ncoil, int chunk, int nblk, double2* __restrict__ part) {
    extern __shared__ double2 tile[];                                          // [ncoil][TS + 1]
    const int b = blockIdx.y, blk = blockIdx.x;
    const int npairs = ncoil * (ncoil + 1) / 2;
    const int s0 = blk * chunk, s1 = min(s0 + chunk, m);
    const double2* yb = y + (size_t)b * ncoil * m;
    int pi[QMAX], pj[QMAX];
    double2 acc[QMAX];
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        const int p = threadIdx.x + q * NT;
        pi[q] = pj[q] = 0;
        if (p < npairs) pair_of(p, ncoil, pi[q], pj[q]);
        acc[q] = make_double2(0.0, 0.0);
    }
    for (int t0 = s0; t0 < s1; t0 += TS) {
        const int cnt = min(TS, s1 - t0);
        for (int e = threadIdx.x; e < ncoil * TS; e += NT) {
            const int c = e / TS, s = e % TS;
            tile[c * (TS + 1) + s] = s < cnt ? yb[(size_t)c * m + t0 + s] : make_double2(0.0, 0.0);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < QMAX; ++q) {
            if (threadIdx.x + q * NT < npairs) {
                const double2* a = tile + pi[q] * (TS + 1);
                const double2* c = tile + pj[q] * (TS + 1);
                double2 v = acc[q];
#pragma unroll 8
                for (int s = 0; s < TS; ++s) {
                    const double2 u = a[s], w = c[s];
                    v.x = fma(u.x, w.x, fma(u.y, w.y, v.x));
                    v.y = fma(u.y, w.x, fma(-u.x, w.y, v.y));
                }
                acc[q] = v;
            }
        }
        __syncthreads();
    }
    double2* out = part + ((size_t)b * nblk + blk) * npairs;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        const int p = threadIdx.x + q * NT;
        if (p < npairs) out[p] = acc[q];
    }
}

// R[mat] (ncoil x ncoil column-major, both triangles) from the partials: blocks ascending per slice; shared: those slice sums, slices ascending
__global__ void __launch_bounds__(NT) k_cc_cov_reduce(const double2* __restrict__ part, int nblk, int ncoil, int B, int shared, double2* __restrict__ R) {
    const int npairs = ncoil * (ncoil + 1) / 2;
    const int p = blockIdx.x * NT + threadIdx.x, mat = blockIdx.y;
    if (p >= npairs) return;
    const int b0 = shared ? 0 : mat, b1 = shared ? B : mat + 1;
    double2 tot = make_double2(0.0, 0.0);
    for (int b = b0; b < b1; ++b) {
        double2 v = make_double2(0.0, 0.0);
        const double2* pp = part + (size_t)b * nblk * npairs + p;
        for (int k = 0; k < nblk; ++k) { const double2 t = pp[(size_t)k * npairs]; v.x += t.x; v.y += t.y; }
        if (b == b0) tot = v; else { tot.x += v.x; tot.y += v.y; }
    }
    int i, j;
    pair_of(p, ncoil, i, j);
    double2* r = R + (size_t)mat * ncoil * ncoil;
    if (i == j) tot.y = 0.0;
    r[i + (size_t)j * ncoil] = tot;
    if (i != j) r[j + (size_t)i * ncoil] = make_double2(tot.x, -tot.y);
}

// K = L^-1 R L^-H in place of R: X = L^-1 R, then K = L^-1 X^H (= K^H = K).  X: scratch of the same size.  One workgroup per matrix.
__global__ void __launch_bounds__(NT) k_cc_whiten(const double2* __restrict__ L, int n, double2* R, double2* X) {
    double2* r = R + (size_t)blockIdx.x * n * n;
    double2* x = X + (size_t)blockIdx.x * n * n;
    for (int c = threadIdx.x; c < n; c += NT)
        for (int i = 0; i < n; ++i) {
            double2 a = r[i + (size_t)c * n];
            for (int j = 0; j < i; ++j) {
                const double2 l = L[i + (size_t)j * n], v = x[j + (size_t)c * n];
                a.x = fma(-l.x, v.x, fma(l.y, v.y, a.x));
                a.y = fma(-l.x, v.y, fma(-l.y, v.x, a.y));
            }
            const double d = L[i + (size_t)i * n].x;
            x[i + (size_t)c * n] = make_double2(a.x / d, a.y / d);
        }
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += NT)
        for (int i = 0; i < n; ++i) {
            const double2 h = x[c + (size_t)i * n];
            double2 a = make_double2(h.x, -h.y);
            for (int j = 0; j < i; ++j) {
                const double2 l = L[i + (size_t)j * n], v = r[j + (size_t)c * n];
                a.x = fma(-l.x, v.x, fma(l.y, v.y, a.x));
                a.y = fma(-l.x, v.y, fma(-l.y, v.x, a.y));
            }
            const double d = L[i + (size_t)i * n].x;
            r[i + (size_t)c * n] = make_double2(a.x / d, a.y / d);          // (column c of R was read by this thread only: safe in place)
        }
}

// W = L^-H U (n x nv column-major per matrix): L^H W = U by back substitution, one column per thread
__global__ void __launch_bounds__(NT) k_cc_wmat(const double2* __restrict__ L, const double2* __restrict__ U, int n, int nv, double2* __restrict__ W) {
    const double2* u = U + (size_t)blockIdx.x * n * nv;
    double2* w = W + (size_t)blockIdx.x * n * nv;
    for (int c = threadIdx.x; c < nv; c += NT)
        for (int i = n - 1; i >= 0; --i) {
            double2 a = u[i + (size_t)c * n];
            for (int j = i + 1; j < n; ++j) {                                   // (L^H)[i, j] = conj(L[j, i])
                const double2 l = L[j + (size_t)i * n], v = w[j + (size_t)c * n];
                a.x = fma(-l.x, v.x, fma(-l.y, v.y, a.x));
                a.y = fma(-l.x, v.y, fma(l.y, v.x, a.y));
            }
            const double d = L[i + (size_t)i * n].x;
            w[i + (size_t)c * n] = make_double2(a.x / d, a.y / d);
        }
}

// out[b][l][i] = sum_j conj(W[j, l]) in[b][j][i], j ascending from 0; W of slice b at W + b * wstride (wstride 0: one W for the stack)
__global__ void __launch_bounds__(NT) k_cc_proj(const double2* __restrict__ in, size_t len, int ncoil, int nv, const double2* __restrict__ W, size_t wstride,
                                                double2* __restrict__ out) {
    __shared__ double2 sw[128 * LG];
    const int b = blockIdx.z, l0 = blockIdx.y * LG;
    const double2* wb = W + (size_t)b * wstride;
    for (int e = threadIdx.x; e < ncoil * LG; e += NT) {
        const int j = e / LG, l = l0 + e % LG;
        sw[e] = l < nv ? wb[j + (size_t)l * ncoil] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= len) return;
    const double2* src = in + (size_t)b * ncoil * len + i;
    double2 acc[LG];
#pragma unroll
    for (int l = 0; l < LG; ++l) acc[l] = make_double2(0.0, 0.0);
    for (int j = 0; j < ncoil; ++j) {
        const double2 x = src[(size_t)j * len];
#pragma unroll
        for (int l = 0; l < LG; ++l) {
            const double2 w = sw[j * LG + l];
            acc[l].x = fma(w.y, x.y, fma(w.x, x.x, acc[l].x));
            acc[l].y = fma(-w.y, x.x, fma(w.x, x.y, acc[l].y));
        }
    }
    double2* dst = out + (size_t)b * nv * len + i;
#pragma unroll
    for (int l = 0; l < LG; ++l)
        if (l0 + l < nv) dst[(size_t)(l0 + l) * len] = acc[l];
}

}  // namespace

int cc_ensure_staging(qmri_ctx* ctx, size_t ny, size_t nm, size_t nyo, size_t nmo) {
    CcWork& w = ctx->cc;
    const int st = [&]() -> int {
        QMRI_TRY(w.sy.ensure(ctx, ny));
        if (nm) QMRI_TRY(w.sm.ensure(ctx, nm));
        QMRI_TRY(w.oy.ensure(ctx, nyo));
        if (nmo) QMRI_TRY(w.om.ensure(ctx, nmo));
        return QMRI_OK;
    }();
    if (st == QMRI_ERR_NOMEM) qmri_set_error(ctx, "out of device memory for the staging of the coil compression");
    return st;
}

// The whole transform on device arrays (api_cc.cpp checks the arguments).  d_psi: device ncoil x ncoil or nullptr.  Writes *nv_out, y_out [B][nv][m],
// maps_out [B][nv][plane] (when d_maps), W (device, [nmat][ncoil][nv], nullable), eig (host, [nmat][ncoil], nullable); nmat = shared ? 1 : B.
int cc_compress_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_y, const double2* d_maps, const double2* d_psi, const qmri_cc_params& prm,
                    int* nv_out, double2* d_yout, double2* d_mout, double2* d_Wout, double* eig_out) {
    OpHost& o = ctx->op;
    CcWork& w = ctx->cc;
    const int n = ncoil, npairs = n * (n + 1) / 2, chunk = cc_chunk(n), nblk = (o.m + chunk - 1) / chunk;
    const int nmat = prm.shared ? 1 : B;
    const size_t nn = (size_t)n * n, plane = (size_t)o.N * o.M;
    const int got = [&]() -> int {
        QMRI_TRY(w.part.ensure(ctx, (size_t)B * nblk * npairs));
        for (DevArr<double2>* a : {&w.R, &w.X, &w.U, &w.W}) QMRI_TRY(a->ensure(ctx, nmat * nn));
        if (d_psi) QMRI_TRY(w.L.ensure(ctx, nn));
        return QMRI_OK;
    }();
    if (got == QMRI_ERR_NOMEM) qmri_set_error(ctx, "out of device memory for the coil compression of %d slices x %d coils", B, n);
    QMRI_TRY(got);
    QMRI_TRY(w.hK.ensure(ctx, nmat * nn));
    QMRI_TRY(w.hbad.ensure(ctx, 1));
    *w.hbad = 0;
    if (d_psi) {
        k_cc_chol<<<1, NT, 0, ctx->stream>>>(d_psi, n, w.L, w.hbad);
        QMRI_HIP(ctx, hipGetLastError());
    }
    const size_t lds = (size_t)n * (TS + 1) * sizeof(double2);           // up to 67.6 KB at 128 coils: above the 64 KB default
    const dim3 gp(nblk, B);
    if (!w.lds_attr) {
        QMRI_HIP(ctx, hipFuncSetAttribute((const void*)k_cc_cov_part<33>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(128 * (TS + 1) * sizeof(double2))));
        w.lds_attr = true;
    }
    switch (cc_qmax(npairs)) {
        case 1: k_cc_cov_part<1><<<gp, NT, lds, ctx->stream>>>(d_y, o.m, n, chunk, nblk, w.part); break;
        case 4: k_cc_cov_part<4><<<gp, NT, lds, ctx->stream>>>(d_y, o.m, n, chunk, nblk, w.part); break;
        case 16: k_cc_cov_part<16><<<gp, NT, lds, ctx->stream>>>(d_y, o.m, n, chunk, nblk, w.part); break;
        default: k_cc_cov_part<33><<<gp, NT, lds, ctx->stream>>>(d_y, o.m, n, chunk, nblk, w.part); break;
    }
    QMRI_HIP(ctx, hipGetLastError());
    k_cc_cov_reduce<<<dim3((npairs + NT - 1) / NT, nmat), NT, 0, ctx->stream>>>(w.part, nblk, n, B, prm.shared, w.R);
    QMRI_HIP(ctx, hipGetLastError());
    if (d_psi) {
        k_cc_whiten<<<nmat, NT, 0, ctx->stream>>>(w.L, n, w.R, w.X);
        QMRI_HIP(ctx, hipGetLastError());
    }
    QMRI_HIP(ctx, hipMemcpyAsync(w.hK, w.R, nmat * nn * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*w.hbad) {
        qmri_set_error(ctx, "invalid argument: the noise covariance is not Hermitian positive definite (Cholesky failed)");
        return QMRI_ERR_INVALID_ARG;
    }
    // the eigensolve (host, api_cc.cpp) and the choice of nv
    std::vector<double> lam(nmat * (size_t)n);
    std::vector<double2> U(nmat * nn);                                      // (K is in w.hK; U goes back through it, pinned)
    int nv = prm.nv;
    for (int k = 0; k < nmat; ++k) {
        QMRI_TRY(cc_eig_host(ctx, n, w.hK + k * nn, lam.data() + (size_t)k * n, U.data() + k * nn));
        if (prm.nv == 0) nv = std::max(k == 0 ? 1 : nv, cc_choose_nv(n, lam.data() + (size_t)k * n, prm.energy));
    }
    *nv_out = nv;
    if (eig_out) std::copy(lam.begin(), lam.end(), eig_out);
    // U_nv: the first nv columns, compact [nmat][n][nv] (the column-major n x n matrix's first n * nv entries)
    for (int k = 0; k < nmat; ++k) std::copy(U.data() + k * nn, U.data() + k * nn + (size_t)n * nv, w.hK + (size_t)k * n * nv);
    QMRI_HIP(ctx, hipMemcpyAsync(w.U, w.hK, (size_t)nmat * n * nv * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    const double2* Wd = w.U;
    if (d_psi) {
        k_cc_wmat<<<nmat, NT, 0, ctx->stream>>>(w.L, w.U, n, nv, w.W);
        QMRI_HIP(ctx, hipGetLastError());
        Wd = w.W;
    }
    const size_t wstride = prm.shared ? 0 : (size_t)n * nv;
    const int gy = (nv + LG - 1) / LG;
    k_cc_proj<<<dim3((unsigned)((o.m + NT - 1) / NT), gy, B), NT, 0, ctx->stream>>>(d_y, (size_t)o.m, n, nv, Wd, wstride, d_yout);
    QMRI_HIP(ctx, hipGetLastError());
    if (d_maps) {
        k_cc_proj<<<dim3((unsigned)((plane + NT - 1) / NT), gy, B), NT, 0, ctx->stream>>>(d_maps, plane, n, nv, Wd, wstride, d_mout);
        QMRI_HIP(ctx, hipGetLastError());
    }
    if (d_Wout) QMRI_HIP(ctx, hipMemcpyAsync(d_Wout, Wd, (size_t)nmat * n * nv * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
    return QMRI_OK;
}
