// llr_kernels.hip -- locally low-rank proximal step (include/qmri.h qmri_llr_prox): singular-value soft-thresholding of the
// b^2 x s Casorati matrix of every b x b block of a stack of coefficient images, and the dual update of the ADMM loop that follows it.
//
// k_llr_prox<b>: one wave per workgroup; b = 8: one block, one pixel per lane; b = 16: one block, four pixels per lane; b = 4: four blocks, 16 lanes
// each.  Per block, all in fp64 and in one fixed order (a block's bits depend on its own pixels, tau and s only -- not on the batch, the slice's
// place in it or the grid around it):
//   1. A (b^2 x s, channel-major with a padded channel stride) goes to LDS; lanes run along N, so a row of the block is one contiguous run of a plane.
//   2. G = A^H A: the s (s + 1) / 2 entries of the upper triangle are spread over the lanes, each summed over the pixels in ascending order on four
//      interleaved accumulators that are added as (0 + 1) + (2 + 3).
//   3. Eigenpairs of G by cyclic Jacobi in LDS, pivots (p, q) in row order, 16 lanes per block: lane k owns row k in the column update and column k
//      in the row update.  A sweep starts only while the off-diagonal norm exceeds 2^-52 trace(G); at most LLR_SWEEPS sweeps, so a non-finite
//      block ends too (its comparisons are false), with non-finite output in that block only.
//   4. f_k = max(0, 1 - tau / sigma_k), sigma_k = sqrt(max(lambda_k, 0)); W = V diag(f) V^H over the lanes; out = A W per pixel.
// No atomics; sigma_max goes out per block and k_llr_smax takes the slice's maximum (a maximum has no summation order).
//
// k_llr_dual: uold <- uold + x - v, z <- v - uold and the partial sums of ||z||^2 in the partition of k_prepare_z (dc_kernels.hip).
#include <cmath>
#include <cstdint>
#include "qmri_internal.h"

namespace {

constexpr int LLR_SWEEPS = 24;               // cap of Jacobi sweeps (s = 16 converges in well under 10)
constexpr double LLR_EPS = 2.220446049250313e-16;
constexpr int NT = 256;                      // k_llr_dual

struct LlrArgs {
    int N, M, s, o1, o2, real;
    long long total;                         // blocks of the whole batch
    double tau;
    const double2* x; const double2* u; double2* out; double* bsmax;
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)); }
// c a + t b with real c and complex t
__device__ __forceinline__ double2 rot(double c, double2 a, double2 t, double2 b) {
    const double2 tb = cmul(t, b);
    return make_double2(fma(c, a.x, tb.x), fma(c, a.y, tb.y));
}

template <int BS>
__global__ __launch_bounds__(64) void k_llr_prox(const LlrArgs a) {
    constexpr int PIX = BS * BS, LPB = PIX < 64 ? PIX : 64, BPW = 64 / LPB, PPL = PIX / LPB, AST = PIX + 1;
    extern __shared__ double2 lds[];
    const int s = a.s, lane = threadIdx.x;
    double2* As = lds;                                   // [BPW][s][AST]
    double2* Gs = As + BPW * s * AST;                    // [BPW][s][s], later W
    double2* Vs = Gs + BPW * s * s;                      // [BPW][s][s]
    double* fs = (double*)(Vs + BPW * s * s);            // [4][16] f, then [4][32] reduction scratch
    double* red = fs + 64;

    const int nbi = a.N / BS, nbj = a.M / BS;
    const size_t plane = (size_t)a.N * a.M;
    // ---- 1. load: lane -> (block of the wave, pixel of the block) ----
    const int blk = lane / LPB, pl = lane % LPB;
    const long long gb = (long long)blockIdx.x * BPW + blk;
    const bool live = gb < a.total;
    size_t base = 0;
    int n0 = 0, m0 = 0;
    if (live) {
        const long long sl = gb / ((long long)nbi * nbj);
        const int r = (int)(gb - sl * nbi * nbj), bj = r / nbi, bi = r - bj * nbi;
        base = (size_t)sl * plane * s;
        n0 = a.o1 + bi * BS;
        m0 = a.o2 + bj * BS;
    }
    size_t idx[PPL];
#pragma unroll
    for (int r = 0; r < PPL; ++r) {
        const int pix = pl + r * LPB;
        int n = n0 + pix % BS, m = m0 + pix / BS;
        if (n >= a.N) n -= a.N;
        if (m >= a.M) m -= a.M;
        idx[r] = base + (size_t)n + (size_t)a.N * m;
        for (int c = 0; c < s; ++c) {
            double2 v = make_double2(0.0, 0.0);
            if (live) {
                v = a.x[idx[r] + c * plane];
                if (a.u) { const double2 w = a.u[idx[r] + c * plane]; v.x += w.x; v.y += w.y; }
                if (a.real) v.y = 0.0;
            }
            As[(blk * s + c) * AST + pix] = v;
        }
    }
    __syncthreads();
    // ---- 2. Gram matrix ----
    const int npairs = s * (s + 1) / 2;
    for (int t = lane; t < BPW * npairs; t += 64) {
        const int tb = t / npairs;
        int j = 0, k = t - tb * npairs;
        while (k >= s - j) { k -= s - j; ++j; }
        k += j;                                          // j <= k
        const double2* aj = As + (tb * s + j) * AST;
        const double2* ak = As + (tb * s + k) * AST;
        double re[4] = {0, 0, 0, 0}, im[4] = {0, 0, 0, 0};
        for (int p = 0; p < PIX; p += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double2 u = aj[p + q], v = ak[p + q];
                re[q] = fma(u.x, v.x, fma(u.y, v.y, re[q]));
                im[q] = fma(u.x, v.y, fma(-u.y, v.x, im[q]));
            }
        }
        const double gr = (re[0] + re[1]) + (re[2] + re[3]), gi = (j == k) ? 0.0 : (im[0] + im[1]) + (im[2] + im[3]);
        Gs[(tb * s + j) * s + k] = make_double2(gr, gi);
        Gs[(tb * s + k) * s + j] = make_double2(gr, -gi);
    }
    // ---- 3. cyclic Jacobi: 16 lanes per block ----
    const int grp = lane >> 4, k = lane & 15;
    const bool act = grp < BPW && k < s;
    const int gq = grp < BPW ? grp : 0;                  // (idle groups read block 0's pivot and change nothing)
    double2* G = Gs + gq * s * s;
    double2* V = Vs + gq * s * s;
    if (act)
        for (int j = 0; j < s; ++j) V[k * s + j] = make_double2(j == k ? 1.0 : 0.0, 0.0);
    for (int sweep = 0; sweep < LLR_SWEEPS; ++sweep) {
        __syncthreads();
        if (act) {
            double o = 0.0;
            for (int j = 0; j < s; ++j)
                if (j != k) { const double2 g = G[k * s + j]; o = fma(g.x, g.x, fma(g.y, g.y, o)); }
            red[grp * 32 + k] = o;
            red[grp * 32 + 16 + k] = G[k * s + k].x;
        }
        __syncthreads();
        bool done = true;
        if (grp < BPW) {
            double o = 0.0, tr = 0.0;
            for (int j = 0; j < s; ++j) { o += red[grp * 32 + j]; tr += red[grp * 32 + 16 + j]; }
            const double lim = tr * LLR_EPS;
            done = o <= lim * lim;
        }
        if (__all(done)) break;
        const bool turn = act && !done;
        for (int p = 0; p < s - 1; ++p)
            for (int q = p + 1; q < s; ++q) {
                __syncthreads();
                const double2 g = G[p * s + q];
                const double app = G[p * s + p].x, aqq = G[q * s + q].x;
                const double ag = sqrt(fma(g.x, g.x, g.y * g.y));
                const bool go = turn && ag > 0.0;
                double c = 1.0, sn = 0.0;
                double2 e = make_double2(1.0, 0.0);
                if (go) {
                    const double th = (aqq - app) / (2.0 * ag);
                    const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(fma(th, th, 1.0)));
                    c = 1.0 / sqrt(fma(tt, tt, 1.0));
                    sn = tt * c;
                    e = make_double2(g.x / ag, g.y / ag);
                }
                const double2 mse_c = make_double2(-sn * e.x, sn * e.y), ce_c = make_double2(c * e.x, -c * e.y);   // -sn conj(e), c conj(e)
                const double2 mse = make_double2(-sn * e.x, -sn * e.y), ce = make_double2(c * e.x, c * e.y);       // -sn e, c e
                __syncthreads();
                if (go) {                                // columns p, q of G and V: lane k owns row k
                    const double2 gp = G[k * s + p], gqv = G[k * s + q];
                    G[k * s + p] = rot(c, gp, mse_c, gqv);
                    G[k * s + q] = rot(sn, gp, ce_c, gqv);
                    const double2 vp = V[k * s + p], vq = V[k * s + q];
                    V[k * s + p] = rot(c, vp, mse_c, vq);
                    V[k * s + q] = rot(sn, vp, ce_c, vq);
                }
                __syncthreads();
                if (go) {                                // rows p, q of G: lane k owns column k
                    const double2 rp = G[p * s + k], rq = G[q * s + k];
                    double2 np_ = rot(c, rp, mse, rq), nq = rot(sn, rp, ce, rq);
                    if (k == p) { np_.y = 0.0; nq = make_double2(0.0, 0.0); }
                    if (k == q) { np_ = make_double2(0.0, 0.0); nq.y = 0.0; }
                    G[p * s + k] = np_;
                    G[q * s + k] = nq;
                }
            }
    }
    __syncthreads();
    // ---- 4. shrink factors, sigma_max of the block, W = V diag(f) V^H ----
    if (act) {
        const double lam = G[k * s + k].x;
        const double sg = lam > 0.0 ? sqrt(lam) : (lam == lam ? 0.0 : lam);
        fs[grp * 16 + k] = sg > a.tau ? 1.0 - a.tau / sg : (sg == sg ? 0.0 : sg);
        red[grp * 32 + k] = sg;
    }
    __syncthreads();
    if (grp < BPW && k == 0 && a.bsmax) {
        const long long gg = (long long)blockIdx.x * BPW + grp;
        if (gg < a.total) {
            double m = 0.0;
            for (int j = 0; j < s; ++j) { const double v = red[grp * 32 + j]; m = (v > m || v != v) ? v : m; }
            a.bsmax[gg] = m;
        }
    }
    for (int t = lane; t < BPW * s * s; t += 64) {
        const int tb = t / (s * s), r = t - tb * s * s, j = r / s, c = r - j * s;
        const double2* Vb = Vs + tb * s * s;
        double2 acc = make_double2(0.0, 0.0);
        for (int kk = 0; kk < s; ++kk) {
            const double f = fs[tb * 16 + kk];
            const double2 vj = Vb[j * s + kk], vc = Vb[c * s + kk];
            const double2 w = make_double2(f * vj.x, f * vj.y);
            acc.x = fma(w.x, vc.x, fma(w.y, vc.y, acc.x));      // w conj(vc)
            acc.y = fma(w.y, vc.x, fma(-w.x, vc.y, acc.y));
        }
        Gs[t] = acc;                                     // (G's eigenvalues were read above; every lane passed the barrier since)
    }
    __syncthreads();
    // ---- 5. out = A W ----
    if (!live) return;
    const double2* W = Gs + blk * s * s;
#pragma unroll
    for (int r = 0; r < PPL; ++r) {
        const int pix = pl + r * LPB;
        double2 av[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) av[j] = j < s ? As[(blk * s + j) * AST + pix] : make_double2(0.0, 0.0);
        for (int c = 0; c < s; ++c) {
            double2 acc = make_double2(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < s) {
                    const double2 w = W[j * s + c];
                    acc.x = fma(av[j].x, w.x, fma(-av[j].y, w.y, acc.x));
                    acc.y = fma(av[j].x, w.y, fma(av[j].y, w.x, acc.y));
                }
            if (a.real) acc.y = 0.0;
            a.out[idx[r] + c * plane] = acc;
        }
    }
}

// the slice's largest block value (NaN wins); one wave per slice
__global__ __launch_bounds__(64) void k_llr_smax(const double* __restrict__ bsmax, int nblk, double* __restrict__ out) {
    const double* p = bsmax + (size_t)blockIdx.x * nblk;
    double m = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) { const double v = p[i]; m = (v > m || v != v) ? v : m; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double v = __shfl_down(m, off, 64); m = (m != m) ? m : ((v > m || v != v) ? v : m); }
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

// Step 3 of the loop on the prox output v (PnP_ADMM.m:144 and the z of :102): uold += x - v; z = v - uold; partial ||z||^2
__global__ __launch_bounds__(NT) void k_llr_dual(size_t n, const double2* __restrict__ x, const double2* __restrict__ v, double2* __restrict__ u,
                                                  double2* __restrict__ z, double* __restrict__ pz) {
    __shared__ double sh[NT / 64];
    const int b = blockIdx.y;
    const size_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const size_t i0 = (size_t)blockIdx.x * chunk, i1 = (i0 + chunk < n) ? i0 + chunk : n;
    double acc = 0.0;
    for (size_t i = i0 + threadIdx.x; i < i1; i += NT) {
        const double2 xv = x[(size_t)b * n + i], vv = v[(size_t)b * n + i];
        double2 uv = u[(size_t)b * n + i];
        uv.x = uv.x + xv.x - vv.x;
        uv.y = uv.y + xv.y - vv.y;
        u[(size_t)b * n + i] = uv;
        const double2 zz = make_double2(vv.x - uv.x, vv.y - uv.y);
        z[(size_t)b * n + i] = zz;
        acc = fma(zz.x, zz.x, fma(zz.y, zz.y, acc));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) sh[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
#pragma unroll
        for (int i = 0; i < NT / 64; ++i) r += sh[i];
        pz[(size_t)b * gridDim.x + blockIdx.x] = r;
    }
}

template <int BS> size_t llr_lds_bytes(int s) {
    constexpr int PIX = BS * BS, LPB = PIX < 64 ? PIX : 64, BPW = 64 / LPB, AST = PIX + 1;
    return (size_t)(BPW * s * AST + 2 * BPW * s * s) * sizeof(double2) + (64 + 128) * sizeof(double);
}

template <int BS> int llr_launch(qmri_ctx* ctx, const LlrArgs& a, int slot) {
    constexpr int PIX = BS * BS, BPW = PIX < 64 ? 64 / PIX : 1;
    const size_t lds = llr_lds_bytes<BS>(a.s);
    if (lds > 48 * 1024 && !ctx->llr_lds_attr[slot]) {
        QMRI_HIP(ctx, hipFuncSetAttribute((const void*)k_llr_prox<BS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)llr_lds_bytes<BS>(16)));
        ctx->llr_lds_attr[slot] = true;
    }
    const long long groups = (a.total + BPW - 1) / BPW;
    k_llr_prox<BS><<<dim3((unsigned)groups), dim3(64), lds, ctx->stream>>>(a);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

}  // namespace

int llr_prox_dev(qmri_ctx* ctx, const LlrPlan& pl, int B, const double2* d_x, const double2* d_u, double2* d_out, double* d_bsmax, double* d_smax) {
    LlrArgs a{};
    a.N = pl.N; a.M = pl.M; a.s = pl.s; a.o1 = pl.o1; a.o2 = pl.o2; a.real = pl.real;
    const long long nblk = (long long)(pl.N / pl.block) * (pl.M / pl.block);
    a.total = nblk * B;
    a.tau = pl.tau;
    a.x = d_x; a.u = d_u; a.out = d_out; a.bsmax = d_bsmax;
    if (a.total > 0x7fffffffLL) { qmri_set_error(ctx, "invalid argument: too many LLR blocks in one launch"); return QMRI_ERR_INVALID_ARG; }
    if (pl.block == 4) QMRI_TRY(llr_launch<4>(ctx, a, 0));
    else if (pl.block == 8) QMRI_TRY(llr_launch<8>(ctx, a, 1));
    else QMRI_TRY(llr_launch<16>(ctx, a, 2));
    if (d_bsmax && d_smax) {
        k_llr_smax<<<dim3(B), dim3(64), 0, ctx->stream>>>(d_bsmax, (int)nblk, d_smax);
        QMRI_HIP(ctx, hipGetLastError());
    }
    return QMRI_OK;
}

int llr_dual_dev(qmri_ctx* ctx, int B, size_t n, const double2* d_x, const double2* d_v, double2* d_u, double2* d_z, double* d_pz, int nblk_z) {
    k_llr_dual<<<dim3(nblk_z, B), dim3(NT), 0, ctx->stream>>>(n, d_x, d_v, d_u, d_z, d_pz);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
