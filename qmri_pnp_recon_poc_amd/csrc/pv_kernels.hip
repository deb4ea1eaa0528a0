// pv_kernels.hip -- tissue-fraction unmixing (include/qmri.h qmri_dict_unmix): every pixel's compressed fingerprint as a
// non-negative combination of C <= 8 chosen atoms, w = argmin_{w >= 0} ||b - A w||_2 by Lawson & Hanson's active-set method on the normal equations.
// An EXTENSION with no reference counterpart; the definition is restated in tests/pv_ref.py.
//
// One pixel per lane, 256 lanes per workgroup, fp64 throughout, no atomics and no cross-lane traffic: a pixel's bits depend on its own x alone.
// Lane p reads X[p + Npix j], so a wave's loads are contiguous.  The components' table (A, G, sum_c a_c, ||a_c||: PV_TAB doubles, the same for
// every lane) sits in LDS and is read at uniform addresses (broadcast, no bank conflict).  The kernel is a template on C: every loop over components
// has constant bounds and is fully unrolled, the passive set P is a bit mask, and the normal equations are solved on the IDENTITY-PADDED system --
// rows and columns outside P replaced by the identity, right-hand side 0 -- so the Cholesky factor, both substitutions and h, w, z are indexed by
// compile-time constants only and stay in registers (a dynamically indexed per-lane array would go to scratch).  The padding adds exact zeros, so
// z_P is what the factorisation of G_PP alone gives.  Lanes of a wave diverge in their iteration counts; that is accepted.
#include "qmri_internal.h"

namespace {
constexpr double PV_DUAL_TOL = 0x1p-48;          // tau_i = 2^-48 ||a_i|| ||b||

// z with G_PP z_P = h_P, z = 0 outside P: Cholesky in ascending index order, then the two substitutions
template <int C>
__device__ __forceinline__ void pv_solve(const double* __restrict__ sG, const double (&h)[C], unsigned P, double (&z)[C]) {
    double L[C][C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const bool pj = (P >> j) & 1u;
        double v = sG[j * PV_MAX_C + j];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= L[j][k] * L[j][k];
        const double d = sqrt(pj ? v : 1.0);
        L[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < C; ++i) {
            double u = sG[i * PV_MAX_C + j];
#pragma unroll
            for (int k = 0; k < j; ++k) u -= L[i][k] * L[j][k];
            L[i][j] = (pj && ((P >> i) & 1u)) ? u / d : 0.0;
        }
    }
    double y[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        double v = ((P >> i) & 1u) ? h[i] : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = C - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < C; ++k) v -= L[k][i] * z[k];
        z[i] = v / L[i][i];
    }
}

template <int C, int MODE>
__global__ __launch_bounds__(256) void k_pv_unmix(const double2* __restrict__ X, int Npix, int s, const double* __restrict__ tab, double* __restrict__ w_out,
                                                  double* __restrict__ frac, double2* __restrict__ pd, double* __restrict__ res, int32_t* __restrict__ flags) {
    __shared__ double st[PV_TAB];
    if (threadIdx.x < PV_TAB) st[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    const double* sA = st + PV_TAB_A; const double* sG = st + PV_TAB_G; const double* sS = st + PV_TAB_ASUM; const double* sN = st + PV_TAB_NA;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Npix) return;
    const double2* xp = X + p;
    const size_t np = (size_t)Npix;

    // a non-finite pixel: all outputs 0, flag bit 1; q = sum x_j^2 on the way
    bool fin = true;
    double qr = 0.0, qi = 0.0;
    for (int j = 0; j < s; ++j) {
        const double2 x = xp[np * j];
        fin = fin && isfinite(x.x) && isfinite(x.y);
        if (MODE == QMRI_PV_PHASE) { qr += x.x * x.x - x.y * x.y; qi += 2.0 * (x.x * x.y); }
    }
    if (!fin) {
#pragma unroll
        for (int c = 0; c < C; ++c) { w_out[p + np * c] = 0.0; if (frac) frac[p + np * c] = 0.0; }
        if (pd) pd[p] = make_double2(0.0, 0.0);
        if (res) res[p] = 0.0;
        if (flags) flags[p] = QMRI_PV_FLAG_NONFINITE;
        return;
    }

    // step 1: b = Re(x e^{-i phi}), kept as (cos phi, sin phi); h = A^T b, ||b||
    double cs = 1.0, sn = 0.0;
    if (MODE == QMRI_PV_PHASE) {
        const double phi0 = (qr == 0.0 && qi == 0.0) ? 0.0 : 0.5 * atan2(qi, qr);
        sincos(phi0, &sn, &cs);
    }
    double h[C], w[C], z[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { h[c] = 0.0; w[c] = 0.0; z[c] = 0.0; }
    double t = 0.0, nb2 = 0.0;
    for (int j = 0; j < s; ++j) {
        const double2 x = xp[np * j];
        const double b = (MODE == QMRI_PV_PHASE) ? x.x * cs + x.y * sn : x.x;
        t += b * sS[j];
        nb2 += b * b;
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] += b * sA[j * PV_MAX_C + c];
    }
    if (MODE == QMRI_PV_PHASE && t < 0.0) {       // phi = phi0 + pi, b = -b0: exact negations
        cs = -cs; sn = -sn;
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = -h[c];
    }
    const double nb = sqrt(nb2);

    // step 2: Lawson-Hanson
    unsigned P = 0u;
    int nsolve = 0, flag = 0;
    for (;;) {
        // outer step: the lowest index with the largest dual above its tau moves into P
        double gbest = 0.0;
        int jbest = -1;
#pragma unroll
        for (int i = 0; i < C; ++i) {
            double g = h[i];
#pragma unroll
            for (int c = 0; c < C; ++c) g -= w[c] * sG[c * PV_MAX_C + i];
            const bool cand = !((P >> i) & 1u) && g > PV_DUAL_TOL * nb * sN[i];
            if (cand && (jbest < 0 || g > gbest)) { gbest = g; jbest = i; }
        }
        if (jbest < 0) break;
        P |= 1u << jbest;
        bool capped = false;
        for (;;) {                                // inner step
            if (nsolve >= 3 * C) { capped = true; break; }
            ++nsolve;
            pv_solve<C>(sG, h, P, z);
            bool allpos = true;
#pragma unroll
            for (int i = 0; i < C; ++i) allpos = allpos && (!((P >> i) & 1u) || z[i] > 0.0);
            if (allpos) {
#pragma unroll
                for (int i = 0; i < C; ++i) w[i] = ((P >> i) & 1u) ? z[i] : 0.0;
                break;
            }
            double r[C], alpha = __builtin_inf();
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const bool neg = ((P >> i) & 1u) && z[i] <= 0.0;
                r[i] = neg ? (w[i] > 0.0 ? w[i] / (w[i] - z[i]) : 0.0) : __builtin_inf();
                alpha = fmin(alpha, r[i]);
            }
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const bool in = (P >> i) & 1u;
                const double wn = w[i] + alpha * (z[i] - w[i]);
                const bool out = in && (r[i] == alpha || wn <= 0.0);      // (r is +inf off the non-positive z: never equal to a finite alpha)
                w[i] = (in && !out) ? wn : 0.0;
                if (out) P &= ~(1u << i);
            }
        }
        if (capped) { flag = QMRI_PV_FLAG_CAP; break; }
    }

    // outputs
    double sw = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) sw += w[c];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        w_out[p + np * c] = w[c];
        if (frac) frac[p + np * c] = (sw > 0.0) ? w[c] / sw : 0.0;
    }
    if (pd) pd[p] = make_double2(sw * cs, sw * sn);
    if (flags) flags[p] = flag;
    if (res) {                                    // ||x e^{-i phi} - A w|| / ||x||, from A and not from G
        double r2 = 0.0, x2 = 0.0;
        for (int j = 0; j < s; ++j) {
            const double2 x = xp[np * j];
            double re = (MODE == QMRI_PV_PHASE) ? x.x * cs + x.y * sn : x.x;
            const double im = (MODE == QMRI_PV_PHASE) ? x.y * cs - x.x * sn : x.y;
#pragma unroll
            for (int c = 0; c < C; ++c) re -= sA[j * PV_MAX_C + c] * w[c];
            r2 += re * re + im * im;
            x2 += x.x * x.x + x.y * x.y;
        }
        res[p] = (x2 > 0.0) ? sqrt(r2) / sqrt(x2) : 0.0;
    }
}

template <int C>
void pv_launch_c(qmri_ctx* ctx, const double2* d_X, int Npix, int mode, const PvHost& pv, double* d_w, double* d_frac, double2* d_pd, double* d_res,
                 int32_t* d_flags) {
    const dim3 grid((unsigned)((Npix + 255) / 256)), block(256);
    if (mode == QMRI_PV_PHASE)
        hipLaunchKernelGGL((k_pv_unmix<C, QMRI_PV_PHASE>), grid, block, 0, ctx->stream, d_X, Npix, pv.s, pv.d_tab.p, d_w, d_frac, d_pd, d_res, d_flags);
    else
        hipLaunchKernelGGL((k_pv_unmix<C, QMRI_PV_REAL>), grid, block, 0, ctx->stream, d_X, Npix, pv.s, pv.d_tab.p, d_w, d_frac, d_pd, d_res, d_flags);
}
}  // namespace

int pv_launch(qmri_ctx* ctx, const double2* d_X, int Npix, int mode, double* d_w, double* d_frac, double2* d_pd, double* d_res, int32_t* d_flags) {
    const PvHost& pv = ctx->dict.pv;
    switch (pv.C) {
        case 1: pv_launch_c<1>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        case 2: pv_launch_c<2>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        case 3: pv_launch_c<3>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        case 4: pv_launch_c<4>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        case 5: pv_launch_c<5>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        case 6: pv_launch_c<6>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        case 7: pv_launch_c<7>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        case 8: pv_launch_c<8>(ctx, d_X, Npix, mode, pv, d_w, d_frac, d_pd, d_res, d_flags); break;
        default: qmri_set_error(ctx, "components not set: call qmri_set_components first"); return QMRI_ERR_STATE;
    }
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
