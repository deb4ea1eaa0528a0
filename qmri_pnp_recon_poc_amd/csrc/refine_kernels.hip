// refine_kernels.hip -- sub-grid refinement of a dictionary match (include/qmri.h qmri_dict_refine): every pixel's (T1, T2, ..)
// moved off the dictionary's grid by fitting the pixel to a quadratic through the matched atom and its neighbours along each refined lut column.
// An EXTENSION with no reference counterpart; the definition is tests/refine_ref.py, which this file follows operation for operation.
//
// 16 lanes per pixel: lane j owns channel j (s <= 16, the rest zero), 4 pixels per wave, 16 per 256-thread workgroup.  A lane keeps x_j, the centre
// atom's a0_j, the model's g_q,j and h_q,j, and the current d_j and residual: fp64 registers, no LDS.  An atom arrives as one coalesced 128-byte row of
// d_arow.  Every sum over the channels is one xor butterfly over the pixel's 16 lanes (masks 15, 7, 2, 1: the DPP row mirror, half mirror and two quad
// permutes, each exactly one 16-lane row wide) -- commutative at every stage, so all 16 lanes hold the same bits, compute the same scalars and
// branch together; several sums share one pass (rsum<N>).  The file is compiled with -ffp-contract=off: the restatement has no fused multiply-add.
// The four pixels of a wave differ in their steps, halvings and moves: a pixel's 16 lanes leave a loop together and wait, masked off, until the
// wave's other pixels leave it -- a DPP operand always comes from the lane's own row, whose lanes are active whenever the lane is.
// No atomics, no scratch, no order that depends on the launch: a pixel's bits depend on that pixel alone.
#include "qmri_internal.h"

namespace {
constexpr double RF_TOL_T = 1e-10, RF_STALL_T = 1e-6, RF_RIDGE = 1e-12, RF_COLLINEAR = 1e-12;
constexpr int RF_MAX_STEPS = 30, RF_MAX_HALVINGS = 10, RF_MAX_MOVES = 4;

template <int CTRL>
__device__ __forceinline__ double rf_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// N sums over the 16 lanes of a pixel in one pass; lane l adds lane l ^ 15, then l ^ 7, l ^ 2, l ^ 1
template <int N>
__device__ __forceinline__ void rsum(double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + rf_dpp<0x140>(v[i]);          // row_mirror
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + rf_dpp<0x141>(v[i]);          // row_half_mirror
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + rf_dpp<0x4E>(v[i]);           // quad_perm [2, 3, 0, 1]
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + rf_dpp<0xB1>(v[i]);           // quad_perm [1, 0, 3, 2]
}

// the point t of the model: d, rho, the residual and f.  false: d . d is zero or not finite
template <int P>
struct RfPoint {
    double d, rr, ri;                 // this lane's channel
    double dd, rho_r, rho_i, f;       // the pixel's
};
template <int P>
__device__ __forceinline__ bool rf_evaluate(double xr, double xi, double a0, const double (&g)[P], const double (&h)[P], const double (&t)[P], RfPoint<P>& o) {
    double d = a0;
#pragma unroll
    for (int q = 0; q < P; ++q) d = d + (t[q] * g[q] + (t[q] * t[q]) * h[q]);
    double s3[3] = {d * d, d * xr, d * xi};
    rsum<3>(s3);
    if (!(s3[0] > 0.0 && s3[0] < __builtin_inf())) return false;
    o.d = d; o.dd = s3[0];
    o.rho_r = s3[1] / s3[0]; o.rho_i = s3[2] / s3[0];
    o.rr = xr - o.rho_r * d; o.ri = xi - o.rho_i * d;
    double s1[1] = {o.rr * o.rr + o.ri * o.ri};
    rsum<1>(s1);
    o.f = s1[0];
    return true;
}

// the Gauss-Newton step at t (point c); pinned coordinates get delta = 0
template <int P>
__device__ __forceinline__ void rf_step(const RfPoint<P>& c, const double (&g)[P], const double (&h)[P], const double (&t)[P], const double (&lo)[P],
                                        const double (&hi)[P], unsigned free_mask, double (&delta)[P]) {
    constexpr int NJJ = P * (P + 1) / 2, N = NJJ + 3 * P + 2;
    double J[P], S[N];
#pragma unroll
    for (int q = 0; q < P; ++q) J[q] = g[q] + (2.0 * t[q]) * h[q];
    {
        int n = 0;
#pragma unroll
        for (int q = 0; q < P; ++q)
#pragma unroll
            for (int r = q; r < P; ++r) S[n++] = J[q] * J[r];
#pragma unroll
        for (int q = 0; q < P; ++q) S[NJJ + q] = J[q] * c.d;
#pragma unroll
        for (int q = 0; q < P; ++q) S[NJJ + P + q] = J[q] * c.rr;
#pragma unroll
        for (int q = 0; q < P; ++q) S[NJJ + 2 * P + q] = J[q] * c.ri;
        S[N - 2] = c.d * c.rr; S[N - 1] = c.d * c.ri;
    }
    rsum<N>(S);
    double JJ[P][P];
    {
        int n = 0;
#pragma unroll
        for (int q = 0; q < P; ++q)
#pragma unroll
            for (int r = q; r < P; ++r) { JJ[q][r] = S[n]; JJ[r][q] = S[n]; ++n; }
    }
    const double* Jd = S + NJJ; const double* Jrr = S + NJJ + P; const double* Jri = S + NJJ + 2 * P;
    const double drr = S[N - 2], dri = S[N - 1], dd = c.dd;
    const double rho2 = c.rho_r * c.rho_r + c.rho_i * c.rho_i;
    double gv[P], H[P][P];
    bool dead[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const double mqq = JJ[q][q] - (Jd[q] * Jd[q]) / dd;
        gv[q] = c.rho_r * (Jrr[q] - (Jd[q] * drr) / dd) + c.rho_i * (Jri[q] - (Jd[q] * dri) / dd);
        dead[q] = !((free_mask >> q) & 1u) || !(mqq > RF_COLLINEAR * JJ[q][q]) || (t[q] >= hi[q] && gv[q] > 0.0) || (t[q] <= lo[q] && gv[q] < 0.0);
#pragma unroll
        for (int r = 0; r < P; ++r) H[q][r] = rho2 * (JJ[q][r] - (Jd[q] * Jd[r]) / dd);
    }
    double tr = 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q)
        if (!dead[q]) tr = tr + H[q][q];
    const double ridge = RF_RIDGE * tr;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        if (dead[q]) gv[q] = 0.0;
        else H[q][q] = H[q][q] + ridge;
    }
    // Cholesky in ascending order; a pinned coordinate's row and column are the identity's
    double L[P][P];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = 0; i < P; ++i) L[i][j] = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double v = H[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) v = v - L[j][k] * L[j][k];
        if (dead[j] || !(v > 0.0)) { dead[j] = true; L[j][j] = 1.0; continue; }
        L[j][j] = sqrt(v);
#pragma unroll
        for (int i = j + 1; i < P; ++i) {
            if (dead[i]) continue;
            double u = H[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) u = u - L[i][k] * L[j][k];
            L[i][j] = u / L[j][j];
        }
    }
    double y[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        y[i] = 0.0;
        if (dead[i]) continue;
        double v = gv[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
        delta[i] = 0.0;
        if (dead[i]) continue;
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < P; ++k) v = v - L[k][i] * delta[k];
        delta[i] = v / L[i][i];
    }
}

// (g, h, lo, hi) of one coordinate from the centre's value and its neighbours' (has_m / has_p: the lower / upper neighbour exists)
__device__ __forceinline__ void rf_coeffs(double a0, double am, double ap, bool has_m, bool has_p, double& g, double& h, double& lo, double& hi) {
    if (has_m && has_p) { g = (ap - am) * 0.5; h = (ap + am) * 0.5 - a0; lo = -1.0; hi = 1.0; }
    else if (has_p) { g = ap - a0; h = 0.0; lo = 0.0; hi = 1.0; }
    else if (has_m) { g = a0 - am; h = 0.0; lo = -1.0; hi = 0.0; }
    else { g = 0.0; h = 0.0; lo = 0.0; hi = 0.0; }
}

struct RfCols { int c[3]; };

template <int P>
__global__ __launch_bounds__(256) void k_dict_refine(const double2* __restrict__ X, int Npix, int s, int K, int Q, const int32_t* __restrict__ dm,
                                                     const double* __restrict__ arow, const int32_t* __restrict__ nbr, const float* __restrict__ lut,
                                                     RfCols cols, double* __restrict__ qmap, double2* __restrict__ pd, double* __restrict__ res,
                                                     double* __restrict__ t_out, int32_t* __restrict__ centre, int32_t* __restrict__ flags_out) {
    const int lane = threadIdx.x & 15;
    const long long pl = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (pl >= Npix) return;                                     // (a pixel's 16 lanes leave together)
    const size_t p = (size_t)pl, np = (size_t)Npix;

    int k = dm[p] - 1;
    if (k < 0 || k >= K) {                                      // skipped: every output 0
        for (int c = lane; c < Q; c += 16)
            if (qmap) qmap[p + np * c] = 0.0;
        if (t_out && lane < P) t_out[p + np * lane] = 0.0;
        if (lane == 0) {
            if (pd) pd[p] = make_double2(0.0, 0.0);
            if (res) res[p] = 0.0;
            if (centre) centre[p] = 0;
            if (flags_out) flags_out[p] = QMRI_RF_FLAG_SKIPPED;
        }
        return;
    }
    double xr = 0.0, xi = 0.0;
    if (lane < s) { const double2 x = X[p + np * lane]; xr = x.x; xi = x.y; }
    double sx[1] = {xr * xr + xi * xi};
    rsum<1>(sx);
    const double xx = sx[0];

    int flags = 0, moves = 0;
    bool have = false;                                          // cur holds a point of the last centre
    double t[P], lo[P], hi[P];
    unsigned free_mask = 0u;
    int nm[P], npl[P];
    RfPoint<P> cur;
    cur.rho_r = cur.rho_i = cur.f = 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q) { t[q] = 0.0; lo[q] = hi[q] = 0.0; nm[q] = npl[q] = -1; }

    const bool x_ok = xx > 0.0 && xx < __builtin_inf();
    if (!x_ok) flags = QMRI_RF_FLAG_DEGENERATE;
    for (bool go = x_ok; go;) {
        // the model of centre k
        const double a0 = arow[(size_t)k * 16 + lane];
        double g[P], h[P];
        free_mask = 0u;
#pragma unroll
        for (int q = 0; q < P; ++q) {
            nm[q] = nbr[((size_t)k * P + q) * 2];
            npl[q] = nbr[((size_t)k * P + q) * 2 + 1];
            const double am = nm[q] >= 0 ? arow[(size_t)nm[q] * 16 + lane] : 0.0;
            const double ap = npl[q] >= 0 ? arow[(size_t)npl[q] * 16 + lane] : 0.0;
            rf_coeffs(a0, am, ap, nm[q] >= 0, npl[q] >= 0, g[q], h[q], lo[q], hi[q]);
            if (nm[q] >= 0 || npl[q] >= 0) free_mask |= 1u << q;
            t[q] = 0.0;
        }
        // the fit
        int fl = 0;
        have = rf_evaluate<P>(xr, xi, a0, g, h, t, cur);
        if (!have) fl = QMRI_RF_FLAG_DEGENERATE;
        for (int steps = 0; have;) {
            double delta[P], tfull[P];
            rf_step<P>(cur, g, h, t, lo, hi, free_mask, delta);
            bool conv = true, big = false;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const double v = t[q] + delta[q];
                tfull[q] = v < lo[q] ? lo[q] : (v > hi[q] ? hi[q] : v);
                const double a = fabs(tfull[q] - t[q]);
                conv = conv && (a <= RF_TOL_T);
                big = big || (a > RF_STALL_T);
            }
            if (conv) break;
            if (steps == RF_MAX_STEPS) { fl |= QMRI_RF_FLAG_CAP; break; }
            double alpha = 1.0, tt[P];
            bool took = false;
            RfPoint<P> tri;
            for (int bt = 0; bt <= RF_MAX_HALVINGS; ++bt) {
#pragma unroll
                for (int q = 0; q < P; ++q) tt[q] = bt == 0 ? tfull[q] : t[q] + alpha * (tfull[q] - t[q]);
                if (rf_evaluate<P>(xr, xi, a0, g, h, tt, tri) && tri.f <= cur.f) { took = true; break; }
                alpha = alpha * 0.5;
            }
            if (!took) {
                if (big) fl |= QMRI_RF_FLAG_STALLED;
                break;
            }
#pragma unroll
            for (int q = 0; q < P; ++q) t[q] = tt[q];
            cur = tri;
            ++steps;
        }
        flags = (flags & QMRI_RF_FLAG_MOVED) | fl;
        // re-centring
        int nxt = -1;
        if (have && moves < RF_MAX_MOVES) {
#pragma unroll
            for (int q = 0; q < P; ++q) {
                if (nxt >= 0) continue;
                if (t[q] == 1.0 && npl[q] >= 0) { if (nbr[((size_t)npl[q] * P + q) * 2 + 1] >= 0) nxt = npl[q]; }
                else if (t[q] == -1.0 && nm[q] >= 0) { if (nbr[((size_t)nm[q] * P + q) * 2] >= 0) nxt = nm[q]; }
            }
        }
        if (nxt < 0) go = false;
        else { k = nxt; ++moves; flags |= QMRI_RF_FLAG_MOVED; }
    }
    if (!x_ok) {                                                // the start atom's neighbours, for the outputs below
#pragma unroll
        for (int q = 0; q < P; ++q) {
            nm[q] = nbr[((size_t)k * P + q) * 2];
            npl[q] = nbr[((size_t)k * P + q) * 2 + 1];
            if (nm[q] >= 0 || npl[q] >= 0) free_mask |= 1u << q;
        }
    }

    // outputs of the last centre
    double theta[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        if (!have) t[q] = 0.0;
        else if (((free_mask >> q) & 1u) && (t[q] == lo[q] || t[q] == hi[q])) flags |= QMRI_RF_FLAG_BOUND;
        const size_t col = (size_t)K * cols.c[q];
        const double l0 = (double)lut[k + col];
        const double lm = nm[q] >= 0 ? (double)lut[nm[q] + col] : 0.0;
        const double lp = npl[q] >= 0 ? (double)lut[npl[q] + col] : 0.0;
        double gl, hl, blo, bhi;
        rf_coeffs(l0, lm, lp, nm[q] >= 0, npl[q] >= 0, gl, hl, blo, bhi);
        theta[q] = l0 + (t[q] * gl + (t[q] * t[q]) * hl);
    }
    if (qmap)
        for (int c = lane; c < Q; c += 16) {
            double v = (double)lut[k + (size_t)K * c];
            if (v != v) v = 0.0;                                // NaN -> 0, as in the match
#pragma unroll
            for (int q = 0; q < P; ++q)
                if (cols.c[q] == c && ((free_mask >> q) & 1u)) v = theta[q];
            qmap[p + np * c] = v;
        }
    if (t_out) {
#pragma unroll
        for (int q = 0; q < P; ++q)
            if (lane == q) t_out[p + np * q] = t[q];
    }
    if (lane == 0) {
        if (pd) pd[p] = have ? make_double2(cur.rho_r, cur.rho_i) : make_double2(0.0, 0.0);
        if (res) res[p] = have ? sqrt(cur.f / xx) : 0.0;
        if (centre) centre[p] = k + 1;
        if (flags_out) flags_out[p] = flags;
    }
}
}  // namespace

int refine_launch(qmri_ctx* ctx, const double2* d_X, int Npix, const int32_t* d_dm, double* d_qmap, double2* d_pd, double* d_res, double* d_t,
                  int32_t* d_centre, int32_t* d_flags) {
    const DictHost& d = ctx->dict;
    const RefineHost& rf = d.rf;
    const dim3 grid((unsigned)(((long long)Npix + 15) / 16)), block(256);
    RfCols cols{{rf.cols[0], rf.cols[1], rf.cols[2]}};
    switch (rf.P) {
        case 1: hipLaunchKernelGGL(k_dict_refine<1>, grid, block, 0, ctx->stream, d_X, Npix, d.s, d.K, d.Q, d_dm, rf.d_arow.p, rf.d_nbr.p, d.d_lut, cols,
                                   d_qmap, d_pd, d_res, d_t, d_centre, d_flags); break;
        case 2: hipLaunchKernelGGL(k_dict_refine<2>, grid, block, 0, ctx->stream, d_X, Npix, d.s, d.K, d.Q, d_dm, rf.d_arow.p, rf.d_nbr.p, d.d_lut, cols,
                                   d_qmap, d_pd, d_res, d_t, d_centre, d_flags); break;
        case 3: hipLaunchKernelGGL(k_dict_refine<3>, grid, block, 0, ctx->stream, d_X, Npix, d.s, d.K, d.Q, d_dm, rf.d_arow.p, rf.d_nbr.p, d.d_lut, cols,
                                   d_qmap, d_pd, d_res, d_t, d_centre, d_flags); break;
        default: qmri_set_error(ctx, "refinement not set: call qmri_set_refine first"); return QMRI_ERR_STATE;
    }
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
