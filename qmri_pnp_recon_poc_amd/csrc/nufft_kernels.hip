// nufft_kernels.hip -- the trajectory operator of qmri_set_operator_nufft, fp64 throughout, gfx950.
//
//   y_i = (1/sqrt(NM)) sum_n (sum_c V(t_i, c) x_c[n]) exp(-i (omega1 n1 + omega2 n2))      and its exact adjoint,
//
// as a 2x oversampled NUFFT on the centred index p = n - (N/2, M/2) (y_i = exp(-i (omega1 N/2 + omega2 M/2)) sum_p ...):
//   forward:  k_nu_pre    x / Phi(p), times the half-bin ramps exp(-i pi (a1 p1 / N + a2 p2 / M)), a in {0,1}^2, stored at q = p mod (N, M)
//             dc_kernels.hip's h- and w-passes (DC_SPECTRUM) on the 4 sub-grids as 4B slices:  S_a[j] = unitary DFT_{NxM}[j]
//                     -- the 2N x 2M DFT of the zero-padded image at bin (2 j1 + a1, 2 j2 + a2), so that no plan above 256 points is needed
//             k_nu_interleave  the 4 sub-grids -> one 2N x 2M grid [k1][k2][c] (a grid point's channels contiguous)
//             k_nu_interp  per sample: w x w grid points around u = (omega1 N / pi, omega2 M / pi), weights phi(u - k), combined with V(t, :)
//   adjoint:  k_nu_spread  output-driven: a workgroup owns a 16 x 16 tile of the oversampled grid (all s channels, all 4 sub-grids) and walks
//                        the samples whose windows reach it, in a fixed order; heavy tiles are split into segments whose partial tiles
//                        k_nu_reduce adds in segment order.  No floating-point atomics: a slice's bits do not depend on the batch.
//             k_nu_adj_w   dense inverse w-pass (conjugate domain, as k_adj_w) + dc_kernels.hip's inverse h-pass on the 4B sub-grids
//             k_nu_post    sum over the 4 sub-grids in a fixed order with the conjugate ramps, times 1 / Phi(p)
// Forward and adjoint evaluate the kernel with the same device function on the same inputs (nu_phi(u - k) with k from nu_k0), so adjointness
// holds to rounding.  Interpolation and spreading are gathers with w^2 reuse per sample: vector fp64 FMA, no MFMA.
//
// With a field map attached (qmri_set_field_map) nufft_launch_fwd / launch_adj run the chain once per time segment l with the
// OFFRES instantiations, which fold the segment's factors in where the data already is in registers or LDS: k_nu_pre times the phase map P_l,
// k_nu_interp times b_l (adding to y for l > 0); k_nu_spread times conj(b_l) as y is staged (after the sample weight), k_nu_post times conj(P_l)
// (adding to x for l > 0).  Segments run one after the other on the stream, so the sums have a fixed order.  The instantiations without OFFRES are
// the ones used without a map and compile to what they were before the parameter existed.
#include "dc_device.h"
#include "nufft_device.h"

using namespace dcdev;
using namespace nudev;

namespace {

// x [B][c][n2][n1] -> g [B][a][c][q2][q1], a = a1 + 2 a2, q = (n + N/2) mod N
// DEAPOD = false: the ramps alone, without 1 / Phi -- the zero-padded 2N x 2M DFT of the Toeplitz normal operator (toep_kernels.hip, "k_toep_pre")
// OFFRES: x times the segment's phase map nu.pm (one table entry per pixel, shared by the channels; no sincos here) first
template <bool DEAPOD, bool OFFRES = false>
__global__ __launch_bounds__(NT) void k_nu_pre(NufftDev nu, const double2* __restrict__ x, double2* __restrict__ g) {
    const int N = nu.N, M = nu.M, b = blockIdx.y;
    const size_t plane = (size_t)N * M, n = plane * nu.s;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i / plane), r = (int)(i - (size_t)c * plane), n2 = r / N, n1 = r - n2 * N;
    double2 v = x[(size_t)b * n + i];
    if (OFFRES) { const double2 p = nu.pm[r]; v = make_double2(v.x * p.x - v.y * p.y, v.x * p.y + v.y * p.x); }
    const double sc = DEAPOD ? nu.dp1[n1] * nu.dp2[n2] : 1.0;
    const double2 x0 = DEAPOD ? make_double2(v.x * sc, v.y * sc) : v;
    const double2 e1 = nu.r1[n1], e2 = nu.r2[n2];
    const double2 x1 = make_double2(x0.x * e1.x - x0.y * e1.y, x0.x * e1.y + x0.y * e1.x);
    const double2 x2 = make_double2(x0.x * e2.x - x0.y * e2.y, x0.x * e2.y + x0.y * e2.x);
    const double2 x3 = make_double2(x1.x * e2.x - x1.y * e2.y, x1.x * e2.y + x1.y * e2.x);
    const int q1 = (n1 + N / 2) % N, q2 = (n2 + M / 2) % M;
    double2* o = g + (size_t)b * 4 * n + (size_t)c * plane + (size_t)q2 * N + q1;
    st_wt(o, x0);
    st_wt(o + n, x1);
    st_wt(o + 2 * n, x2);
    st_wt(o + 3 * n, x3);
}

// the sub-grid spectra S [B][a][c][j1][j2] -> the oversampled grid G [B][k1][k2][c] (k = 2 j + a; a grid point's s channels contiguous)
__global__ __launch_bounds__(NT) void k_nu_interleave(NufftDev nu, const double2* __restrict__ S, double2* __restrict__ G) {
    const int N = nu.N, M = nu.M, s = nu.s, b = blockIdx.y;
    const size_t plane = (size_t)N * M, n = plane * s;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= 4 * n) return;
    const int k = (int)(i / s), c = (int)(i - (size_t)k * s), k1 = k / (2 * M), k2 = k - k1 * 2 * M;
    const double2 v = S[(size_t)b * 4 * n + (size_t)((k1 & 1) + 2 * (k2 & 1)) * n + (size_t)c * plane + (size_t)(k1 >> 1) * M + (k2 >> 1)];
    st_wt(G + (size_t)b * 4 * n + i, v);
}

// forward interpolation: one lane per sample, in the plan's bin order, on the interleaved grid G
// OFFRES: the sample times the segment's coefficient nu.bl (sorted order, as u and ph), added to y for the segments after the first
template <int W, bool OFFRES = false>
__global__ __launch_bounds__(NT) void k_nu_interp(NufftDev nu, const double2* __restrict__ S, double2* __restrict__ y) {
    const int e = blockIdx.x * NT + threadIdx.x, b = blockIdx.y;
    if (e >= nu.m) return;
    const int N = nu.N, M = nu.M, s = nu.s;
    const size_t n = (size_t)N * M * s;
    const double2 u = nu.u[e];
    const double inv_hw = 1.0 / nu.hw;
    const int k01 = nu_k0(u.x, nu.hw), k02 = nu_k0(u.y, nu.hw);
    double w1[W], w2[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { w1[i] = nu_phi(u.x - (double)(k01 + i), inv_hw, nu.beta); w2[i] = nu_phi(u.y - (double)(k02 + i), inv_hw, nu.beta); }
    double ar[DC_MAXS], ai[DC_MAXS];
#pragma unroll
    for (int c = 0; c < DC_MAXS; ++c) { ar[c] = 0.0; ai[c] = 0.0; }
    const double2* Sb = S + (size_t)b * 4 * n;
    for (int i1 = 0; i1 < W; ++i1) {
        const int k1 = nu_wrap(k01 + i1, 2 * N);
#pragma unroll 4
        for (int i2 = 0; i2 < W; ++i2) {
            const int k2 = nu_wrap(k02 + i2, 2 * M);
            const double wt = w1[i1] * w2[i2];
            const double2* p = Sb + ((size_t)k1 * 2 * M + k2) * s;
#pragma unroll
            for (int c = 0; c < DC_MAXS; ++c)
                if (c < s) { const double2 v = p[c]; ar[c] = fma(wt, v.x, ar[c]); ai[c] = fma(wt, v.y, ai[c]); }
        }
    }
    const double* vr = nu.Vt + (size_t)nu.t[e] * s;
    double re = 0.0, im = 0.0;
#pragma unroll
    for (int c = 0; c < DC_MAXS; ++c)
        if (c < s) { const double v = vr[c]; re = fma(v, ar[c], re); im = fma(v, ai[c], im); }
    const double2 ph = nu.ph[e];
    if (OFFRES) {
        const double2 v = make_double2(re * ph.x - im * ph.y, re * ph.y + im * ph.x), bl = nu.bl[e];
        double2 o = make_double2(v.x * bl.x - v.y * bl.y, v.x * bl.y + v.y * bl.x);
        double2* dst = y + (size_t)b * nu.m + nu.perm[e];
        if (nu.acc) { const double2 p = *dst; o.x += p.x; o.y += p.y; }
        *dst = o;
        return;
    }
    y[(size_t)b * nu.m + nu.perm[e]] = make_double2(re * ph.x - im * ph.y, re * ph.y + im * ph.x);
}

// adjoint spreading: one workgroup per (segment, slice); thread (r1, r2) owns grid point (16 t1 + r1, 16 t2 + r2) of the 2N x 2M grid
constexpr int NU_CH = 64;        // samples staged in LDS at a time
// WEIGHTED: y times the attached sample weight (nu.wgt, ABI order) as it is staged -- the weighted adjoint of DESIGN.md section 21, no pass over y
// OFFRES: then times conj(b_l) of the segment (nu.bl, sorted order) -- it composes with WEIGHTED: A_f^H (w .* y)
template <bool WEIGHTED, bool OFFRES = false>
__global__ __launch_bounds__(NT) void k_nu_spread(NufftDev nu, const double2* __restrict__ y, double2* __restrict__ grid, double2* __restrict__ part) {
    __shared__ double2 vy[NU_CH * DC_MAXS];           // V(t, c) * conj(ph) * y of the staged samples
    __shared__ double wl[NU_CH][2 * NU_TB];           // their weights along both axes at the tile's 16 + 16 grid lines (0 outside the window)
    const NuSeg sg = nu.seg[blockIdx.x];
    const int b = blockIdx.y, tid = threadIdx.x, s = nu.s, N = nu.N, M = nu.M;
    const int t1 = sg.tile / nu.ntile2, t2 = sg.tile - t1 * nu.ntile2;
    const int r1 = tid >> 4, r2 = tid & 15;
    const double inv_hw = 1.0 / nu.hw;
    double ar[DC_MAXS], ai[DC_MAXS];
#pragma unroll
    for (int c = 0; c < DC_MAXS; ++c) { ar[c] = 0.0; ai[c] = 0.0; }
    for (int i0 = sg.b; i0 < sg.e; i0 += NU_CH) {
        const int cnt = min(NU_CH, sg.e - i0);
        __syncthreads();
        for (int it = tid; it < cnt * s; it += NT) {
            const int j = it / s, c = it - j * s;
            const int e = nu.list[i0 + j];
            double2 yv = y[(size_t)b * nu.m + nu.perm[e]];
            const double2 ph = nu.ph[e];
            if (WEIGHTED) { const double wq = nu.wgt[nu.perm[e]]; yv.x *= wq; yv.y *= wq; }
            if (OFFRES) { const double2 bl = nu.bl[e]; yv = make_double2(yv.x * bl.x + yv.y * bl.y, yv.y * bl.x - yv.x * bl.y); }       // y * conj(b_l)
            const double yr = yv.x * ph.x + yv.y * ph.y, yi = yv.y * ph.x - yv.x * ph.y;      // y * conj(ph)
            const double v = nu.Vt[(size_t)nu.t[e] * s + c];
            vy[j * DC_MAXS + c] = make_double2(v * yr, v * yi);
        }
        for (int it = tid; it < cnt * 2 * NU_TB; it += NT) {
            const int j = it / (2 * NU_TB), r = it - j * (2 * NU_TB), ax = r >= NU_TB, rr = r - ax * NU_TB;
            const double2 u = nu.u[nu.list[i0 + j]];
            const double uu = ax ? u.y : u.x;
            const int G = ax ? 2 * M : 2 * N;
            const int k0 = nu_k0(uu, nu.hw);
            const int off = nu_wrap((ax ? t2 : t1) * NU_TB + rr - k0, G);
            wl[j][r] = off < nu.w ? nu_phi(uu - (double)(k0 + off), inv_hw, nu.beta) : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double wt = wl[j][r1] * wl[j][NU_TB + r2];
#pragma unroll
            for (int c = 0; c < DC_MAXS; ++c)
                if (c < s) { const double2 v = vy[j * DC_MAXS + c]; ar[c] = fma(wt, v.x, ar[c]); ai[c] = fma(wt, v.y, ai[c]); }
        }
    }
    const size_t plane = (size_t)N * M, n = plane * s;
    if (sg.slot >= 0) {
        double2* p = part + ((size_t)b * nu.nslot + sg.slot) * (size_t)s * NT + tid;
#pragma unroll
        for (int c = 0; c < DC_MAXS; ++c) if (c < s) st_wt(p + (size_t)c * NT, make_double2(ar[c], ai[c]));
        return;
    }
    const int k1 = t1 * NU_TB + r1, k2 = t2 * NU_TB + r2;
    double2* o = grid + (size_t)b * 4 * n + ((size_t)k1 * 2 * M + k2) * s;
#pragma unroll
    for (int c = 0; c < DC_MAXS; ++c) if (c < s) st_wt(o + c, make_double2(ar[c], ai[c]));
}

// the partial tiles of a split tile, added in segment order; one workgroup per (split tile, slice, channel)
__global__ __launch_bounds__(NT) void k_nu_reduce(NufftDev nu, const double2* __restrict__ part, double2* __restrict__ grid) {
    const NuRed rd = nu.red[blockIdx.x];
    const int b = blockIdx.y, c = blockIdx.z, tid = threadIdx.x, s = nu.s, M = nu.M;
    const int t1 = rd.tile / nu.ntile2, t2 = rd.tile - t1 * nu.ntile2;
    const size_t plane = (size_t)nu.N * M, n = plane * s;
    const int k1 = t1 * NU_TB + (tid >> 4), k2 = t2 * NU_TB + (tid & 15);
    double2* o = grid + (size_t)b * 4 * n + ((size_t)k1 * 2 * M + k2) * s;
    double re = 0.0, im = 0.0;
    for (int q = 0; q < rd.nslot; ++q) {
        const double2 v = part[((size_t)b * nu.nslot + rd.slot0 + q) * (size_t)s * NT + (size_t)c * NT + tid];
        re += v.x; im += v.y;
    }
    st_wt(o + c, make_double2(re, im));
}

// dense inverse w-pass: one workgroup per (k-row kh, sub-grid slice), the s channel lines of sub-grid (kh, .) of the interleaved grid conjugated,
// FFT along w; output in
// the layout k_adj_w leaves for k_adj_h (tmp [c][kh][w], conjugate domain)
template <int R1, int R2>
__global__ __launch_bounds__(NT) void k_nu_adj_w(OpDev op, const double2* __restrict__ spec, double2* __restrict__ tmp) {
    typedef Plan<R1, R2> P;
    constexpr int M = P::N;
    __shared__ cd lds[DC_MAXS * P::LINE];
    const int tid = threadIdx.x, b = blockIdx.y, kh = blockIdx.x, s = op.s, N = op.N;
    const size_t n = (size_t)s * N * M;
    for (int i = tid; i < s * M; i += NT) {
        const int c = i / M, kw = i - c * M;
        const int k1 = 2 * kh + (b & 3 & 1), k2 = 2 * kw + ((b & 3) >> 1);          // sub-grid a = b % 4 of slice b / 4
        const double2 v = spec[(size_t)(b >> 2) * 4 * n + ((size_t)k1 * 2 * M + k2) * s + c];
        lds[c * P::LINE + kw] = mk(v.x, -v.y);
    }
    cd out[R2];
    int line2, k1;
    if (fft_lds<R1, R2, false>(lds, s, op.tw_w, out, line2, k1)) {
        double2* dst = tmp + (size_t)b * n + ((size_t)line2 * N + kh) * M;
#pragma unroll
        for (int k2 = 0; k2 < R2; ++k2) st_wt(dst + k1 + R1 * k2, out[k2]);
    }
}

// images of the 4 sub-grids [B][a][c][q2][q1] -> x [B][c][n2][n1]: sum over a = 0..3 in order of conj(ramp_a) * g_a, times 1 / Phi(p)
// DEAPOD = false: without 1 / Phi -- the crop of the 2N x 2M inverse DFT (toep_kernels.hip, "k_toep_post")
// OFFRES: then times the conjugate of the segment's phase map, added to x for the segments after the first
template <bool DEAPOD, bool OFFRES = false>
__global__ __launch_bounds__(NT) void k_nu_post(NufftDev nu, const double2* __restrict__ g, double2* __restrict__ x) {
    const int N = nu.N, M = nu.M, b = blockIdx.y;
    const size_t plane = (size_t)N * M, n = plane * nu.s;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i / plane), r = (int)(i - (size_t)c * plane), n2 = r / N, n1 = r - n2 * N;
    const int q1 = (n1 + N / 2) % N, q2 = (n2 + M / 2) % M;
    const double2* p = g + (size_t)b * 4 * n + (size_t)c * plane + (size_t)q2 * N + q1;
    const double2 g0 = p[0], g1 = p[n], g2 = p[2 * n], g3 = p[3 * n];
    const double2 e1 = nu.r1[n1], e2 = nu.r2[n2];
    // conj(e1) g1, conj(e2) g2, conj(e1) conj(e2) g3 (the last as conj(e2) (conj(e1) g3))
    const double2 h1 = make_double2(g1.x * e1.x + g1.y * e1.y, g1.y * e1.x - g1.x * e1.y);
    const double2 h2 = make_double2(g2.x * e2.x + g2.y * e2.y, g2.y * e2.x - g2.x * e2.y);
    const double2 t3 = make_double2(g3.x * e1.x + g3.y * e1.y, g3.y * e1.x - g3.x * e1.y);
    const double2 h3 = make_double2(t3.x * e2.x + t3.y * e2.y, t3.y * e2.x - t3.x * e2.y);
    const double re = ((g0.x + h1.x) + h2.x) + h3.x, im = ((g0.y + h1.y) + h2.y) + h3.y;
    if (OFFRES) {
        const double sc = DEAPOD ? nu.dp1[n1] * nu.dp2[n2] : 1.0;
        const double vr = re * sc, vi = im * sc;
        const double2 p = nu.pm[r];
        double2 o = make_double2(vr * p.x + vi * p.y, vi * p.x - vr * p.y);                 // v * conj(P_l)
        if (nu.acc) { const double2 q = x[(size_t)b * n + i]; o.x += q.x; o.y += q.y; }
        x[(size_t)b * n + i] = o;
    } else if (DEAPOD) {
        const double sc = nu.dp1[n1] * nu.dp2[n2];
        x[(size_t)b * n + i] = make_double2(re * sc, im * sc);
    } else {
        x[(size_t)b * n + i] = make_double2(re, im);
    }
}

template <int R1, int R2>
int launch_adj_w_t(qmri_ctx* ctx, const OpDev& op, int B4, const double2* spec, double2* tmp) {
    k_nu_adj_w<R1, R2><<<dim3(op.N, B4), dim3(NT), 0, ctx->stream>>>(op, spec, tmp);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

NufftDev nufft_dev(const qmri_ctx* ctx) {
    const OpHost& o = ctx->op;
    const NufftHost& h = o.nu;
    NufftDev d;
    d.N = o.N; d.M = o.M; d.s = o.s; d.T = o.T; d.m = o.m; d.w = h.w;
    d.beta = h.beta; d.hw = 0.5 * h.w;
    d.ntile2 = 2 * o.M / NU_TB; d.nseg = h.nseg; d.nred = h.nred; d.nslot = h.nslot;
    d.Vt = o.d_Vt; d.u = (const double2*)h.d_u; d.ph = (const double2*)h.d_ph; d.t = h.d_t; d.perm = h.d_perm; d.list = h.d_list;
    d.seg = h.d_seg; d.red = h.d_red; d.dp1 = h.d_dp; d.dp2 = h.d_dp + o.N; d.r1 = h.d_r; d.r2 = h.d_r + o.N;
    d.wgt = h.w_set ? h.d_w : nullptr;
    d.pm = nullptr; d.bl = nullptr; d.acc = 0;
    return d;
}
// the view of segment l of the attached field map
NufftDev nufft_dev_seg(const qmri_ctx* ctx, int l) {
    NufftDev d = nufft_dev(ctx);
    const NufftHost& h = ctx->op.nu;
    d.pm = h.d_pm + (size_t)l * ctx->op.N * ctx->op.M;
    d.bl = h.d_bl + (size_t)l * ctx->op.m;
    d.acc = l > 0;
    return d;
}

template <int W> int launch_interp_t(qmri_ctx* ctx, const NufftDev& nu, int B, const double2* S, double2* y) {
    if (nu.bl) k_nu_interp<W, true><<<dim3((nu.m + NT - 1) / NT, B), dim3(NT), 0, ctx->stream>>>(nu, S, y);
    else k_nu_interp<W><<<dim3((nu.m + NT - 1) / NT, B), dim3(NT), 0, ctx->stream>>>(nu, S, y);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int launch_interp(qmri_ctx* ctx, const NufftDev& nu, int B, const double2* S, double2* y) {
    switch (nu.w) {
#define NU_W_CASE_(w_) case w_: return launch_interp_t<w_>(ctx, nu, B, S, y);
        NU_W_CASE_(2) NU_W_CASE_(3) NU_W_CASE_(4) NU_W_CASE_(5) NU_W_CASE_(6) NU_W_CASE_(7) NU_W_CASE_(8) NU_W_CASE_(9)
        NU_W_CASE_(10) NU_W_CASE_(11) NU_W_CASE_(12) NU_W_CASE_(13) NU_W_CASE_(14) NU_W_CASE_(15) NU_W_CASE_(16)
#undef NU_W_CASE_
        default: qmri_set_error(ctx, "NUFFT kernel width %d unsupported (2..%d)", nu.w, NU_WMAX); return QMRI_ERR_UNSUPPORTED;
    }
}

}  // namespace

NufftDev nufft_dev_view(const qmri_ctx* ctx) { return nufft_dev(ctx); }

// the half-bin ramps of k_nu_pre / k_nu_post without the deapodisation: x [B][n] -> g [B][4][n] and back (toep_kernels.hip)
int nufft_launch_ramps(qmri_ctx* ctx, int B, const double2* x, double2* g) {
    const OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    k_nu_pre<false><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nufft_dev(ctx), x, g);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
int nufft_launch_unramps(qmri_ctx* ctx, int B, const double2* g, double2* x) {
    const OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    k_nu_post<false><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nufft_dev(ctx), g, x);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

// ... with a phase plane pm [N*M] of the field-aware normal operator: x .* pm on the way in, conj(pm) on the way out, added
// to x when acc
int nufft_launch_ramps_pm(qmri_ctx* ctx, int B, const double2* x, double2* g, const double2* pm) {
    const OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    NufftDev nu = nufft_dev(ctx);
    nu.pm = pm;
    k_nu_pre<false, true><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nu, x, g);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
int nufft_launch_unramps_pm(qmri_ctx* ctx, int B, const double2* g, double2* x, const double2* pm, bool acc) {
    const OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    NufftDev nu = nufft_dev(ctx);
    nu.pm = pm; nu.acc = acc ? 1 : 0;
    k_nu_post<false, true><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nu, g, x);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int nufft_launch_fwd(qmri_ctx* ctx, int B, const double2* x, double2* y) {
    OpHost& o = ctx->op;
    if (o.kind != OP_NUFFT || B < 1 || B > o.maxB) { qmri_set_error(ctx, "nufft_launch_fwd: no trajectory operator / batch out of range (internal)"); return QMRI_ERR_STATE; }
    const OpDev op = qmri_opdev(ctx);
    const size_t n = (size_t)o.N * o.M * o.s;
    if (o.nu.fm_set) {
        // a field map: the chain once per segment, the B entries of the call at a time (the work buffers hold max_batch entries, which the callers
        // fill), y = sum_l b_l .* NUFFT(P_l .* x) in segment order
        for (int l = 0; l < o.nu.fm_L; ++l) {
            const NufftDev nl = nufft_dev_seg(ctx, l);
            k_nu_pre<true, true><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nl, x, o.nu.d_g);
            QMRI_HIP(ctx, hipGetLastError());
            QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, 4 * B, o.nu.d_g, o.nu.d_grid, o.nu.d_g, nullptr));
            k_nu_interleave<<<dim3((unsigned)((4 * n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nl, o.nu.d_g, o.nu.d_grid);
            QMRI_HIP(ctx, hipGetLastError());
            QMRI_TRY(launch_interp(ctx, nl, B, o.nu.d_grid, y));
        }
        return QMRI_OK;
    }
    const NufftDev nu = nufft_dev(ctx);
    k_nu_pre<true><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nu, x, o.nu.d_g);
    QMRI_HIP(ctx, hipGetLastError());
    // the 4 sub-grids of every slice as 4B slices through the dense spectrum passes (d_grid as their workspace, the spectra back into d_g)
    QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, 4 * B, o.nu.d_g, o.nu.d_grid, o.nu.d_g, nullptr));
    k_nu_interleave<<<dim3((unsigned)((4 * n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nu, o.nu.d_g, o.nu.d_grid);
    QMRI_HIP(ctx, hipGetLastError());
    return launch_interp(ctx, nu, B, o.nu.d_grid, y);
}

// plain: the uncorrected transform even while a field map is attached (the Toeplitz set-ups build point-spread functions of the trajectory alone)
static int launch_adj(qmri_ctx* ctx, int B, const double2* y, double2* x, bool weighted, bool plain) {
    OpHost& o = ctx->op;
    if (o.kind != OP_NUFFT || B < 1 || B > o.maxB) { qmri_set_error(ctx, "nufft_launch_adj: no trajectory operator / batch out of range (internal)"); return QMRI_ERR_STATE; }
    const NufftDev nu = nufft_dev(ctx);
    if (weighted && !nu.wgt) { qmri_set_error(ctx, "nufft_launch_adj_w: no sample weights attached (internal)"); return QMRI_ERR_STATE; }
    const OpDev op = qmri_opdev(ctx);
    const size_t n = (size_t)o.N * o.M * o.s;
    if (o.nu.fm_set && !plain) {
        // x = sum_l conj(P_l) .* NUFFT^H(conj(b_l) .* (w .*) y) in segment order: the exact transpose of the forward's segments
        for (int l = 0; l < o.nu.fm_L; ++l) {
            const NufftDev nl = nufft_dev_seg(ctx, l);
            if (weighted) k_nu_spread<true, true><<<dim3(nl.nseg, B), dim3(NT), 0, ctx->stream>>>(nl, y, o.nu.d_grid, o.nu.d_part);
            else k_nu_spread<false, true><<<dim3(nl.nseg, B), dim3(NT), 0, ctx->stream>>>(nl, y, o.nu.d_grid, o.nu.d_part);
            QMRI_HIP(ctx, hipGetLastError());
            if (nl.nred > 0) {
                k_nu_reduce<<<dim3(nl.nred, B, nl.s), dim3(NT), 0, ctx->stream>>>(nl, o.nu.d_part, o.nu.d_grid);
                QMRI_HIP(ctx, hipGetLastError());
            }
            QMRI_TRY(with_plan(ctx, op.M, [&](auto p) { return launch_adj_w_t<decltype(p)::R1, decltype(p)::R2>(ctx, op, 4 * B, o.nu.d_grid, o.nu.d_g); }));
            QMRI_TRY(dc_launch_adj_h(ctx, op, 4 * B, o.nu.d_g, o.nu.d_grid));
            k_nu_post<true, true><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nl, o.nu.d_grid, x);
            QMRI_HIP(ctx, hipGetLastError());
        }
        return QMRI_OK;
    }
    if (weighted) k_nu_spread<true><<<dim3(nu.nseg, B), dim3(NT), 0, ctx->stream>>>(nu, y, o.nu.d_grid, o.nu.d_part);
    else k_nu_spread<false><<<dim3(nu.nseg, B), dim3(NT), 0, ctx->stream>>>(nu, y, o.nu.d_grid, o.nu.d_part);
    QMRI_HIP(ctx, hipGetLastError());
    if (nu.nred > 0) {
        k_nu_reduce<<<dim3(nu.nred, B, nu.s), dim3(NT), 0, ctx->stream>>>(nu, o.nu.d_part, o.nu.d_grid);
        QMRI_HIP(ctx, hipGetLastError());
    }
    QMRI_TRY(with_plan(ctx, op.M, [&](auto p) { return launch_adj_w_t<decltype(p)::R1, decltype(p)::R2>(ctx, op, 4 * B, o.nu.d_grid, o.nu.d_g); }));
    QMRI_TRY(dc_launch_adj_h(ctx, op, 4 * B, o.nu.d_g, o.nu.d_grid));
    k_nu_post<true><<<dim3((unsigned)((n + NT - 1) / NT), B), dim3(NT), 0, ctx->stream>>>(nu, o.nu.d_grid, x);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int nufft_launch_adj(qmri_ctx* ctx, int B, const double2* y, double2* x) { return launch_adj(ctx, B, y, x, false, false); }
int nufft_launch_adj_w(qmri_ctx* ctx, int B, const double2* y, double2* x) { return launch_adj(ctx, B, y, x, true, false); }
int nufft_launch_adj_plain(qmri_ctx* ctx, int B, const double2* y, double2* x) { return launch_adj(ctx, B, y, x, false, true); }
