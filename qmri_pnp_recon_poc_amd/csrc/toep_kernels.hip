// toep_kernels.hip -- the normal operator A^H A of a trajectory operator as a block-Toeplitz convolution, fp64, gfx950.
//
//   (A^H A x)_c[n] = sum_c' sum_n' q_{c,c'}[n - n'] x_c'[n'],     q_{c,c'}[d] = (1/NM) sum_i V(t_i, c) V(t_i, c') exp(i omega_i . d)
//                  = crop_{N x M}( IDFT_{2N x 2M}( K^(k) . DFT_{2N x 2M}(zero-padded x) ) ),
// K^(k) the s x s matrix of 2N x 2M DFTs of q with the lines d1 = -N, d2 = -M set to zero: Hermitian at every bin, stored as its upper triangle.
//
// Set-up (toep_prepare, once per trajectory): per source channel c' and quadrant off in {0, -N} x {0, -M}, the adjoint NUFFT of
// y_i = V(t_i, c') exp(i omega_i . off) is sqrt(NM) q_{., c'}[n + off] for every c at once (k_toep_synth + nufft_launch_adj).  k_toep_combine folds
// the four quadrants of a 2N x 2M line pair into the four N x M sub-grids (bin 2 j + a = DFT_N of (q[n] + (-1)^a q[n + N]) exp(-i pi a n / N)), so
// that no FFT above 256 points is needed; dc_kernels.hip's dense passes transform them; k_toep_pack keeps c <= c'.
//
// Apply (toep_apply, the hot path): the ramps of k_nu_pre without 1 / Phi (nufft_launch_ramps), the dense forward passes, k_toep_mul, k_toep_adj_w
// and the dense inverse h-pass, the conjugate ramps of k_nu_post without 1 / Phi (nufft_launch_unramps).  No gather, no floating-point atomics;
// every image of a batch goes through the same instructions in the same order, so a slice's bits do not depend on the batch.
//
// With a field map attached and qmri_nufft_prepare_normal_fm called for it toep_apply runs A_f^H A_f ~ sum_l P_l^H T_l P_l: per
// segment l of the difference phase the same chain on that segment's K^ (built by toep_build_weighted with the real sample weights c_l(tau_i)), the
// ramps as their OFFRES instantiations (x times the phase plane P_l on the way in, conj(P_l) on the way out, adding for l > 0).
//
// Solver (qmri_cg_toep_batch_dev, QMRI_SOLVER_TOEPLITZ): conjugate gradients on (A_mc^H A_mc + r I) x = A_mc^H y + r z with
// A_mc^H A_mc x = sum_j conj(C_j) . T (C_j . x), the discipline of the multi-coil LSQR (mc_kernels.hip): scalars on the device, norms from PS fixed
// partials per slice added in one order, per-slice stopping, one event wait per chunk of iterations.
#include <cmath>
#include <vector>
#include "dc_device.h"

using namespace dcdev;

namespace {
constexpr int PS = 256;          // partial sums per slice vector

__device__ __forceinline__ int toep_pair(int c, int cp) { return cp * (cp + 1) / 2 + c; }      // c <= cp

// y[perm[e]] = V(t_e, cp) exp(-i pi (b1 u1 + b2 u2)):  omega . off with off = (-b1 N, -b2 M) and u = omega (N, M) / pi
// WEIGHTED: times the real weight cw[e] (sorted order) -- segment l of the field-aware normal operator, cw = c_l(tau)
template <bool WEIGHTED>
__global__ __launch_bounds__(NT) void k_toep_synth(NufftDev nu, int cp, int b1, int b2, const double* __restrict__ cw, double2* __restrict__ y) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= nu.m) return;
    const double2 u = nu.u[e];
    double sn, cs;
    sincospi(-((double)b1 * u.x + (double)b2 * u.y), &sn, &cs);
    double v = nu.Vt[(size_t)nu.t[e] * nu.s + cp];
    if (WEIGHTED) v *= cw[e];
    y[nu.perm[e]] = make_double2(v * cs, v * sn);
}

// Q [quadrant b = b1 + 2 b2][c][n2][n1] -> h [a = a1 + 2 a2][c][n2][n1] = (1/4) ramp_a[n] sum_b (-1)^(a1 b1 + a2 b2) Q_b[n], the lines n1 = 0 of
// b1 = 1 and n2 = 0 of b2 = 1 (d = -N, -M) dropped.  ramp_a[n] = exp(-i pi (a1 n1 / N + a2 n2 / M)) = (-i r1[n1])^a1 (-i r2[n2])^a2 with the
// centred ramps r of the NUFFT plan (exp(-i pi (n - N/2) / N) = i exp(-i pi n / N)).
__global__ __launch_bounds__(NT) void k_toep_combine(NufftDev nu, const double2* __restrict__ Q, double2* __restrict__ h) {
    const int N = nu.N, M = nu.M;
    const size_t plane = (size_t)N * M, n = plane * nu.s;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int r = (int)(i % plane), n2 = r / N, n1 = r - n2 * N;
    const double k1 = n1 ? 1.0 : 0.0, k2 = n2 ? 1.0 : 0.0;             // (the adjoint's values are finite: a product with 0 drops the line)
    const double2 q0 = Q[i], l1 = Q[n + i], l2 = Q[2 * n + i], l3 = Q[3 * n + i];
    const double2 q1 = make_double2(l1.x * k1, l1.y * k1), q2 = make_double2(l2.x * k2, l2.y * k2), q3 = make_double2(l3.x * (k1 * k2), l3.y * (k1 * k2));
    const double2 r1 = nu.r1[n1], r2 = nu.r2[n2];
    const double2 e1 = make_double2(r1.y, -r1.x), e2 = make_double2(r2.y, -r2.x);      // -i r
    const double2 s0 = make_double2(0.25 * (((q0.x + q1.x) + q2.x) + q3.x), 0.25 * (((q0.y + q1.y) + q2.y) + q3.y));
    const double2 s1 = make_double2(0.25 * (((q0.x - q1.x) + q2.x) - q3.x), 0.25 * (((q0.y - q1.y) + q2.y) - q3.y));
    const double2 s2 = make_double2(0.25 * (((q0.x + q1.x) - q2.x) - q3.x), 0.25 * (((q0.y + q1.y) - q2.y) - q3.y));
    const double2 s3 = make_double2(0.25 * (((q0.x - q1.x) - q2.x) + q3.x), 0.25 * (((q0.y - q1.y) - q2.y) + q3.y));
    const double2 h1 = make_double2(s1.x * e1.x - s1.y * e1.y, s1.x * e1.y + s1.y * e1.x);
    const double2 h2 = make_double2(s2.x * e2.x - s2.y * e2.y, s2.x * e2.y + s2.y * e2.x);
    const double2 t3 = make_double2(s3.x * e1.x - s3.y * e1.y, s3.x * e1.y + s3.y * e1.x);
    const double2 h3 = make_double2(t3.x * e2.x - t3.y * e2.y, t3.x * e2.y + t3.y * e2.x);
    st_wt(h + i, s0);
    st_wt(h + n + i, h1);
    st_wt(h + 2 * n + i, h2);
    st_wt(h + 3 * n + i, h3);
}

// the spectra S [a][c][j1][j2] of column cp -> K^ [pair(c, cp)][a][j1][j2] for c <= cp; the diagonal is real (its imaginary part is NUFFT error)
__global__ __launch_bounds__(NT) void k_toep_pack(int s, size_t plane, int cp, const double2* __restrict__ S, double2* __restrict__ K) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= 4 * plane) return;
    const size_t a = i / plane, j = i - a * plane;
    double2 v = S[a * plane * s + (size_t)c * plane + j];
    if (c == cp) v.y = 0.0;
    st_wt(K + (size_t)toep_pair(c, cp) * 4 * plane + i, v);
}

// per bin: X_c <- sum_c' K^_{c,c'} X_c' on the sub-grid spectra X [B][a][c][j1][j2], one lane per bin (a, j1, j2) and BC images per pass: the
// 2 s BC doubles of X and of the sums stay in registers while the s (s + 1) / 2 pair planes stream through once (coalesced 16-byte loads), the lower
// triangle by conjugation.  Explicit fma in one fixed order: an image's bits are the same at any BC and any position.
template <int BC>
__global__ __launch_bounds__(NT) void k_toep_mul(int s, size_t plane, int B, const double2* __restrict__ K, double2* __restrict__ X) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= 4 * plane) return;
    const size_t a = i / plane, j = i - a * plane, n = plane * s;
    for (int b0 = 0; b0 < B; b0 += BC) {
        double xr[BC][DC_MAXS], xi[BC][DC_MAXS], ar[BC][DC_MAXS], ai[BC][DC_MAXS];
#pragma unroll
        for (int q = 0; q < BC; ++q) {
            const double2* p = X + ((size_t)min(b0 + q, B - 1) * 4 + a) * n + j;
#pragma unroll
            for (int c = 0; c < DC_MAXS; ++c) {
                ar[q][c] = 0.0; ai[q][c] = 0.0; xr[q][c] = 0.0; xi[q][c] = 0.0;
                if (c < s) { const double2 v = p[(size_t)c * plane]; xr[q][c] = v.x; xi[q][c] = v.y; }
            }
        }
#pragma unroll
        for (int cp = 0; cp < DC_MAXS; ++cp) {
#pragma unroll
            for (int c = 0; c <= cp; ++c) {
                if (cp >= s) continue;
                const double2 k = K[(size_t)toep_pair(c, cp) * 4 * plane + i];
#pragma unroll
                for (int q = 0; q < BC; ++q) {
                    if (c == cp) {
                        ar[q][c] = fma(k.x, xr[q][c], ar[q][c]);
                        ai[q][c] = fma(k.x, xi[q][c], ai[q][c]);
                    } else {
                        ar[q][c] = fma(-k.y, xi[q][cp], fma(k.x, xr[q][cp], ar[q][c]));        // K X_c'
                        ai[q][c] = fma(k.y, xr[q][cp], fma(k.x, xi[q][cp], ai[q][c]));
                        ar[q][cp] = fma(k.y, xi[q][c], fma(k.x, xr[q][c], ar[q][cp]));         // conj(K) X_c
                        ai[q][cp] = fma(-k.y, xr[q][c], fma(k.x, xi[q][c], ai[q][cp]));
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < BC; ++q) {
            double2* p = X + ((size_t)min(b0 + q, B - 1) * 4 + a) * n + j;
#pragma unroll
            for (int c = 0; c < DC_MAXS; ++c)
                if (c < s && b0 + q < B) st_wt(p + (size_t)c * plane, make_double2(ar[q][c], ai[q][c]));
        }
    }
}

// dense inverse w-pass (k_nu_adj_w's twin on the sub-grid layout): one workgroup per (k-row kh, sub-grid slice), the s channel lines of S [c][kh][.]
// conjugated, FFT along w; output as k_adj_w leaves it for k_adj_h (tmp [c][kh][w], conjugate domain)
template <int R1, int R2>
__global__ __launch_bounds__(NT) void k_toep_adj_w(OpDev op, const double2* __restrict__ spec, double2* __restrict__ tmp) {
    typedef Plan<R1, R2> P;
    constexpr int M = P::N;
    __shared__ cd lds[DC_MAXS * P::LINE];
    const int tid = threadIdx.x, b = blockIdx.y, kh = blockIdx.x, s = op.s, N = op.N;
    const size_t n = (size_t)s * N * M;
    for (int i = tid; i < s * M; i += NT) {
        const int c = i / M, kw = i - c * M;
        const double2 v = spec[(size_t)b * n + ((size_t)c * N + kh) * M + kw];
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
template <int R1, int R2>
int launch_toep_adj_w_t(qmri_ctx* ctx, const OpDev& op, int B4, const double2* spec, double2* tmp) {
    k_toep_adj_w<R1, R2><<<dim3(op.N, B4), dim3(NT), 0, ctx->stream>>>(op, spec, tmp);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

// ---------------------------------------------------------------------------------------------------
// conjugate gradients on (A_mc^H A_mc + r I) x = b.  Per slice in LsqrState: n2b = ||b||, tolb = tol ||b||, sc[0].phi = ||res||^2 of the recurrence,
// sc[0].alpha, sc[0].beta, iter / done / flag.  Grid of the vector kernels: PS x B, a slice's vector strided over its PS workgroups.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double tcg_block_sum(double v, double* sh) {      // lanes by a fixed tree, waves in index order (valid in thread 0)
    v = wave_sum_all(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int w = 0; w < NT / 64; ++w) t += sh[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ double tcg_wave_sum(const double* p, int cnt) {   // one wave: lane l adds p[l], p[l + 64], ..., then the tree
    double v = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 64) v += p[i];
    return wave_sum_all(v);
}

// b = t + r z (into t), partial |b|^2
__global__ __launch_bounds__(NT) void k_tcg_rhs(size_t n, double r, const double2* __restrict__ z, double2* __restrict__ t, double* __restrict__ pb) {
    __shared__ double sh[NT / 64];
    const size_t o = (size_t)blockIdx.y * n;
    double a = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        const double2 tv = t[o + i], zv = z[o + i];
        const double2 w = make_double2(fma(r, zv.x, tv.x), fma(r, zv.y, tv.y));
        t[o + i] = w;
        a = fma(w.x, w.x, fma(w.y, w.y, a));
    }
    a = tcg_block_sum(a, sh);
    if (threadIdx.x == 0) pb[(size_t)blockIdx.y * PS + blockIdx.x] = a;
}
// res = b - (q + r x) with q = A_mc^H A_mc x,  p = res,  partial |res|^2
__global__ __launch_bounds__(NT) void k_tcg_res0(size_t n, double r, const double2* __restrict__ bv, const double2* __restrict__ q, const double2* __restrict__ x,
                                                 double2* __restrict__ res, double2* __restrict__ p, double* __restrict__ pr) {
    __shared__ double sh[NT / 64];
    const size_t o = (size_t)blockIdx.y * n;
    double a = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        const double2 b = bv[o + i], qv = q[o + i], xv = x[o + i];
        const double2 w = make_double2(b.x - fma(r, xv.x, qv.x), b.y - fma(r, xv.y, qv.y));
        res[o + i] = w; p[o + i] = w;
        a = fma(w.x, w.x, fma(w.y, w.y, a));
    }
    a = tcg_block_sum(a, sh);
    if (threadIdx.x == 0) pr[(size_t)blockIdx.y * PS + blockIdx.x] = a;
}
// q += r p,  partial real(<p, q>)
__global__ __launch_bounds__(NT) void k_tcg_pq(size_t n, double r, const double2* __restrict__ p, const LsqrState* __restrict__ st, double2* __restrict__ q,
                                               double* __restrict__ pq) {
    __shared__ double sh[NT / 64];
    if (st[blockIdx.y].done) return;
    const size_t o = (size_t)blockIdx.y * n;
    double a = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        const double2 pv = p[o + i], qv = q[o + i];
        const double2 w = make_double2(fma(r, pv.x, qv.x), fma(r, pv.y, qv.y));
        q[o + i] = w;
        a = fma(pv.x, w.x, fma(pv.y, w.y, a));
    }
    a = tcg_block_sum(a, sh);
    if (threadIdx.x == 0) pq[(size_t)blockIdx.y * PS + blockIdx.x] = a;
}
// x += alpha p,  res -= alpha q,  partial |res|^2
__global__ __launch_bounds__(NT) void k_tcg_xr(size_t n, const double2* __restrict__ p, const double2* __restrict__ q, const LsqrState* __restrict__ st,
                                               double2* __restrict__ x, double2* __restrict__ res, double* __restrict__ pr) {
    __shared__ double sh[NT / 64];
    if (st[blockIdx.y].done) return;
    const size_t o = (size_t)blockIdx.y * n;
    const double al = st[blockIdx.y].sc[0].alpha;
    double a = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        const double2 pv = p[o + i], qv = q[o + i], xv = x[o + i], rv = res[o + i];
        x[o + i] = make_double2(fma(al, pv.x, xv.x), fma(al, pv.y, xv.y));
        const double2 w = make_double2(fma(-al, qv.x, rv.x), fma(-al, qv.y, rv.y));
        res[o + i] = w;
        a = fma(w.x, w.x, fma(w.y, w.y, a));
    }
    a = tcg_block_sum(a, sh);
    if (threadIdx.x == 0) pr[(size_t)blockIdx.y * PS + blockIdx.x] = a;
}
// p = res + beta p
__global__ __launch_bounds__(NT) void k_tcg_p(size_t n, const double2* __restrict__ res, const LsqrState* __restrict__ st, double2* __restrict__ p) {
    if (st[blockIdx.y].done) return;
    const size_t o = (size_t)blockIdx.y * n;
    const double be = st[blockIdx.y].sc[0].beta;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        const double2 rv = res[o + i], pv = p[o + i];
        p[o + i] = make_double2(fma(be, pv.x, rv.x), fma(be, pv.y, rv.y));
    }
}

enum { TCG_INIT = 0, TCG_ALPHA = 1, TCG_BETA = 2 };
struct TcgArgs { LsqrState* st; LsqrState* hst; double *pb, *pr, *pq; int ii, maxit; double tol; };
__device__ void tcg_tell(const TcgArgs& a, int b, const LsqrState& s) {
    LsqrState* h = a.hst + b;
    h->iter = s.iter; h->flag = s.flag; h->done = s.done;
}
// the scalar recurrences and the stop rule, one wave per slice (grid: B x 64)
__global__ __launch_bounds__(64) void k_tcg_scalar(int stage, TcgArgs a) {
    const int b = blockIdx.x;
    LsqrState& S = a.st[b];
    LsqrScalars& q = S.sc[0];
    if (stage != TCG_INIT && S.done) return;
    if (stage == TCG_INIT) {
        const double sb = tcg_wave_sum(a.pb + (size_t)b * PS, PS), sr = tcg_wave_sum(a.pr + (size_t)b * PS, PS);
        if (threadIdx.x) return;
        S.n2b = sqrt(sb);
        S.tolb = a.tol * S.n2b;
        q.phi = sr; q.alpha = 0.0; q.beta = 0.0;
        S.iter = 0; S.done = 0; S.flag = 1;
        if (sqrt(sr) <= S.tolb) { S.done = 1; S.flag = 0; }
        else if (a.maxit == 0) S.done = 1;
        tcg_tell(a, b, S);
    } else if (stage == TCG_ALPHA) {
        const double pq = tcg_wave_sum(a.pq + (size_t)b * PS, PS);
        if (threadIdx.x) return;
        if (!(pq > 0.0)) { S.done = 1; S.iter = a.ii - 1; S.flag = 3; tcg_tell(a, b, S); return; }      // breakdown (non-finite data)
        q.alpha = q.phi / pq;
    } else {
        const double sr = tcg_wave_sum(a.pr + (size_t)b * PS, PS);
        if (threadIdx.x) return;
        q.beta = sr / q.phi;
        q.phi = sr;
        if (sqrt(sr) <= S.tolb) { S.done = 1; S.iter = a.ii; S.flag = 0; }
        else if (a.ii == a.maxit) { S.done = 1; S.iter = a.maxit; S.flag = 1; }
        if (S.done) tcg_tell(a, b, S);
    }
}

// q [B][n] = A_mc^H A_mc p: the coil images of all slices through toep_apply max_batch at a time, added coil after coil in ascending order
int tcg_normal_chunks(qmri_ctx* ctx, int B, int ncoil, const double2* maps, const double2* p, const LsqrState* st, double2* q) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    for (int g0 = 0; g0 < B * ncoil; g0 += o.maxB) {
        const int cnt = std::min(o.maxB, B * ncoil - g0);
        QMRI_TRY(mc_launch_coil_mul(ctx, ncoil, g0, cnt, p, maps, st, w.scr));
        QMRI_TRY(toep_apply(ctx, cnt, w.scr, w.scr));
        QMRI_TRY(mc_launch_coil_sum(ctx, ncoil, g0, cnt, w.scr, maps, st, q));
    }
    return QMRI_OK;
}
}  // namespace

// K^ of one Toeplitz operator into khat [pair][a][j1][j2]; d_c == nullptr: the plain one, else the samples weighted by d_c [m] (sorted order).  The
// adjoint NUFFTs are the PLAIN transform whether or not a field map is attached: the point-spread function is the trajectory's.
int toep_build_weighted(qmri_ctx* ctx, const double* d_c, double2* khat) {
    OpHost& o = ctx->op;
    NufftHost& h = o.nu;
    if (o.kind != OP_NUFFT) { qmri_set_error(ctx, "toep_prepare: no trajectory operator (internal)"); return QMRI_ERR_STATE; }
    const size_t plane = (size_t)o.N * o.M, n = plane * o.s;
    DevBuf<double2> Q, y;
    QMRI_TRY(Q.ensure(ctx, 4 * n));
    QMRI_TRY(y.ensure(ctx, (size_t)o.m));
    const NufftDev nu = nufft_dev_view(ctx);
    const OpDev op = qmri_opdev(ctx);
    for (int cp = 0; cp < o.s; ++cp) {
        for (int b = 0; b < 4; ++b) {
            if (d_c) k_toep_synth<true><<<dim3((o.m + NT - 1) / NT), dim3(NT), 0, ctx->stream>>>(nu, cp, b & 1, b >> 1, d_c, y);
            else k_toep_synth<false><<<dim3((o.m + NT - 1) / NT), dim3(NT), 0, ctx->stream>>>(nu, cp, b & 1, b >> 1, nullptr, y);
            QMRI_HIP(ctx, hipGetLastError());
            QMRI_TRY(nufft_launch_adj_plain(ctx, 1, y, Q + (size_t)b * n));
        }
        k_toep_combine<<<dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, ctx->stream>>>(nu, Q, h.d_g);
        QMRI_HIP(ctx, hipGetLastError());
        // the four sub-grids as four slices through the dense spectrum passes (unitary: 1 / sqrt(NM), which the adjoint's own 1 / sqrt(NM) left over)
        QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, 4, h.d_g, h.d_grid, h.d_g, nullptr));
        k_toep_pack<<<dim3((unsigned)((4 * plane + NT - 1) / NT), cp + 1), dim3(NT), 0, ctx->stream>>>(o.s, plane, cp, h.d_g, khat);
        QMRI_HIP(ctx, hipGetLastError());
    }
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));           // (Q and y are released on return)
    return QMRI_OK;
}

int toep_prepare(qmri_ctx* ctx) {
    OpHost& o = ctx->op;
    NufftHost& h = o.nu;
    if (o.kind != OP_NUFFT) { qmri_set_error(ctx, "toep_prepare: no trajectory operator (internal)"); return QMRI_ERR_STATE; }
    if (h.fm_set && h.fmn_ready && !h.fmn_plain) return QMRI_OK;      // the field-aware transform is the one in force: the plain one is not needed
    if (h.khat_ready) return QMRI_OK;
    const size_t plane = (size_t)o.N * o.M, npair = (size_t)o.s * (o.s + 1) / 2;
    if (!h.d_khat) QMRI_TRY(ctx->op.pool.alloc(ctx, &h.d_khat, npair * 4 * plane));
    QMRI_TRY(toep_build_weighted(ctx, nullptr, h.d_khat));
    h.khat_ready = true;
    return QMRI_OK;
}

// the passes between the ramps: d_g [B][4][n] -> spectra, times khat, back to the sub-grid images in d_g
static int toep_core(qmri_ctx* ctx, const OpDev& op, int B, const double2* khat) {
    OpHost& o = ctx->op;
    const size_t plane = (size_t)o.N * o.M;
    const unsigned gm = (unsigned)((4 * plane + NT - 1) / NT);
    QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, 4 * B, o.nu.d_g, o.nu.d_grid, o.nu.d_g, nullptr));
    if (B == 1) k_toep_mul<1><<<dim3(gm), dim3(NT), 0, ctx->stream>>>(o.s, plane, B, khat, o.nu.d_g);
    else k_toep_mul<2><<<dim3(gm), dim3(NT), 0, ctx->stream>>>(o.s, plane, B, khat, o.nu.d_g);
    QMRI_HIP(ctx, hipGetLastError());
    QMRI_TRY(with_plan(ctx, op.M, [&](auto p) { return launch_toep_adj_w_t<decltype(p)::R1, decltype(p)::R2>(ctx, op, 4 * B, o.nu.d_g, o.nu.d_grid); }));
    return dc_launch_adj_h(ctx, op, 4 * B, o.nu.d_grid, o.nu.d_g);
}

int toep_apply(qmri_ctx* ctx, int B, const double2* x, double2* out) {
    OpHost& o = ctx->op;
    NufftHost& h = o.nu;
    if (o.kind != OP_NUFFT || B < 1 || B > o.maxB) { qmri_set_error(ctx, "toep_apply: no trajectory operator / batch out of range (internal)"); return QMRI_ERR_STATE; }
    if (h.fm_set && !h.fmn_ready) { qmri_set_error(ctx, "toep_apply: a field map without its normal operator (internal)"); return QMRI_ERR_STATE; }
    const OpDev op = qmri_opdev(ctx);
    if (h.fm_set && !h.fmn_plain) {
        // A_f^H A_f x ~ sum_l conj(P_l) .* T_l (P_l .* x), segments one after the other on the stream; every output element is owned by one thread
        // of k_nu_post, which stores for l = 0 and adds for l > 0.  out == x: the later segments read the copy of x made here.
        const size_t plane = (size_t)o.N * o.M, n = plane * o.s, kseg = (size_t)o.s * (o.s + 1) / 2 * 4 * plane;
        if (x == out && h.fmn_L > 1) {
            QMRI_HIP(ctx, hipMemcpyAsync(h.d_xs, x, (size_t)B * n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
            x = h.d_xs;
        }
        for (int l = 0; l < h.fmn_L; ++l) {
            const double2* pm = h.d_pm_n + (size_t)l * plane;
            QMRI_TRY(nufft_launch_ramps_pm(ctx, B, x, h.d_g, pm));
            QMRI_TRY(toep_core(ctx, op, B, h.d_khat_fm + (size_t)l * kseg));
            QMRI_TRY(nufft_launch_unramps_pm(ctx, B, h.d_g, out, pm, l > 0));
        }
        return QMRI_OK;
    }
    QMRI_TRY(toep_prepare(ctx));
    QMRI_TRY(nufft_launch_ramps(ctx, B, x, h.d_g));
    QMRI_TRY(toep_core(ctx, op, B, h.d_khat));
    return nufft_launch_unramps(ctx, B, h.d_g, out);
}

// CG on (A_mc^H A_mc + r I) x = A_mc^H y + r z for B slices from x0 = d_x (device, overwritten with the solutions); operands as qmri_lsqr_mc_batch_dev.
// Stops at the first k with ||res_k|| <= tol ||b|| (res the recurrence's residual; flag 0), or at maxit (flag 1); iters_out reports k.
int qmri_cg_toep_batch_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                           double2* d_x, int32_t* iters_out, int32_t* flags_out) {
    OpHost& o = ctx->op;
    QMRI_TRY(toep_prepare(ctx));
    QMRI_TRY(mc_ensure_work(ctx, B, ncoil));
    McWork& w = o.mc;
    const size_t n = (size_t)o.N * o.M * o.s;
    double2 *res = w.ub, *p = w.v, *q = w.d, *bv = w.t;
    TcgArgs a{w.st, w.hst, w.part, w.part + (size_t)B * PS, w.part + 2 * (size_t)B * PS, 0, maxit, tol};
    const dim3 gs(PS, B), blk(NT);
    QMRI_TRY(mc_adjoint_batch_dev(ctx, B, ncoil, d_maps, d_y, bv));          // the one gather of the x-update
    k_tcg_rhs<<<gs, blk, 0, ctx->stream>>>(n, r, d_z, bv, a.pb);
    QMRI_HIP(ctx, hipGetLastError());
    QMRI_TRY(tcg_normal_chunks(ctx, B, ncoil, d_maps, d_x, nullptr, q));
    k_tcg_res0<<<gs, blk, 0, ctx->stream>>>(n, r, bv, q, d_x, res, p, a.pr);
    QMRI_HIP(ctx, hipGetLastError());
    k_tcg_scalar<<<dim3(B), dim3(64), 0, ctx->stream>>>(TCG_INIT, a);
    QMRI_HIP(ctx, hipGetLastError());
    if (!ctx->ev_state) QMRI_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_state, hipEventDisableTiming));
    QMRI_HIP(ctx, hipEventRecord(ctx->ev_state, ctx->stream));
    QMRI_HIP(ctx, hipEventSynchronize(ctx->ev_state));
    bool any = false;
    for (int b = 0; b < B; ++b) any |= !w.hst[b].done;
    int ii = 1, chunk = std::max(1, std::min(maxit, w.pred_cg));
    for (; any;) {
        const int last = std::min(maxit, ii + chunk - 1);
        for (; ii <= last; ++ii) {
            a.ii = ii;
            QMRI_TRY(tcg_normal_chunks(ctx, B, ncoil, d_maps, p, w.st, q));
            k_tcg_pq<<<gs, blk, 0, ctx->stream>>>(n, r, p, w.st, q, a.pq);
            QMRI_HIP(ctx, hipGetLastError());
            k_tcg_scalar<<<dim3(B), dim3(64), 0, ctx->stream>>>(TCG_ALPHA, a);
            QMRI_HIP(ctx, hipGetLastError());
            k_tcg_xr<<<gs, blk, 0, ctx->stream>>>(n, p, q, w.st, d_x, res, a.pr);
            QMRI_HIP(ctx, hipGetLastError());
            k_tcg_scalar<<<dim3(B), dim3(64), 0, ctx->stream>>>(TCG_BETA, a);
            QMRI_HIP(ctx, hipGetLastError());
            k_tcg_p<<<gs, blk, 0, ctx->stream>>>(n, res, w.st, p);
            QMRI_HIP(ctx, hipGetLastError());
        }
        QMRI_HIP(ctx, hipEventRecord(ctx->ev_state, ctx->stream));
        QMRI_HIP(ctx, hipEventSynchronize(ctx->ev_state));
        bool active = false;
        for (int b = 0; b < B; ++b) active |= !w.hst[b].done;
        if (!active || ii > maxit) break;
        chunk = std::max(2, w.pred_cg / 4);
    }
    int most = 0;
    for (int b = 0; b < B; ++b) {
        if (iters_out) iters_out[b] = w.hst[b].iter;
        if (flags_out) flags_out[b] = w.hst[b].flag;
        most = std::max(most, (int)w.hst[b].iter);
    }
    w.pred_cg = std::max(1, most);
    return QMRI_OK;
}
