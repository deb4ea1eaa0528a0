// offres_kernels.hip -- attach-time kernels of the time-segmented off-resonance correction (qmri_set_field_map), fp64, gfx950.
//
//   exp(-i 2 pi f tau_i) ~ sum_{l<L} b_l(tau_i) exp(-i 2 pi f tauhat_l)        (f: the map minus its centre frequency f0)
//
//   k_offres_pm     the phase maps P_l[n] = exp(-i 2 pi f[n] tauhat_l), one table entry per (segment, pixel): the only sincos of the map; the
//                   operator's own kernels (nufft_kernels.hip, OFFRES instantiations) read the table
//   k_offres_coef   per sample, in the plan's sorted order: the right-hand side r_l = sum_h p_h conj(G_hl) exp(-i 2 pi f_h tau_i) over the
//                   histogram bins in ascending order, the two substitutions with the host's Cholesky factor of G^H P G + eps I, the fit
//                   |exp(-i 2 pi f_h tau_i) - sum_l b_l G_hl| over the occupied bins, and b_l exp(-i 2 pi f0 tau_i) stored [l][sample].
//                   A workgroup owns OF_SB = 16 samples; thread (j, q) = (tid / 16, tid % 16) works on sample j, as segment q for the
//                   right-hand side and as bin lane q for the fit.  exp(-i 2 pi f_h tau_j) is staged in LDS OF_HC bins at a time.
//   k_offres_fit    the workgroups' partial maxima and sums -> one maximum and one sum, in a fixed order
//   k_offres_ncoef  the REAL coefficients of the field-aware normal operator (qmri_nufft_prepare_normal_fm), which segments the
//                   difference phase exp(i 2 pi g tau), g = f[n] - f[n'].  The ridge system (R + eps I) c = rho is the least-squares problem of the
//                   stacked table B = [sqrt(p~_j) cos; sqrt(p~_j) sin; sqrt(eps) I] and is solved through the host's thin QR of B (B = Q U), not
//                   through R, whose condition is the square of B's: y_l = sum_j sqrt(p~_j) (Q_jl^cos cos 2 pi g_j tau_i + Q_jl^sin sin 2 pi g_j
//                   tau_i) over the difference histogram in ascending order (= the forward substitution's result), the back substitution U c = y,
//                   the fit |exp(i 2 pi g_j tau_i) - sum_l c_l exp(i 2 pi g_j tauhat_l)| over the occupied bins, and c_l stored [l][sample].
//                   L <= 32: a workgroup owns ON_SB = 8 samples, thread (j, q) = (tid / 32, tid % 32).  Partials go through k_offres_fit.
// Every sum has a fixed order and nothing is atomic: the coefficients and the reported fit are the same bits on every call.
#include <cmath>

#include "qmri_internal.h"

namespace {
constexpr int NT = 256;
constexpr int OF_SB = 16;        // samples per workgroup
constexpr int OF_LMAX = 16;      // segments at most (= the lanes per sample)
constexpr int OF_HC = 64;        // histogram bins staged at a time

__device__ __forceinline__ double2 cis_m2pi(double a) {          // exp(-i 2 pi a)
    double s, c;
    sincospi(-2.0 * a, &s, &c);
    return make_double2(c, s);
}

__global__ __launch_bounds__(NT) void k_offres_pm(int L, size_t plane, const double* __restrict__ f, double f0, const double* __restrict__ tauhat,
                                                  double2* __restrict__ pm) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (size_t)L * plane) return;
    const int l = (int)(i / plane);
    const size_t r = i - (size_t)l * plane;
    pm[i] = cis_m2pi((f[r] - f0) * tauhat[l]);
}

// block-wide maximum and sum in a fixed order (a tree over the thread index)
__device__ __forceinline__ void block_max_sum(double* smx, double* ssm, double& mx, double& sm) {
    const int tid = threadIdx.x;
    smx[tid] = mx; ssm[tid] = sm;
    __syncthreads();
    for (int st = NT / 2; st > 0; st >>= 1) {
        if (tid < st) { smx[tid] = fmax(smx[tid], smx[tid + st]); ssm[tid] += ssm[tid + st]; }
        __syncthreads();
    }
    mx = smx[0]; sm = ssm[0];
}

__global__ __launch_bounds__(NT) void k_offres_coef(int L, int nbins, int m, int exact, const double2* __restrict__ hist, const double2* __restrict__ G,
                                                    const double2* __restrict__ chol, const double* __restrict__ ts,
                                                    const int32_t* __restrict__ perm, double f0, double2* __restrict__ bl, double* __restrict__ pmax,
                                                    double* __restrict__ psum) {
    __shared__ double2 E[OF_SB][OF_HC];
    __shared__ double2 bs[OF_SB][OF_LMAX];           // right-hand side, then the solution
    __shared__ double2 C[OF_LMAX * OF_LMAX];
    __shared__ double tau[OF_SB];
    __shared__ double smx[NT], ssm[NT];
    const int tid = threadIdx.x, j = tid >> 4, q = tid & 15;
    const int e0 = blockIdx.x * OF_SB, e = e0 + j;
    const bool valid = e < m;
    if (tid < OF_SB) tau[tid] = (e0 + tid < m) ? ts[perm[e0 + tid]] : 0.0;
    for (int i = tid; i < L * L; i += NT) C[i] = chol[i];
    __syncthreads();
    double mx = 0.0, sm = 0.0;
    if (exact) {
        bs[j][q] = make_double2(q == 0 ? 1.0 : 0.0, 0.0);
        __syncthreads();
    } else {
        // ---- right-hand sides
        double rr = 0.0, ri = 0.0;
        for (int h0 = 0; h0 < nbins; h0 += OF_HC) {
            __syncthreads();
            for (int i = tid; i < OF_SB * OF_HC; i += NT) {
                const int jj = i / OF_HC, hh = i - jj * OF_HC, h = h0 + hh;
                E[jj][hh] = (h < nbins && e0 + jj < m) ? cis_m2pi(hist[h].y * tau[jj]) : make_double2(0.0, 0.0);
            }
            __syncthreads();
            if (q < L) {
                const int hn = min(OF_HC, nbins - h0);
                for (int hh = 0; hh < hn; ++hh) {
                    const double p = hist[h0 + hh].x;
                    const double2 g = G[(size_t)(h0 + hh) * L + q], ev = E[j][hh];
                    rr = fma(p, ev.x * g.x + ev.y * g.y, rr);         // p E conj(G)
                    ri = fma(p, ev.y * g.x - ev.x * g.y, ri);
                }
            }
        }
        bs[j][q] = make_double2(rr, ri);
        __syncthreads();
        // ---- C C^H b = r: one lane per sample, forward then backward, in place (the diagonal of C is real)
        if (q == 0 && valid) {
            for (int r = 0; r < L; ++r) {
                double2 a = bs[j][r];
                for (int k = 0; k < r; ++k) {
                    const double2 c = C[r * L + k], z = bs[j][k];
                    a.x -= c.x * z.x - c.y * z.y; a.y -= c.x * z.y + c.y * z.x;
                }
                const double d = 1.0 / C[r * L + r].x;
                bs[j][r] = make_double2(a.x * d, a.y * d);
            }
            for (int r = L - 1; r >= 0; --r) {
                double2 a = bs[j][r];
                for (int k = r + 1; k < L; ++k) {
                    const double2 c = C[k * L + r], z = bs[j][k];                            // conj(C[k][r]) * b_k
                    a.x -= c.x * z.x + c.y * z.y; a.y -= c.x * z.y - c.y * z.x;
                }
                const double d = 1.0 / C[r * L + r].x;
                bs[j][r] = make_double2(a.x * d, a.y * d);
            }
        }
        __syncthreads();
        // ---- the fit over the occupied bins
        if (valid) {
            for (int h = q; h < nbins; h += 16) {
                const double p = hist[h].x;
                if (!(p > 0.0)) continue;
                const double2 ev = cis_m2pi(hist[h].y * tau[j]);
                double ar = 0.0, ai = 0.0;
                for (int l = 0; l < L; ++l) {
                    const double2 b = bs[j][l], g = G[(size_t)h * L + l];
                    ar += b.x * g.x - b.y * g.y; ai += b.x * g.y + b.y * g.x;
                }
                const double dr = ev.x - ar, di = ev.y - ai, d2 = dr * dr + di * di;
                mx = fmax(mx, d2);
                sm = fma(p, d2, sm);
            }
        }
    }
    block_max_sum(smx, ssm, mx, sm);
    if (tid == 0) { pmax[blockIdx.x] = mx; psum[blockIdx.x] = sm; }
    if (valid && q < L) {
        const double2 c = cis_m2pi(f0 * tau[j]), b = bs[j][q];
        bl[(size_t)q * m + e] = make_double2(b.x * c.x - b.y * c.y, b.x * c.y + b.y * c.x);
    }
}

constexpr int ON_SB = 8;         // samples per workgroup of k_offres_ncoef
constexpr int ON_LMAX = 32;      // segments at most (= the lanes per sample)
constexpr int ON_BMAX = 2047;    // difference bins at most (2 * 1024 - 1)

__global__ __launch_bounds__(NT) void k_offres_ncoef(int L, int nb, int m, const double2* __restrict__ dh, const double2* __restrict__ G,
                                                     const double2* __restrict__ Qw, const double* __restrict__ U, const double* __restrict__ ts,
                                                     const int32_t* __restrict__ perm, double* __restrict__ cl, double* __restrict__ pmax,
                                                     double* __restrict__ psum) {
    __shared__ double2 E[ON_SB][OF_HC];
    __shared__ double cs[ON_SB][ON_LMAX];            // right-hand side, then the solution
    __shared__ double C[ON_LMAX * ON_LMAX];          // U, upper, row-major
    __shared__ double tau[ON_SB];
    __shared__ double smx[NT], ssm[NT];
    const int tid = threadIdx.x, j = tid >> 5, q = tid & 31;
    const int e0 = blockIdx.x * ON_SB, e = e0 + j;
    const bool valid = e < m;
    if (tid < ON_SB) tau[tid] = (e0 + tid < m) ? ts[perm[e0 + tid]] : 0.0;
    for (int i = tid; i < L * L; i += NT) C[i] = U[i];
    // ---- y = Q^T (sqrt(p~) e)
    double rr = 0.0;
    for (int h0 = 0; h0 < nb; h0 += OF_HC) {
        __syncthreads();
        for (int i = tid; i < ON_SB * OF_HC; i += NT) {
            const int jj = i / OF_HC, hh = i - jj * OF_HC, h = h0 + hh;
            double2 v = make_double2(0.0, 0.0);
            if (h < nb && e0 + jj < m) { const double2 c = cis_m2pi(dh[h].y * tau[jj]); v = make_double2(c.x, -c.y); }       // exp(+i 2 pi g tau)
            E[jj][hh] = v;
        }
        __syncthreads();
        if (q < L) {
            const int hn = min(OF_HC, nb - h0);
            for (int hh = 0; hh < hn; ++hh) {
                const double2 g = Qw[(size_t)(h0 + hh) * L + q], ev = E[j][hh];       // (sqrt(p~_j) is folded into the table)
                rr = fma(ev.x, g.x, rr);
                rr = fma(ev.y, g.y, rr);
            }
        }
    }
    cs[j][q] = rr;
    __syncthreads();
    // ---- U c = y: one lane per sample, back substitution in place
    if (q == 0 && valid) {
        for (int r = L - 1; r >= 0; --r) {
            double a = cs[j][r];
            for (int k = r + 1; k < L; ++k) a -= C[r * L + k] * cs[j][k];
            cs[j][r] = a / C[r * L + r];
        }
    }
    __syncthreads();
    // ---- the fit over the occupied difference bins
    double mx = 0.0, sm = 0.0;
    if (valid) {
        for (int h = q; h < nb; h += 32) {
            const double p = dh[h].x;
            if (!(p > 0.0)) continue;
            const double2 c = cis_m2pi(dh[h].y * tau[j]);
            double ar = 0.0, ai = 0.0;
            for (int l = 0; l < L; ++l) {
                const double2 g = G[(size_t)h * L + l];
                ar = fma(cs[j][l], g.x, ar); ai = fma(cs[j][l], g.y, ai);
            }
            const double dr = c.x - ar, di = -c.y - ai, d2 = dr * dr + di * di;
            mx = fmax(mx, d2);
            sm = fma(p, d2, sm);
        }
    }
    block_max_sum(smx, ssm, mx, sm);
    if (tid == 0) { pmax[blockIdx.x] = mx; psum[blockIdx.x] = sm; }
    if (valid && q < L) cl[(size_t)q * m + e] = cs[j][q];
}

__global__ __launch_bounds__(NT) void k_offres_fit(int nblk, const double* __restrict__ pmax, const double* __restrict__ psum, double* __restrict__ out) {
    __shared__ double smx[NT], ssm[NT];
    double mx = 0.0, sm = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NT) { mx = fmax(mx, pmax[i]); sm += psum[i]; }
    block_max_sum(smx, ssm, mx, sm);
    if (threadIdx.x == 0) { out[0] = mx; out[1] = sm; }
}
}  // namespace

int offres_phase_maps_dev(qmri_ctx* ctx, int L, size_t plane, const double* d_f, double f0, const double* d_tauhat, double2* d_pm) {
    const size_t cnt = (size_t)L * plane;
    k_offres_pm<<<dim3((unsigned)((cnt + NT - 1) / NT)), dim3(NT), 0, ctx->stream>>>(L, plane, d_f, f0, d_tauhat, d_pm);
    QMRI_HIP(ctx, hipGetLastError());
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

int offres_coefficients_dev(qmri_ctx* ctx, int L, int nbins, bool exact, const double2* d_hist, const double2* d_G, const double2* d_chol,
                            const double* d_ts, double f0, double2* d_bl, OffresFit* fit) {
    const OpHost& o = ctx->op;
    if (o.kind != OP_NUFFT || L < 1 || L > OF_LMAX || nbins < 1) { qmri_set_error(ctx, "offres_coefficients_dev: bad plan (internal)"); return QMRI_ERR_STATE; }
    const int nblk = (o.m + OF_SB - 1) / OF_SB;
    DevBuf<double> d_part;
    QMRI_TRY(d_part.ensure(ctx, 2 * (size_t)nblk + 2));
    k_offres_coef<<<dim3(nblk), dim3(NT), 0, ctx->stream>>>(L, nbins, o.m, exact ? 1 : 0, d_hist, d_G, d_chol, d_ts, o.nu.d_perm, f0, d_bl, d_part, d_part + nblk);
    QMRI_HIP(ctx, hipGetLastError());
    k_offres_fit<<<dim3(1), dim3(NT), 0, ctx->stream>>>(nblk, d_part, d_part + nblk, d_part + 2 * (size_t)nblk);
    QMRI_HIP(ctx, hipGetLastError());
    double out[2] = {0.0, 0.0};
    QMRI_HIP(ctx, hipMemcpyAsync(out, d_part + 2 * (size_t)nblk, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fit->fit_max = std::sqrt(out[0]);
    fit->fit_rms = std::sqrt(out[1] / (double)o.m);
    return QMRI_OK;
}

int offres_ncoefficients_dev(qmri_ctx* ctx, int L, int nb, const double2* d_dh, const double2* d_G, const double2* d_Qw, const double* d_U,
                             const double* d_ts, double* d_c, OffresFit* fit) {
    const OpHost& o = ctx->op;
    if (o.kind != OP_NUFFT || L < 2 || L > ON_LMAX || nb < 1 || nb > ON_BMAX) { qmri_set_error(ctx, "offres_ncoefficients_dev: bad plan (internal)"); return QMRI_ERR_STATE; }
    const int nblk = (o.m + ON_SB - 1) / ON_SB;
    DevBuf<double> d_part;
    QMRI_TRY(d_part.ensure(ctx, 2 * (size_t)nblk + 2));
    k_offres_ncoef<<<dim3(nblk), dim3(NT), 0, ctx->stream>>>(L, nb, o.m, d_dh, d_G, d_Qw, d_U, d_ts, o.nu.d_perm, d_c, d_part, d_part + nblk);
    QMRI_HIP(ctx, hipGetLastError());
    k_offres_fit<<<dim3(1), dim3(NT), 0, ctx->stream>>>(nblk, d_part, d_part + nblk, d_part + 2 * (size_t)nblk);
    QMRI_HIP(ctx, hipGetLastError());
    double out[2] = {0.0, 0.0};
    QMRI_HIP(ctx, hipMemcpyAsync(out, d_part + 2 * (size_t)nblk, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fit->fit_max = std::sqrt(out[0]);
    fit->fit_rms = std::sqrt(out[1] / (double)o.m);
    return QMRI_OK;
}
