// offres_plan.h -- what the host computes for the off-resonance correction of a trajectory operator, in plain C++ (no HIP, no context): the histogram
// of the field map, the segment times, the L x L coefficient system of qmri_set_field_map with its Cholesky factor, the difference histogram and the
// twice-orthogonalised QR tables of qmri_nufft_prepare_normal_fm.  DESIGN.md sections 22 and 23; kernels: offres_kernels.hip;
// tests/cpp/offres_plan_test.cpp runs these functions under the host sanitizers.  api_offres.cpp validates, searches L (the fit comes back from the
// device), calls these once per tried L and uploads the results.  Complex tables are std::complex<double> or interleaved (x, y) doubles: both are
// the device's double2 byte for byte.
#ifndef QMRI_OFFRES_PLAN_H         // (a guard, not #pragma once: the header is also compiled on its own)
#define QMRI_OFFRES_PLAN_H

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <vector>

namespace offres {
constexpr double PI = 3.14159265358979323846;
constexpr int OFFRES_LMAX = 16, OFFRES_NBINS_DEF = 256, OFFRES_NBINS_MIN = 16, OFFRES_NBINS_MAX = 1024;
constexpr int OFFRES_NLMAX = 32;          // segments of the field-aware normal operator at most
constexpr double OFFRES_TOL_DEF = 1e-4;
typedef std::complex<double> cplx;

// lower Cholesky factor (row-major, in place) of the Hermitian positive definite A [L][L]; false on a pivot that is not positive
inline bool cholesky(std::vector<cplx>& A, int L) {
    for (int r = 0; r < L; ++r) {
        for (int k = 0; k <= r; ++k) {
            cplx a = A[(size_t)r * L + k];
            for (int q = 0; q < k; ++q) a -= A[(size_t)r * L + q] * std::conj(A[(size_t)k * L + q]);
            if (k == r) {
                if (!(a.real() > 0.0) || !std::isfinite(a.real())) return false;
                A[(size_t)r * L + r] = cplx(std::sqrt(a.real()), 0.0);
            } else {
                A[(size_t)r * L + k] = a / A[(size_t)k * L + k].real();
            }
        }
        for (int k = r + 1; k < L; ++k) A[(size_t)r * L + k] = cplx(0.0, 0.0);
    }
    return true;
}

// thin QR B = Q U of the real B [rows][L], stored by columns, by modified Gram-Schmidt with every column orthogonalised twice (Q is then orthonormal
// to rounding whatever B's condition): Q overwrites B, U [L][L] upper, row-major; false on a column that vanishes
inline bool qr_mgs2(std::vector<double>& B, size_t rows, int L, std::vector<double>& U) {
    U.assign((size_t)L * L, 0.0);
    for (int k = 0; k < L; ++k) {
        double* bk = &B[(size_t)k * rows];
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < k; ++i) {
                const double* bi = &B[(size_t)i * rows];
                double r = 0.0;
                for (size_t t = 0; t < rows; ++t) r += bi[t] * bk[t];
                for (size_t t = 0; t < rows; ++t) bk[t] -= r * bi[t];
                U[(size_t)i * L + k] += r;
            }
        double nn = 0.0;
        for (size_t t = 0; t < rows; ++t) nn += bk[t] * bk[t];
        nn = std::sqrt(nn);
        if (!(nn > 0.0) || !std::isfinite(nn)) return false;
        for (size_t t = 0; t < rows; ++t) bk[t] /= nn;
        U[(size_t)k * L + k] = nn;
    }
    return true;
}

// the histogram (p_h, f_h) of f - f0, f0 = (f_min + f_max) / 2: nbins equal bins on [f_min - f0, f_max - f0], f_h the centres, p_h the fraction of
// pixels.  A constant map (f_max == f_min) has one bin at 0.
struct MapHist {
    bool constant = false;
    int nbins = 0;
    double f0 = 0.0;
    std::vector<size_t> cnt;              // [nbins] pixels per bin
    std::vector<double> pf;               // [nbins][2] (p_h, f_h)
    double p(int b) const { return pf[2 * (size_t)b]; }
    double f(int b) const { return pf[2 * (size_t)b + 1]; }
};
inline MapHist map_histogram(const double* f_hz, size_t plane, double f_min, double f_max, int nbins) {
    MapHist h;
    const bool constant = f_max == f_min;
    const double f0 = 0.5 * (f_min + f_max), lo = f_min - f0, width = (f_max - f_min) / nbins;
    if (constant) nbins = 1;
    h.constant = constant; h.nbins = nbins; h.f0 = f0;
    std::vector<size_t>& cnt = h.cnt;
    cnt.assign((size_t)nbins, 0);
    for (size_t i = 0; i < plane; ++i) {
        int b = constant ? 0 : (int)std::floor(((f_hz[i] - f0) - lo) / width);
        cnt[(size_t)std::min(std::max(b, 0), nbins - 1)] += 1;
    }
    h.pf.resize(2 * (size_t)nbins);
    for (int b = 0; b < nbins; ++b) { h.pf[2 * (size_t)b] = (double)cnt[b] / (double)plane; h.pf[2 * (size_t)b + 1] = constant ? 0.0 : lo + (b + 0.5) * width; }
    return h;
}

// the L segment times, equally spaced on [t_min, t_max]; L = 1: t_min.  The last one is t_max itself: (L - 1) r / (L - 1) can round an ulp off r
inline std::vector<double> segment_times(double t_min, double t_max, int L) {
    std::vector<double> tauhat((size_t)L, t_min);
    if (L > 1) {
        for (int l = 0; l < L; ++l) tauhat[l] = t_min + l * (t_max - t_min) / (L - 1);
        tauhat[L - 1] = t_max;
    }
    return tauhat;
}

// the coefficient system of qmri_set_field_map at L segments: G [nbins][L] = exp(-i 2 pi f_h tauhat_l) and the lower Cholesky factor C [L][L]
// (row-major) of G^H P G + eps I, eps = 1e-12 tr(G^H P G) / L.  ok = false: the system is not positive definite.
struct FitSystem {
    bool ok = false;
    std::vector<double> tauhat;           // [L]
    std::vector<cplx> G, C;
};
inline FitSystem fit_system(const MapHist& hist, double t_min, double t_max, int L) {
    FitSystem s;
    const int nbins = hist.nbins;
    std::vector<double>& tauhat = s.tauhat;
    tauhat = segment_times(t_min, t_max, L);
    std::vector<cplx>& G = s.G; std::vector<cplx>& A = s.C;
    G.resize((size_t)nbins * L); A.assign((size_t)L * L, cplx(0.0, 0.0));
    for (int b = 0; b < nbins; ++b)
        for (int l = 0; l < L; ++l) { const double a = -2.0 * PI * hist.f(b) * tauhat[l]; G[(size_t)b * L + l] = cplx(std::cos(a), std::sin(a)); }
    for (int b = 0; b < nbins; ++b)
        for (int r = 0; r < L; ++r)
            for (int k = 0; k < L; ++k) A[(size_t)r * L + k] += hist.p(b) * std::conj(G[(size_t)b * L + r]) * G[(size_t)b * L + k];
    double tr = 0.0;
    for (int r = 0; r < L; ++r) tr += A[(size_t)r * L + r].real();
    for (int r = 0; r < L; ++r) A[(size_t)r * L + r] += 1e-12 * tr / L;
    s.ok = cholesky(A, L);
    return s;
}

// the difference histogram: the autocorrelation of the map's p [nbins], 2 nbins - 1 bins at g_j = j width, j = -(nbins - 1) .. nbins - 1.
// -> [2 nbins - 1][2] (p~_j, g_j)
inline std::vector<double> diff_histogram(const std::vector<double>& p, double width) {
    const int nbins = (int)p.size(), nb = 2 * nbins - 1;
    std::vector<double> dh(2 * (size_t)nb);
    for (int j = -(nbins - 1); j <= nbins - 1; ++j) {
        double a = 0.0;
        for (int b = std::max(0, j); b < std::min(nbins, nbins + j); ++b) a += p[b] * p[b - j];
        dh[2 * (size_t)(j + nbins - 1)] = a; dh[2 * (size_t)(j + nbins - 1) + 1] = j * width;
    }
    return dh;
}

// the tables of qmri_nufft_prepare_normal_fm at L segments from the difference histogram dh [nb][2]: G [nb][L][2] = exp(i 2 pi g_j tauhat_l), and
// the thin QR B = Q U of the stacked table below as Qw [nb][L][2] (sqrt(p~_j) times Q's cos / sin row of bin j) and U [L][L] (upper, row-major).
// ok = false: a column of B vanished.
struct NormalTables {
    bool ok = false;
    std::vector<double> tauhat;           // [L]
    std::vector<double> G, Qw, U;
};
inline NormalTables normal_tables(const std::vector<double>& dh, double t_min, double t_max, int L) {
    NormalTables s;
    const int nb = (int)(dh.size() / 2);
    std::vector<double>& tauhat = s.tauhat;
    tauhat = segment_times(t_min, t_max, L);
    std::vector<double>& G = s.G;
    G.resize(2 * (size_t)nb * L);
    for (int j = 0; j < nb; ++j)
        for (int l = 0; l < L; ++l) { const double a = 2.0 * PI * dh[2 * (size_t)j + 1] * tauhat[l]; G[2 * ((size_t)j * L + l)] = std::cos(a); G[2 * ((size_t)j * L + l) + 1] = std::sin(a); }
    // (R + eps I) c = rho, R = sum_j p~_j (cos cos + sin sin), eps = 1e-12 tr(R) / L = 1e-12 sum_j p~_j, is the least-squares problem of the stacked
    // table B = [sqrt(p~_j) cos; sqrt(p~_j) sin; sqrt(eps) I] with the right-hand side [sqrt(p~) cos 2 pi g tau; sqrt(p~) sin 2 pi g tau; 0].  It is
    // solved through B = Q U: c = U^-1 Q^T b.  U is R + eps I's Cholesky factor transposed and Q^T b the forward substitution's result, but
    // formed at B's condition, not at its square: through R itself fit_max at L' = 8 (condition 3e9) came out 1e-6 relative from the solution
    const size_t rows = 2 * (size_t)nb + L;
    double psum = 0.0;
    for (int j = 0; j < nb; ++j) psum += dh[2 * (size_t)j];
    std::vector<double> B(rows * L, 0.0);
    std::vector<double> w((size_t)nb);
    for (int j = 0; j < nb; ++j) w[j] = std::sqrt(dh[2 * (size_t)j]);
    for (int l = 0; l < L; ++l) {
        for (int j = 0; j < nb; ++j) {
            B[(size_t)l * rows + 2 * j] = w[j] * G[2 * ((size_t)j * L + l)];
            B[(size_t)l * rows + 2 * j + 1] = w[j] * G[2 * ((size_t)j * L + l) + 1];
        }
        B[(size_t)l * rows + 2 * nb + l] = std::sqrt(1e-12 * psum);
    }
    if (!qr_mgs2(B, rows, L, s.U)) return s;          // (the ridge rows keep every column's norm >= sqrt(eps) > 0: not reachable with a finite map)
    std::vector<double>& Qw = s.Qw;
    Qw.resize(2 * (size_t)nb * L);
    for (int j = 0; j < nb; ++j)
        for (int l = 0; l < L; ++l) { Qw[2 * ((size_t)j * L + l)] = w[j] * B[(size_t)l * rows + 2 * j]; Qw[2 * ((size_t)j * L + l) + 1] = w[j] * B[(size_t)l * rows + 2 * j + 1]; }
    s.ok = true;
    return s;
}

}  // namespace offres

#endif
