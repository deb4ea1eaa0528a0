// nufft_plan.h -- everything the host decides or computes for a trajectory (NUFFT) operator, in plain C++ (no HIP, no context): the kernel's
// constants, the exact spiral, the plan of qmri_set_operator_nufft (samples binned by tile, spreading lists cut into segments with partial-sum slots,
// deapodisation, half-bin ramps, sample phases) and the kernel sums of the density compensation.  DESIGN.md sections 14 and 21; kernels:
// nufft_kernels.hip, dcf_kernels.hip, toep_kernels.hip; tests/cpp/nufft_plan_test.cpp runs these functions under the host sanitizers.
// api_nufft.cpp and api_dcf.cpp validate, call these, and move the results to the device; nothing else decides.
#ifndef QMRI_NUFFT_PLAN_H          // (a guard, not #pragma once: the header is also compiled on its own)
#define QMRI_NUFFT_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "op_plan.h"               // spiral_points, SPIRAL_DELTA

// ---------------------------------------------------------------------------------------------------
// what the kernels share with the plan.  Samples are sorted by the 16 x 16 tile of the 2N x 2M oversampled grid that holds their position
// ("bins"); for the output-driven spreading every tile has the list of samples whose kernel windows reach it, cut into segments of <= seg samples.
// ---------------------------------------------------------------------------------------------------
constexpr int NU_TB = 16;        // tile side (oversampled grid points) of the spreading; 2N and 2M are multiples of it for every supported side
constexpr int NU_SEG = 512;      // samples per spreading segment by default (a heavier tile is split; its partial tiles are summed in segment order)
constexpr int NU_WMAX = 16;      // widest kernel
constexpr int NU_WDEF = 12;      // default width: measured relative error 2.7e-11 (10^(1-w) ~ 1e-11)
struct NuSeg { int32_t tile, b, e, slot; };      // tile index (t1 * ntile2 + t2), list range, partial slot (-1: the segment writes the grid itself)
struct NuRed { int32_t tile, slot0, nslot, pad; };

// beta of the "exponential of semicircle" kernel at 2x oversampling (Barnett, Magland, af Klinteberg 2019: beta = 2.30 w)
constexpr double nu_beta(int w) { return 2.30 * w; }
inline bool nufft_kernel_ok(int w) { return w >= 2 && w <= NU_WMAX; }

namespace nuplan {
constexpr double PI = 3.14159265358979323846;

// Gauss-Legendre nodes and weights on [-1, 1] (Newton on P_n from the Chebyshev guesses)
inline void gauss_legendre(int n, std::vector<double>& x, std::vector<double>& wt) {
    x.assign(n, 0.0); wt.assign(n, 0.0);
    for (int i = 0; i < (n + 1) / 2; ++i) {
        double z = std::cos(PI * (i + 0.75) / (n + 0.5)), dp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1.0, p1 = 0.0;
            for (int k = 1; k <= n; ++k) { const double p2 = p1; p1 = p0; p0 = ((2.0 * k - 1.0) * z * p1 - (k - 1.0) * p2) / k; }
            dp = n * (z * p0 - p1) / (z * z - 1.0);
            const double dz = p0 / dp;
            z -= dz;
            if (std::fabs(dz) < 1e-16) break;
        }
        x[i] = -z; x[n - 1 - i] = z;
        wt[i] = wt[n - 1 - i] = 2.0 / ((1.0 - z * z) * dp * dp);
    }
}

// 1 / Phi(n - L/2), n < L:  Phi(p) = int_{-w/2}^{w/2} phi(u) cos(2 pi u p / (2L)) du, the kernel's transform at the image index
inline void deapodisation(int L, int w, double beta, double* out) {
    std::vector<double> gx, gw;
    gauss_legendre(200, gx, gw);
    const double hw = 0.5 * w;
    for (int n = 0; n < L; ++n) {
        const double p = n - L / 2;
        double acc = 0.0;
        for (size_t q = 0; q < gx.size(); ++q) {
            const double u = gx[q] * hw, t = 1.0 - gx[q] * gx[q];
            acc += gw[q] * hw * std::exp(beta * (std::sqrt(std::max(t, 0.0)) - 1.0)) * std::cos(2.0 * PI * u * p / (2.0 * L));
        }
        out[n] = 1.0 / acc;
    }
}

inline int wrap(int k, int G) { k %= G; return k < 0 ? k + G : k; }

// the host twin of nu_phi (nufft_device.h)
inline double phi_host(double d, double hw, double beta) {
    const double z = d / hw, t = 1.0 - z * z;
    return t >= 0.0 ? std::exp(beta * (std::sqrt(t) - 1.0)) : 0.0;
}
// I = sum_k psi(k) over the window [k0, k0 + w) of a sample at u = 0, k0 = ceil(-w / 2) as nu_k0 gives it
inline double kernel_sum(int w, double beta) {
    const double hw = 0.5 * w;
    const int k0 = (int)std::ceil(0.0 - hw);
    double a = 0.0;
    for (int i = 0; i < w; ++i) a += phi_host(0.0 - (double)(k0 + i), hw, beta);
    return a;
}
// the scale of the density-compensation weights.  One factor per axis: the kernel is the same along both, the grid sides are
// not (they enter through T / 4 cells per image cell alone)
inline double dcf_kappa(int T, int w, double beta) {
    const double I1 = kernel_sum(w, beta), I2 = kernel_sum(w, beta);
    return 0.25 * (double)T * (I1 * I1) * (I2 * I2);
}

// The exact spiral of qmri_build_spiral_traj: spiral_points rotated by SPIRAL_DELTA per frame, omega = pi r (cos, sin).  Fills frame_ptr[0..T] and
// the first `cap` pairs of omega, and returns the number of samples m = S T; m > cap: the caller's array was too small (as the mask builders).
inline long spiral_traj_build(int S, int T, int32_t* frame_ptr, double* omega, int cap) {
    std::vector<double> theta, rad;
    spiral_points(S, theta, rad);
    const long m = (long)S * T;
    for (int f = 0; f < T; ++f) {
        frame_ptr[f] = (int32_t)((long)f * S);
        const double rot = (double)f * SPIRAL_DELTA;
        for (int j = 0; j < S; ++j) {
            const long i = (long)f * S + j;
            if (i >= cap) continue;
            omega[2 * i] = PI * (rad[j] * std::cos(theta[j] + rot));
            omega[2 * i + 1] = PI * (rad[j] * std::sin(theta[j] + rot));
        }
    }
    frame_ptr[T] = (int32_t)m;
    return m;
}

// ---------------------------------------------------------------------------------------------------
// the plan: every array qmri_set_operator_nufft uploads for the trajectory.  Complex tables are interleaved (re, im) doubles.
// ---------------------------------------------------------------------------------------------------
struct NufftPlan {
    std::vector<double> u, ph;           // [m][2] sorted: oversampled grid coordinates (omega1 N / pi, omega2 M / pi); exp(-i (omega1 N/2 + omega2 M/2))
    std::vector<int32_t> t, perm;        // [m] sorted: frame; sorted position -> ABI index
    std::vector<int32_t> list;           // spreading lists of the tiles, tile after tile (sorted positions)
    std::vector<NuSeg> segs;             // the lists' segments, heaviest first
    std::vector<NuRed> reds;             // one per split tile: the partial slots the reduce kernel sums, in list order
    int nslot = 0;                       // partial slots in all
    std::vector<double> dp;              // [N] then [M]: deapodisation 1 / Phi at n - N/2
    std::vector<double> ramp;            // [N][2] then [M][2]: exp(-i pi (n - N/2) / N), the half-bin ramps
};

// frame_ptr [T + 1] and omega [m][2] as qmri_set_operator_nufft has checked them (finite, |omega| <= pi, m = frame_ptr[T] > 0); w a supported
// width; seg >= 1 samples per segment
inline NufftPlan nu_plan(int N, int M, int T, const int32_t* frame_ptr, const double* omega, int w, int seg) {
    NufftPlan pl;
    const int m = frame_ptr[T];
    const double hw = 0.5 * w, beta = nu_beta(w);
    // ---- samples sorted by the tile of the oversampled grid that holds floor(u) (stable: ABI order inside a tile)
    const int G1 = 2 * N, G2 = 2 * M, nt1 = G1 / NU_TB, nt2 = G2 / NU_TB;
    std::vector<double> u(2 * (size_t)m), ph(2 * (size_t)m);
    std::vector<int32_t> frame_of(m), bin(m);
    for (int t = 0; t < T; ++t)
        for (int i = frame_ptr[t]; i < frame_ptr[t + 1]; ++i) frame_of[i] = t;
    for (int i = 0; i < m; ++i) {
        const double w1 = omega[2 * i], w2 = omega[2 * i + 1];
        u[2 * i] = w1 * N / PI;
        u[2 * i + 1] = w2 * M / PI;
        const double a = -(w1 * (N / 2) + w2 * (M / 2));
        ph[2 * i] = std::cos(a); ph[2 * i + 1] = std::sin(a);
        const int k1 = wrap((int)std::floor(u[2 * i]), G1), k2 = wrap((int)std::floor(u[2 * i + 1]), G2);
        bin[i] = (k1 / NU_TB) * nt2 + k2 / NU_TB;
    }
    std::vector<int32_t> order(m);
    for (int i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bin[a] < bin[b]; });
    std::vector<double>& su = pl.u; std::vector<double>& sph = pl.ph;
    std::vector<int32_t>& st = pl.t; std::vector<int32_t>& sperm = pl.perm;
    su.resize(2 * (size_t)m); sph.resize(2 * (size_t)m); st.resize(m); sperm.resize(m);
    for (int e = 0; e < m; ++e) {
        const int i = order[e];
        su[2 * e] = u[2 * i]; su[2 * e + 1] = u[2 * i + 1];
        sph[2 * e] = ph[2 * i]; sph[2 * e + 1] = ph[2 * i + 1];
        st[e] = frame_of[i]; sperm[e] = i;
    }
    // ---- spreading lists: every tile the kernel window [k0, k0 + w) of a sample reaches (k0 = ceil(u - w/2), as the kernels compute it)
    std::vector<std::vector<int32_t>> tl((size_t)nt1 * nt2);
    for (int e = 0; e < m; ++e) {
        int ta[4], tb[4], na = 0, nb = 0;           // (w <= 16 = NU_TB: at most 2 tiles per axis)
        const int k01 = (int)std::ceil(su[2 * e] - hw), k02 = (int)std::ceil(su[2 * e + 1] - hw);
        for (int i = 0; i < w; ++i) {
            const int t1 = wrap(k01 + i, G1) / NU_TB, t2 = wrap(k02 + i, G2) / NU_TB;
            if (std::find(ta, ta + na, t1) == ta + na) ta[na++] = t1;
            if (std::find(tb, tb + nb, t2) == tb + nb) tb[nb++] = t2;
        }
        for (int a = 0; a < na; ++a)
            for (int b = 0; b < nb; ++b) tl[(size_t)ta[a] * nt2 + tb[b]].push_back(e);
    }
    std::vector<int32_t>& list = pl.list;
    std::vector<NuSeg>& segs = pl.segs;
    std::vector<NuRed>& reds = pl.reds;
    int nslot = 0;
    const int SEG = seg;
    for (int tile = 0; tile < nt1 * nt2; ++tile) {
        const std::vector<int32_t>& L = tl[tile];
        const int b0 = (int)list.size(), len = (int)L.size();
        list.insert(list.end(), L.begin(), L.end());
        const int ns = std::max(1, (len + SEG - 1) / SEG);
        if (ns == 1) { segs.push_back(NuSeg{tile, b0, b0 + len, -1}); continue; }
        reds.push_back(NuRed{tile, nslot, ns, 0});
        for (int q = 0; q < ns; ++q) segs.push_back(NuSeg{tile, b0 + q * SEG, b0 + std::min(len, (q + 1) * SEG), nslot++});
    }
    // heaviest segments first: the full ones of the split tiles are issued before the rest
    std::stable_sort(segs.begin(), segs.end(), [](const NuSeg& a, const NuSeg& b) { return (a.e - a.b) > (b.e - b.b); });
    pl.nslot = nslot;
    // ---- deapodisation and half-bin ramps, at the centred index n - N/2
    pl.dp.resize((size_t)N + M);
    deapodisation(N, w, beta, pl.dp.data());
    deapodisation(M, w, beta, pl.dp.data() + N);
    std::vector<double>& ramp = pl.ramp;
    ramp.resize(2 * ((size_t)N + M));
    for (int n = 0; n < N; ++n) { const double a = -PI * (n - N / 2) / N; ramp[2 * (size_t)n] = std::cos(a); ramp[2 * (size_t)n + 1] = std::sin(a); }
    for (int n = 0; n < M; ++n) { const double a = -PI * (n - M / 2) / M; ramp[2 * ((size_t)N + n)] = std::cos(a); ramp[2 * ((size_t)N + n) + 1] = std::sin(a); }
    return pl;
}

}  // namespace nuplan

#endif
