// api_nufft.cpp -- trajectory operators: the exact spiral builder, the host plan of the NUFFT (bins, spreading
// segments, deapodisation) and the refusals of the calls a trajectory cannot serve.  The kernels are in nufft_kernels.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "qmri_internal.h"
#include "fft_codelets.h"

namespace {
constexpr double PI = 3.14159265358979323846;
constexpr int NU_WDEF = 12;      // default width: measured relative error 2.7e-11 (10^(1-w) ~ 1e-11)

// beta of the "exponential of semicircle" kernel at 2x oversampling (Barnett, Magland, af Klinteberg 2019: beta = 2.30 w)
double nu_beta(int w) { return 2.30 * w; }

// Gauss-Legendre nodes and weights on [-1, 1] (Newton on P_n from the Chebyshev guesses)
void gauss_legendre(int n, std::vector<double>& x, std::vector<double>& wt) {
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
void deapodisation(int L, int w, double beta, double* out) {
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
}  // namespace

int nufft_check_gridded(qmri_ctx* ctx, const char* what, const char* instead) {
    if (ctx->op.kind != OP_NUFFT) return QMRI_OK;
    qmri_set_error(ctx, "%s is not available on a trajectory operator (qmri_set_operator_nufft): %s", what, instead);
    return QMRI_ERR_UNSUPPORTED;
}

extern "C" int qmri_build_spiral_traj(qmri_ctx* ctx, int N, int S, int T, int32_t* frame_ptr, double* omega, int cap, int* m_out) {
    QMRI_CHECK_ARG(ctx, N > 0 && S > 1 && T > 0 && frame_ptr && (omega || cap == 0) && m_out && cap >= 0, "qmri_build_spiral_traj arguments");
    std::vector<double> theta, rad;
    spiral_points(S, theta, rad);
    const long m = (long)S * T;
    if (m > 0x7fffffffL) { qmri_set_error(ctx, "S * T = %ld samples exceed the int32 index range", m); return QMRI_ERR_INVALID_ARG; }
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
    *m_out = (int)m;
    if (m > cap) { qmri_set_error(ctx, "omega capacity %d too small, need %ld", cap, m); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

extern "C" int qmri_set_operator_nufft(qmri_ctx* ctx, int N, int M, int s, int T, const double* V, const int32_t* frame_ptr, const double* omega,
                                       int max_batch, const qmri_nufft_params* p) {
    // the argument checks come first and need no context or device (ctx == NULL: their message is qmri_last_error(NULL))
    QMRI_CHECK_ARG(ctx, V && frame_ptr && omega, "V / frame_ptr / omega must not be NULL");
    QMRI_CHECK_ARG(ctx, N > 0 && M > 0 && s > 0 && T > 0 && max_batch > 0, "N, M, s, T, max_batch must be positive");
    if (!dc_size_supported(N) || !dc_size_supported(M)) {
        qmri_set_error(ctx, "grid %d x %d unsupported: the FFT kernels implement N, M in {" QFFT_SIDES_TEXT "}, chosen independently", N, M);
        return QMRI_ERR_UNSUPPORTED;
    }
    if (s > 10 || T > 65535) { qmri_set_error(ctx, "s <= 10 and T <= 65535 required (got s=%d T=%d)", s, T); return QMRI_ERR_UNSUPPORTED; }
    const int w = (p && p->width) ? p->width : NU_WDEF;
    if (p) for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "qmri_nufft_params.reserved must be zero");
    if (!nufft_kernel_ok(w)) { qmri_set_error(ctx, "NUFFT kernel width %d unsupported: 2 <= width <= %d (0 = default %d)", w, NU_WMAX, NU_WDEF); return QMRI_ERR_UNSUPPORTED; }
    QMRI_CHECK_ARG(ctx, frame_ptr[0] == 0, "frame_ptr[0] must be 0");
    for (int t = 0; t < T; ++t) QMRI_CHECK_ARG(ctx, frame_ptr[t + 1] >= frame_ptr[t], "frame_ptr must be non-decreasing");
    const int m = frame_ptr[T];
    QMRI_CHECK_ARG(ctx, m > 0, "empty measurement set");
    for (long i = 0; i < 2L * m; ++i)
        if (!(std::isfinite(omega[i]) && std::fabs(omega[i]) <= PI)) {
            qmri_set_error(ctx, "invalid argument: omega[%ld] (sample %ld) = %g is not a finite value in [-pi, pi]", i % 2, i / 2, omega[i]);
            return QMRI_ERR_INVALID_ARG;
        }

    QMRI_CHECK_ARG(ctx, ctx, "ctx must not be NULL");
    // (every check above is host arithmetic on the arguments; the device is touched from here on)
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    qmri_free_operator(ctx);
    OpHost& o = ctx->op;
    NufftHost& h = o.nu;
    o.kind = OP_NUFFT;
    o.N = N; o.M = M; o.s = s; o.T = T; o.m = m; o.maxB = max_batch;
    o.V.assign(V, V + (size_t)T * s);
    o.frame_ptr.assign(frame_ptr, frame_ptr + T + 1);
    h.w = w; h.beta = nu_beta(w);
    const double hw = 0.5 * w;

    // ---- plan: samples sorted by the tile of the oversampled grid that holds floor(u) (stable: ABI order inside a tile)
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
    std::vector<double> su(2 * (size_t)m), sph(2 * (size_t)m);
    std::vector<int32_t> st(m), sperm(m);
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
    std::vector<int32_t> list;
    std::vector<NuSeg> segs;
    std::vector<NuRed> reds;
    int nslot = 0;
    const int SEG = std::max(32, qmri_knob(K_NUFFT_SEG));
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
    h.nseg = (int)segs.size(); h.nred = (int)reds.size(); h.nslot = nslot;
    // ---- deapodisation and half-bin ramps, at the centred index n - N/2
    std::vector<double> dp((size_t)N + M);
    deapodisation(N, w, h.beta, dp.data());
    deapodisation(M, w, h.beta, dp.data() + N);
    std::vector<double2> ramp((size_t)N + M);
    for (int n = 0; n < N; ++n) { const double a = -PI * (n - N / 2) / N; ramp[n] = make_double2(std::cos(a), std::sin(a)); }
    for (int n = 0; n < M; ++n) { const double a = -PI * (n - M / 2) / M; ramp[(size_t)N + n] = make_double2(std::cos(a), std::sin(a)); }
    std::vector<double> Vt((size_t)T * s);
    for (int t = 0; t < T; ++t)
        for (int c = 0; c < s; ++c) Vt[(size_t)t * s + c] = V[t + (size_t)T * c];
    std::vector<double2> tw((size_t)N + M);
    for (int j = 0; j < N; ++j) { const double a = 2.0 * PI * j / N; tw[j] = make_double2(std::cos(a), -std::sin(a)); }
    for (int j = 0; j < M; ++j) { const double a = 2.0 * PI * j / M; tw[(size_t)N + j] = make_double2(std::cos(a), -std::sin(a)); }

    const size_t n = (size_t)N * M * s, B = (size_t)max_batch;
    QMRI_TRY(o.pool.upload(ctx, &o.d_Vt, Vt.data(), Vt.size()));
    QMRI_TRY(o.pool.upload(ctx, &o.d_tw, tw.data(), tw.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_u, su.data(), su.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_ph, sph.data(), sph.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_t, st.data(), st.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_perm, sperm.data(), sperm.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_list, list.data(), list.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_seg, segs.data(), segs.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_red, reds.data(), reds.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_dp, dp.data(), dp.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_r, ramp.data(), ramp.size()));
    const std::vector<double2> ones((size_t)N * M, make_double2(1.0, 0.0));
    QMRI_TRY(o.pool.upload(ctx, &h.d_ones, ones.data(), ones.size()));
    QMRI_TRY(o.pool.alloc(ctx, &h.d_g, 4 * B * n));
    QMRI_TRY(o.pool.alloc(ctx, &h.d_grid, 4 * B * n));
    QMRI_TRY(o.pool.alloc(ctx, &h.d_part, B * std::max(nslot, 1) * (size_t)s * 256));
    // what the host-array entry points and the image-domain LSQR / ADMM loop use (as qmri_set_operator allocates them)
    LsqrDev& ls = o.ls;
    ls.nblk_z = 256;
    QMRI_TRY(o.pool.alloc(ctx, &o.d_xa, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_xb, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_ya, B * (size_t)m));
    QMRI_TRY(o.pool.alloc(ctx, &ls.pz, B * (size_t)ls.nblk_z));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_x, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_u, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_vv, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_z, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_mm, B * (size_t)ls.nblk_z * 2));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_norm, B * 2));
    QMRI_HIP(ctx, hipDeviceSynchronize());          // (as qmri_set_operator: the blocking copies must have landed before the context's stream reads them)
    o.ready = true;
    return QMRI_OK;
}
