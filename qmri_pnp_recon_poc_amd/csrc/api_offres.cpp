// api_offres.cpp -- off-resonance correction of a trajectory operator by time segmentation: qmri_set_field_map checks its
// arguments, builds the histogram of the map, the segment times and the Cholesky factor of the L x L coefficient system on the host, and has the
// device compute the per-sample coefficients, their fit and the phase maps (offres_kernels.hip).  The segment loop itself is in nufft_launch_fwd /
// launch_adj (nufft_kernels.hip).  Every refusal is decided on the host before the device is selected.
// qmri_nufft_prepare_normal_fm builds the field-aware Toeplitz normal operator of the attached map: the difference histogram,
// the QR factors of the real coefficient table, and per segment the K^ of toep_kernels.hip with the samples weighted by the segment's coefficients.
#include <cmath>
#include <complex>
#include <vector>

#include "qmri_internal.h"

namespace {
constexpr double PI = 3.14159265358979323846;
constexpr int OFFRES_LMAX = 16, OFFRES_NBINS_DEF = 256, OFFRES_NBINS_MIN = 16, OFFRES_NBINS_MAX = 1024;
constexpr int OFFRES_NLMAX = 32;          // segments of the field-aware normal operator at most
constexpr double OFFRES_TOL_DEF = 1e-4;
typedef std::complex<double> cplx;

// lower Cholesky factor (row-major, in place) of the Hermitian positive definite A [L][L]; false on a pivot that is not positive
bool cholesky(std::vector<cplx>& A, int L) {
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
bool qr_mgs2(std::vector<double>& B, size_t rows, int L, std::vector<double>& U) {
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

}  // namespace

int offres_refuse_toeplitz(qmri_ctx* ctx, const char* what) {
    if (!ctx || !ctx->op.ready || ctx->op.kind != OP_NUFFT || !ctx->op.nu.fm_set) return QMRI_OK;
    if (ctx->op.nu.fmn_ready) return QMRI_OK;           // (qmri_nufft_prepare_normal_fm has built the transform of THIS map)
    qmri_set_error(ctx, "%s is not available while a field map is attached (qmri_set_field_map) and its normal operator is not prepared: build it with "
                        "qmri_nufft_prepare_normal_fm, or use QMRI_SOLVER_LSQR (the image-domain LSQR runs the corrected operator), or clear the map with "
                        "qmri_set_field_map(ctx, NULL, ...)", what);
    return QMRI_ERR_UNSUPPORTED;
}

void offres_drop_normal(NufftHost& h) {
    h.fmn_ready = false; h.fmn_plain = false; h.fmn_L = 0;
    h.d_khat_fm.reset(); h.d_pm_n.reset(); h.d_xs.reset();
}

extern "C" int qmri_set_field_map(qmri_ctx* ctx, const double* f_hz, const double* t_s, const qmri_offres_params* p, qmri_offres_info* info) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    int nseg = 0, nbins = OFFRES_NBINS_DEF;
    double tol = OFFRES_TOL_DEF;
    if (f_hz && p) {
        QMRI_CHECK_ARG(ctx, p->nseg >= 0 && p->nseg <= OFFRES_LMAX, "qmri_offres_params.nseg must be in 1..16 (0 = auto)");
        QMRI_CHECK_ARG(ctx, p->nbins == 0 || (p->nbins >= OFFRES_NBINS_MIN && p->nbins <= OFFRES_NBINS_MAX), "qmri_offres_params.nbins must be in 16..1024 (0 = default 256)");
        QMRI_CHECK_ARG(ctx, std::isfinite(p->tol) && p->tol >= 0.0, "qmri_offres_params.tol must be finite and >= 0 (0 = default 1e-4)");
        for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "qmri_offres_params.reserved must be zero");
        nseg = p->nseg;
        if (p->nbins) nbins = p->nbins;
        if (p->tol > 0.0) tol = p->tol;
    }
    if (!ctx->op.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator_nufft first"); return QMRI_ERR_STATE; }
    if (ctx->op.kind != OP_NUFFT) {
        qmri_set_error(ctx, "qmri_set_field_map needs a trajectory operator (qmri_set_operator_nufft): a gridded mask has no readout times, every sample of a "
                            "frame is taken to be measured at once");
        return QMRI_ERR_UNSUPPORTED;
    }
    OpHost& o = ctx->op;
    NufftHost& h = o.nu;
    const size_t plane = (size_t)o.N * o.M;
    double f_min = 0.0, f_max = 0.0, t_min = 0.0, t_max = 0.0;
    if (f_hz) {
        QMRI_CHECK_ARG(ctx, t_s, "t_s must not be NULL when a field map is given");
        f_min = f_max = f_hz[0];
        for (size_t i = 0; i < plane; ++i) {
            if (!std::isfinite(f_hz[i])) { qmri_set_error(ctx, "invalid argument: f_hz[%zu] = %g is not finite", i, f_hz[i]); return QMRI_ERR_INVALID_ARG; }
            f_min = std::min(f_min, f_hz[i]); f_max = std::max(f_max, f_hz[i]);
        }
        t_min = t_max = t_s[0];
        for (int i = 0; i < o.m; ++i) {
            if (!std::isfinite(t_s[i])) { qmri_set_error(ctx, "invalid argument: t_s[%d] = %g is not finite", i, t_s[i]); return QMRI_ERR_INVALID_ARG; }
            t_min = std::min(t_min, t_s[i]); t_max = std::max(t_max, t_s[i]);
        }
        QMRI_CHECK_ARG(ctx, !(nseg == 1 && f_max != f_min), "nseg = 1 needs a constant map: one segment cannot follow a field that varies (nseg = 0 chooses)");
    }
    // (every check above is host arithmetic on the arguments; the device is touched from here on)
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h.fm_set = false;
    h.fm_L = 0;
    offres_drop_normal(h);          // the field-aware normal operator belongs to the map it was built for
    h.fm_f.clear(); h.fm_ts.clear(); h.fm_p.clear();        // (the host copies go with the map; filled again below once the new one is attached)
    if (!f_hz) return QMRI_OK;

    const bool constant = f_max == f_min;
    const double f0 = 0.5 * (f_min + f_max), lo = f_min - f0, width = (f_max - f_min) / nbins;
    // the histogram (p_h, f_h) of f - f0: equal bins on [f_min - f0, f_max - f0], f_h the centres
    if (constant) nbins = 1;
    std::vector<double2> hist((size_t)nbins);
    {
        std::vector<size_t> cnt((size_t)nbins, 0);
        for (size_t i = 0; i < plane; ++i) {
            int b = constant ? 0 : (int)std::floor(((f_hz[i] - f0) - lo) / width);
            cnt[(size_t)std::min(std::max(b, 0), nbins - 1)] += 1;
        }
        for (int b = 0; b < nbins; ++b) hist[b] = make_double2((double)cnt[b] / (double)plane, constant ? 0.0 : lo + (b + 0.5) * width);
    }
    DevPool tmp;
    double* d_f = nullptr; double* d_ts = nullptr; double2* d_hist = nullptr;
    QMRI_TRY(tmp.upload(ctx, &d_f, f_hz, plane));
    QMRI_TRY(tmp.upload(ctx, &d_ts, t_s, (size_t)o.m));
    QMRI_TRY(tmp.upload(ctx, &d_hist, hist.data(), hist.size()));
    const int L_first = constant ? 1 : (nseg ? nseg : 2), L_last = constant ? 1 : (nseg ? nseg : OFFRES_LMAX);
    QMRI_TRY(h.d_bl.ensure(ctx, (size_t)L_last * o.m));           // (sized here, at attach time: auto mode for its largest L)
    OffresFit fit{0.0, 0.0};
    std::vector<double> tauhat;
    int L = L_first, reached = 0;
    for (L = L_first; L <= L_last; ++L) {
        tauhat.assign((size_t)L, t_min);
        for (int l = 1; l < L; ++l) tauhat[l] = t_min + l * (t_max - t_min) / (L - 1);
        std::vector<cplx> G((size_t)nbins * L), A((size_t)L * L, cplx(0.0, 0.0));
        for (int b = 0; b < nbins; ++b)
            for (int l = 0; l < L; ++l) { const double a = -2.0 * PI * hist[b].y * tauhat[l]; G[(size_t)b * L + l] = cplx(std::cos(a), std::sin(a)); }
        for (int b = 0; b < nbins; ++b)
            for (int r = 0; r < L; ++r)
                for (int k = 0; k < L; ++k) A[(size_t)r * L + k] += hist[b].x * std::conj(G[(size_t)b * L + r]) * G[(size_t)b * L + k];
        double tr = 0.0;
        for (int r = 0; r < L; ++r) tr += A[(size_t)r * L + r].real();
        for (int r = 0; r < L; ++r) A[(size_t)r * L + r] += 1e-12 * tr / L;
        if (!cholesky(A, L)) { qmri_set_error(ctx, "qmri_set_field_map: the %d x %d coefficient system is not positive definite", L, L); return QMRI_ERR_INVALID_ARG; }
        std::vector<double2> Gd(G.size()), Cd(A.size());
        for (size_t i = 0; i < G.size(); ++i) Gd[i] = make_double2(G[i].real(), G[i].imag());
        for (size_t i = 0; i < A.size(); ++i) Cd[i] = make_double2(A[i].real(), A[i].imag());
        DevPool per;
        double2* d_G = nullptr; double2* d_C = nullptr;
        QMRI_TRY(per.upload(ctx, &d_G, Gd.data(), Gd.size()));
        QMRI_TRY(per.upload(ctx, &d_C, Cd.data(), Cd.size()));
        QMRI_TRY(offres_coefficients_dev(ctx, L, nbins, constant, d_hist, d_G, d_C, d_ts, f0, h.d_bl, &fit));
        reached = fit.fit_max <= tol;
        if (reached || L == L_last) break;
    }
    // the phase maps of the chosen segments, [L][N*M]
    QMRI_TRY(h.d_pm.ensure(ctx, (size_t)L * plane));
    double* d_tau = nullptr;
    QMRI_TRY(tmp.upload(ctx, &d_tau, tauhat.data(), tauhat.size()));
    QMRI_TRY(offres_phase_maps_dev(ctx, L, plane, d_f, f0, d_tau, h.d_pm));
    QMRI_HIP(ctx, hipDeviceSynchronize());          // (as qmri_set_operator: everything has landed before the context's stream reads it)
    h.fm_L = L;
    h.fm_set = true;
    // what qmri_nufft_prepare_normal_fm is defined by
    h.fm_f.assign(f_hz, f_hz + plane); h.fm_ts.assign(t_s, t_s + o.m);
    h.fm_p.resize((size_t)nbins);
    for (int b = 0; b < nbins; ++b) h.fm_p[b] = hist[b].x;
    h.fm_f0 = f0; h.fm_fmin = f_min; h.fm_fmax = f_max; h.fm_tmin = t_min; h.fm_tmax = t_max; h.fm_nbins = nbins;
    if (info) {
        *info = qmri_offres_info{};
        info->nseg = L; info->tol_reached = reached;
        info->fit_max = fit.fit_max; info->fit_rms = fit.fit_rms;
        info->f_min = f_min; info->f_max = f_max; info->t_min = t_min; info->t_max = t_max;
    }
    return QMRI_OK;
}

extern "C" int qmri_nufft_prepare_normal_fm(qmri_ctx* ctx, const qmri_offres_normal_params* p, qmri_offres_normal_info* info) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    int nseg = 0;
    double tol = OFFRES_TOL_DEF;
    if (p) {
        QMRI_CHECK_ARG(ctx, p->nseg == 0 || (p->nseg >= 2 && p->nseg <= OFFRES_NLMAX), "qmri_offres_normal_params.nseg must be in 2..32 (0 = auto)");
        QMRI_CHECK_ARG(ctx, std::isfinite(p->tol) && p->tol >= 0.0, "qmri_offres_normal_params.tol must be finite and >= 0 (0 = default 1e-4)");
        for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "qmri_offres_normal_params.reserved must be zero");
        nseg = p->nseg;
        if (p->tol > 0.0) tol = p->tol;
    }
    if (!ctx->op.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator_nufft first"); return QMRI_ERR_STATE; }
    if (ctx->op.kind != OP_NUFFT) {
        qmri_set_error(ctx, "qmri_nufft_prepare_normal_fm needs a trajectory operator (qmri_set_operator_nufft) with a field map; a gridded operator has "
                            "neither a Toeplitz normal operator nor readout times");
        return QMRI_ERR_UNSUPPORTED;
    }
    OpHost& o = ctx->op;
    NufftHost& h = o.nu;
    if (!h.fm_set) {
        qmri_set_error(ctx, "qmri_nufft_prepare_normal_fm: no field map attached: attach one with qmri_set_field_map first; without a map the plain "
                            "normal operator is built by qmri_nufft_prepare_normal");
        return QMRI_ERR_STATE;
    }
    // (every check above is host arithmetic on the arguments and the context; the device is touched from here on)
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t plane = (size_t)o.N * o.M, n = plane * o.s, kseg = (size_t)o.s * (o.s + 1) / 2 * 4 * plane;
    if (h.fm_fmax == h.fm_fmin) {
        // a constant map: the difference phase is identically 1 and the normal operator is the plain one, exactly
        QMRI_TRY(toep_prepare(ctx));              // (builds the plain transform, or finds the one built before the map)
        h.fmn_ready = true; h.fmn_plain = true; h.fmn_L = 1;
        if (info) { *info = qmri_offres_normal_info{}; info->nseg = 1; info->tol_reached = 1; info->khat_bytes = (uint64_t)(kseg * sizeof(double2)); }
        return QMRI_OK;
    }
    // the difference histogram: the autocorrelation of the map's, 2 nbins - 1 bins at g_j = j (f_max - f_min) / nbins, j = -(nbins - 1) .. nbins - 1
    const int nbins = h.fm_nbins, nb = 2 * nbins - 1;
    const double width = (h.fm_fmax - h.fm_fmin) / nbins;
    std::vector<double2> dh((size_t)nb);
    for (int j = -(nbins - 1); j <= nbins - 1; ++j) {
        double a = 0.0;
        for (int b = std::max(0, j); b < std::min(nbins, nbins + j); ++b) a += h.fm_p[b] * h.fm_p[b - j];
        dh[(size_t)(j + nbins - 1)] = make_double2(a, j * width);
    }
    DevPool tmp;
    double* d_ts = nullptr; double2* d_dh = nullptr; double* d_c = nullptr;
    const int L_first = nseg ? nseg : 2, L_last = nseg ? nseg : OFFRES_NLMAX;
    QMRI_TRY(tmp.upload(ctx, &d_ts, h.fm_ts.data(), h.fm_ts.size()));
    QMRI_TRY(tmp.upload(ctx, &d_dh, dh.data(), dh.size()));
    QMRI_TRY(tmp.alloc(ctx, &d_c, (size_t)L_last * o.m));
    // the tables of one tried L', allocated once at the largest L' of the search
    double2* d_G = nullptr; double2* d_Qw = nullptr; double* d_U = nullptr;
    QMRI_TRY(tmp.alloc(ctx, &d_G, (size_t)nb * L_last));
    QMRI_TRY(tmp.alloc(ctx, &d_Qw, (size_t)nb * L_last));
    QMRI_TRY(tmp.alloc(ctx, &d_U, (size_t)L_last * L_last));
    OffresFit fit{0.0, 0.0};
    std::vector<double> tauhat;
    int L = L_first, reached = 0;
    for (L = L_first; L <= L_last; ++L) {
        tauhat.resize((size_t)L);
        for (int l = 0; l < L; ++l) tauhat[l] = h.fm_tmin + l * (h.fm_tmax - h.fm_tmin) / (L - 1);
        std::vector<double2> G((size_t)nb * L);
        for (int j = 0; j < nb; ++j)
            for (int l = 0; l < L; ++l) { const double a = 2.0 * PI * dh[j].y * tauhat[l]; G[(size_t)j * L + l] = make_double2(std::cos(a), std::sin(a)); }
        // (R + eps I) c = rho, R = sum_j p~_j (cos cos + sin sin), eps = 1e-12 tr(R) / L = 1e-12 sum_j p~_j, is the least-squares problem of the stacked
        // table B = [sqrt(p~_j) cos; sqrt(p~_j) sin; sqrt(eps) I] with the right-hand side [sqrt(p~) cos 2 pi g tau; sqrt(p~) sin 2 pi g tau; 0].  It is
        // solved through B = Q U: c = U^-1 Q^T b.  U is R + eps I's Cholesky factor transposed and Q^T b the forward substitution's result, but
        // formed at B's condition, not at its square: through R itself fit_max at L' = 8 (condition 3e9) came out 1e-6 relative from the solution
        const size_t rows = 2 * (size_t)nb + L;
        double psum = 0.0;
        for (int j = 0; j < nb; ++j) psum += dh[j].x;
        std::vector<double> B(rows * L, 0.0), U;
        std::vector<double> w((size_t)nb);
        for (int j = 0; j < nb; ++j) w[j] = std::sqrt(dh[j].x);
        for (int l = 0; l < L; ++l) {
            for (int j = 0; j < nb; ++j) {
                B[(size_t)l * rows + 2 * j] = w[j] * G[(size_t)j * L + l].x;
                B[(size_t)l * rows + 2 * j + 1] = w[j] * G[(size_t)j * L + l].y;
            }
            B[(size_t)l * rows + 2 * nb + l] = std::sqrt(1e-12 * psum);
        }
        if (!qr_mgs2(B, rows, L, U)) {          // (the ridge rows keep every column's norm >= sqrt(eps) > 0: not reachable with a finite map)
            qmri_set_error(ctx, "qmri_nufft_prepare_normal_fm: the %d-column coefficient table is rank deficient (internal)", L);
            return QMRI_ERR_STATE;
        }
        std::vector<double2> Qw((size_t)nb * L);
        for (int j = 0; j < nb; ++j)
            for (int l = 0; l < L; ++l) Qw[(size_t)j * L + l] = make_double2(w[j] * B[(size_t)l * rows + 2 * j], w[j] * B[(size_t)l * rows + 2 * j + 1]);
        QMRI_HIP(ctx, hipMemcpy(d_G, G.data(), G.size() * sizeof(double2), hipMemcpyHostToDevice));
        QMRI_HIP(ctx, hipMemcpy(d_Qw, Qw.data(), Qw.size() * sizeof(double2), hipMemcpyHostToDevice));
        QMRI_HIP(ctx, hipMemcpy(d_U, U.data(), U.size() * sizeof(double), hipMemcpyHostToDevice));
        QMRI_TRY(offres_ncoefficients_dev(ctx, L, nb, d_dh, d_G, d_Qw, d_U, d_ts, d_c, &fit));
        reached = fit.fit_max <= tol;
        if (reached || L == L_last) break;
    }
    // everything the transform needs is allocated before the context changes: on a failure the context is as it was before the call
    DevBuf<double2> khat, pm, xs;
    QMRI_TRY(khat.ensure(ctx, (size_t)L * kseg));
    QMRI_TRY(pm.ensure(ctx, (size_t)L * plane));
    QMRI_TRY(xs.ensure(ctx, (size_t)o.maxB * n));
    double* d_f = nullptr; double* d_tau = nullptr;
    QMRI_TRY(tmp.upload(ctx, &d_f, h.fm_f.data(), h.fm_f.size()));
    QMRI_TRY(tmp.upload(ctx, &d_tau, tauhat.data(), tauhat.size()));
    QMRI_TRY(offres_phase_maps_dev(ctx, L, plane, d_f, h.fm_f0, d_tau, pm.p));
    for (int l = 0; l < L; ++l) QMRI_TRY(toep_build_weighted(ctx, d_c + (size_t)l * o.m, khat.p + (size_t)l * kseg));
    QMRI_HIP(ctx, hipDeviceSynchronize());
    offres_drop_normal(h);
    h.d_khat_fm = std::move(khat); h.d_pm_n = std::move(pm); h.d_xs = std::move(xs);
    h.fmn_L = L; h.fmn_plain = false; h.fmn_ready = true;
    if (info) {
        *info = qmri_offres_normal_info{};
        info->nseg = L; info->tol_reached = reached;
        info->fit_max = fit.fit_max; info->fit_rms = fit.fit_rms;
        info->khat_bytes = (uint64_t)((size_t)L * kseg * sizeof(double2));
    }
    return QMRI_OK;
}
