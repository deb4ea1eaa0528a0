// api_offres.cpp -- off-resonance correction of a trajectory operator by time segmentation: qmri_set_field_map checks its
// arguments, builds the histogram of the map, the segment times and the Cholesky factor of the L x L coefficient system on the host, and has the
// device compute the per-sample coefficients, their fit and the phase maps (offres_kernels.hip).  The segment loop itself is in nufft_launch_fwd /
// launch_adj (nufft_kernels.hip).  Every refusal is decided on the host before the device is selected.
#include <cmath>
#include <complex>
#include <vector>

#include "qmri_internal.h"

namespace {
constexpr double PI = 3.14159265358979323846;
constexpr int OFFRES_LMAX = 16, OFFRES_NBINS_DEF = 256, OFFRES_NBINS_MIN = 16, OFFRES_NBINS_MAX = 1024;
constexpr double OFFRES_TOL_DEF = 1e-4;
typedef std::complex<double> cplx;

// device buffers that live for one call
struct Temp {
    std::vector<void*> ptrs;
    ~Temp() { for (void* p : ptrs) if (p) (void)hipFree(p); }
    template <typename T> int upload(qmri_ctx* ctx, T** d, const T* src, size_t count) {
        QMRI_TRY(dev_alloc(ctx, d, count));
        ptrs.push_back(*d);
        QMRI_HIP(ctx, hipMemcpy(*d, src, count * sizeof(T), hipMemcpyHostToDevice));
        return QMRI_OK;
    }
};

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

int ensure(qmri_ctx* ctx, double2** p, size_t* cap, size_t count) {
    if (*p && *cap >= count) return QMRI_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    QMRI_TRY(dev_alloc(ctx, p, count));
    *cap = count;
    return QMRI_OK;
}
}  // namespace

int offres_refuse_toeplitz(qmri_ctx* ctx, const char* what) {
    if (!ctx || !ctx->op.ready || ctx->op.kind != OP_NUFFT || !ctx->op.nu.fm_set) return QMRI_OK;
    qmri_set_error(ctx, "%s is not available while a field map is attached (qmri_set_field_map): A^H A is then L^2 Toeplitz terms, which are not built; "
                        "use QMRI_SOLVER_LSQR (the image-domain LSQR runs the corrected operator), or clear the map with qmri_set_field_map(ctx, NULL, ...)", what);
    return QMRI_ERR_UNSUPPORTED;
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
    Temp tmp;
    double* d_f = nullptr; double* d_ts = nullptr; double2* d_hist = nullptr;
    QMRI_TRY(tmp.upload(ctx, &d_f, f_hz, plane));
    QMRI_TRY(tmp.upload(ctx, &d_ts, t_s, (size_t)o.m));
    QMRI_TRY(tmp.upload(ctx, &d_hist, hist.data(), hist.size()));
    const int L_first = constant ? 1 : (nseg ? nseg : 2), L_last = constant ? 1 : (nseg ? nseg : OFFRES_LMAX);
    QMRI_TRY(ensure(ctx, &h.d_bl, &h.bl_cap, (size_t)L_last * o.m));           // (sized here, at attach time: auto mode for its largest L)
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
        Temp per;
        double2* d_G = nullptr; double2* d_C = nullptr;
        QMRI_TRY(per.upload(ctx, &d_G, Gd.data(), Gd.size()));
        QMRI_TRY(per.upload(ctx, &d_C, Cd.data(), Cd.size()));
        QMRI_TRY(offres_coefficients_dev(ctx, L, nbins, constant, d_hist, d_G, d_C, d_ts, f0, h.d_bl, &fit));
        reached = fit.fit_max <= tol;
        if (reached || L == L_last) break;
    }
    // the phase maps of the chosen segments, [L][N*M]
    QMRI_TRY(ensure(ctx, &h.d_pm, &h.pm_cap, (size_t)L * plane));
    double* d_tau = nullptr;
    QMRI_TRY(tmp.upload(ctx, &d_tau, tauhat.data(), tauhat.size()));
    QMRI_TRY(offres_phase_maps_dev(ctx, L, plane, d_f, f0, d_tau, h.d_pm));
    QMRI_HIP(ctx, hipDeviceSynchronize());          // (as qmri_set_operator: everything has landed before the context's stream reads it)
    h.fm_L = L;
    h.fm_set = true;
    if (info) {
        *info = qmri_offres_info{};
        info->nseg = L; info->tol_reached = reached;
        info->fit_max = fit.fit_max; info->fit_rms = fit.fit_rms;
        info->f_min = f_min; info->f_max = f_max; info->t_min = t_min; info->t_max = t_max;
    }
    return QMRI_OK;
}
