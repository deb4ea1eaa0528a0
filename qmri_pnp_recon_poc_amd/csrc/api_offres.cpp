// api_offres.cpp -- off-resonance correction of a trajectory operator by time segmentation: qmri_set_field_map checks its
// arguments, has offres_plan.h build the histogram of the map and, per tried L, the segment times and the Cholesky factor of the L x L coefficient
// system, and has the device compute the per-sample coefficients, their fit and the phase maps (offres_kernels.hip).  The segment loop itself is in
// nufft_launch_fwd / launch_adj (nufft_kernels.hip).  Every refusal is decided on the host before the device is selected.
// qmri_nufft_prepare_normal_fm builds the field-aware Toeplitz normal operator of the attached map: the difference histogram
// and the QR tables of the real coefficient system come from offres_plan.h, and per segment the K^ of toep_kernels.hip with the samples weighted by
// the segment's coefficients.  Both searches of L stay here: the fit that ends them comes back from the device.
#include <cmath>
#include <vector>

#include "qmri_internal.h"

using namespace offres;

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

    const MapHist hist = map_histogram(f_hz, plane, f_min, f_max, nbins);
    const bool constant = hist.constant;
    const double f0 = hist.f0;
    nbins = hist.nbins;
    DevPool tmp;
    double* d_f = nullptr; double* d_ts = nullptr; double2* d_hist = nullptr;
    QMRI_TRY(tmp.upload(ctx, &d_f, f_hz, plane));
    QMRI_TRY(tmp.upload(ctx, &d_ts, t_s, (size_t)o.m));
    QMRI_TRY(tmp.upload(ctx, &d_hist, (const double2*)hist.pf.data(), (size_t)nbins));
    const int L_first = constant ? 1 : (nseg ? nseg : 2), L_last = constant ? 1 : (nseg ? nseg : OFFRES_LMAX);
    QMRI_TRY(h.d_bl.ensure(ctx, (size_t)L_last * o.m));           // (sized here, at attach time: auto mode for its largest L)
    OffresFit fit{0.0, 0.0};
    FitSystem sys;
    int L = L_first, reached = 0;
    for (L = L_first; L <= L_last; ++L) {
        sys = fit_system(hist, t_min, t_max, L);
        if (!sys.ok) { qmri_set_error(ctx, "qmri_set_field_map: the %d x %d coefficient system is not positive definite", L, L); return QMRI_ERR_INVALID_ARG; }
        DevPool per;
        double2* d_G = nullptr; double2* d_C = nullptr;
        QMRI_TRY(per.upload(ctx, &d_G, (const double2*)sys.G.data(), sys.G.size()));
        QMRI_TRY(per.upload(ctx, &d_C, (const double2*)sys.C.data(), sys.C.size()));
        QMRI_TRY(offres_coefficients_dev(ctx, L, nbins, constant, d_hist, d_G, d_C, d_ts, f0, h.d_bl, &fit));
        reached = fit.fit_max <= tol;
        if (reached || L == L_last) break;
    }
    // the phase maps of the chosen segments, [L][N*M]
    QMRI_TRY(h.d_pm.ensure(ctx, (size_t)L * plane));
    double* d_tau = nullptr;
    QMRI_TRY(tmp.upload(ctx, &d_tau, sys.tauhat.data(), sys.tauhat.size()));
    QMRI_TRY(offres_phase_maps_dev(ctx, L, plane, d_f, f0, d_tau, h.d_pm));
    QMRI_HIP(ctx, hipDeviceSynchronize());          // (as qmri_set_operator: everything has landed before the context's stream reads it)
    h.fm_L = L;
    h.fm_set = true;
    // what qmri_nufft_prepare_normal_fm is defined by
    h.fm_f.assign(f_hz, f_hz + plane); h.fm_ts.assign(t_s, t_s + o.m);
    h.fm_p.resize((size_t)nbins);
    for (int b = 0; b < nbins; ++b) h.fm_p[b] = hist.p(b);
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
    const std::vector<double> dh = diff_histogram(h.fm_p, (h.fm_fmax - h.fm_fmin) / nbins);
    DevPool tmp;
    double* d_ts = nullptr; double2* d_dh = nullptr; double* d_c = nullptr;
    const int L_first = nseg ? nseg : 2, L_last = nseg ? nseg : OFFRES_NLMAX;
    QMRI_TRY(tmp.upload(ctx, &d_ts, h.fm_ts.data(), h.fm_ts.size()));
    QMRI_TRY(tmp.upload(ctx, &d_dh, (const double2*)dh.data(), (size_t)nb));
    QMRI_TRY(tmp.alloc(ctx, &d_c, (size_t)L_last * o.m));
    // the tables of one tried L', allocated once at the largest L' of the search
    double2* d_G = nullptr; double2* d_Qw = nullptr; double* d_U = nullptr;
    QMRI_TRY(tmp.alloc(ctx, &d_G, (size_t)nb * L_last));
    QMRI_TRY(tmp.alloc(ctx, &d_Qw, (size_t)nb * L_last));
    QMRI_TRY(tmp.alloc(ctx, &d_U, (size_t)L_last * L_last));
    OffresFit fit{0.0, 0.0};
    NormalTables tb;
    int L = L_first, reached = 0;
    for (L = L_first; L <= L_last; ++L) {
        tb = normal_tables(dh, h.fm_tmin, h.fm_tmax, L);
        if (!tb.ok) {
            qmri_set_error(ctx, "qmri_nufft_prepare_normal_fm: the %d-column coefficient table is rank deficient (internal)", L);
            return QMRI_ERR_STATE;
        }
        QMRI_HIP(ctx, hipMemcpy(d_G, tb.G.data(), tb.G.size() * sizeof(double), hipMemcpyHostToDevice));
        QMRI_HIP(ctx, hipMemcpy(d_Qw, tb.Qw.data(), tb.Qw.size() * sizeof(double), hipMemcpyHostToDevice));
        QMRI_HIP(ctx, hipMemcpy(d_U, tb.U.data(), tb.U.size() * sizeof(double), hipMemcpyHostToDevice));
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
    QMRI_TRY(tmp.upload(ctx, &d_tau, tb.tauhat.data(), tb.tauhat.size()));
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
