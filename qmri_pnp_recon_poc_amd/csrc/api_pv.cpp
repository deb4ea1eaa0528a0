// api_pv.cpp -- C ABI of the tissue-fraction unmixing (include/qmri.h; kernel: pv_kernels.hip).  An EXTENSION with no reference
// counterpart.  The components are formed here, on the host, from the dictionary's host copy; every refusal is decided before the device is
// selected, and the argument rules that need no context leave their message in qmri_last_error(NULL) when ctx == NULL.
#include <cmath>
#include <cstdint>
#include <cstring>
#include "qmri_internal.h"

int pv_form_components(const float* D, const float* normD, int K, int s, int C, const int32_t* atoms, double* tab, double* min_pivot, std::string* msg) {
    auto fail = [&](const std::string& m) { if (msg) *msg = m; return (int)QMRI_ERR_INVALID_ARG; };
    for (int c = 0; c < C; ++c) {
        if (atoms[c] < 1 || atoms[c] > K) return fail("atom " + std::to_string(atoms[c]) + " is outside 1.." + std::to_string(K) + " (indices are 1-based)");
        for (int e = 0; e < c; ++e)
            if (atoms[e] == atoms[c]) return fail("atom " + std::to_string(atoms[c]) + " is named twice");
    }
    std::memset(tab, 0, PV_TAB * sizeof(double));
    double* A = tab + PV_TAB_A; double* G = tab + PV_TAB_G; double* asum = tab + PV_TAB_ASUM; double* na = tab + PV_TAB_NA;
    for (int c = 0; c < C; ++c) {
        const size_t k = (size_t)atoms[c] - 1;
        bool zero = true;
        for (int j = 0; j < s; ++j) {
            const double v = (double)normD[k] * (double)D[k + (size_t)K * j];
            if (!std::isfinite(v)) return fail("atom " + std::to_string(atoms[c]) + " is not finite");
            if (v != 0.0) zero = false;
            A[j * PV_MAX_C + c] = v;
        }
        if (zero) return fail("atom " + std::to_string(atoms[c]) + " is zero");
    }
    if (C > s) return fail("more components (" + std::to_string(C) + ") than channels (" + std::to_string(s) + ")");
    for (int a = 0; a < C; ++a)
        for (int b = 0; b < C; ++b) {
            double g = 0.0;
            for (int j = 0; j < s; ++j) g += A[j * PV_MAX_C + a] * A[j * PV_MAX_C + b];       // channels ascending
            G[a * PV_MAX_C + b] = g;
        }
    for (int j = 0; j < s; ++j) {
        double t = 0.0;
        for (int c = 0; c < C; ++c) t += A[j * PV_MAX_C + c];
        asum[j] = t;
    }
    for (int c = 0; c < C; ++c) na[c] = std::sqrt(G[c * PV_MAX_C + c]);
    // Cholesky (ascending) of G scaled to a unit diagonal: its smallest pivot says how far the components are from collinear
    double L[PV_MAX_C][PV_MAX_C] = {};
    double pmin = 1.0;
    for (int j = 0; j < C; ++j) {
        double v = G[j * PV_MAX_C + j] / (na[j] * na[j]);
        for (int k = 0; k < j; ++k) v -= L[j][k] * L[j][k];
        pmin = std::min(pmin, v);
        if (!(v > 1e-10)) return fail("the components are collinear: scaled Cholesky pivot " + std::to_string(v) + " at component " + std::to_string(j + 1) + " (must exceed 1e-10)");
        L[j][j] = std::sqrt(v);
        for (int i = j + 1; i < C; ++i) {
            double u = G[i * PV_MAX_C + j] / (na[i] * na[j]);
            for (int k = 0; k < j; ++k) u -= L[i][k] * L[j][k];
            L[i][j] = u / L[j][j];
        }
    }
    *min_pivot = pmin;
    return QMRI_OK;
}

extern "C" int qmri_set_components(qmri_ctx* ctx, int C, const int32_t* atoms, qmri_pv_info* info) {
    QMRI_CHECK_ARG(ctx, C >= 0 && C <= PV_MAX_C, "0 <= C <= 8 components (0 clears)");
    QMRI_CHECK_ARG(ctx, C == 0 || atoms, "atoms must not be NULL");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    DictHost& d = ctx->dict;
    if (C == 0) {                                               // (the table stays allocated: an unmixing in flight may still read it)
        d.pv.C = d.pv.s = 0; d.pv.min_pivot = 0.0;
        if (info) *info = qmri_pv_info{};
        return QMRI_OK;
    }
    if (!d.ready) { qmri_set_error(ctx, "dictionary not set: call qmri_set_dictionary first"); return QMRI_ERR_STATE; }
    if (d.wide) { qmri_set_error(ctx, "components are supported for dictionaries of s <= 16 channels (got %d)", d.s); return QMRI_ERR_UNSUPPORTED; }
    double tab[PV_TAB], pmin = 0.0;
    std::string msg;
    if (pv_form_components(d.D_h.data(), d.normD_h.data(), d.K, d.s, C, atoms, tab, &pmin, &msg) != QMRI_OK) {
        qmri_set_error(ctx, "invalid argument: %s", msg.c_str());
        return QMRI_ERR_INVALID_ARG;
    }
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));           // an unmixing in flight reads the old table
    QMRI_TRY(d.pv.d_tab.ensure(ctx, PV_TAB));
    QMRI_HIP(ctx, hipMemcpy(d.pv.d_tab.p, tab, sizeof tab, hipMemcpyHostToDevice));
    d.pv.C = C; d.pv.s = d.s; d.pv.min_pivot = pmin;
    if (info) { *info = qmri_pv_info{}; info->min_pivot = pmin; info->C = C; info->s = d.s; }
    return QMRI_OK;
}

namespace {
int unmix_checks(qmri_ctx* ctx, const void* X, int Npix, int mode, const void* w) {
    QMRI_CHECK_ARG(ctx, Npix >= 1, "Npix >= 1");
    QMRI_CHECK_ARG(ctx, X && w, "X / w must not be NULL");
    QMRI_CHECK_ARG(ctx, mode == QMRI_PV_REAL || mode == QMRI_PV_PHASE, "mode must be QMRI_PV_REAL (0) or QMRI_PV_PHASE (1)");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    if (!ctx->dict.pv.C) { qmri_set_error(ctx, "components not set: call qmri_set_components first"); return QMRI_ERR_STATE; }
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_dict_unmix_dev(qmri_ctx* ctx, const void* d_X, int Npix, int mode, double* d_w, double* d_frac, double* d_pd, double* d_res,
                                   int32_t* d_flags) {
    QMRI_TRY(unmix_checks(ctx, d_X, Npix, mode, d_w));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return pv_launch(ctx, (const double2*)d_X, Npix, mode, d_w, d_frac, (double2*)d_pd, d_res, d_flags);
}

extern "C" int qmri_dict_unmix(qmri_ctx* ctx, const void* X, int Npix, int mode, double* w, double* frac, double* pd, double* res, int32_t* flags) {
    QMRI_TRY(unmix_checks(ctx, X, Npix, mode, w));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const PvHost& pv = ctx->dict.pv;
    const size_t n = (size_t)Npix, nx = n * pv.s, nw = n * pv.C;
    DevBuf<double2> dX, dpd; DevBuf<double> dw, df, dr; DevBuf<int32_t> dfl;
    QMRI_TRY(dX.ensure(ctx, nx));
    QMRI_TRY(dw.ensure(ctx, nw));
    if (frac) QMRI_TRY(df.ensure(ctx, nw));
    if (pd) QMRI_TRY(dpd.ensure(ctx, n));
    if (res) QMRI_TRY(dr.ensure(ctx, n));
    if (flags) QMRI_TRY(dfl.ensure(ctx, n));
    QMRI_HIP(ctx, hipMemcpyAsync(dX.p, X, nx * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(pv_launch(ctx, dX.p, Npix, mode, dw.p, df.p, dpd.p, dr.p, dfl.p));
    QMRI_HIP(ctx, hipMemcpyAsync(w, dw.p, nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (frac) QMRI_HIP(ctx, hipMemcpyAsync(frac, df.p, nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (pd) QMRI_HIP(ctx, hipMemcpyAsync(pd, dpd.p, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    if (res) QMRI_HIP(ctx, hipMemcpyAsync(res, dr.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (flags) QMRI_HIP(ctx, hipMemcpyAsync(flags, dfl.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
