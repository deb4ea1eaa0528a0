// api_fmap.cpp -- C ABI of the field-map estimate from multi-echo images (include/qmri.h; kernels: fmap_kernels.hip).  An
// EXTENSION with no reference counterpart.  Every refusal is decided here, on the host, before the device is selected; with ctx == NULL the message
// of the first failing check is left in qmri_last_error(NULL), so the argument rules can be exercised on a machine without a GPU.
#include <cmath>
#include <cstdint>
#include "qmri_internal.h"

namespace {
constexpr int FMAP_MAX_COILS = 128, FMAP_MAX_SIDE = 4096, FMAP_MAX_SLICES = 4096, FMAP_MAX_ITERS = 100000, FMAP_DEFAULT_ITERS = 200;
constexpr double FMAP_DEFAULT_BETA = 0.01, FMAP_TWO_PI = 6.283185307179586476925286766559;

// QMRI_OK, or the code of the first failing check with its message set on ctx (ctx may be NULL).  host: Y and f_init can be read here
int fmap_checks(qmri_ctx* ctx, int nslices, int nechoes, int ncoil, int N, int M, const void* Y, const double* t_s, const double* f_init,
                const qmri_fieldmap_params* p, const double* f_out, bool host) {
    QMRI_CHECK_ARG(ctx, Y && t_s && f_out, "Y / t_s / f_out must not be NULL");
    QMRI_CHECK_ARG(ctx, nslices >= 1 && nslices <= FMAP_MAX_SLICES, "nslices must satisfy 1 <= nslices <= 4096");
    QMRI_CHECK_ARG(ctx, nechoes >= 2 && nechoes <= 8, "nechoes must satisfy 2 <= nechoes <= 8");
    QMRI_CHECK_ARG(ctx, ncoil >= 1, "ncoil >= 1");
    if (ncoil > FMAP_MAX_COILS) { qmri_set_error(ctx, "unsupported: the field map estimate takes at most 128 coils (ncoil > 128)"); return QMRI_ERR_UNSUPPORTED; }
    QMRI_CHECK_ARG(ctx, N >= 2 && N <= FMAP_MAX_SIDE && M >= 2 && M <= FMAP_MAX_SIDE, "N and M must satisfy 2 <= N, M <= 4096");
    for (int l = 0; l < nechoes; ++l) {
        QMRI_CHECK_ARG(ctx, std::isfinite(t_s[l]), "t_s must be finite");
        QMRI_CHECK_ARG(ctx, l == 0 || t_s[l] > t_s[l - 1], "t_s must be strictly increasing");
    }
    if (p) {
        QMRI_CHECK_ARG(ctx, p->iters >= 0 && p->iters <= FMAP_MAX_ITERS, "iters must satisfy 0 <= iters <= 100000 (0: the default 200)");
        QMRI_CHECK_ARG(ctx, std::isfinite(p->beta) && p->beta >= 0.0, "beta must be finite and >= 0 (0: the default 0.01)");
        QMRI_CHECK_ARG(ctx, p->phase_sign >= -1 && p->phase_sign <= 1, "phase_sign must be -1, +1 or 0 (the default -1)");
        for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "reserved must be 0");
    }
    QMRI_CHECK_ARG(ctx, !f_init || f_init != f_out || host, "d_f_out must not alias d_f_init");
    if (host) {
        const double* y = static_cast<const double*>(Y);
        const size_t ny = (size_t)2 * nslices * nechoes * ncoil * N * M, nf = (size_t)nslices * N * M;
        for (size_t i = 0; i < ny; ++i) QMRI_CHECK_ARG(ctx, std::isfinite(y[i]), "Y must be finite");
        if (f_init)
            for (size_t i = 0; i < nf; ++i) QMRI_CHECK_ARG(ctx, std::isfinite(f_init[i]), "f_init must be finite");
    }
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

FmapPlan fmap_plan(int nslices, int nechoes, int ncoil, int N, int M, const double* t_s, const qmri_fieldmap_params* p) {
    FmapPlan pl{};
    pl.nslices = nslices; pl.L = nechoes; pl.C = ncoil; pl.N = N; pl.M = M;
    pl.iters = p && p->iters ? p->iters : FMAP_DEFAULT_ITERS;
    pl.sign = p && p->phase_sign > 0 ? 1 : -1;
    const double b = p && p->beta != 0.0 ? p->beta : FMAP_DEFAULT_BETA, span = FMAP_TWO_PI * (t_s[nechoes - 1] - t_s[0]);
    pl.beta = b * (span * span);
    pl.unwrap_limit_hz = 1.0 / (2.0 * (t_s[1] - t_s[0]));
    for (int a = 0; a < nechoes; ++a)
        for (int c = a + 1; c < nechoes; ++c) {
            pl.pa[pl.P] = a; pl.pb[pl.P] = c;
            pl.d[pl.P++] = FMAP_TWO_PI * (t_s[c] - t_s[a]);
        }
    return pl;
}
}  // namespace

extern "C" int qmri_field_map_estimate_dev(qmri_ctx* ctx, int nslices, int nechoes, int ncoil, int N, int M, const void* d_Y, const double* t_s,
                                           const double* d_f_init, const qmri_fieldmap_params* p, double* d_f_out, double* d_trust_out,
                                           qmri_fieldmap_info* info) {
    QMRI_TRY(fmap_checks(ctx, nslices, nechoes, ncoil, N, M, d_Y, t_s, d_f_init, p, d_f_out, false));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return fmap_estimate_dev(ctx, fmap_plan(nslices, nechoes, ncoil, N, M, t_s, p), (const double2*)d_Y, d_f_init, d_f_out, d_trust_out, info);
}

extern "C" int qmri_field_map_estimate(qmri_ctx* ctx, int nslices, int nechoes, int ncoil, int N, int M, const void* Y, const double* t_s,
                                       const double* f_init, const qmri_fieldmap_params* p, double* f_out, double* trust_out, qmri_fieldmap_info* info) {
    QMRI_TRY(fmap_checks(ctx, nslices, nechoes, ncoil, N, M, Y, t_s, f_init, p, f_out, true));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nf = (size_t)nslices * N * M, ny = nf * nechoes * ncoil;
    DevBuf<double2> dY;
    DevBuf<double> dinit, df, dtrust;
    QMRI_TRY(dY.ensure(ctx, ny));
    QMRI_TRY(df.ensure(ctx, nf));
    if (f_init) QMRI_TRY(dinit.ensure(ctx, nf));
    if (trust_out) QMRI_TRY(dtrust.ensure(ctx, nf));
    QMRI_HIP(ctx, hipMemcpyAsync(dY.p, Y, ny * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    if (f_init) QMRI_HIP(ctx, hipMemcpyAsync(dinit.p, f_init, nf * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(fmap_estimate_dev(ctx, fmap_plan(nslices, nechoes, ncoil, N, M, t_s, p), dY.p, dinit.p, df.p, dtrust.p, info));
    QMRI_HIP(ctx, hipMemcpyAsync(f_out, df.p, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (trust_out) QMRI_HIP(ctx, hipMemcpyAsync(trust_out, dtrust.p, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
