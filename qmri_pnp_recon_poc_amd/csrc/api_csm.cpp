// api_csm.cpp -- C ABI of the coil-map estimate (include/qmri.h; kernels: csm_kernels.hip).  A multi-coil EXTENSION with no reference counterpart.
// Every refusal is decided here, on the host, before the device is selected; with ctx == NULL the message of the first failing check is left in
// qmri_last_error(NULL), so the argument rules can be exercised on a machine without a GPU.
#include <cmath>
#include "qmri_internal.h"

namespace {
constexpr int CSM_MAX_COILS = 128;

// QMRI_OK, or the code of the first failing check with its message set on ctx (ctx may be NULL)
int csm_checks(qmri_ctx* ctx, int nslices, int ncoil, int N, int M, const void* calib, const qmri_csm_params* p, const void* maps_out, bool dev) {
    QMRI_CHECK_ARG(ctx, p, "coil map params must not be NULL");
    QMRI_CHECK_ARG(ctx, calib && maps_out, "calib / maps_out must not be NULL");
    QMRI_CHECK_ARG(ctx, nslices >= 1, "nslices >= 1");
    QMRI_CHECK_ARG(ctx, ncoil >= 1, "ncoil >= 1");
    if (ncoil > CSM_MAX_COILS) { qmri_set_error(ctx, "unsupported: the coil map estimate takes at most 128 coils (ncoil > 128)"); return QMRI_ERR_UNSUPPORTED; }
    if (!dc_size_supported(N) || !dc_size_supported(M)) {
        qmri_set_error(ctx, "invalid argument: N=%d, M=%d: each side must be one of the operator's supported sizes (32, 64, 96, 112, 128, 160, 192, 224, 256)", N, M);
        return QMRI_ERR_INVALID_ARG;
    }
    QMRI_CHECK_ARG(ctx, p->kind == QMRI_CSM_KSPACE || p->kind == QMRI_CSM_IMAGES, "kind must be QMRI_CSM_KSPACE or QMRI_CSM_IMAGES");
    if (p->kind == QMRI_CSM_KSPACE) {
        QMRI_CHECK_ARG(ctx, p->cN % 2 == 0 && p->cN >= 8 && p->cN <= N, "cN must be even with 8 <= cN <= N");
        QMRI_CHECK_ARG(ctx, p->cM % 2 == 0 && p->cM >= 8 && p->cM <= M, "cM must be even with 8 <= cM <= M");
        QMRI_CHECK_ARG(ctx, p->window == 0 || p->window == 1, "window must be 0 or 1");
    }
    QMRI_CHECK_ARG(ctx, p->patch >= 0 && p->patch <= 4, "patch must satisfy 0 <= patch <= 4");
    QMRI_CHECK_ARG(ctx, p->phase_ref == QMRI_CSM_PHASE_OBJECT || p->phase_ref == QMRI_CSM_PHASE_COIL, "phase_ref must be QMRI_CSM_PHASE_OBJECT or QMRI_CSM_PHASE_COIL");
    QMRI_CHECK_ARG(ctx, std::isfinite(p->thresh) && p->thresh >= 0.0, "thresh must be finite and >= 0");
    QMRI_CHECK_ARG(ctx, !dev || maps_out != calib, "d_maps_out must not alias d_calib");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    if (!ctx->op.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first (the coil map estimate runs on its FFT passes)"); return QMRI_ERR_STATE; }
    if (N != ctx->op.N || M != ctx->op.M) {
        qmri_set_error(ctx, "invalid argument: N=%d, M=%d are not the operator's grid (%d x %d)", N, M, ctx->op.N, ctx->op.M);
        return QMRI_ERR_INVALID_ARG;
    }
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_coil_maps_dev(qmri_ctx* ctx, int nslices, int ncoil, int N, int M, const void* d_calib, const qmri_csm_params* p, void* d_maps_out,
                                  void* d_img_out, double* d_lambda_out, qmri_csm_info* info) {
    QMRI_TRY(csm_checks(ctx, nslices, ncoil, N, M, d_calib, p, d_maps_out, true));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return csm_maps_dev(ctx, nslices, ncoil, (const double2*)d_calib, *p, (double2*)d_maps_out, (double2*)d_img_out, d_lambda_out, info);
}

extern "C" int qmri_coil_maps(qmri_ctx* ctx, int nslices, int ncoil, int N, int M, const void* calib, const qmri_csm_params* p, void* maps_out, void* img_out,
                              double* lambda_out, qmri_csm_info* info) {
    QMRI_TRY(csm_checks(ctx, nslices, ncoil, N, M, calib, p, maps_out, false));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t plane = (size_t)N * M, nimg = (size_t)nslices * ncoil;
    const size_t ncal = nimg * (p->kind == QMRI_CSM_KSPACE ? (size_t)p->cN * p->cM : plane);
    DevBuf<double2> cal, maps, img;
    DevBuf<double> lam;
    QMRI_TRY(cal.ensure(ctx, ncal));
    QMRI_TRY(maps.ensure(ctx, nimg * plane));
    if (img_out) QMRI_TRY(img.ensure(ctx, (size_t)nslices * plane));
    if (lambda_out) QMRI_TRY(lam.ensure(ctx, (size_t)nslices * plane));
    QMRI_HIP(ctx, hipMemcpyAsync(cal.p, calib, ncal * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(csm_maps_dev(ctx, nslices, ncoil, cal, *p, maps, img_out ? img.p : nullptr, lambda_out ? lam.p : nullptr, info));
    QMRI_HIP(ctx, hipMemcpyAsync(maps_out, maps.p, nimg * plane * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    if (img_out) QMRI_HIP(ctx, hipMemcpyAsync(img_out, img.p, (size_t)nslices * plane * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    if (lambda_out) QMRI_HIP(ctx, hipMemcpyAsync(lambda_out, lam.p, (size_t)nslices * plane * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
