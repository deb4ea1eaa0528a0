// api_dcf.cpp -- density compensation for trajectory operators: qmri_nufft_dcf (Pipe-Menon weights on the plan's own kernel),
// qmri_set_sample_weights, and the weighted adjoints qmri_adjoint_w(_dev, _mc).  The iteration's kernels are in dcf_kernels.hip; the multiply by w is
// fused into the staging of k_nu_spread (nufft_kernels.hip).  The kernel sum and the scale kappa of the weights are nufft_plan.h's.  Every refusal is
// decided on the host before the device is selected.
#include <cmath>

#include "qmri_internal.h"

namespace {
constexpr int DCF_NITER_DEF = 20, DCF_NITER_MAX = 200;

int require_trajectory(qmri_ctx* ctx, const char* what) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    if (!ctx->op.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator_nufft first"); return QMRI_ERR_STATE; }
    if (ctx->op.kind != OP_NUFFT) {
        qmri_set_error(ctx, "%s needs a trajectory operator (qmri_set_operator_nufft): a gridded mask samples every k location it holds once per frame "
                            "and needs no density compensation; use qmri_adjoint", what);
        return QMRI_ERR_UNSUPPORTED;
    }
    return QMRI_OK;
}
int require_weights(qmri_ctx* ctx, const char* what) {
    if (ctx->op.nu.w_set) return QMRI_OK;
    qmri_set_error(ctx, "%s: no sample weights attached: call qmri_nufft_dcf or qmri_set_sample_weights first", what);
    return QMRI_ERR_STATE;
}
int ensure_weight_array(qmri_ctx* ctx) {
    NufftHost& h = ctx->op.nu;
    QMRI_TRY(h.d_w.ensure(ctx, (size_t)ctx->op.m));
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_nufft_dcf(qmri_ctx* ctx, const qmri_dcf_params* p, double* w_out, qmri_dcf_info* info) {
    QMRI_TRY(require_trajectory(ctx, "qmri_nufft_dcf"));
    int niter = DCF_NITER_DEF;
    double tol = 0.0;
    if (p) {
        QMRI_CHECK_ARG(ctx, p->niter >= 0 && p->niter <= DCF_NITER_MAX, "qmri_dcf_params.niter must be in 1..200 (0 = default 20)");
        QMRI_CHECK_ARG(ctx, std::isfinite(p->tol) && p->tol >= 0.0, "qmri_dcf_params.tol must be finite and >= 0 (0 = never stop early)");
        for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "qmri_dcf_params.reserved must be zero");
        if (p->niter) niter = p->niter;
        tol = p->tol;
    }
    OpHost& o = ctx->op;
    const double kappa = nuplan::dcf_kappa(o.T, o.nu.w, o.nu.beta);
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    o.nu.w_set = false;
    QMRI_TRY(ensure_weight_array(ctx));
    qmri_dcf_info got{};
    QMRI_TRY(dcf_weights_dev(ctx, niter, tol, kappa, o.nu.d_w, &got));
    if (w_out) QMRI_HIP(ctx, hipMemcpy(w_out, o.nu.d_w, (size_t)o.m * sizeof(double), hipMemcpyDeviceToHost));
    o.nu.w_set = true;
    if (info) *info = got;
    return QMRI_OK;
}

extern "C" int qmri_set_sample_weights(qmri_ctx* ctx, const double* w) {
    QMRI_TRY(require_trajectory(ctx, "qmri_set_sample_weights"));
    OpHost& o = ctx->op;
    if (w)
        for (int i = 0; i < o.m; ++i)
            if (!(std::isfinite(w[i]) && w[i] >= 0.0)) {
                qmri_set_error(ctx, "invalid argument: w[%d] = %g is not a finite value >= 0", i, w[i]);
                return QMRI_ERR_INVALID_ARG;
            }
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    o.nu.w_set = false;
    if (!w) return QMRI_OK;
    QMRI_TRY(ensure_weight_array(ctx));
    QMRI_HIP(ctx, hipMemcpy(o.nu.d_w, w, (size_t)o.m * sizeof(double), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipDeviceSynchronize());          // (as qmri_set_operator: the blocking copy must have landed before the context's stream reads it)
    o.nu.w_set = true;
    return QMRI_OK;
}

extern "C" int qmri_adjoint_w_dev(qmri_ctx* ctx, const void* d_y, void* d_x, int batch) {
    QMRI_TRY(require_trajectory(ctx, "qmri_adjoint_w_dev"));
    QMRI_CHECK_ARG(ctx, d_x && d_y && batch >= 1 && batch <= ctx->op.maxB, "qmri_adjoint_w_dev arguments / batch > max_batch");
    QMRI_TRY(require_weights(ctx, "qmri_adjoint_w_dev"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return nufft_launch_adj_w(ctx, batch, (const double2*)d_y, (double2*)d_x);
}

extern "C" int qmri_adjoint_w(qmri_ctx* ctx, const void* y, void* x) {
    QMRI_TRY(require_trajectory(ctx, "qmri_adjoint_w"));
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    QMRI_TRY(require_weights(ctx, "qmri_adjoint_w"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_ya, y, (size_t)o.m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(nufft_launch_adj_w(ctx, 1, o.d_ya, o.d_xa));
    QMRI_HIP(ctx, hipMemcpyAsync(x, o.d_xa, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// qmri_adjoint_mc (api_operator.cpp) with the weighted spreading
extern "C" int qmri_adjoint_w_mc(qmri_ctx* ctx, const void* y, void* x) {
    QMRI_TRY(require_trajectory(ctx, "qmri_adjoint_w_mc"));
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    OpHost& o = ctx->op;
    if (!o.ncoil) { qmri_set_error(ctx, "no coil maps set: call qmri_set_coils first"); return QMRI_ERR_STATE; }
    QMRI_TRY(require_weights(ctx, "qmri_adjoint_w_mc"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    for (int j0 = 0; j0 < o.ncoil; j0 += o.maxB) {
        const int cnt = std::min(o.maxB, o.ncoil - j0);
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_ya, (const double2*)y + (size_t)j0 * o.m, (size_t)cnt * o.m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(nufft_launch_adj_w(ctx, cnt, o.d_ya, o.d_x));
        QMRI_TRY(ew_launch_coil_sum(ctx, n, plane, cnt, o.d_x, o.d_coils + (size_t)j0 * plane, o.d_xa, j0 > 0));
    }
    QMRI_HIP(ctx, hipMemcpyAsync(x, o.d_xa, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
