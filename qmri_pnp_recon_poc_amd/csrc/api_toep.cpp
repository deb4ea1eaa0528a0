// api_toep.cpp -- the Toeplitz normal operator of a trajectory operator and the solver built on it: the entry points
// qmri_nufft_prepare_normal, qmri_normal(_dev), and the choice of x-update solver the multi-coil loops make.  The kernels are in toep_kernels.hip.
#include "qmri_internal.h"

namespace {
// The context has a trajectory operator, else QMRI_ERR_STATE / QMRI_ERR_UNSUPPORTED with a message that names the gridded route.  Host checks only:
// the caller selects the device after its own argument checks, so every refusal is decided before the device is touched.
int require_trajectory(qmri_ctx* ctx, const char* what, const char* instead) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    if (!ctx->op.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    if (ctx->op.kind != OP_NUFFT) {
        qmri_set_error(ctx, "%s needs a trajectory operator (qmri_set_operator_nufft); on a gridded operator %s", what, instead);
        return QMRI_ERR_UNSUPPORTED;
    }
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_nufft_prepare_normal(qmri_ctx* ctx) {
    QMRI_TRY(require_trajectory(ctx, "qmri_nufft_prepare_normal", "there is no Toeplitz normal operator to build"));
    QMRI_TRY(offres_refuse_toeplitz(ctx, "qmri_nufft_prepare_normal"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return toep_prepare(ctx);           // (with a field map and its own transform in force this builds nothing)
}

extern "C" int qmri_normal_dev(qmri_ctx* ctx, const void* d_x, void* d_out, int batch) {
    QMRI_TRY(require_trajectory(ctx, "qmri_normal_dev", "use qmri_adjoint_dev(qmri_forward_dev(x))"));
    QMRI_CHECK_ARG(ctx, d_x && d_out && batch >= 1 && batch <= ctx->op.maxB, "qmri_normal_dev arguments / batch > max_batch");
    QMRI_TRY(offres_refuse_toeplitz(ctx, "qmri_normal_dev"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return toep_apply(ctx, batch, (const double2*)d_x, (double2*)d_out);
}

extern "C" int qmri_normal(qmri_ctx* ctx, const void* x, int x_is_complex, void* out) {
    QMRI_TRY(require_trajectory(ctx, "qmri_normal", "use qmri_adjoint(qmri_forward(x))"));
    QMRI_CHECK_ARG(ctx, x && out, "x / out must not be NULL");
    QMRI_TRY(offres_refuse_toeplitz(ctx, "qmri_normal"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    if (x_is_complex) {
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_xa, x, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    } else {
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_xb, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(ew_launch_real_to_complex(ctx, n, (const double*)o.d_xb, o.d_xa));
    }
    QMRI_TRY(toep_apply(ctx, 1, o.d_xa, o.d_xa));
    QMRI_HIP(ctx, hipMemcpyAsync(out, o.d_xa, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

int toep_check_solver(qmri_ctx* ctx, int solver) {
    if (solver != QMRI_SOLVER_TOEPLITZ) return QMRI_OK;
    if (!ctx->op.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    if (ctx->op.kind == OP_NUFFT) return offres_refuse_toeplitz(ctx, "QMRI_SOLVER_TOEPLITZ");      // (a field map whose normal operator is not prepared)
    qmri_set_error(ctx, "QMRI_SOLVER_TOEPLITZ needs a trajectory operator (qmri_set_operator_nufft): on a gridded operator A^H A is already diagonal "
                        "per k-space location; use QMRI_SOLVER_LSQR (the k-space LSQR)");
    return QMRI_ERR_UNSUPPORTED;
}

int mc_xupdate_dev(qmri_ctx* ctx, int solver, int B, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                   double2* d_x, int32_t* iters_out, int32_t* flags_out) {
    if (solver == QMRI_SOLVER_TOEPLITZ) QMRI_TRY(offres_refuse_toeplitz(ctx, "QMRI_SOLVER_TOEPLITZ"));     // (a transform built before the map is never used with it)
    if (solver == QMRI_SOLVER_TOEPLITZ) return qmri_cg_toep_batch_dev(ctx, B, ncoil, d_maps, d_y, d_z, r, tol, maxit, d_x, iters_out, flags_out);
    return qmri_lsqr_mc_batch_dev(ctx, B, ncoil, d_maps, d_y, d_z, r, tol, maxit, d_x, iters_out, flags_out);
}
