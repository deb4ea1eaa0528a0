// api_sms.cpp -- C ABI of the simultaneous multi-slice (SMS) extension (include/qmri.h; kernels: sms_kernels.hip; schedule: sms_plan.h; DESIGN.md
// section 31).  An EXTENSION with no reference counterpart.  Every refusal is decided here, on the host, before the device is selected; with
// ctx == NULL the message of the first failing check is left in qmri_last_error(NULL), so the argument rules can be exercised on a machine without a GPU.
#include <cmath>
#include <cstdint>
#include "qmri_internal.h"

namespace {
int sms_no_ctx() {
    qmri_set_error(nullptr, "invalid argument: ctx must not be NULL");
    return QMRI_ERR_INVALID_ARG;
}

// the checks every _sms call shares: the arguments first (they need no context), then the state, then what the state cannot serve
int sms_require(qmri_ctx* ctx, int G, int ncoil, const void* maps, const void* y) {
    QMRI_CHECK_ARG(ctx, G >= 1 && ncoil >= 1 && ncoil <= 1024, "G >= 1 and 1 <= ncoil <= 1024");
    QMRI_CHECK_ARG(ctx, maps && y, "maps / y must not be NULL");
    if (!ctx) return sms_no_ctx();
    const OpHost& o = ctx->op;
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator or qmri_set_operator_nufft first"); return QMRI_ERR_STATE; }
    if (!o.sms.Z) { qmri_set_error(ctx, "no simultaneous multi-slice phases set: call qmri_set_sms first"); return QMRI_ERR_STATE; }
    if (o.kind == OP_NUFFT && o.nu.fm_set) {
        qmri_set_error(ctx, "a field map is attached to the operator: one map cannot serve the %d slices of a simultaneous multi-slice group", o.sms.Z);
        return QMRI_ERR_UNSUPPORTED;
    }
    return QMRI_OK;
}

// the loop's own checks: the solver, Step 2, and how many slice images a launch holds
int sms_admm_checks(qmri_ctx* ctx, int groups, const qmri_admm_params* prm, const char* what) {
    QMRI_CHECK_ARG(ctx, prm, "params must not be NULL");
    if (prm->solver == QMRI_SOLVER_TOEPLITZ) {
        qmri_set_error(ctx, "QMRI_SOLVER_TOEPLITZ is not available for simultaneous multi-slice groups: the normal operator of Z coupled slices needs "
                            "Z^2 point-spread functions, which are not built; use QMRI_SOLVER_LSQR");
        return QMRI_ERR_UNSUPPORTED;
    }
    if (prm->solver == QMRI_SOLVER_DIRECT) {
        qmri_set_error(ctx, "the DIRECT solver is not available for simultaneous multi-slice groups: its closed form needs one slice per k-space; use "
                            "QMRI_SOLVER_LSQR");
        return QMRI_ERR_UNSUPPORTED;
    }
    QMRI_TRY(mc_admm_check(ctx, prm));
    const int B = groups * ctx->op.sms.Z;
    if (groups < 1 || B > ctx->op.maxB || (!(ctx->llr.on || ctx->wav.on) && B > ctx->net.maxB)) {
        qmri_set_error(ctx, "invalid argument: %s x Z = %d slice images exceed max_batch of the operator or the denoiser", what, B);
        return QMRI_ERR_INVALID_ARG;
    }
    return QMRI_OK;
}

// the loop of mc_admm_loop with the coupled x-update, on device arrays: G Z <= max_batch slice images (d_x0 NULL: x = A_sms' y)
int sms_admm_group(qmri_ctx* ctx, int G, int ncoil, const double2* d_maps, const double2* d_y, const qmri_admm_params* prm, const double2* d_x0,
                   double2* d_x, int32_t* li_out) {
    const OpHost& o = ctx->op;
    const int B = G * o.sms.Z;
    const size_t n = (size_t)o.N * o.M * o.s;
    AdmmSolve sv;
    sv.nsolve = G;
    sv.start = [&](double2* x) -> int {
        if (!d_x0) return sms_adjoint_dev(ctx, G, ncoil, d_maps, d_y, x);
        QMRI_HIP(ctx, hipMemcpyAsync(x, d_x0, (size_t)B * n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
        return QMRI_OK;
    };
    sv.solve = [&](const double2* z, double2* x, int32_t* li) {
        return sms_lsqr_dev(ctx, G, ncoil, d_maps, d_y, z, prm->gamma, prm->cg_tol, prm->cg_maxit, x, li, nullptr);
    };
    return mc_admm_loop(ctx, B, prm, sv, d_x, li_out, prm->iters);
}

// the staging of the host-array calls (McWork's, sized for G groups): maps -> sm, y -> sy, images -> sz / sx
struct Staging { double2 *sm, *sy, *sx, *sz; size_t maps_n, y_n, x_n; };
int sms_stage(qmri_ctx* ctx, int G, int ncoil, Staging* sg) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    const size_t sl = (size_t)G * o.sms.Z, plane = (size_t)o.N * o.M;
    sg->maps_n = sl * ncoil * plane; sg->y_n = (size_t)G * ncoil * o.m; sg->x_n = sl * plane * o.s;
    const int st = [&]() -> int {
        QMRI_TRY(w.sm.ensure(ctx, sg->maps_n));
        QMRI_TRY(w.sy.ensure(ctx, sg->y_n));
        QMRI_TRY(w.sx.ensure(ctx, sg->x_n));
        return w.sz.ensure(ctx, sg->x_n);
    }();
    if (st == QMRI_ERR_NOMEM) qmri_set_error(ctx, "out of device memory for the staging of %d simultaneous multi-slice groups x %d coils", G, ncoil);
    sg->sm = w.sm; sg->sy = w.sy; sg->sx = w.sx; sg->sz = w.sz;
    return st;
}
int to_dev(qmri_ctx* ctx, double2* dst, const void* src, size_t count) {
    QMRI_HIP(ctx, hipMemcpyAsync(dst, src, count * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    return QMRI_OK;
}
int to_host(qmri_ctx* ctx, void* dst, const double2* src, size_t count) {
    QMRI_HIP(ctx, hipMemcpyAsync(dst, src, count * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_set_sms(qmri_ctx* ctx, int Z, const void* E) {
    QMRI_CHECK_ARG(ctx, Z >= 0 && Z <= sms::MAX_Z, "Z must satisfy 0 <= Z <= 8 (0 clears the simultaneous multi-slice phases)");
    if (!ctx) return sms_no_ctx();
    OpHost& o = ctx->op;
    if (Z == 0 || !E) {                                           // cleared; the device arrays stay for the next set
        o.sms.Z = 0;
        o.sms.E.clear();
        o.sms.on_device = false;
        return QMRI_OK;
    }
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator or qmri_set_operator_nufft first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, (long)o.T * Z <= sms::MAX_E, "T x Z must not exceed 8192 phase values");
    const double* e = (const double*)E;
    for (size_t i = 0; i < (size_t)2 * o.T * Z; ++i) QMRI_CHECK_ARG(ctx, std::isfinite(e[i]), "every value of E must be finite");
    if (o.kind == OP_NUFFT && o.nu.fm_set) {
        qmri_set_error(ctx, "a field map is attached to the operator: one map cannot serve the %d slices of a simultaneous multi-slice group", Z);
        return QMRI_ERR_UNSUPPORTED;
    }
    const double2* e2 = (const double2*)E;
    o.sms.E.assign(e2, e2 + (size_t)o.T * Z);
    o.sms.Z = Z;
    o.sms.on_device = false;                                      // (uploaded, after a wait for the stream, by the first call that needs it)
    return QMRI_OK;
}

extern "C" int qmri_forward_sms(qmri_ctx* ctx, int G, int ncoil, const void* maps, const void* x, int x_is_complex, void* y) {
    QMRI_TRY(sms_require(ctx, G, ncoil, maps, y));
    QMRI_CHECK_ARG(ctx, x, "x must not be NULL");
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    Staging sg;
    QMRI_TRY(sms_stage(ctx, G, ncoil, &sg));
    QMRI_TRY(to_dev(ctx, sg.sm, maps, sg.maps_n));
    if (x_is_complex) QMRI_TRY(to_dev(ctx, sg.sx, x, sg.x_n));
    else {
        QMRI_HIP(ctx, hipMemcpyAsync(sg.sz, x, sg.x_n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(ew_launch_real_to_complex(ctx, sg.x_n, (const double*)sg.sz, sg.sx));
    }
    QMRI_TRY(sms_forward_dev(ctx, G, ncoil, sg.sm, sg.sx, sg.sy));
    return to_host(ctx, y, sg.sy, sg.y_n);
}

extern "C" int qmri_adjoint_sms(qmri_ctx* ctx, int G, int ncoil, const void* maps, const void* y, void* x) {
    QMRI_TRY(sms_require(ctx, G, ncoil, maps, y));
    QMRI_CHECK_ARG(ctx, x, "x must not be NULL");
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    Staging sg;
    QMRI_TRY(sms_stage(ctx, G, ncoil, &sg));
    QMRI_TRY(to_dev(ctx, sg.sm, maps, sg.maps_n));
    QMRI_TRY(to_dev(ctx, sg.sy, y, sg.y_n));
    QMRI_TRY(sms_adjoint_dev(ctx, G, ncoil, sg.sm, sg.sy, sg.sx));
    return to_host(ctx, x, sg.sx, sg.x_n);
}

extern "C" int qmri_xupdate_sms(qmri_ctx* ctx, int G, int ncoil, const void* maps, const void* y, const void* z, double r, double tol, int maxit,
                                const void* x0, void* x_out, int32_t* iters_out, int32_t* flags_out) {
    QMRI_TRY(sms_require(ctx, G, ncoil, maps, y));
    QMRI_CHECK_ARG(ctx, z && x_out && r > 0 && maxit >= 0, "z / x_out must not be NULL, r > 0, maxit >= 0");
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    Staging sg;
    QMRI_TRY(sms_stage(ctx, G, ncoil, &sg));
    QMRI_TRY(to_dev(ctx, sg.sm, maps, sg.maps_n));
    QMRI_TRY(to_dev(ctx, sg.sy, y, sg.y_n));
    QMRI_TRY(to_dev(ctx, sg.sz, z, sg.x_n));
    if (x0) QMRI_TRY(to_dev(ctx, sg.sx, x0, sg.x_n));
    else QMRI_HIP(ctx, hipMemsetAsync(sg.sx, 0, sg.x_n * sizeof(double2), ctx->stream));
    QMRI_TRY(sms_lsqr_dev(ctx, G, ncoil, sg.sm, sg.sy, sg.sz, r, tol, maxit, sg.sx, iters_out, flags_out));
    return to_host(ctx, x_out, sg.sx, sg.x_n);
}

extern "C" int qmri_pnp_admm_sms_dev(qmri_ctx* ctx, int G, int ncoil, const void* d_maps, const void* d_y, const qmri_admm_params* prm, const void* d_x0,
                                     void* d_x_out, int32_t* lsqr_iters_out) {
    QMRI_TRY(sms_require(ctx, G, ncoil, d_maps, d_y));
    QMRI_CHECK_ARG(ctx, d_x_out && d_x_out != d_x0, "x_out must not be NULL and must not alias x0");
    QMRI_TRY(sms_admm_checks(ctx, G, prm, "G"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(sms_admm_group(ctx, G, ncoil, (const double2*)d_maps, (const double2*)d_y, prm, (const double2*)d_x0, (double2*)d_x_out, lsqr_iters_out));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_pnp_admm_sms(qmri_ctx* ctx, int G, int groups_per_launch, int ncoil, const void* maps, const void* y, const qmri_admm_params* prm,
                                 const void* x0, void* x_out, int32_t* lsqr_iters_out) {
    QMRI_TRY(sms_require(ctx, G, ncoil, maps, y));
    QMRI_CHECK_ARG(ctx, x_out && groups_per_launch >= 1, "x_out must not be NULL, groups_per_launch >= 1");
    const int gpl = std::min(groups_per_launch, G);
    QMRI_TRY(sms_admm_checks(ctx, gpl, prm, "groups_per_launch"));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const OpHost& o = ctx->op;
    const size_t plane = (size_t)o.N * o.M, n = plane * o.s, Z = (size_t)o.sms.Z;
    for (int g0 = 0; g0 < G; g0 += gpl) {                         // (the first run is the largest: the staging is sized once)
        const int Gr = std::min(gpl, G - g0);
        Staging sg;
        QMRI_TRY(sms_stage(ctx, Gr, ncoil, &sg));
        QMRI_TRY(to_dev(ctx, sg.sm, (const double2*)maps + (size_t)g0 * Z * ncoil * plane, sg.maps_n));
        QMRI_TRY(to_dev(ctx, sg.sy, (const double2*)y + (size_t)g0 * ncoil * o.m, sg.y_n));
        if (x0) QMRI_TRY(to_dev(ctx, sg.sz, (const double2*)x0 + (size_t)g0 * Z * n, sg.x_n));
        QMRI_TRY(sms_admm_group(ctx, Gr, ncoil, sg.sm, sg.sy, prm, x0 ? sg.sz : nullptr, sg.sx,
                                lsqr_iters_out ? lsqr_iters_out + (size_t)g0 * prm->iters : nullptr));
        QMRI_TRY(to_host(ctx, (double2*)x_out + (size_t)g0 * Z * n, sg.sx, sg.x_n));      // returns x, not v
    }
    return QMRI_OK;
}
