// api_refine.cpp -- C ABI of the sub-grid refinement of a dictionary match (include/qmri.h; kernel: refine_kernels.hip; lines: refine_plan.h; DESIGN.md
// section 30).  An EXTENSION with no reference counterpart.  The lines and the table of unnormalised atoms are formed here, on the host, from the
// dictionary's host copy; every refusal is decided before the device is selected, and the argument rules that need no context leave their message in
// qmri_last_error(NULL) when ctx == NULL.
#include <cstdint>
#include <cstring>
#include <utility>
#include "qmri_internal.h"

extern "C" int qmri_dict_lines(int K, int Q, const float* lut, const float* normD, int P, const int32_t* cols, int32_t* nbr_out, int32_t* info) {
    QMRI_CHECK_ARG(nullptr, lut && normD && cols && nbr_out && info, "lut / normD / cols / nbr_out / info must not be NULL");
    QMRI_CHECK_ARG(nullptr, K >= 1 && Q >= 1, "K >= 1 and Q >= 1");
    QMRI_CHECK_ARG(nullptr, P >= 1 && P <= rplan::MAX_P, "1 <= P <= 3 refined columns");
    const std::string bad = rplan::dict_lines(K, Q, lut, normD, P, cols, nbr_out, info);
    if (!bad.empty()) { qmri_set_error(nullptr, "invalid argument: %s", bad.c_str()); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

extern "C" int qmri_set_refine(qmri_ctx* ctx, int P, const int32_t* cols, qmri_refine_info* info) {
    QMRI_CHECK_ARG(ctx, P >= 0 && P <= rplan::MAX_P, "0 <= P <= 3 refined columns (0 clears)");
    QMRI_CHECK_ARG(ctx, P == 0 || cols, "cols must not be NULL");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    DictHost& d = ctx->dict;
    if (P == 0) {                                               // (the tables stay allocated: a fit in flight may still read them)
        d.rf.P = 0;
        if (info) *info = qmri_refine_info{};
        return QMRI_OK;
    }
    if (!d.ready) { qmri_set_error(ctx, "dictionary not set: call qmri_set_dictionary first"); return QMRI_ERR_STATE; }
    if (d.wide) { qmri_set_error(ctx, "refinement is supported for dictionaries of s <= 16 channels (got %d)", d.s); return QMRI_ERR_UNSUPPORTED; }
    std::vector<int32_t> nbr((size_t)d.K * P * 2);
    int32_t count[3][3] = {};
    const std::string bad = rplan::dict_lines(d.K, d.Q, d.lut_h.data(), d.normD_h.data(), P, cols, nbr.data(), &count[0][0]);
    if (!bad.empty()) { qmri_set_error(ctx, "invalid argument: %s", bad.c_str()); return QMRI_ERR_INVALID_ARG; }
    std::vector<double> arow((size_t)d.K * rplan::ROW);
    rplan::atom_rows(d.K, d.s, d.D_h.data(), d.normD_h.data(), arow.data());
    // new tables beside the old ones; the old ones go only when the new ones are in place
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    DevArr<int32_t> d_nbr; DevArr<double> d_arow;
    QMRI_TRY(d_nbr.ensure(ctx, nbr.size()));
    QMRI_TRY(d_arow.ensure(ctx, arow.size()));
    QMRI_HIP(ctx, hipMemcpy(d_nbr.p, nbr.data(), nbr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(d_arow.p, arow.data(), arow.size() * sizeof(double), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));           // a fit in flight reads the old tables
    d.rf.d_nbr = std::move(d_nbr); d.rf.d_arow = std::move(d_arow);
    d.rf.P = P;
    for (int q = 0; q < 3; ++q) d.rf.cols[q] = q < P ? cols[q] : 0;
    std::memcpy(d.rf.count, count, sizeof count);
    if (info) {
        *info = qmri_refine_info{};
        info->P = P; info->K = d.K; info->s = d.s;
        std::memcpy(info->count, count, sizeof count);
    }
    return QMRI_OK;
}

namespace {
int refine_checks(qmri_ctx* ctx, const void* X, int Npix, const void* dm) {
    QMRI_CHECK_ARG(ctx, Npix >= 1, "Npix >= 1");
    QMRI_CHECK_ARG(ctx, X && dm, "X / dm must not be NULL");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    if (!ctx->dict.ready || !ctx->dict.rf.P) { qmri_set_error(ctx, "refinement not set: call qmri_set_refine first"); return QMRI_ERR_STATE; }
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_dict_refine_dev(qmri_ctx* ctx, const void* d_X, int Npix, const int32_t* d_dm, double* d_qmap, double* d_pd, double* d_res, double* d_t,
                                    int32_t* d_centre, int32_t* d_flags) {
    QMRI_TRY(refine_checks(ctx, d_X, Npix, d_dm));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return refine_launch(ctx, (const double2*)d_X, Npix, d_dm, d_qmap, (double2*)d_pd, d_res, d_t, d_centre, d_flags);
}

extern "C" int qmri_dict_refine(qmri_ctx* ctx, const void* X, int Npix, const int32_t* dm, double* qmap, double* pd, double* res, double* t, int32_t* centre,
                                int32_t* flags) {
    QMRI_TRY(refine_checks(ctx, X, Npix, dm));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const DictHost& d = ctx->dict;
    const size_t n = (size_t)Npix, nx = n * d.s, nq = n * d.Q, nt = n * d.rf.P;
    DevBuf<double2> dX, dpd; DevBuf<double> dq, dr, dt; DevBuf<int32_t> ddm, dc, dfl;
    QMRI_TRY(dX.ensure(ctx, nx));
    QMRI_TRY(ddm.ensure(ctx, n));
    if (qmap) QMRI_TRY(dq.ensure(ctx, nq));
    if (pd) QMRI_TRY(dpd.ensure(ctx, n));
    if (res) QMRI_TRY(dr.ensure(ctx, n));
    if (t) QMRI_TRY(dt.ensure(ctx, nt));
    if (centre) QMRI_TRY(dc.ensure(ctx, n));
    if (flags) QMRI_TRY(dfl.ensure(ctx, n));
    QMRI_HIP(ctx, hipMemcpyAsync(dX.p, X, nx * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(ddm.p, dm, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(refine_launch(ctx, dX.p, Npix, ddm.p, dq.p, dpd.p, dr.p, dt.p, dc.p, dfl.p));
    if (qmap) QMRI_HIP(ctx, hipMemcpyAsync(qmap, dq.p, nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (pd) QMRI_HIP(ctx, hipMemcpyAsync(pd, dpd.p, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    if (res) QMRI_HIP(ctx, hipMemcpyAsync(res, dr.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (t) QMRI_HIP(ctx, hipMemcpyAsync(t, dt.p, nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (centre) QMRI_HIP(ctx, hipMemcpyAsync(centre, dc.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (flags) QMRI_HIP(ctx, hipMemcpyAsync(flags, dfl.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
