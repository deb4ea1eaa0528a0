// api_b1.cpp -- C ABI of the B1 estimate from the fingerprints (include/qmri.h; kernels: dictb_kernels.hip).  An EXTENSION with no
// reference counterpart.  Every refusal is decided before the device is selected, and the argument rules that need no context leave their message
// in qmri_last_error(NULL) when ctx == NULL.
#include <cmath>
#include <cstdint>
#include <cstring>
#include "qmri_internal.h"

namespace {

int need_ctx(qmri_ctx* ctx) {
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

// a narrow dictionary with groups
int scores_ready(qmri_ctx* ctx) {
    const DictHost& d = ctx->dict;
    if (!d.ready) { qmri_set_error(ctx, "dictionary not set: call qmri_set_dictionary first"); return QMRI_ERR_STATE; }
    if (d.wide) { qmri_set_error(ctx, "group scores are supported for dictionaries of s <= 16 channels (got %d)", d.s); return QMRI_ERR_UNSUPPORTED; }
    if (!d.G) { qmri_set_error(ctx, "dictionary groups not set: call qmri_set_dictionary_groups first"); return QMRI_ERR_STATE; }
    return QMRI_OK;
}

int scores_checks(qmri_ctx* ctx, const void* X, int Npix, const void* score) {
    QMRI_CHECK_ARG(ctx, Npix >= 1, "Npix >= 1");
    QMRI_CHECK_ARG(ctx, X && score, "X / score must not be NULL");
    QMRI_TRY(need_ctx(ctx));
    return scores_ready(ctx);
}

int pool_checks(qmri_ctx* ctx, int G, const double* group_val, int N, int M, int nslices, const void* score, int hw) {
    QMRI_CHECK_ARG(ctx, G >= 1 && G <= 256, "1 <= G <= 256 groups");
    QMRI_CHECK_ARG(ctx, group_val, "group_val must not be NULL");
    for (int g = 0; g < G; ++g)
        QMRI_CHECK_ARG(ctx, std::isfinite(group_val[g]) && (g == 0 || group_val[g] > group_val[g - 1]), "group_val must be finite and strictly ascending");
    QMRI_CHECK_ARG(ctx, hw >= 0 && hw <= 32, "0 <= half_window <= 32");
    QMRI_CHECK_ARG(ctx, N >= 1 && M >= 1 && nslices >= 1, "N, M, nslices >= 1");
    QMRI_CHECK_ARG(ctx, score, "score must not be NULL");
    return need_ctx(ctx);
}

int estimate_checks(qmri_ctx* ctx, const void* X, int N, int M, int nslices, const qmri_b1est_params* params, int* hw) {
    QMRI_CHECK_ARG(ctx, X, "X must not be NULL");
    QMRI_CHECK_ARG(ctx, N >= 1 && M >= 1 && nslices >= 1, "N, M, nslices >= 1");
    QMRI_CHECK_ARG(ctx, (double)N * M * nslices <= 2147483647.0, "N M nslices must fit a 32-bit pixel count");
    *hw = 4;
    if (params) {
        for (int r = 0; r < 7; ++r) QMRI_CHECK_ARG(ctx, params->reserved[r] == 0, "qmri_b1est_params.reserved must be zero");
        *hw = params->half_window;
    }
    QMRI_CHECK_ARG(ctx, *hw >= 0 && *hw <= 32, "0 <= half_window <= 32");
    QMRI_TRY(need_ctx(ctx));
    return scores_ready(ctx);
}

// slices per run so that the scratch, G * N * M * 12 bytes per slice (score 4 B + box sums 8 B), stays under 256 MB (knob b1_scratch_mb; one
// slice at least)
int slices_per_run(int G, int N, int M, int nslices) {
    const double per = 12.0 * G * N * M;
    const double r = std::floor((double)std::max(0, qmri_knob(K_B1_SCRATCH_MB)) * 1048576.0 / per);
    return (int)std::max(1.0, std::min((double)nslices, r));
}

int pool_run(qmri_ctx* ctx, int G, const double* group_val, int N, int M, int nslices, const float* d_score, const uint8_t* d_mask, int hw, double* d_b1,
             int32_t* d_grp, double* d_conf) {
    DictHost& D = ctx->dict;
    QMRI_TRY(D.d_bval.ensure(ctx, 256));
    QMRI_HIP(ctx, hipMemcpyAsync(D.d_bval.p, group_val, (size_t)G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const size_t ntot = (size_t)N * M * nslices;
    const int per = slices_per_run(G, N, M, nslices);
    for (int sl = 0; sl < nslices; sl += per)
        QMRI_TRY(b1_launch_pool(ctx, G, D.d_bval, N, M, sl, std::min(per, nslices - sl), d_score, ntot, 0, d_mask, hw, d_b1, d_grp, d_conf));
    return QMRI_OK;
}

int estimate_run(qmri_ctx* ctx, const double2* d_X, int N, int M, int nslices, const uint8_t* d_mask, int hw, double* d_b1, int32_t* d_grp, double* d_conf) {
    DictHost& D = ctx->dict;
    const size_t nm = (size_t)N * M, ntot = nm * nslices;
    const int per = slices_per_run(D.G, N, M, nslices);
    QMRI_TRY(D.d_bscore.ensure(ctx, (size_t)D.G * nm * per));
    for (int sl = 0; sl < nslices; sl += per) {
        const int nsl = std::min(per, nslices - sl);
        const size_t p0 = (size_t)sl * nm;
        QMRI_TRY(dictb_launch_scores(ctx, d_X, ntot, p0, (int)(nm * nsl), D.d_bscore));
        QMRI_TRY(b1_launch_pool(ctx, D.G, D.d_gval, N, M, sl, nsl, D.d_bscore, nm * nsl, p0, d_mask, hw, d_b1, d_grp, d_conf));
    }
    return QMRI_OK;
}

}  // namespace

extern "C" int qmri_dict_group_scores_dev(qmri_ctx* ctx, const void* d_X, int Npix, float* d_score) {
    QMRI_TRY(scores_checks(ctx, d_X, Npix, d_score));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return dictb_launch_scores(ctx, (const double2*)d_X, (size_t)Npix, 0, Npix, d_score);
}

extern "C" int qmri_dict_group_scores(qmri_ctx* ctx, const void* X, int Npix, float* score) {
    QMRI_TRY(scores_checks(ctx, X, Npix, score));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const DictHost& d = ctx->dict;
    const size_t nx = (size_t)Npix * d.s, ns = (size_t)Npix * d.G;
    DevBuf<double2> dX; DevBuf<float> ds;
    QMRI_TRY(dX.ensure(ctx, nx));
    QMRI_TRY(ds.ensure(ctx, ns));
    QMRI_HIP(ctx, hipMemcpyAsync(dX.p, X, nx * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(dictb_launch_scores(ctx, dX.p, (size_t)Npix, 0, Npix, ds.p));
    QMRI_HIP(ctx, hipMemcpyAsync(score, ds.p, ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_b1_pool_dev(qmri_ctx* ctx, int G, const double* group_val, int N, int M, int nslices, const float* d_score, const uint8_t* d_mask,
                                int half_window, double* d_b1, int32_t* d_grp, double* d_conf) {
    QMRI_TRY(pool_checks(ctx, G, group_val, N, M, nslices, d_score, half_window));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return pool_run(ctx, G, group_val, N, M, nslices, d_score, d_mask, half_window, d_b1, d_grp, d_conf);
}

extern "C" int qmri_b1_pool(qmri_ctx* ctx, int G, const double* group_val, int N, int M, int nslices, const float* score, const uint8_t* mask, int half_window,
                            double* b1, int32_t* grp, double* conf) {
    QMRI_TRY(pool_checks(ctx, G, group_val, N, M, nslices, score, half_window));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N * M * nslices;
    DevBuf<float> ds; DevBuf<uint8_t> dm; DevBuf<double> db, dc; DevBuf<int32_t> dg;
    QMRI_TRY(ds.ensure(ctx, n * G));
    if (mask) QMRI_TRY(dm.ensure(ctx, n));
    if (b1) QMRI_TRY(db.ensure(ctx, n));
    if (grp) QMRI_TRY(dg.ensure(ctx, n));
    if (conf) QMRI_TRY(dc.ensure(ctx, n));
    QMRI_HIP(ctx, hipMemcpyAsync(ds.p, score, n * G * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (mask) QMRI_HIP(ctx, hipMemcpyAsync(dm.p, mask, n, hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(pool_run(ctx, G, group_val, N, M, nslices, ds.p, dm.p, half_window, db.p, dg.p, dc.p));
    if (b1) QMRI_HIP(ctx, hipMemcpyAsync(b1, db.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (grp) QMRI_HIP(ctx, hipMemcpyAsync(grp, dg.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (conf) QMRI_HIP(ctx, hipMemcpyAsync(conf, dc.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_b1_estimate_dev(qmri_ctx* ctx, const void* d_X, int N, int M, int nslices, const uint8_t* d_mask, const qmri_b1est_params* params,
                                    double* d_b1, int32_t* d_grp, double* d_conf, qmri_b1est_info* info) {
    int hw = 4;
    QMRI_TRY(estimate_checks(ctx, d_X, N, M, nslices, params, &hw));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    if (info) *info = qmri_b1est_info{};                        // (filled by the host variant only: nothing here waits for the device)
    return estimate_run(ctx, (const double2*)d_X, N, M, nslices, d_mask, hw, d_b1, d_grp, d_conf);
}

extern "C" int qmri_b1_estimate(qmri_ctx* ctx, const void* X, int N, int M, int nslices, const uint8_t* mask, const qmri_b1est_params* params, double* b1,
                                int32_t* grp, double* conf, qmri_b1est_info* info) {
    int hw = 4;
    QMRI_TRY(estimate_checks(ctx, X, N, M, nslices, params, &hw));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const DictHost& d = ctx->dict;
    const size_t n = (size_t)N * M * nslices, nx = n * d.s;
    const bool want_g = grp || info, want_c = conf || info;
    DevBuf<double2> dX; DevBuf<uint8_t> dm; DevBuf<double> db, dc; DevBuf<int32_t> dg;
    QMRI_TRY(dX.ensure(ctx, nx));
    if (mask) QMRI_TRY(dm.ensure(ctx, n));
    if (b1) QMRI_TRY(db.ensure(ctx, n));
    if (want_g) QMRI_TRY(dg.ensure(ctx, n));
    if (want_c) QMRI_TRY(dc.ensure(ctx, n));
    QMRI_HIP(ctx, hipMemcpyAsync(dX.p, X, nx * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    if (mask) QMRI_HIP(ctx, hipMemcpyAsync(dm.p, mask, n, hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(estimate_run(ctx, dX.p, N, M, nslices, dm.p, hw, db.p, dg.p, dc.p));
    std::vector<int32_t> hg; std::vector<double> hc;
    if (info && !grp) hg.resize(n);
    if (info && !conf) hc.resize(n);
    int32_t* og = grp ? grp : hg.data();
    double* oc = conf ? conf : hc.data();
    if (b1) QMRI_HIP(ctx, hipMemcpyAsync(b1, db.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (want_g) QMRI_HIP(ctx, hipMemcpyAsync(og, dg.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (want_c) QMRI_HIP(ctx, hipMemcpyAsync(oc, dc.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {                                                 // pixels in ascending order
        *info = qmri_b1est_info{};
        double sum = 0.0;
        for (size_t p = 0; p < n; ++p) {
            if (og[p] > 0) { ++info->n_estimated; sum += oc[p]; }
            else ++info->n_unmatched;
        }
        info->mean_conf = info->n_estimated ? sum / info->n_estimated : 0.0;
    }
    return QMRI_OK;
}
