// api_dict.cpp -- dictionary match of libqmri.so: the dictionary's device form (qmri_set_dictionary), its groups (qmri_set_dictionary_groups) and the
// qmri_dict_match* entry points.
//
// Replaces (reference file:line): mrf_dtm_cpu.m:1-166.
#include "qmri_internal.h"

#include <algorithm>
#include <cmath>

void qmri_free_dict(qmri_ctx* ctx) {
    DictHost& d = ctx->dict;
    const int filter_on = d.filter_on; const float margin_scale = d.margin_scale;
    d = DictHost();
    d.filter_on = filter_on; d.margin_scale = margin_scale;
}

extern "C" int qmri_set_dictionary(qmri_ctx* ctx, int K, int s, int Q, const float* D, const float* normD, const float* lut) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_CHECK_ARG(ctx, D && normD && lut, "D / normD / lut must not be NULL");
    QMRI_CHECK_ARG(ctx, K > 0 && s > 0 && Q > 0, "K, s, Q must be positive");
    if (s > 1024) { qmri_set_error(ctx, "dictionary match supports s <= 1024 channels (got %d)", s); return QMRI_ERR_UNSUPPORTED; }
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    qmri_free_dict(ctx);
    DictHost& d = ctx->dict;
    d.K = K; d.s = s; d.Q = Q;
    if (s > 16) {
        // wide dictionaries (uncompressed fingerprints, s = T; mrf_dtm_cpu.m:41-50 is T-generic): channel-blocked GEMM, dictw_kernels.hip
        d.wide = 1;
        int st = dictw_pack_dictionary(ctx, D, K, s);
        if (st == QMRI_OK) st = d.pool.alloc(ctx, &d.d_normD, (size_t)K);
        if (st == QMRI_OK) st = d.pool.alloc(ctx, &d.d_lut, (size_t)K * Q);
        if (st != QMRI_OK) { qmri_free_dict(ctx); return st; }
        QMRI_HIP(ctx, hipMemcpy(d.d_normD, normD, (size_t)K * sizeof(float), hipMemcpyHostToDevice));
        QMRI_HIP(ctx, hipMemcpy(d.d_lut, lut, (size_t)K * Q * sizeof(float), hipMemcpyHostToDevice));
        QMRI_HIP(ctx, hipDeviceSynchronize());                    // (blocking copies on the NULL stream; this context's stream is not ordered with it)
        d.ready = true;
        return QMRI_OK;
    }
    d.D_h.assign(D, D + (size_t)K * s); d.normD_h.assign(normD, normD + K);     // host copy for qmri_set_components (api_pv.cpp)
    d.lut_h.assign(lut, lut + (size_t)K * Q);                                   // ... and, with it, for qmri_set_refine (api_refine.cpp)
    d.ntiles = (K + 31) / 32;
    const int npair = (s + 1) / 2;
    // [tile][lane][NPL] with NPL = 4 or 8 floats per lane (its A-fragment value of every channel pair, zero padded): a lane fetches its
    // share of a tile with one or two 16-byte requests (dict_kernels.hip)
    const int npl = (npair <= 4) ? 4 : 8;
    std::vector<float> pack((size_t)d.ntiles * 64 * npl, 0.f);
    for (int t = 0; t < d.ntiles; ++t)
        for (int q = 0; q < npair; ++q)
            for (int lane = 0; lane < 64; ++lane) {
                const int atom = t * 32 + (lane & 31), c = 2 * q + (lane >> 5);
                if (atom < K && c < s) pack[((size_t)t * 64 + lane) * npl + q] = D[(size_t)atom + (size_t)K * c];
            }
    QMRI_TRY(d.pool.alloc(ctx, &d.d_pack, pack.size()));
    QMRI_TRY(d.pool.alloc(ctx, &d.d_normD, (size_t)K));
    QMRI_TRY(d.pool.alloc(ctx, &d.d_lut, (size_t)K * Q));
    QMRI_HIP(ctx, hipMemcpy(d.d_pack, pack.data(), pack.size() * sizeof(float), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(d.d_normD, normD, (size_t)K * sizeof(float), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(d.d_lut, lut, (size_t)K * Q * sizeof(float), hipMemcpyHostToDevice));
    // f16 pieces for the filter: a = g D in (-1, 1) with one power of two g, hi = f16(a), lo = f16(a - hi) (the difference is exact in f32)
    {
        float dmax = 0.f; double r2max = 0.0; bool finite = true;
        for (int a = 0; a < K && finite; ++a) {
            double r2 = 0.0;
            for (int c = 0; c < s; ++c) {
                const float v = D[(size_t)a + (size_t)K * c];
                if (!std::isfinite(v)) { finite = false; break; }
                dmax = std::max(dmax, std::fabs(v)); r2 += (double)v * v;
            }
            r2max = std::max(r2max, r2);
        }
        if (finite && dmax > 1e-30f && dmax < 1e30f) {
            int e = 0; (void)std::frexp(dmax, &e);
            const float g = std::ldexp(1.f, -e);                            // g dmax in [0.5, 1)
            std::vector<_Float16> p16((size_t)d.ntiles * 64 * 16, (_Float16)0.f);
            for (int t = 0; t < d.ntiles; ++t)
                for (int lane = 0; lane < 64; ++lane) {
                    const int atom = t * 32 + (lane & 31);
                    _Float16* hi = &p16[((size_t)t * 128 + lane) * 8], *lo = hi + 64 * 8;     // [tile][hi | lo][lane][8]
                    for (int jj = 0; jj < 8; ++jj) {
                        const int c = 8 * (lane >> 5) + jj;
                        if (atom >= K || c >= s) continue;
                        const float a = D[(size_t)atom + (size_t)K * c] * g;
                        hi[jj] = (_Float16)a; lo[jj] = (_Float16)(a - (float)hi[jj]);
                    }
                }
            QMRI_TRY(d.pool.alloc(ctx, &d.d_pack16, p16.size() * sizeof(_Float16) / sizeof(uint4)));
            QMRI_HIP(ctx, hipMemcpy(d.d_pack16, p16.data(), p16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
            d.marg_coef = (float)(std::ldexp(1.0, -14) * r2max * (double)g * (double)g * 1.001);
        }
    }
    QMRI_HIP(ctx, hipDeviceSynchronize());                        // (blocking copies on the NULL stream; this context's stream is not ordered with it)
    d.ready = true;
    return QMRI_OK;
}

extern "C" int qmri_debug_dict_filter(qmri_ctx* ctx, int on, float margin_scale) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_CHECK_ARG(ctx, margin_scale >= 0.f, "margin_scale must be >= 0");
    ctx->dict.filter_on = on ? 1 : 0;
    ctx->dict.margin_scale = margin_scale;
    return QMRI_OK;
}

extern "C" int qmri_dict_match_xfit_dev(qmri_ctx* ctx, const void* d_X, int Npix, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm, float* d_xfit) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->dict.ready) { qmri_set_error(ctx, "dictionary not set: call qmri_set_dictionary first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, d_X && Npix > 0, "X must not be NULL and Npix > 0");
    return dict_launch(ctx, (const double2*)d_X, Npix, d_qmap, d_pd, d_mt, d_dm, (float2*)d_xfit);
}

extern "C" int qmri_dict_match_dev(qmri_ctx* ctx, const void* d_X, int Npix, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm) {
    return qmri_dict_match_xfit_dev(ctx, d_X, Npix, d_qmap, d_pd, d_mt, d_dm, nullptr);
}

// The host-array form of a match (`who` for its messages): X, and the selector of a grouped match (sel, else NULL), go to the device, the match
// runs there, and the outputs the caller asked for come back.  grp is a grouped match's.
static int dict_match_staged(qmri_ctx* ctx, const char* who, const void* X, int Npix, const double* sel, float* qmap, float* pd, float* mt, int32_t* dm,
                             int32_t* grp, float* xfit) {
    const DictHost& d = ctx->dict;
    const size_t nx = (size_t)Npix * d.s;
    DevBuf<double2> dX; DevBuf<double> dsel; DevBuf<float> dq, dp, dmt; DevBuf<int32_t> ddm, dgrp; DevBuf<float2> dxf;
    auto fail = [&](const char* what) { qmri_set_error(ctx, "%s failed in %s", what, who); return QMRI_ERR_HIP; };
    QMRI_TRY(dX.ensure(ctx, nx));
    if (sel) QMRI_TRY(dsel.ensure(ctx, (size_t)Npix));
    if (qmap) QMRI_TRY(dq.ensure(ctx, (size_t)Npix * d.Q));
    if (pd) QMRI_TRY(dp.ensure(ctx, (size_t)Npix * 2));
    if (mt) QMRI_TRY(dmt.ensure(ctx, (size_t)Npix));
    if (dm) QMRI_TRY(ddm.ensure(ctx, (size_t)Npix));
    if (grp) QMRI_TRY(dgrp.ensure(ctx, (size_t)Npix));
    if (xfit) QMRI_TRY(dxf.ensure(ctx, nx));
    if (hipMemcpyAsync(dX, X, nx * sizeof(double2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("H2D copy");
    if (sel && hipMemcpyAsync(dsel, sel, (size_t)Npix * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("H2D copy");
    if (sel) QMRI_TRY(dictg_launch(ctx, dX, Npix, dsel, dq, dp, dmt, ddm, dgrp, dxf));
    else QMRI_TRY(dict_launch(ctx, dX, Npix, dq, dp, dmt, ddm, dxf));
    if (qmap && hipMemcpyAsync(qmap, dq, (size_t)Npix * d.Q * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail("D2H copy");
    if (pd && hipMemcpyAsync(pd, dp, (size_t)Npix * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail("D2H copy");
    if (mt && hipMemcpyAsync(mt, dmt, (size_t)Npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail("D2H copy");
    if (dm && hipMemcpyAsync(dm, ddm, (size_t)Npix * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail("D2H copy");
    if (grp && hipMemcpyAsync(grp, dgrp, (size_t)Npix * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail("D2H copy");
    if (xfit && hipMemcpyAsync(xfit, dxf, nx * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail("D2H copy");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("synchronize");
    return QMRI_OK;
}

extern "C" int qmri_dict_match_xfit(qmri_ctx* ctx, const void* X, int Npix, float* qmap, float* pd, float* mt, int32_t* dm, float* xfit) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->dict.ready) { qmri_set_error(ctx, "dictionary not set: call qmri_set_dictionary first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, X && Npix > 0, "X must not be NULL and Npix > 0");
    return dict_match_staged(ctx, "qmri_dict_match", X, Npix, nullptr, qmap, pd, mt, dm, nullptr, xfit);
}

extern "C" int qmri_dict_match(qmri_ctx* ctx, const void* X, int Npix, float* qmap, float* pd, float* mt, int32_t* dm) {
    return qmri_dict_match_xfit(ctx, X, Npix, qmap, pd, mt, dm, nullptr);
}

// ---- groups of a dictionary and the grouped match (extension) ----------------------------------------------------------
extern "C" int qmri_set_dictionary_groups(qmri_ctx* ctx, int G, const int32_t* group_ptr, const double* group_val) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    if (G == 0) {                                                       // clears
        QMRI_HIP(ctx, hipSetDevice(ctx->device));
        QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        dictg_free(ctx);
        return QMRI_OK;
    }
    QMRI_CHECK_ARG(ctx, G >= 1 && G <= 256, "1 <= G <= 256 groups (0 clears)");
    QMRI_CHECK_ARG(ctx, group_ptr && group_val, "group_ptr / group_val must not be NULL");
    for (int g = 0; g < G; ++g) {
        QMRI_CHECK_ARG(ctx, group_ptr[g + 1] > group_ptr[g], "group_ptr must be strictly increasing (no empty group)");
        QMRI_CHECK_ARG(ctx, std::isfinite(group_val[g]) && (g == 0 || group_val[g] > group_val[g - 1]), "group_val must be finite and strictly ascending");
    }
    QMRI_CHECK_ARG(ctx, group_ptr[0] == 0, "group_ptr[0] must be 0");
    if (!ctx->dict.ready) { qmri_set_error(ctx, "dictionary not set: call qmri_set_dictionary first"); return QMRI_ERR_STATE; }
    if (ctx->dict.wide) { qmri_set_error(ctx, "groups are supported for dictionaries of s <= 16 channels (got %d)", ctx->dict.s); return QMRI_ERR_UNSUPPORTED; }
    QMRI_CHECK_ARG(ctx, group_ptr[G] == ctx->dict.K, "group_ptr[G] must be K");
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return dictg_set_groups(ctx, G, group_ptr, group_val);
}

static int grouped_ready(qmri_ctx* ctx, const void* X, int Npix, const double* sel) {
    if (!ctx->dict.ready) { qmri_set_error(ctx, "dictionary not set: call qmri_set_dictionary first"); return QMRI_ERR_STATE; }
    if (!ctx->dict.G) { qmri_set_error(ctx, "dictionary groups not set: call qmri_set_dictionary_groups first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, X && sel && Npix > 0, "X / sel must not be NULL and Npix > 0");
    return QMRI_OK;
}

extern "C" int qmri_dict_match_grouped_dev(qmri_ctx* ctx, const void* d_X, int Npix, const double* d_sel, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm,
                                           int32_t* d_grp, float* d_xfit) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(grouped_ready(ctx, d_X, Npix, d_sel));
    return dictg_launch(ctx, (const double2*)d_X, Npix, d_sel, d_qmap, d_pd, d_mt, d_dm, d_grp, (float2*)d_xfit);
}

extern "C" int qmri_dict_match_grouped(qmri_ctx* ctx, const void* X, int Npix, const double* sel, float* qmap, float* pd, float* mt, int32_t* dm, int32_t* grp,
                                       float* xfit) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(grouped_ready(ctx, X, Npix, sel));
    return dict_match_staged(ctx, "qmri_dict_match_grouped", X, Npix, sel, qmap, pd, mt, dm, grp, xfit);
}
