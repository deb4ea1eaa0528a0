// api_wav.cpp -- C ABI of the joint wavelet soft-thresholding step (include/qmri.h; kernels: wav_kernels.hip; geometry: wav_plan.h; DESIGN.md
// section 29).  An EXTENSION with no reference counterpart.  Every refusal is decided here, on the host, before the device is selected; with
// ctx == NULL the message of the first failing check is left in qmri_last_error(NULL), so the argument rules can be exercised on a machine without a GPU.
#include <cmath>
#include <cstdint>
#include "qmri_internal.h"

namespace {
int wav_param_checks(qmri_ctx* ctx, const qmri_wavelet_params* p) {
    QMRI_CHECK_ARG(ctx, std::isfinite(p->tau) && p->tau >= 0.0, "tau must be finite and >= 0");
    QMRI_CHECK_ARG(ctx, p->levels >= 0 && p->levels <= wav::MAX_LEVELS, "levels must be 1 .. 4 (0: the default 3)");
    QMRI_CHECK_ARG(ctx, wav::filter_known(p->filter), "filter must be QMRI_WAVELET_HAAR (0) or QMRI_WAVELET_DB2 (1)");
    QMRI_CHECK_ARG(ctx, p->joint == 0 || p->joint == 1, "joint must be 0 or 1");
    for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "reserved must be 0");
    return QMRI_OK;
}

int wav_checks(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* x, const qmri_wavelet_params* p, int o1, int o2, const void* out) {
    QMRI_CHECK_ARG(ctx, x && p && out, "x / p / out must not be NULL");
    QMRI_CHECK_ARG(ctx, nslices >= 1, "nslices >= 1");
    QMRI_CHECK_ARG(ctx, s >= 1 && s <= wav::MAX_S, "s must satisfy 1 <= s <= 16");
    QMRI_TRY(wav_param_checks(ctx, p));
    const int L = wav::levels_or_default(p->levels), T = wav::taps(p->filter), P = 1 << L;
    if (!wav::sizes_ok(N, M, L, T)) {
        qmri_set_error(ctx, "invalid argument: N and M must be multiples of 2^levels with N / 2^(levels-1) and M / 2^(levels-1) at least the filter "
                            "length (N = %d, M = %d, levels = %d, %d taps)", N, M, L, T);
        return QMRI_ERR_INVALID_ARG;
    }
    QMRI_CHECK_ARG(ctx, o1 >= 0 && o1 < P && o2 >= 0 && o2 < P, "the offsets must satisfy 0 <= o1, o2 < 2^levels");
    QMRI_CHECK_ARG(ctx, (uint64_t)nslices * (uint64_t)s * (uint64_t)wav::tiles(N) * (uint64_t)wav::tiles(M) <= 0x7fffffffull &&
                            (uint64_t)nslices * (uint64_t)wav::shrink_groups_per_slice(N, M) <= 0x7fffffffull, "too many tiles in one call");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

// the launches on device arrays and the read-back of cmax; d_x is complex
int wav_run(qmri_ctx* ctx, int N, int M, int s, int nslices, const double2* d_x, bool real, const qmri_wavelet_params* p, int o1, int o2, double2* d_out,
            double* cmax_out) {
    const WavPlan pl = {N, M, s, wav::levels_or_default(p->levels), p->filter, p->joint, o1, o2, real ? 1 : 0, p->tau};
    if (cmax_out) QMRI_TRY(ctx->wav_cmax.ensure(ctx, (size_t)nslices));
    QMRI_TRY(wav_prox_dev(ctx, pl, nslices, d_x, nullptr, d_out, cmax_out ? ctx->wav_cmax.p : nullptr));
    if (cmax_out) QMRI_HIP(ctx, hipMemcpyAsync(cmax_out, ctx->wav_cmax.p, (size_t)nslices * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_wavelet_prox_dev(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* d_x, int x_is_complex, const qmri_wavelet_params* p,
                                     int o1, int o2, void* d_out, double* cmax_out) {
    QMRI_TRY(wav_checks(ctx, N, M, s, nslices, d_x, p, o1, o2, d_out));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return wav_run(ctx, N, M, s, nslices, (const double2*)d_x, !x_is_complex, p, o1, o2, (double2*)d_out, cmax_out);
}

extern "C" int qmri_wavelet_prox(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* x, int x_is_complex, const qmri_wavelet_params* p, int o1,
                                 int o2, void* out, double* cmax_out) {
    QMRI_TRY(wav_checks(ctx, N, M, s, nslices, x, p, o1, o2, out));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)nslices * N * M * s;
    DevBuf<double2> dx;
    DevBuf<double> dr;
    QMRI_TRY(dx.ensure(ctx, n));
    if (x_is_complex) QMRI_HIP(ctx, hipMemcpyAsync(dx.p, x, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    else {
        QMRI_TRY(dr.ensure(ctx, n));
        QMRI_HIP(ctx, hipMemcpyAsync(dr.p, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(ew_launch_real_to_complex(ctx, n, dr.p, dx.p));
    }
    QMRI_TRY(wav_run(ctx, N, M, s, nslices, dx.p, !x_is_complex, p, o1, o2, dx.p, cmax_out));    // in place (cmax is the input's)
    QMRI_HIP(ctx, hipMemcpyAsync(out, dx.p, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_set_wavelet(qmri_ctx* ctx, const qmri_wavelet_params* p) {
    if (p) {
        QMRI_TRY(wav_param_checks(ctx, p));
        QMRI_CHECK_ARG(ctx, p->shift == 0 || p->shift == 1, "shift must be 0 or 1");
    }
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    if (!p) { ctx->wav = WavState{}; return QMRI_OK; }
    if (ctx->llr.on) {
        qmri_set_error(ctx, "the LLR regulariser is set: one regulariser at a time, clear it with qmri_set_llr(ctx, NULL) first");
        return QMRI_ERR_STATE;
    }
    ctx->wav.on = true;
    ctx->wav.tau = p->tau;
    ctx->wav.levels = wav::levels_or_default(p->levels);
    ctx->wav.filter = p->filter;
    ctx->wav.joint = p->joint;
    ctx->wav.shift = p->shift;
    return QMRI_OK;
}
