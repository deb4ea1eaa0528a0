// api_llr.cpp -- C ABI of the locally low-rank proximal step (include/qmri.h; kernels: llr_kernels.hip).  An EXTENSION with no
// reference counterpart.  Every refusal is decided here, on the host, before the device is selected; with ctx == NULL the message of the first
// failing check is left in qmri_last_error(NULL), so the argument rules can be exercised on a machine without a GPU.
#include <cmath>
#include <cstdint>
#include "qmri_internal.h"

namespace {
constexpr int LLR_MAX_S = 16, LLR_MAX_SIDE = 16384;

int llr_param_checks(qmri_ctx* ctx, const qmri_llr_params* p) {
    QMRI_CHECK_ARG(ctx, std::isfinite(p->tau) && p->tau >= 0.0, "tau must be finite and >= 0");
    QMRI_CHECK_ARG(ctx, p->block == 0 || p->block == 4 || p->block == 8 || p->block == 16, "block must be 4, 8 or 16 (0: the default 8)");
    for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "reserved must be 0");
    return QMRI_OK;
}

int llr_checks(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* x, const qmri_llr_params* p, int o1, int o2, const void* out) {
    QMRI_CHECK_ARG(ctx, x && p && out, "x / p / out must not be NULL");
    QMRI_CHECK_ARG(ctx, nslices >= 1, "nslices >= 1");
    QMRI_CHECK_ARG(ctx, s >= 1 && s <= LLR_MAX_S, "s must satisfy 1 <= s <= 16");
    QMRI_TRY(llr_param_checks(ctx, p));
    const int b = p->block ? p->block : 8;
    if (N < b || M < b || N > LLR_MAX_SIDE || M > LLR_MAX_SIDE || N % b || M % b) {
        qmri_set_error(ctx, "invalid argument: N and M must be positive multiples of the block side (N = %d, M = %d, block = %d)", N, M, b);
        return QMRI_ERR_INVALID_ARG;
    }
    QMRI_CHECK_ARG(ctx, o1 >= 0 && o1 < b && o2 >= 0 && o2 < b, "the offsets must satisfy 0 <= o1, o2 < block");
    QMRI_CHECK_ARG(ctx, (uint64_t)nslices * (uint64_t)(N / b) * (uint64_t)(M / b) <= 0x7fffffffull, "too many blocks in one call");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

// the launches on device arrays and the read-back of sigma_max; d_x is complex
int llr_run(qmri_ctx* ctx, int N, int M, int s, int nslices, const double2* d_x, bool real, const qmri_llr_params* p, int o1, int o2, double2* d_out,
            double* sigma_max_out) {
    const int b = p->block ? p->block : 8;
    const LlrPlan pl = {N, M, s, b, o1, o2, real ? 1 : 0, p->tau};
    DevBuf<double> bs, sm;
    if (sigma_max_out) {
        QMRI_TRY(bs.ensure(ctx, (size_t)nslices * (N / b) * (M / b)));
        QMRI_TRY(sm.ensure(ctx, (size_t)nslices));
    }
    QMRI_TRY(llr_prox_dev(ctx, pl, nslices, d_x, nullptr, d_out, bs.p, sm.p));
    if (sigma_max_out) QMRI_HIP(ctx, hipMemcpyAsync(sigma_max_out, sm.p, (size_t)nslices * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
}  // namespace

void llr_offsets(int it, int block, int shift, int* o1, int* o2) {
    *o1 = *o2 = 0;
    if (!shift) return;
    const int q = it % (block * block);
    *o1 = q % block;
    *o2 = (q / block + q) % block;
}

extern "C" int qmri_llr_prox_dev(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* d_x, int x_is_complex, const qmri_llr_params* p, int o1,
                                 int o2, void* d_out, double* sigma_max_out) {
    QMRI_TRY(llr_checks(ctx, N, M, s, nslices, d_x, p, o1, o2, d_out));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return llr_run(ctx, N, M, s, nslices, (const double2*)d_x, !x_is_complex, p, o1, o2, (double2*)d_out, sigma_max_out);
}

extern "C" int qmri_llr_prox(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* x, int x_is_complex, const qmri_llr_params* p, int o1, int o2,
                             void* out, double* sigma_max_out) {
    QMRI_TRY(llr_checks(ctx, N, M, s, nslices, x, p, o1, o2, out));
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
    QMRI_TRY(llr_run(ctx, N, M, s, nslices, dx.p, !x_is_complex, p, o1, o2, dx.p, sigma_max_out));    // in place (sigma_max is the input's)
    QMRI_HIP(ctx, hipMemcpyAsync(out, dx.p, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_set_llr(qmri_ctx* ctx, const qmri_llr_params* p) {
    if (p) {
        QMRI_TRY(llr_param_checks(ctx, p));
        QMRI_CHECK_ARG(ctx, p->shift == 0 || p->shift == 1, "shift must be 0 or 1");
    }
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    if (!p) { ctx->llr = LlrState{}; return QMRI_OK; }
    if (ctx->wav.on) {
        qmri_set_error(ctx, "the wavelet regulariser is set: one regulariser at a time, clear it with qmri_set_wavelet(ctx, NULL) first");
        return QMRI_ERR_STATE;
    }
    ctx->llr.on = true;
    ctx->llr.tau = p->tau;
    ctx->llr.block = p->block ? p->block : 8;
    ctx->llr.shift = p->shift;
    return QMRI_OK;
}
