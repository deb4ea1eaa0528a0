// api_nufft.cpp -- trajectory operators: qmri_build_spiral_traj and qmri_set_operator_nufft check their arguments, have
// nufft_plan.h build the exact spiral and the host plan of the NUFFT (bins, spreading segments, deapodisation), and move the plan to the device;
// and the refusals of the calls a trajectory cannot serve.  The kernels are in nufft_kernels.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "qmri_internal.h"
#include "fft_codelets.h"

using nuplan::PI;

// The two kernel parameters that the interface documents (include/qmri.h: width 0 is 12; DESIGN.md section 14: beta = 2.30 w), checked against the
// values the code takes from nufft_plan.h: a change there that the documents do not follow does not compile.
namespace stated {
constexpr int NU_WDEF = 12;
constexpr double nu_beta(int w) { return 2.30 * w; }
}  // namespace stated
static_assert(stated::NU_WDEF == ::NU_WDEF && stated::nu_beta(1) == ::nu_beta(1) && stated::nu_beta(NU_WMAX) == ::nu_beta(NU_WMAX), "nufft_plan.h disagrees");

int nufft_check_gridded(qmri_ctx* ctx, const char* what, const char* instead) {
    if (ctx->op.kind != OP_NUFFT) return QMRI_OK;
    qmri_set_error(ctx, "%s is not available on a trajectory operator (qmri_set_operator_nufft): %s", what, instead);
    return QMRI_ERR_UNSUPPORTED;
}

extern "C" int qmri_build_spiral_traj(qmri_ctx* ctx, int N, int S, int T, int32_t* frame_ptr, double* omega, int cap, int* m_out) {
    QMRI_CHECK_ARG(ctx, N > 0 && S > 1 && T > 0 && frame_ptr && (omega || cap == 0) && m_out && cap >= 0, "qmri_build_spiral_traj arguments");
    if ((long)S * T > 0x7fffffffL) { qmri_set_error(ctx, "S * T = %ld samples exceed the int32 index range", (long)S * T); return QMRI_ERR_INVALID_ARG; }
    const long m = nuplan::spiral_traj_build(S, T, frame_ptr, omega, cap);
    *m_out = (int)m;
    if (m > cap) { qmri_set_error(ctx, "omega capacity %d too small, need %ld", cap, m); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

extern "C" int qmri_set_operator_nufft(qmri_ctx* ctx, int N, int M, int s, int T, const double* V, const int32_t* frame_ptr, const double* omega,
                                       int max_batch, const qmri_nufft_params* p) {
    // the argument checks come first and need no context or device (ctx == NULL: their message is qmri_last_error(NULL))
    QMRI_CHECK_ARG(ctx, V && frame_ptr && omega, "V / frame_ptr / omega must not be NULL");
    QMRI_CHECK_ARG(ctx, N > 0 && M > 0 && s > 0 && T > 0 && max_batch > 0, "N, M, s, T, max_batch must be positive");
    if (!dc_size_supported(N) || !dc_size_supported(M)) {
        qmri_set_error(ctx, "grid %d x %d unsupported: the FFT kernels implement N, M in {" QFFT_SIDES_TEXT "}, chosen independently", N, M);
        return QMRI_ERR_UNSUPPORTED;
    }
    if (s > 10 || T > 65535) { qmri_set_error(ctx, "s <= 10 and T <= 65535 required (got s=%d T=%d)", s, T); return QMRI_ERR_UNSUPPORTED; }
    const int w = (p && p->width) ? p->width : NU_WDEF;
    if (p) for (int r : p->reserved) QMRI_CHECK_ARG(ctx, r == 0, "qmri_nufft_params.reserved must be zero");
    if (!nufft_kernel_ok(w)) { qmri_set_error(ctx, "NUFFT kernel width %d unsupported: 2 <= width <= %d (0 = default %d)", w, NU_WMAX, NU_WDEF); return QMRI_ERR_UNSUPPORTED; }
    QMRI_CHECK_ARG(ctx, frame_ptr[0] == 0, "frame_ptr[0] must be 0");
    for (int t = 0; t < T; ++t) QMRI_CHECK_ARG(ctx, frame_ptr[t + 1] >= frame_ptr[t], "frame_ptr must be non-decreasing");
    const int m = frame_ptr[T];
    QMRI_CHECK_ARG(ctx, m > 0, "empty measurement set");
    for (long i = 0; i < 2L * m; ++i)
        if (!(std::isfinite(omega[i]) && std::fabs(omega[i]) <= PI)) {
            qmri_set_error(ctx, "invalid argument: omega[%ld] (sample %ld) = %g is not a finite value in [-pi, pi]", i % 2, i / 2, omega[i]);
            return QMRI_ERR_INVALID_ARG;
        }

    QMRI_CHECK_ARG(ctx, ctx, "ctx must not be NULL");
    // (every check above is host arithmetic on the arguments; the device is touched from here on)
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    qmri_free_operator(ctx);
    OpHost& o = ctx->op;
    NufftHost& h = o.nu;
    o.kind = OP_NUFFT;
    o.N = N; o.M = M; o.s = s; o.T = T; o.m = m; o.maxB = max_batch;
    o.V.assign(V, V + (size_t)T * s);
    o.frame_ptr.assign(frame_ptr, frame_ptr + T + 1);
    h.w = w; h.beta = nu_beta(w);

    // the plan (nufft_plan.h): samples sorted by tile, spreading lists and their segments, deapodisation, ramps and sample phases
    const nuplan::NufftPlan pl = nuplan::nu_plan(N, M, T, frame_ptr, omega, w, std::max(32, qmri_knob(K_NUFFT_SEG)));
    h.nseg = (int)pl.segs.size(); h.nred = (int)pl.reds.size(); h.nslot = pl.nslot;
    std::vector<double> Vt((size_t)T * s);
    for (int t = 0; t < T; ++t)
        for (int c = 0; c < s; ++c) Vt[(size_t)t * s + c] = V[t + (size_t)T * c];
    std::vector<double2> tw((size_t)N + M);
    for (int j = 0; j < N; ++j) { const double a = 2.0 * PI * j / N; tw[j] = make_double2(std::cos(a), -std::sin(a)); }
    for (int j = 0; j < M; ++j) { const double a = 2.0 * PI * j / M; tw[(size_t)N + j] = make_double2(std::cos(a), -std::sin(a)); }

    const size_t n = (size_t)N * M * s, B = (size_t)max_batch;
    QMRI_TRY(o.pool.upload(ctx, &o.d_Vt, Vt.data(), Vt.size()));
    QMRI_TRY(o.pool.upload(ctx, &o.d_tw, tw.data(), tw.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_u, pl.u.data(), pl.u.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_ph, pl.ph.data(), pl.ph.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_t, pl.t.data(), pl.t.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_perm, pl.perm.data(), pl.perm.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_list, pl.list.data(), pl.list.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_seg, pl.segs.data(), pl.segs.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_red, pl.reds.data(), pl.reds.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_dp, pl.dp.data(), pl.dp.size()));
    QMRI_TRY(o.pool.upload(ctx, &h.d_r, (const double2*)pl.ramp.data(), pl.ramp.size() / 2));
    const std::vector<double2> ones((size_t)N * M, make_double2(1.0, 0.0));
    QMRI_TRY(o.pool.upload(ctx, &h.d_ones, ones.data(), ones.size()));
    QMRI_TRY(o.pool.alloc(ctx, &h.d_g, 4 * B * n));
    QMRI_TRY(o.pool.alloc(ctx, &h.d_grid, 4 * B * n));
    QMRI_TRY(o.pool.alloc(ctx, &h.d_part, B * std::max(pl.nslot, 1) * (size_t)s * 256));
    // what the host-array entry points and the image-domain LSQR / ADMM loop use (as qmri_set_operator allocates them)
    LsqrDev& ls = o.ls;
    ls.nblk_z = 256;
    QMRI_TRY(o.pool.alloc(ctx, &o.d_xa, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_xb, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_ya, B * (size_t)m));
    QMRI_TRY(o.pool.alloc(ctx, &ls.pz, B * (size_t)ls.nblk_z));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_x, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_u, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_vv, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_z, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_mm, B * (size_t)ls.nblk_z * 2));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_norm, B * 2));
    QMRI_HIP(ctx, hipDeviceSynchronize());          // (as qmri_set_operator: the blocking copies must have landed before the context's stream reads them)
    o.ready = true;
    return QMRI_OK;
}
