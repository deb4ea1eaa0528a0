// api_admm.cpp -- PnP-ADMM drivers of libqmri.so: the gridded loop (fused or not, LSQR or DIRECT), the multi-coil loop, the NUFFT route through it,
// and the qmri_pnp_admm* / qmri_xupdate_mc* entry points.
//
// Replaces (reference file:line): PnP_ADMM.m:1-148.
#include "qmri_internal.h"

#include <algorithm>
#include <chrono>
#include <cstdio>

struct StageTimer {
    qmri_ctx* ctx;
    bool on, marks;
    int cur = -1;
    explicit StageTimer(qmri_ctx* c) : ctx(c), on(c->prof_level == 1 || c->prof_level == 2), marks(c->prof_level == 3) {
        c->marks_n = 0;
        for (double& v : c->last_call_ms) v = 0.0;
    }
    void start() {
        if (on) (void)hipEventRecord(ctx->ev[0], ctx->stream);
        if (marks) {
            if (ctx->marks_n + 2 > ctx->marks.size()) {
                hipEvent_t a = nullptr, b = nullptr;
                if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { marks = false; return; }
                ctx->marks.push_back(a); ctx->marks.push_back(b); ctx->mark_kind.push_back(0);
            }
            cur = (int)ctx->marks_n;
            (void)hipEventRecord(ctx->marks[cur], ctx->stream);
        }
    }
    void stop(double& acc) {
        if (on) {
            (void)hipEventRecord(ctx->ev[1], ctx->stream);
            (void)hipEventSynchronize(ctx->ev[1]);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
            acc += ms;
            ctx->last_call_ms[kind_of(acc)] += ms;
        }
        if (marks && cur >= 0) {
            (void)hipEventRecord(ctx->marks[cur + 1], ctx->stream);
            ctx->mark_kind[cur / 2] = kind_of(acc);
            ctx->marks_n = (size_t)cur + 2;
            cur = -1;
        }
    }
    int kind_of(const double& acc) const {
        const qmri_profile& p = ctx->prof;
        return (&acc == &p.ms_xupdate) ? 0 : (&acc == &p.ms_denoiser) ? 1 : (&acc == &p.ms_elementwise) ? 2 : 3;
    }
    // after the call's final synchronisation: the marks become stage times (profile and last_call_ms)
    void resolve() {
        if (!marks) return;
        for (size_t i = 0; i + 1 < ctx->marks_n; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ctx->marks[i], ctx->marks[i + 1]) != hipSuccess) continue;
            const int k = ctx->mark_kind[i / 2];
            ctx->last_call_ms[k] += ms;
            (k == 0 ? ctx->prof.ms_xupdate : k == 1 ? ctx->prof.ms_denoiser : k == 2 ? ctx->prof.ms_elementwise : ctx->prof.ms_diag) += ms;
        }
        ctx->marks_n = 0;
    }
};

// The denoiser step's mode (qmri_admm_params.denoiser_type, include/qmri.h) and the network it needs: real TSMIs take s (+1) -> s channels,
// complex TSMIs (QMRI_DENOISER_COMPLEX) take 2s (+1) -> 2s.  Complex mode refuses any other network as a state error,
// and so does real mode a network made for complex TSMIs (the wrong denoiser is set for this call); real mode's other misfits stay argument errors.
static int admm_net_fits(qmri_ctx* ctx, const qmri_admm_params* prm, int* multi_out, bool* cpx_out) {
    const OpHost& o = ctx->op;
    const NetPlan& net = ctx->net;
    QMRI_CHECK_ARG(ctx, prm->denoiser_type >= 0 && prm->denoiser_type <= (QMRI_DENOISER_COMPLEX | QMRI_DENOISER_MULTI_LEVEL),
                   "denoiser_type must be 0 .. 3 (QMRI_DENOISER_MULTI_LEVEL | QMRI_DENOISER_COMPLEX)");
    const int multi = (prm->denoiser_type & QMRI_DENOISER_MULTI_LEVEL) ? 1 : 0;
    const bool cpx = (prm->denoiser_type & QMRI_DENOISER_COMPLEX) != 0;
    const int planes = cpx ? 2 * o.s : o.s, other = cpx ? o.s : 2 * o.s;
    if (net.H != o.N || net.W != o.M || net.desc.in_nc != planes + multi || net.desc.out_nc != planes) {
        const bool other_domain = net.desc.in_nc == other + multi && net.desc.out_nc == other;
        qmri_set_error(ctx, "denoiser (%d x %d, %d -> %d channels) does not fit the operator (%d x %d x %d, %s, %s TSMIs: %d -> %d channels needed)",
                       net.H, net.W, net.desc.in_nc, net.desc.out_nc, o.N, o.M, o.s, multi ? "multi_level" : "single_level",
                       cpx ? "complex" : "real", planes + multi, planes);
        return (cpx || other_domain) ? QMRI_ERR_STATE : QMRI_ERR_INVALID_ARG;
    }
    *multi_out = multi;
    *cpx_out = cpx;
    return QMRI_OK;
}

// What Step 2 needs before a loop starts.  With the LLR regulariser set (qmri_set_llr) no network is involved: denoiser_type
// keeps its range, its multi_level bit is ignored, and the block side must divide the grid of the operator in force.
// The joint wavelet soft-thresholding (qmri_set_wavelet) takes the same place: its size rule (wav_plan.h) must hold on that grid.
static bool admm_regulariser_on(const qmri_ctx* ctx) { return ctx->llr.on || ctx->wav.on; }      // a training-free Step 2: no network is involved
static int admm_step_fits(qmri_ctx* ctx, const qmri_admm_params* prm, int* multi_out, bool* cpx_out) {
    if (!admm_regulariser_on(ctx)) return admm_net_fits(ctx, prm, multi_out, cpx_out);
    const OpHost& o = ctx->op;
    QMRI_CHECK_ARG(ctx, prm->denoiser_type >= 0 && prm->denoiser_type <= (QMRI_DENOISER_COMPLEX | QMRI_DENOISER_MULTI_LEVEL),
                   "denoiser_type must be 0 .. 3 (QMRI_DENOISER_MULTI_LEVEL | QMRI_DENOISER_COMPLEX)");
    if (ctx->wav.on) {
        if (!wav::sizes_ok(o.N, o.M, ctx->wav.levels, wav::taps(ctx->wav.filter)) || o.s > wav::MAX_S) {
            qmri_set_error(ctx, "invalid argument: the wavelet regulariser (%d levels, %d taps, at most 16 channels) does not fit the operator (%d x %d x %d): "
                                "2^levels must divide both sides and the last level's input must be at least the filter length",
                           ctx->wav.levels, wav::taps(ctx->wav.filter), o.N, o.M, o.s);
            return QMRI_ERR_INVALID_ARG;
        }
    } else if (o.N % ctx->llr.block || o.M % ctx->llr.block || o.s > 16) {
        qmri_set_error(ctx, "invalid argument: the LLR regulariser (block side %d, at most 16 channels) does not fit the operator (%d x %d x %d): the "
                            "block side must divide both sides", ctx->llr.block, o.N, o.M, o.s);
        return QMRI_ERR_INVALID_ARG;
    }
    *multi_out = 0;
    *cpx_out = (prm->denoiser_type & QMRI_DENOISER_COMPLEX) != 0;
    return QMRI_OK;
}

// The start of both loops (PnP_ADMM.m:86-90) on the context's v / u / z: v = x, uold = 0 and, with `z_now`, z = v - uold.  The gridded loop passes
// z_now = false and makes z itself inside iteration 0, under the x-update's stage timer and never when iters = 0.
static int admm_start(qmri_ctx* ctx, int B, const double2* d_x, bool z_now) {
    OpHost& o = ctx->op;
    const size_t nb = (size_t)B * o.N * o.M * o.s * sizeof(double2);
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_vv, d_x, nb, hipMemcpyDeviceToDevice, ctx->stream));                    // v = x
    QMRI_HIP(ctx, hipMemsetAsync(o.d_u, 0, nb, ctx->stream));                                                // uold = 0
    if (z_now) QMRI_TRY(dc_launch_prepare_z(ctx, qmri_opdev(ctx), o.ls, B, o.d_vv, o.d_u, o.d_z));           // z = v - uold
    return QMRI_OK;
}

// What the denoiser step of either loop needs to know; tm (null from the multi-coil loop, which records no stage times) is the gridded loop's stage timer
struct DenoiserStep { int B; const qmri_admm_params* prm; int multi; bool cpx; const double2* d_x; StageTimer* tm; };

// Step 2 (PnP_ADMM.m:115-138): v = real(x+uold) -> [0,1] -> net   (complex TSMIs: cat(3, real, imag) of x+uold).  mm_ready: the
// partial min / max (mm_nblk per slice) came with the solve's last h-pass.  The range guard of this forward is read at the next synchronisation point:
// k_act_check has written it to the pinned host words; only the gridded loop (copy_range_flag) on a network with more layers than words copies the device flag.
static int admm_to_net(qmri_ctx* ctx, const DenoiserStep& d, int mm_nblk, bool mm_ready, bool copy_range_flag) {
    OpHost& o = ctx->op;
    NetPlan& net = ctx->net;
    const size_t plane = (size_t)o.N * o.M;
    if (d.tm) d.tm->start();
    QMRI_TRY(ew_launch_minmax_normalise(ctx, d.B, plane * o.s, (int)plane, o.N, o.s, d.multi, d.prm->noise_std, d.d_x, o.d_u, o.d_mm, o.d_norm, mm_nblk, net.ten[NT_IN32],
                                        mm_ready, d.cpx));
    if (d.tm) { d.tm->stop(ctx->prof.ms_elementwise); d.tm->start(); }
    QMRI_TRY(net_forward(ctx, d.B));
    if (copy_range_flag && net.sp6 == 2 && (int)net.layers.size() + 1 > net.h_range_words)
        QMRI_HIP(ctx, hipMemcpyAsync(net.h_range_flag, net.d_range_flag, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    if (d.tm) d.tm->stop(ctx->prof.ms_denoiser);
    return QMRI_OK;
}

// The denoiser step as three launches (both loops; the gridded one's fused form folds the third into the next x-update): step 2, then step 3
// (PnP_ADMM.m:138,144): v = I*range + min ; uold = uold + x - v ; z = v - uold with the partials of ||z||^2
// With the LLR regulariser set, two launches: v = LLR_tau(x + uold) at the offsets of iteration `it`, then step 3 on v.
// With the wavelet regulariser set, v = Wav_tau(x + uold) in its 2 L + 1 launches, then the same step 3.
static int admm_denoiser_step(qmri_ctx* ctx, const DenoiserStep& d, bool copy_range_flag, int it) {
    OpHost& o = ctx->op;
    NetPlan& net = ctx->net;
    const size_t plane = (size_t)o.N * o.M;
    if (ctx->wav.on) {
        const WavState& w = ctx->wav;
        WavPlan pl = {o.N, o.M, o.s, w.levels, w.filter, w.joint, 0, 0, d.cpx ? 0 : 1, w.tau};
        wav::offsets(it, 1 << w.levels, w.shift, &pl.o1, &pl.o2);
        if (d.tm) d.tm->start();
        QMRI_TRY(wav_prox_dev(ctx, pl, d.B, d.d_x, o.d_u, o.d_vv, nullptr));
        if (d.tm) { d.tm->stop(ctx->prof.ms_denoiser); d.tm->start(); }
        QMRI_TRY(llr_dual_dev(ctx, d.B, plane * o.s, d.d_x, o.d_vv, o.d_u, o.d_z, o.ls.pz, o.ls.nblk_z));
        if (d.tm) d.tm->stop(ctx->prof.ms_elementwise);
        return QMRI_OK;
    }
    if (ctx->llr.on) {
        LlrPlan pl = {o.N, o.M, o.s, ctx->llr.block, 0, 0, d.cpx ? 0 : 1, ctx->llr.tau};
        llr_offsets(it, pl.block, ctx->llr.shift, &pl.o1, &pl.o2);
        if (d.tm) d.tm->start();
        QMRI_TRY(llr_prox_dev(ctx, pl, d.B, d.d_x, o.d_u, o.d_vv, nullptr, nullptr));
        if (d.tm) { d.tm->stop(ctx->prof.ms_denoiser); d.tm->start(); }
        QMRI_TRY(llr_dual_dev(ctx, d.B, plane * o.s, d.d_x, o.d_vv, o.d_u, o.d_z, o.ls.pz, o.ls.nblk_z));
        if (d.tm) d.tm->stop(ctx->prof.ms_elementwise);
        return QMRI_OK;
    }
    QMRI_TRY(admm_to_net(ctx, d, o.ls.nblk_z, false, copy_range_flag));
    if (d.tm) d.tm->start();
    QMRI_TRY(ew_launch_unnormalise_dual(ctx, d.B, plane * o.s, (int)plane, o.N, net.ten[NT_OUT32], net.ten[NT_IN32], net.desc.residual_noise, o.d_norm, d.d_x, o.d_u,
                                        nullptr /* v itself is never read again: z = v - u goes to the next x-update */, o.d_z, o.ls.pz, o.ls.nblk_z, o.s, d.cpx));
    if (d.tm) d.tm->stop(ctx->prof.ms_elementwise);
    return QMRI_OK;
}

// ---------------------------------------------------------------------------------------------------
// Multi-coil extension (no reference counterpart: README.md:63 -- parity unpinned; mc_kernels.hip): the x-update and the PnP-ADMM loop of
// PnP_ADMM.m:76-146 with A replaced by the SENSE operator.  B slices, each with its own maps ([B][ncoil][N*M]), y ([B][ncoil][m]) and x ([B][n]);
// the single-slice entry points are B = 1 calls on the maps of qmri_set_coils.  The batched calls neither read nor change those maps.
// ---------------------------------------------------------------------------------------------------
static int mc_require(qmri_ctx* ctx, int nslices, int ncoil, const void* maps, const void* y) {
    const OpHost& o = ctx->op;
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, nslices >= 1 && ncoil >= 1 && ncoil <= 1024, "nslices >= 1 and 1 <= ncoil <= 1024");
    QMRI_CHECK_ARG(ctx, maps && y, "maps / y_mc must not be NULL");
    return QMRI_OK;
}
int mc_admm_check(qmri_ctx* ctx, const qmri_admm_params* prm) {
    const NetPlan& net = ctx->net;
    if (!net.ready && !admm_regulariser_on(ctx)) { qmri_set_error(ctx, "denoiser not set: call qmri_set_denoiser first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, prm, "params must not be NULL");
    QMRI_TRY(toep_check_solver(ctx, prm->solver));            // (QMRI_SOLVER_TOEPLITZ: a trajectory operator only)
    QMRI_CHECK_ARG(ctx, prm->iters >= 0 && prm->gamma > 0 && prm->cg_maxit >= 0 && (prm->solver == QMRI_SOLVER_LSQR || prm->solver == QMRI_SOLVER_TOEPLITZ),
                   "iters >= 0, gamma > 0, cg_maxit >= 0, LSQR solver required");
    int multi = 0;
    bool cpx = false;
    return admm_step_fits(ctx, prm, &multi, &cpx);
}

// PnP_ADMM.m:76-146 for B <= max_batch slice images, all on the device (returns x as :148).  sv.start makes the start image (:84 or the caller's x0)
// and sv.solve is the x-update (:102) with its sv.nsolve LSQR counts: B of them in the multi-coil loop, one per group in the simultaneous
// multi-slice loop (api_sms.cpp).  When the network's range guard trips, the loop starts again from the inputs with no second allocation.
int mc_admm_loop(qmri_ctx* ctx, int B, const qmri_admm_params* prm, const AdmmSolve& sv, double2* d_x, int32_t* li_out, int li_stride) {
    OpHost& o = ctx->op;
    const bool reg = admm_regulariser_on(ctx);                                                      // (no network: nothing can trip, nothing is waited for)
    const int multi = (!reg && (prm->denoiser_type & QMRI_DENOISER_MULTI_LEVEL)) ? 1 : 0;   // (checked by mc_admm_check)
    const bool cpx = (prm->denoiser_type & QMRI_DENOISER_COMPLEX) != 0;
    std::vector<int32_t> li((size_t)sv.nsolve);
    for (int attempt = 0;; ++attempt) {
        QMRI_TRY(sv.start(d_x));
        QMRI_TRY(admm_start(ctx, B, d_x, true));                  // v = x, uold = 0, z = v - uold
        bool again = false;
        for (int it = 0; it < prm->iters; ++it) {
            QMRI_TRY(sv.solve(o.d_z, d_x, li.data()));                                                                                              // :102
            if (li_out) for (int b = 0; b < sv.nsolve; ++b) li_out[(size_t)b * li_stride + it] = li[b];
            QMRI_TRY(admm_denoiser_step(ctx, {B, prm, multi, cpx, d_x, nullptr}, false, it));                                                       // :115-144
            if (reg) continue;
            QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
            QMRI_TRY(net_range_tripped(ctx, again));              // (f16 range / hand-off guards: the network is re-packed or the form switched; start again)
            if (again) break;
        }
        if (!again) break;
        ctx->admm_repeats += 1;
        if (attempt >= 2) { qmri_set_error(ctx, "the denoiser's range guard tripped three times in a row in the multi-coil PnP-ADMM loop"); return QMRI_ERR_HIP; }
    }
    o.xhat_valid = false;
    return QMRI_OK;
}

// ... with the SENSE operator: d_x0 NULL: x = A_mc' y as :84 (d_x must not alias d_x0)
static int mc_admm_group(qmri_ctx* ctx, int B, int ncoil, const double2* d_maps, const double2* d_y, const qmri_admm_params* prm, const double2* d_x0,
                         double2* d_x, int32_t* li_out, int li_stride) {
    const size_t n = (size_t)ctx->op.N * ctx->op.M * ctx->op.s;
    AdmmSolve sv;
    sv.nsolve = B;
    sv.start = [&](double2* x) -> int {
        if (!d_x0) return mc_adjoint_batch_dev(ctx, B, ncoil, d_maps, d_y, x);
        QMRI_HIP(ctx, hipMemcpyAsync(x, d_x0, (size_t)B * n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
        return QMRI_OK;
    };
    sv.solve = [&](const double2* z, double2* x, int32_t* li) {
        return mc_xupdate_dev(ctx, prm->solver, B, ncoil, d_maps, d_y, z, prm->gamma, prm->cg_tol, prm->cg_maxit, x, li, nullptr);
    };
    return mc_admm_loop(ctx, B, prm, sv, d_x, li_out, li_stride);
}

// One staged multi-coil run (the host-array entry points and the NUFFT route): the caller's operands go to the context's staging buffers (McWork), run(w)
// works on those, and sx comes back as x.  Counts follow from B and ncoil; a null operand is not staged.  sync: the call ends synchronised (a stack's last run).
struct McStaged {
    const void* maps;                   // -> sm [B][ncoil][N*M] (null: the run uses the maps of qmri_set_coils / the unit coil)
    const void* y;                      // -> sy [B][ncoil][m]
    const void* to_sz;                  // -> sz [B][n]: z of an x-update, x0 of a reconstruction
    const void* to_sx; bool zero_sx;    // -> sx [B][n]: x0 of an x-update, which starts from zeros without one
    void* x_out;                        // <- sx [B][n]
    bool on_device = false;             // the caller's arrays are device arrays (the NUFFT route), else host arrays
};
template <typename Run> static int mc_staged(qmri_ctx* ctx, int B, int ncoil, const McStaged& sg, bool sync, Run run) {
    OpHost& o = ctx->op;
    const size_t plane = (size_t)o.N * o.M, nx = (size_t)B * plane * o.s * sizeof(double2), img = (size_t)B * ncoil;
    const hipMemcpyKind in = sg.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, out = sg.on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    QMRI_TRY(mc_ensure_staging(ctx, B, ncoil));
    McWork& w = o.mc;
    if (sg.maps) QMRI_HIP(ctx, hipMemcpyAsync(w.sm, sg.maps, img * plane * sizeof(double2), in, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(w.sy, sg.y, img * o.m * sizeof(double2), in, ctx->stream));
    if (sg.to_sz) QMRI_HIP(ctx, hipMemcpyAsync(w.sz, sg.to_sz, nx, in, ctx->stream));
    if (sg.to_sx) QMRI_HIP(ctx, hipMemcpyAsync(w.sx, sg.to_sx, nx, in, ctx->stream));
    else if (sg.zero_sx) QMRI_HIP(ctx, hipMemsetAsync(w.sx, 0, nx, ctx->stream));
    QMRI_TRY(run(w));
    QMRI_HIP(ctx, hipMemcpyAsync(sg.x_out, w.sx, nx, out, ctx->stream));
    if (sync) QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// A trajectory operator (qmri_set_operator_nufft): one slice through the multi-coil loop with one unit coil -- the k-space LSQR and the fused
// launches around it need a gridded mask.  The same bits as qmri_pnp_admm_mc with that coil.
static int pnp_admm_nufft(qmri_ctx* ctx, int nslices, const void* d_y, const qmri_admm_params* prm, const void* d_x0, void* d_x_out,
                          double* diag_out, int32_t* lsqr_iters_out) {
    if (nslices != 1) {
        qmri_set_error(ctx, "PnP-ADMM of %d slices in one call is not available on a trajectory operator (qmri_set_operator_nufft): reconstruct them "
                            "one at a time, or as a stack with qmri_pnp_admm_mc_batch and one unit coil per slice", nslices);
        return QMRI_ERR_UNSUPPORTED;
    }
    if (prm && prm->solver != QMRI_SOLVER_LSQR && prm->solver != QMRI_SOLVER_TOEPLITZ) {
        qmri_set_error(ctx, "the DIRECT solver is not available on a trajectory operator (qmri_set_operator_nufft): its closed form needs a gridded "
                            "mask; use QMRI_SOLVER_LSQR");
        return QMRI_ERR_UNSUPPORTED;
    }
    if (prm && prm->want_diag && diag_out) {
        qmri_set_error(ctx, "the per-iteration diagnostics are not available on a trajectory operator (qmri_set_operator_nufft): set want_diag = 0 "
                            "and evaluate the result with qmri_forward");
        return QMRI_ERR_UNSUPPORTED;
    }
    QMRI_TRY(mc_admm_check(ctx, prm));
    QMRI_CHECK_ARG(ctx, d_y && d_x_out && d_x_out != d_x0, "y / x_out must not be NULL, x_out must not alias x0");
    // staged as qmri_pnp_admm_mc stages it (the caller's y may be o.d_ya, which the multi-coil transforms use as their scratch)
    return mc_staged(ctx, 1, 1, {nullptr, d_y, d_x0, nullptr, false, d_x_out, true}, true, [&](McWork& w) {
        return mc_admm_group(ctx, 1, 1, ctx->op.nu.d_ones, w.sy, prm, d_x0 ? w.sz : nullptr, w.sx, lsqr_iters_out, prm->iters);
    });
}

// One attempt at the reconstruction.  *repeat: the attempt does not count -- the one-launch LSQR timed out or a guard of the network tripped, and the
// context has been changed so that the cause cannot fire again (two-launch iteration / bf16 scheme / one launch per layer): qmri_pnp_admm_dev runs it once more.
static int pnp_admm_dev_impl(qmri_ctx* ctx, int nslices, const void* d_y, const qmri_admm_params* prm, const void* d_x0,
                             const void* d_gt, void* d_x_out, double* diag_out, int32_t* lsqr_iters_out, bool* repeat) {
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->op.ready && ctx->op.kind == OP_NUFFT) return pnp_admm_nufft(ctx, nslices, d_y, prm, d_x0, d_x_out, diag_out, lsqr_iters_out);
    OpHost& o = ctx->op;
    NetPlan& net = ctx->net;
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    const bool reg = admm_regulariser_on(ctx);                          // Step 2 is a training-free prox (LLR or wavelet): no network, so no fused launches, no range guard and no repeat
    if (!net.ready && !reg) { qmri_set_error(ctx, "denoiser not set: call qmri_set_denoiser first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, d_y && prm && d_x_out, "y / params / x_out must not be NULL");
    const int B = nslices;
    QMRI_CHECK_ARG(ctx, B >= 1 && B <= o.maxB && (reg || B <= net.maxB), "nslices exceeds max_batch of the operator or the denoiser");
    QMRI_CHECK_ARG(ctx, prm->iters >= 0 && prm->gamma > 0 && prm->cg_maxit >= 0, "iters >= 0, gamma > 0, cg_maxit >= 0 required");
    int multi = 0;
    bool cpx = false;
    QMRI_TRY(admm_step_fits(ctx, prm, &multi, &cpx));
    const OpDev op = qmri_opdev(ctx);
    const size_t plane = (size_t)o.N * o.M, n = plane * o.s, nb = (size_t)B * n * sizeof(double2);
    const double2* y = (const double2*)d_y;
    StageTimer tm(ctx);

    QMRI_TRY(dc_launch_sort_y(ctx, op, o.ls, B, y));
    if (d_x0) QMRI_HIP(ctx, hipMemcpyAsync(o.d_x, d_x0, nb, hipMemcpyDeviceToDevice, ctx->stream));        // x = param.X0
    else QMRI_TRY(dc_launch_adj(ctx, op, B, y, o.d_tmp, o.d_x));                    // F.adjoint(Y)
    QMRI_TRY(admm_start(ctx, B, o.d_x, false));            // v = x, uold = 0; z = v - uold in iteration 0
    if (prm->solver == QMRI_SOLVER_DIRECT) {
        QMRI_TRY(qmri_prepare_direct(ctx, prm->gamma));
        const double2* aty = o.d_x;
        if (d_x0) { QMRI_TRY(dc_launch_adj(ctx, op, B, y, o.d_tmp, o.d_xa)); aty = o.d_xa; }
        QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, B, aty, o.d_tmp, o.d_chat, nullptr));
    } else if (prm->solver != QMRI_SOLVER_LSQR) {
        QMRI_TRY(toep_check_solver(ctx, prm->solver));
        qmri_set_error(ctx, "unknown solver %d", prm->solver);
        return QMRI_ERR_INVALID_ARG;
    }
    if (prm->want_diag && diag_out) QMRI_TRY(o.d_diag.ensure(ctx, (size_t)B * std::max(prm->iters, 1) * 2));
    std::vector<int32_t> it_b(B);
    o.xhat_valid = false;                                  // x was just set: its spectrum is not known yet
    const bool diag = prm->want_diag && diag_out;
    bool range_trip = false;
    // LSQR state per (ADMM iteration, slice) in pinned memory: with the one-launch LSQR kernel the host does not wait inside the loop at all
    // (qmri_lsqr_run, "deferred") -- the kernels of all iterations are queued back to back and the counts are read after the final
    // synchronisation; an event or a host round trip per x-update left the GPU idle for ~6 us each
    std::vector<char> deferred_it((size_t)std::max(prm->iters, 1), 0);
    if (prm->solver == QMRI_SOLVER_LSQR) QMRI_TRY(o.h_ring.ensure(ctx, std::max<size_t>((size_t)prm->iters * B, 128)));
    // Round 4: the small launches around the network are folded into their neighbours (LSQR solver; knob fuse_ew = 0 restores the separate kernels
    // for A/Bs): un-normalise + dual update + z + the h-pass of z's transform + the forward pass's |output| report = ONE launch (k_dual_fwd_h);
    // the w-pass of z rides in the solve's first kernel (k_ks_init_a<FWDW>); the min / max of real(x + u) come out of the solve's last h-pass.
    const bool fused = qmri_knob(K_FUSE_EW) != 0 && prm->solver == QMRI_SOLVER_LSQR && !reg;
    const int hb = dc_hpass_blocks(op);
    bool z_in_tmp = false;                                 // o.d_tmp holds the h-pass of z (and ls.pz hb partial sums per slice)
    struct DeferGuard { NetPlan& n; ~DeferGuard() { n.act_defer = false; n.act_pending_valid = false; } } defer_guard{net};
    net.act_defer = fused;
    const DenoiserStep step = {B, prm, multi, cpx, o.d_x, &tm};
    for (int it = 0; it < prm->iters; ++it) {
        // Step 1 (PnP_ADMM.m:102): x = argmin ||y - Ax||^2 + r ||x - (v - uold)||^2
        tm.start();
        if (it == 0) QMRI_TRY(dc_launch_prepare_z(ctx, op, o.ls, B, o.d_vv, o.d_u, o.d_z));   // later: fused into the dual update
        if (prm->solver == QMRI_SOLVER_LSQR) {
            bool deferred = false;
            LsqrFuse lf;
            if (fused) { lf.z_hpass_nblk = z_in_tmp ? hb : 0; lf.mm_u = o.d_u; lf.mm = o.d_mm; lf.mm_cpx = cpx; }
            QMRI_TRY(qmri_lsqr_run(ctx, B, o.d_z, prm->gamma, prm->cg_tol, prm->cg_maxit, o.d_x, it_b.data(), nullptr,
                                   diag ? o.d_pd : nullptr,            // (the data-fidelity partials come with the solve)
                                   o.h_ring + (size_t)it * B, &deferred, &lf));
            deferred_it[it] = deferred ? 1 : 0;
            if (!deferred && lsqr_iters_out) for (int b = 0; b < B; ++b) lsqr_iters_out[(size_t)b * prm->iters + it] = it_b[b];
            // The range guard of earlier forwards is on the host (pinned words written by k_act_check).  After a wait inside qmri_lsqr_run (the
            // two-launch iteration) it is current up to the previous iteration; without one it is whatever has arrived.  A tripped guard ends
            // this attempt at once instead of after all iterations.
            if (it > 0 && !reg && net.sp6 == 2 && host_range_tripped(net)) { range_trip = true; tm.stop(ctx->prof.ms_xupdate); break; }
        } else {
            QMRI_TRY(dc_launch_direct(ctx, op, B, o.d_z, o.d_chat, prm->gamma, o.d_tmp, o.d_x));
            if (lsqr_iters_out) for (int b = 0; b < B; ++b) lsqr_iters_out[(size_t)b * prm->iters + it] = 0;
        }
        tm.stop(ctx->prof.ms_xupdate);
        if (prm->want_diag && diag_out) {                                                                    // PnP_ADMM.m:106-109
            tm.start();
            if (prm->solver != QMRI_SOLVER_LSQR) QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_DIAG, B, o.d_x, o.d_tmp, nullptr, o.d_pd));
            QMRI_TRY(ew_launch_diag(ctx, op, o.ls, B, o.d_x, (const double2*)d_gt, o.d_pd, o.d_diag, prm->iters, it));
            tm.stop(ctx->prof.ms_diag);
        }
        // Steps 2 and 3 (PnP_ADMM.m:115-144): the denoiser on v = real(x+uold), then uold = uold + x - v
        if (!fused) QMRI_TRY(admm_denoiser_step(ctx, step, !reg, it));
        else {
            QMRI_TRY(admm_to_net(ctx, step, hb, true, true));
            tm.start();
            const PTensor &out32 = net.ten[NT_OUT32], &in32 = net.ten[NT_IN32];
            const DualArgs da = {out32.base1(), in32.base1(), out32.hp, (int)out32.plane(), out32.batch_stride(), in32.batch_stride(),
                                 net.desc.residual_noise, o.d_norm, o.d_x, o.d_u, o.ls.pz, cpx ? 1 : 0};
            ActCheckArgs ac{};
            if (net.act_pending_valid) { ac = net.act_pending; net.act_pending_valid = false; }
            QMRI_TRY(dc_launch_dual_fwd_h(ctx, op, B, da, ac, o.d_tmp));
            z_in_tmp = true;
            tm.stop(ctx->prof.ms_elementwise);
        }
        ctx->prof.admm_iters += 1;
    }
    if (!range_trip) {
        QMRI_HIP(ctx, hipMemcpyAsync(d_x_out, o.d_x, nb, hipMemcpyDeviceToDevice, ctx->stream));             // returns x, not v
    }
    if (prm->want_diag && diag_out && prm->iters > 0 && !range_trip)
        QMRI_HIP(ctx, hipMemcpyAsync(diag_out, o.d_diag, (size_t)B * prm->iters * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tm.resolve();                                                  // (profile level 3: the stage marks of this call)
    QMRI_TRY(qmri_prof_chain_finish(ctx));                         // (profile level 2: the LSQR launches since the last forward pass)
    if (prm->solver == QMRI_SOLVER_LSQR && !range_trip) {          // LSQR counts of the iterations whose state was deferred; a timed-out one-launch kernel
        bool timed_out = false;
        for (int it = 0; it < prm->iters; ++it) {
            if (!deferred_it[it]) continue;
            for (int b = 0; b < B; ++b) {
                const LsqrState& h = o.h_ring[(size_t)it * B + b];
                if (h.flag == 77) timed_out = true;
                const int n_it = h.done ? h.iter : prm->cg_maxit;
                if (lsqr_iters_out) lsqr_iters_out[(size_t)b * prm->iters + it] = n_it;
                ctx->prof.lsqr_iters += n_it;
            }
        }
        if (timed_out) {                                           // (never seen) everything after it is garbage: once more with the two-launch iteration
            fprintf(stderr, "libqmri: the one-launch LSQR timed out waiting for a partial sum; repeating the reconstruction with the two-launch iteration\n");
            ctx->ks_persist = 0;
            ctx->ks_timeouts += 1;
            *repeat = true;
            return QMRI_OK;
        }
    }
    // f16 range guard: the network now runs on the bf16 scheme; the inputs are untouched (d_x_out must not alias d_x0), run again
    if (prm->iters > 0 && !reg) QMRI_TRY(net_range_tripped(ctx, *repeat));
    return QMRI_OK;
}

// (the wall clock of the call, repeats included, for qmri_get_health; no cap on the repeats: each cause can fire once per state of the context)
extern "C" int qmri_pnp_admm_dev(qmri_ctx* ctx, int nslices, const void* d_y, const qmri_admm_params* prm, const void* d_x0,
                                 const void* d_gt, void* d_x_out, double* diag_out, int32_t* lsqr_iters_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    const auto prof_at_entry = ctx->prof;                  // (an attempt that is repeated must not stay in the profile: the repeated run is the one that counts)
    int st = QMRI_OK;
    for (bool repeat = true; st == QMRI_OK && repeat;) {
        repeat = false;
        st = pnp_admm_dev_impl(ctx, nslices, d_y, prm, d_x0, d_gt, d_x_out, diag_out, lsqr_iters_out, &repeat);
        if (st == QMRI_OK && repeat) { ctx->prof = prof_at_entry; ctx->admm_repeats += 1; }
    }
    ctx->last_call_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

extern "C" int qmri_xupdate_mc_batch(qmri_ctx* ctx, int nslices, int ncoil, const void* maps, const void* y_mc, const void* z, double r, double tol, int maxit,
                                     const void* x0, void* x_out, int32_t* iters_out, int32_t* flags_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(mc_require(ctx, nslices, ncoil, maps, y_mc));
    QMRI_CHECK_ARG(ctx, z && x_out && r > 0 && maxit >= 0, "z / x_out must not be NULL, r > 0, maxit >= 0");
    return mc_staged(ctx, nslices, ncoil, {maps, y_mc, z, x0, true, x_out}, true, [&](McWork& w) {
        return qmri_lsqr_mc_batch_dev(ctx, nslices, ncoil, w.sm, w.sy, w.sz, r, tol, maxit, w.sx, iters_out, flags_out);
    });
}

extern "C" int qmri_pnp_admm_mc_dev(qmri_ctx* ctx, int nslices, int ncoil, const void* d_maps, const void* d_y, const qmri_admm_params* prm,
                                    const void* d_x0, void* d_x_out, int32_t* lsqr_iters_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(mc_require(ctx, nslices, ncoil, d_maps, d_y));
    QMRI_TRY(mc_admm_check(ctx, prm));
    QMRI_CHECK_ARG(ctx, d_x_out && d_x_out != d_x0, "x_out must not be NULL and must not alias x0");
    QMRI_CHECK_ARG(ctx, nslices <= ctx->op.maxB && (admm_regulariser_on(ctx) || nslices <= ctx->net.maxB), "nslices exceeds max_batch of the operator or the denoiser");
    QMRI_TRY(mc_admm_group(ctx, nslices, ncoil, (const double2*)d_maps, (const double2*)d_y, prm, (const double2*)d_x0, (double2*)d_x_out,
                           lsqr_iters_out, prm->iters));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_pnp_admm_mc_batch(qmri_ctx* ctx, int nslices, int slices_per_launch, int ncoil, const void* maps, const void* y_mc,
                                      const qmri_admm_params* prm, const void* x0, void* x_out, int32_t* lsqr_iters_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(mc_require(ctx, nslices, ncoil, maps, y_mc));
    QMRI_TRY(mc_admm_check(ctx, prm));
    QMRI_CHECK_ARG(ctx, x_out && slices_per_launch >= 1, "x_out must not be NULL, slices_per_launch >= 1");
    OpHost& o = ctx->op;
    const int spl = std::min(slices_per_launch, nslices);
    QMRI_CHECK_ARG(ctx, spl <= o.maxB && (admm_regulariser_on(ctx) || spl <= ctx->net.maxB), "slices_per_launch exceeds max_batch of the operator or the denoiser");
    const size_t plane = (size_t)o.N * o.M, n = plane * o.s;
    for (int b0 = 0; b0 < nslices; b0 += spl) {            // (the first run is the largest: the staging is sized once)
        const int B = std::min(spl, nslices - b0);
        const size_t img0 = (size_t)b0 * ncoil;
        const McStaged sg = {(const double2*)maps + img0 * plane, (const double2*)y_mc + img0 * o.m, x0 ? (const double2*)x0 + (size_t)b0 * n : nullptr,
                             nullptr, false, (double2*)x_out + (size_t)b0 * n};
        QMRI_TRY(mc_staged(ctx, B, ncoil, sg, b0 + spl >= nslices, [&](McWork& w) {
            return mc_admm_group(ctx, B, ncoil, w.sm, w.sy, prm, x0 ? w.sz : nullptr, w.sx,
                                 lsqr_iters_out ? lsqr_iters_out + (size_t)b0 * prm->iters : nullptr, prm->iters);
        }));
    }
    return QMRI_OK;
}

extern "C" int qmri_xupdate_mc(qmri_ctx* ctx, const void* y_mc, const void* z, double r, double tol, int maxit, const void* x0, void* x_out,
                               int32_t* iters_out, int32_t* flag_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    OpHost& o = ctx->op;
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    if (!o.ncoil) { qmri_set_error(ctx, "no coil maps set: call qmri_set_coils first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, y_mc && z && x_out && r > 0 && maxit >= 0, "y / z / x_out must not be NULL, r > 0, maxit >= 0");
    return mc_staged(ctx, 1, o.ncoil, {nullptr, y_mc, z, x0, true, x_out}, true, [&](McWork& w) {
        return qmri_lsqr_mc_batch_dev(ctx, 1, o.ncoil, o.d_coils, w.sy, w.sz, r, tol, maxit, w.sx, iters_out, flag_out);
    });
}

extern "C" int qmri_pnp_admm_mc(qmri_ctx* ctx, const void* y_mc, const qmri_admm_params* prm, const void* x0, void* x_out, int32_t* lsqr_iters_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    OpHost& o = ctx->op;
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    if (!o.ncoil) { qmri_set_error(ctx, "no coil maps set: call qmri_set_coils first"); return QMRI_ERR_STATE; }
    QMRI_TRY(mc_admm_check(ctx, prm));
    QMRI_CHECK_ARG(ctx, y_mc && x_out, "y / params / x_out must not be NULL");
    return mc_staged(ctx, 1, o.ncoil, {nullptr, y_mc, x0, nullptr, false, x_out}, true, [&](McWork& w) {      // returns x, not v
        return mc_admm_group(ctx, 1, o.ncoil, o.d_coils, w.sy, prm, x0 ? w.sz : nullptr, w.sx, lsqr_iters_out, prm->iters);
    });
}

extern "C" int qmri_pnp_admm(qmri_ctx* ctx, const void* y, const qmri_admm_params* p, const void* x0, const void* gt,
                             void* x_out, double* diag_out, int32_t* lsqr_iters_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    OpHost& o = ctx->op;
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, y && p && x_out, "y / params / x_out must not be NULL");
    const size_t n = (size_t)o.N * o.M * o.s;
    DevBuf<double2> d_gt;
    double2* d_x0 = nullptr;
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_ya, y, (size_t)o.m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    if (x0) { d_x0 = o.d_xb; QMRI_HIP(ctx, hipMemcpyAsync(d_x0, x0, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream)); }
    if (gt) {
        QMRI_TRY(d_gt.ensure(ctx, n));
        if (hipMemcpyAsync(d_gt, gt, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            qmri_set_error(ctx, "copy of gt_tsmi to the device failed");
            return QMRI_ERR_HIP;
        }
    }
    QMRI_TRY(qmri_pnp_admm_dev(ctx, 1, o.d_ya, p, d_x0, d_gt, o.d_xa, diag_out, lsqr_iters_out));
    if (hipMemcpyAsync(x_out, o.d_xa, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        qmri_set_error(ctx, "copy of the result to the host failed");
        return QMRI_ERR_HIP;
    }
    return QMRI_OK;
}

// A slice stack from host buffers through ONE context (the MATLAB route for `PnP_ADMM_hip(Y, param)` with a measurement matrix): the slices
// advance slices_per_launch at a time through qmri_pnp_admm_dev.  Plain and synchronous -- copy in, reconstruct, copy out per launch;
// qmri_recon_batch is the pipelined, multi-device form of the same work.
extern "C" int qmri_pnp_admm_batch(qmri_ctx* ctx, int nslices, int slices_per_launch, const void* y, const qmri_admm_params* p, const void* x0,
                                   const void* gt, void* x_out, double* diag_out, int32_t* lsqr_iters_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    OpHost& o = ctx->op;
    if (!o.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    if (!ctx->net.ready && !admm_regulariser_on(ctx)) { qmri_set_error(ctx, "denoiser not set: call qmri_set_denoiser first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, y && p && x_out && nslices >= 1 && slices_per_launch >= 1, "y / params / x_out must not be NULL, nslices and slices_per_launch >= 1");
    if (std::min(slices_per_launch, nslices) > 1)
        QMRI_TRY(nufft_check_gridded(ctx, "qmri_pnp_admm_batch with more than one slice per launch",
                                     "use slices_per_launch = 1, or qmri_pnp_admm_mc_batch with one unit coil per slice"));
    const int spl = std::min(slices_per_launch, nslices);
    QMRI_CHECK_ARG(ctx, spl <= o.maxB && (admm_regulariser_on(ctx) || spl <= ctx->net.maxB), "slices_per_launch exceeds max_batch of the operator or the denoiser");
    const size_t n = (size_t)o.N * o.M * o.s, m = (size_t)o.m, it = (size_t)std::max(p->iters, 0);
    DevBuf<double2> dY, dX, dX0, dGT;
    auto fail = [&](const char* what) { qmri_set_error(ctx, "%s failed in qmri_pnp_admm_batch", what); return QMRI_ERR_HIP; };
    QMRI_TRY(dY.ensure(ctx, spl * m));
    QMRI_TRY(dX.ensure(ctx, spl * n));
    if (x0) QMRI_TRY(dX0.ensure(ctx, spl * n));
    if (gt) QMRI_TRY(dGT.ensure(ctx, spl * n));
    for (int s0 = 0; s0 < nslices; s0 += spl) {
        const size_t cnt = (size_t)std::min(spl, nslices - s0);
        if (hipMemcpyAsync(dY, (const double2*)y + (size_t)s0 * m, cnt * m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("H2D copy");
        if (x0 && hipMemcpyAsync(dX0, (const double2*)x0 + (size_t)s0 * n, cnt * n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("H2D copy");
        if (gt && hipMemcpyAsync(dGT, (const double2*)gt + (size_t)s0 * n, cnt * n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("H2D copy");
        QMRI_TRY(qmri_pnp_admm_dev(ctx, (int)cnt, dY, p, dX0, dGT, dX, diag_out ? diag_out + (size_t)s0 * it * 2 : nullptr,
                                   lsqr_iters_out ? lsqr_iters_out + (size_t)s0 * it : nullptr));
        if (hipMemcpyAsync((double2*)x_out + (size_t)s0 * n, dX, cnt * n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("D2H copy");
    }
    return QMRI_OK;
}
