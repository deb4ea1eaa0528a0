// api_xupdate.cpp -- the x-update of a gridded operator: the DIRECT solver's tables, the k-space LSQR driver and qmri_xupdate.
//
// Replaces (reference file:line): the lsqr x-update call site PnP_ADMM.m:102 with afun PnP_ADMM.m:153-171.
#include "qmri_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

// (G_k + r I)^-1 for every sampled k (op_plan.h direct_inverse_tables), once per r
int qmri_prepare_direct(qmri_ctx* ctx, double r) {
    OpHost& o = ctx->op;
    if (o.ginv_r == r) return QMRI_OK;
    const std::vector<double> ginv = direct_inverse_tables(o.V, o.kptr_h, o.ent_h, o.s, o.T, r);
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_ginv, ginv.data(), ginv.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    o.ginv_r = r;
    return QMRI_OK;
}

// LSQR on B slices, iterated in k-space (kslsqr_kernels.hip).  Requires ls.yk / ny2 (dc_launch_sort_y) and ls.pz
// (dc_launch_prepare_z) to be current.  d_x holds x0 on entry and the solution on return; when o.xhat_valid the spectrum of
// x0 is taken from the previous solve instead of being recomputed.  pdiag (or null) receives [B][N] partials of ||y - A x||^2.
// hslot / deferred (round 3): a caller that does not need the iteration count at once passes B pinned LsqrState entries of its own and a flag;
// when the one-launch kernel runs, the call returns WITHOUT waiting (*deferred = true, iters_out / flag_out untouched): the kernel leaves
// iter / done / flag in hslot, to be read after the caller's next synchronisation (state 77 there = the kernel timed out: the caller repeats
// its work with ctx->ks_persist = 0).  The ADMM loop uses this so that the host never waits inside a reconstruction.
// fuse (round 4, nullable): what the ADMM loop has already done in neighbouring launches, or wants done in this solve's last one --
// z_hpass_nblk > 0: o.d_tmp holds the h-pass of z's transform and ls.pz that many partial sums of |z|^2 per slice (k_dual_fwd_h), d_z is not read;
// mm_u / mm: the final h-pass also leaves the partial min / max of real(x + mm_u) per workgroup in mm (k_adj_h; mm_cpx: of both parts).
int qmri_lsqr_run(qmri_ctx* ctx, int B, const double2* d_z, double r, double tol, int maxit, double2* d_x,
                  int32_t* iters_out, int32_t* flag_out, double* pdiag, LsqrState* hslot, bool* deferred, const LsqrFuse* fuse) {
    OpHost& o = ctx->op;
    QMRI_TRY(nufft_check_gridded(ctx, "the k-space LSQR", "the image-domain LSQR of the qmri_*_mc calls applies (internal)"));
    const OpDev op = qmri_opdev(ctx);
    KsDev ks = o.ks;
    ks.sr = std::sqrt(r); ks.tol = tol; ks.maxit = maxit; ks.ii = 0; ks.pdiag = pdiag;
    LsqrState* const hs = hslot ? hslot : o.h_state;
    ks.hst = hs;
    if (deferred) *deferred = false;
    const bool z_fused = fuse && fuse->z_hpass_nblk > 0;
    const double2* const mm_u = fuse ? fuse->mm_u : nullptr;
    double* const mm = fuse ? fuse->mm : nullptr;
    const bool mm_cpx = fuse && fuse->mm_cpx;
    if (z_fused && !o.xhat_valid) { qmri_set_error(ctx, "qmri_lsqr_run: a transformed z needs the spectrum of x (internal)"); return QMRI_ERR_STATE; }
    if (!o.xhat_valid) QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, B, d_x, o.d_tmp, ks.xhat, nullptr));
    if (z_fused) ks.nblk_z = fuse->z_hpass_nblk;
    else QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_FWD_H_ONLY, B, d_z, o.d_tmp, nullptr, nullptr));
    // Round 5: when the one-launch kernel will run, it takes the first Golub-Kahan step (beta0, v = B'u / beta0, d = 0) itself -- k_ks_b<INIT>
    // is not launched, v and d never exist in memory (knob lsqr_fold = 0: the separate launch, same bits)
    if (ctx->ks_persist < 0) ctx->ks_persist = qmri_knob(K_LSQR_PERSIST) ? 1 : 0;
    int per_launch = 0;
    if (ctx->ks_persist > 0 && maxit >= 1) QMRI_TRY(ks_persist_plan(ctx, op, ks, B, &per_launch));
    const bool fold = per_launch > 0 && qmri_knob(K_LSQR_FOLD) != 0;
    QMRI_TRY(ks_launch_init(ctx, op, ks, B, o.d_tmp, !fold));           // w-pass of z (-> ks.zhat) + first Golub-Kahan vectors
    // The predicted number of iterations is launched, then -- speculatively -- the kernels that turn the solution back into
    // an image.  The host waits only for the copy of the LSQR state (an event between the two), so the device keeps working
    // while the host wakes up and enqueues the next stage.  If a slice was not done yet (rare: counts fall from one x-update
    // to the next), two more iterations at a time follow and the final kernels run again from the untouched inputs.
    if (!ctx->ev_state) QMRI_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_state, hipEventDisableTiming));
    // Round 3: all iterations in ONE launch when the grid is resident at once (k_ks_persist: the iteration's state stays on chip, the
    // two sums per iteration are in-kernel hand-offs instead of kernel boundaries); the two-launch iteration otherwise (EPI masks,
    // cut0, slice batches) and after a time-out of the persistent kernel (never seen; the inputs are untouched then).
    bool persisted = false;
    if (per_launch > 0) {
        if (!ctx->d_ks_gran.p) {
            const size_t nb = ks_gran_bytes(ks.G, o.maxB);
            QMRI_TRY(ctx->d_ks_gran.ensure(ctx, nb));
            QMRI_HIP(ctx, hipMemsetAsync(ctx->d_ks_gran, 0, nb, ctx->stream));      // (tag 0 is never used)
        }
        const unsigned tag0 = ctx->ks_tag;
        QMRI_TRY(ks_launch_persist(ctx, op, ks, B, ctx->d_ks_gran, tag0, fold, &persisted));
        if (persisted) {
            ctx->ks_tag += 2u * (unsigned)(maxit + 2);
            QMRI_TRY(ks_launch_final(ctx, op, ks, B, o.d_tmp));
            QMRI_TRY(dc_launch_adj_h(ctx, op, B, o.d_tmp, d_x, mm_u, mm, mm_cpx));
            if (deferred) {                                        // the caller reads hslot after its own synchronisation
                *deferred = true;
                std::swap(o.ks.xhat, o.ks.xhat_out);
                o.xhat_valid = true;
                return QMRI_OK;
            }
            // Not deferred (qmri_xupdate): wait for the stream -- the kernels above are a few tens of microseconds, any HIP error ends the wait,
            // and k_ks_final_w has then overridden the state if a workgroup of the one-launch kernel gave up.  (The ADMM loop never waits here:
            // it reads its pinned slots after its own final synchronisation.)
            QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
            for (int b = 0; b < B; ++b)
                if ((unsigned)__atomic_load_n(&hs[b].pad, __ATOMIC_ACQUIRE) != tag0) {
                    qmri_set_error(ctx, "the one-launch LSQR kernel ended without reporting its state");
                    return QMRI_ERR_HIP;
                }
            bool timed_out = false;
            for (int b = 0; b < B; ++b) timed_out = timed_out || hs[b].flag == 77;
            if (timed_out) {                                       // repeat with the two-launch iteration, from the untouched inputs
                fprintf(stderr, "libqmri: the one-launch LSQR timed out waiting for a partial sum; using the two-launch iteration from now on\n");
                ctx->ks_persist = 0;
                ctx->ks_timeouts += 1;
                persisted = false;
                QMRI_TRY(ks_launch_init(ctx, op, ks, B));
            }
        }
    }
    // (guard: the first Golub-Kahan step was left to a one-launch kernel that then did not run -- the plan is the same in both places, so this
    //  cannot happen; if it ever does, the two-launch iteration must not start from an unset state)
    if (fold && !persisted && !(ctx->ks_persist == 0)) QMRI_TRY(ks_launch_init(ctx, op, ks, B));
    int launched = 0;
    int chunk = std::min(std::max(ctx->lsqr_pred, 1), std::max(maxit, 1));
    bool all_done = persisted;
    // (do ... while: with maxit == 0 the final kernels still run once and return x0 -- the assembled spectrum and the diagnostics' partial
    //  sums must exist whatever the iteration count)
    if (!persisted) do {
        const int nthis = std::min(chunk, maxit - launched);
        for (int k = 0; k < nthis; ++k) {
            ks.ii = launched + k + 1;
            QMRI_TRY(ks_launch_iter(ctx, op, ks, B));
        }
        launched += std::max(nthis, 0);
        // (no copy of the state: k_ks_b writes iter / done / flag of every slice to the pinned host array itself, ks.hst)
        QMRI_HIP(ctx, hipEventRecord(ctx->ev_state, ctx->stream));
        QMRI_TRY(ks_launch_final(ctx, op, ks, B, o.d_tmp));              // reads ks.xhat (x0), writes ks.xhat_out
        QMRI_TRY(dc_launch_adj_h(ctx, op, B, o.d_tmp, d_x, mm_u, mm, mm_cpx));
        QMRI_HIP(ctx, hipEventSynchronize(ctx->ev_state));
        all_done = true;
        for (int b = 0; b < B; ++b) all_done = all_done && hs[b].done;
        chunk = 2;
    } while (launched < maxit && !all_done);
    std::swap(o.ks.xhat, o.ks.xhat_out);                                  // the assembled spectrum is the next solve's xhat0
    o.xhat_valid = true;
    int worst = 0;
    for (int b = 0; b < B; ++b) {
        const int it = hs[b].done ? hs[b].iter : maxit;
        if (iters_out) iters_out[b] = it;
        if (flag_out) flag_out[b] = hs[b].done ? hs[b].flag : 1;
        worst = std::max(worst, it);
        ctx->prof.lsqr_iters += it;
    }
    ctx->lsqr_pred = worst + 1;      // convergence is detected one iteration after the last x update; counts fall from one x-update to the next
    return QMRI_OK;
}

extern "C" int qmri_xupdate(qmri_ctx* ctx, const void* y, const void* z, double r, double tol, int maxit, int solver,
                            void* x, int32_t* iters_out, int32_t* flag_out) {
    if (solver == QMRI_SOLVER_TOEPLITZ) QMRI_TRY(offres_refuse_toeplitz(ctx, "QMRI_SOLVER_TOEPLITZ"));      // (a field map attached: decided on the host)
    REQUIRE_OP(ctx);
    QMRI_CHECK_ARG(ctx, y && z && x && r > 0 && maxit >= 0, "qmri_xupdate arguments");
    OpHost& o = ctx->op;
    if (o.kind == OP_NUFFT) {
        // a trajectory: A^H A is not block-diagonal in k-space, so the k-space LSQR does not apply -- the image-domain LSQR with one unit coil,
        // staged as qmri_xupdate_mc stages it (the same bits as that call with the unit map)
        if (solver != QMRI_SOLVER_LSQR && solver != QMRI_SOLVER_TOEPLITZ) {
            qmri_set_error(ctx, "the DIRECT solver is not available on a trajectory operator (qmri_set_operator_nufft): its closed form needs a gridded "
                                "mask; use QMRI_SOLVER_LSQR");
            return QMRI_ERR_UNSUPPORTED;
        }
        const size_t n = (size_t)o.N * o.M * o.s;
        QMRI_TRY(mc_ensure_staging(ctx, 1, 1));
        McWork& w = o.mc;
        QMRI_HIP(ctx, hipMemcpyAsync(w.sy, y, (size_t)o.m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
        QMRI_HIP(ctx, hipMemcpyAsync(w.sz, z, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
        QMRI_HIP(ctx, hipMemcpyAsync(w.sx, x, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(mc_xupdate_dev(ctx, solver, 1, 1, o.nu.d_ones, w.sy, w.sz, r, tol, maxit, w.sx, iters_out, flag_out));
        QMRI_HIP(ctx, hipMemcpyAsync(x, w.sx, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
        QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return QMRI_OK;
    }
    const OpDev op = qmri_opdev(ctx);
    const size_t n = (size_t)o.N * o.M * o.s;
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_ya, y, (size_t)o.m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_z, z, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_x, x, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    if (solver == QMRI_SOLVER_LSQR) {
        QMRI_TRY(dc_launch_sort_y(ctx, op, o.ls, 1, o.d_ya));
        // ||z||^2 partials: reuse prepare_z with u = 0
        QMRI_HIP(ctx, hipMemsetAsync(o.d_u, 0, n * sizeof(double2), ctx->stream));
        QMRI_TRY(dc_launch_prepare_z(ctx, op, o.ls, 1, o.d_z, o.d_u, o.d_vv));
        o.xhat_valid = false;
        QMRI_TRY(qmri_lsqr_run(ctx, 1, o.d_vv, r, tol, maxit, o.d_x, iters_out, flag_out, nullptr, nullptr, nullptr, nullptr));
    } else if (solver == QMRI_SOLVER_DIRECT) {
        QMRI_TRY(qmri_prepare_direct(ctx, r));
        QMRI_TRY(dc_launch_adj(ctx, op, 1, o.d_ya, o.d_tmp, o.d_xa));
        QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, 1, o.d_xa, o.d_tmp, o.d_chat, nullptr));
        QMRI_TRY(dc_launch_direct(ctx, qmri_opdev(ctx), 1, o.d_z, o.d_chat, r, o.d_tmp, o.d_x));
        if (iters_out) *iters_out = 0;
        if (flag_out) *flag_out = 0;
    } else {
        QMRI_TRY(toep_check_solver(ctx, solver));
        qmri_set_error(ctx, "unknown solver %d", solver);
        return QMRI_ERR_INVALID_ARG;
    }
    QMRI_HIP(ctx, hipMemcpyAsync(x, o.d_x, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return qmri_prof_chain_finish(ctx);
}

// test / A-B hook: 1 = all LSQR iterations in one launch where the grid is resident (default), 0 = the two-launch iteration
extern "C" int qmri_debug_lsqr_persist(qmri_ctx* ctx, int on) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    ctx->ks_persist = (on == 2) ? 2 : (on ? 1 : 0);               // (2: test hook -- one partial sum is withheld, the time-out path must take over)
    if (ctx->d_ks_gran.p && ctx->op.ready) {                         // a fresh start: forget an earlier time-out (the sticky word behind the granules)
        QMRI_HIP(ctx, hipSetDevice(ctx->device));
        QMRI_HIP(ctx, hipMemsetAsync((char*)ctx->d_ks_gran.p + ks_gran_bytes(ctx->op.ks.G, ctx->op.maxB) - 64, 0, 64, ctx->stream));
    }
    return QMRI_OK;
}

// diagnostic: phase stamps of the most recent LSQR launches (see lsqr_kernels.hip); out holds 2*512*16 values
extern "C" int qmri_debug_lsqr_stamps(qmri_ctx* ctx, unsigned long long* out) {
    if (!ctx || !ctx->op.ks.stamps) return QMRI_ERR_STATE;
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    QMRI_HIP(ctx, hipMemcpy(out, ctx->op.ks.stamps, (size_t)2 * 512 * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return QMRI_OK;
}
