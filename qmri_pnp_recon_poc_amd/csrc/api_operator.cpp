// api_operator.cpp -- the gridded forward operator of libqmri.so: mask entry points, qmri_set_operator, forward / adjoint and the coil maps.
// What is decided or computed on the host -- masks, the k-sorted sample list, the LSQR work units -- is op_plan.h; this file validates, calls it and
// moves the results to the device.
//
// Replaces (reference file:line): struct F main_recon_tsmis_FFT.m:228-229; setup_subsampling_spiralgrided.m:1-43; setup_subsampling_epi.m:1-36.
#include "qmri_internal.h"
#include "fft_codelets.h"

#include <algorithm>
#include <cmath>

// ---------------------------------------------------------------------------------------------------
// mask builders (op_plan.h mask_build_spiral / mask_build_epi)
// ---------------------------------------------------------------------------------------------------
extern "C" int qmri_build_spiral(qmri_ctx* ctx, int N, int S, int T, int32_t* frame_ptr, int32_t* kidx, int cap, int* m_out) {
    QMRI_CHECK_ARG(ctx, N > 0 && S > 1 && T > 0 && frame_ptr && (kidx || cap == 0) && m_out, "qmri_build_spiral arguments");
    const long m = mask_build_spiral(N, S, T, frame_ptr, kidx, cap);
    *m_out = (int)m;
    if (m > cap) { qmri_set_error(ctx, "kidx capacity %d too small, need %ld", cap, m); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

extern "C" int qmri_build_epi(qmri_ctx* ctx, int N, int M, double percentage, int T, int32_t* frame_ptr, int32_t* kidx,
                              int cap, int* m_out) {
    QMRI_CHECK_ARG(ctx, N > 0 && M > 0 && T > 0 && percentage > 0 && frame_ptr && (kidx || cap == 0) && m_out,
                   "qmri_build_epi arguments");
    const long m = mask_build_epi(N, M, percentage, T, frame_ptr, kidx, cap);
    *m_out = (int)m;
    if (m > cap) { qmri_set_error(ctx, "kidx capacity %d too small, need %ld", cap, m); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

// ---------------------------------------------------------------------------------------------------
// operator
// ---------------------------------------------------------------------------------------------------
OpDev qmri_opdev(const qmri_ctx* ctx) {
    const OpHost& o = ctx->op;
    OpDev d;
    d.N = o.N; d.M = o.M; d.s = o.s; d.T = o.T; d.m = o.m;
    d.Vt = o.d_Vt; d.ent = o.d_ent; d.perm = o.d_perm; d.kptr = o.d_kptr; d.tw_h = o.d_tw; d.tw_w = o.d_tw + o.N;
    d.kslot = o.d_kslot; d.ginv = o.d_ginv;
    return d;
}

void qmri_free_operator(qmri_ctx* ctx) {
    ctx->d_ks_gran.reset(); ctx->ks_persist_cap = -1;    // (sized for this operator's work units)
    ctx->op = OpHost();
}

// the workspaces of a planned operator (o.ks.G, ks.ns set): staging, the LSQR's vectors on the sampled k and its partial sums, the ADMM state
static int op_alloc_workspaces(qmri_ctx* ctx, OpHost& o) {
    const int N = o.N, M = o.M, s = o.s, m = o.m;
    LsqrDev& ls = o.ls;
    KsDev& ks = o.ks;
    const size_t n = (size_t)N * M * s, B = (size_t)o.maxB;
    ls.nblk_z = 256;
    // per-slice partial sums of |z|^2 (ls.pz) and partial min / max (d_mm): nblk_z from the stand-alone kernels, or one per h-pass workgroup
    // when k_dual_fwd_h / k_adj_h produce them (dc_hpass_blocks: s*M/L, 320 at 256 x 256 where the h-pass takes 8 lines per workgroup)
    OpDev dims{};
    dims.N = N; dims.M = M; dims.s = s;
    const size_t npart = (size_t)std::max(ls.nblk_z, dc_hpass_blocks(dims));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_tmp, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_xa, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_xb, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_ya, B * (size_t)m));
    QMRI_TRY(o.pool.alloc(ctx, &ls.st, B));
    QMRI_TRY(o.pool.alloc(ctx, &ls.pz, B * npart));
    QMRI_TRY(o.pool.alloc(ctx, &ls.py, B * (size_t)DC_SORT_BLOCKS));
    for (int par = 0; par < 2; ++par) {
        QMRI_TRY(o.pool.alloc(ctx, &ks.pu[par], B * 2 * ks.G));
        QMRI_TRY(o.pool.alloc(ctx, &ks.pv[par], B * ks.G));
    }
    QMRI_TRY(o.pool.alloc(ctx, &ks.pinit, B * 2 * N));
    QMRI_TRY(o.pool.alloc(ctx, &ks.pR, B * N));
    QMRI_TRY(o.pool.alloc(ctx, &ks.cx, B * ks.ns * s));
    QMRI_TRY(o.pool.alloc(ctx, &ks.cv, B * ks.ns * s));
    QMRI_TRY(o.pool.alloc(ctx, &ks.cd, B * ks.ns * s));
    QMRI_TRY(o.pool.alloc(ctx, &ks.cub, B * ks.ns * s));
    QMRI_TRY(o.pool.alloc(ctx, &ks.ut, B * (size_t)m));
    QMRI_TRY(o.pool.alloc(ctx, &ks.xhat, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &ks.zhat, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &ks.xhat_out, B * n));
    ks.stamps = nullptr;
    if (qmri_knob(K_LSQR_STAMPS) > 0) { QMRI_TRY(o.pool.alloc(ctx, &ks.stamps, (size_t)2 * 512 * 16)); QMRI_HIP(ctx, hipMemset(ks.stamps, 0, 2 * 512 * 16 * 8)); }
    QMRI_TRY(o.pool.alloc(ctx, &ls.yk, B * (size_t)m));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_x, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_u, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_vv, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_z, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_chat, B * n));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_mm, B * npart * 2));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_norm, B * 2));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_pd, B * ((size_t)N + 2 * ls.nblk_z)));
    QMRI_HIP(ctx, hipMemset(ls.st, 0, B * sizeof(LsqrState)));
    QMRI_TRY(o.h_state.ensure(ctx, B));
    ks.hst = nullptr; ks.st = ls.st; ks.pz = ls.pz; ks.nblk_z = ls.nblk_z; ks.yk = ls.yk; ks.pdiag = nullptr;
    o.xhat_valid = false;
    o.ginv_r = -1.0;
    return QMRI_OK;
}

extern "C" int qmri_set_operator(qmri_ctx* ctx, int N, int M, int s, int T, const double* V, const int32_t* frame_ptr,
                                 const int32_t* kidx, int max_batch) {
    // ---- 1. validate
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_CHECK_ARG(ctx, V && frame_ptr && kidx, "V / frame_ptr / kidx must not be NULL");
    QMRI_CHECK_ARG(ctx, N > 0 && M > 0 && s > 0 && T > 0 && max_batch > 0, "N, M, s, T, max_batch must be positive");
    if (!dc_size_supported(N) || !dc_size_supported(M)) {
        qmri_set_error(ctx, "grid %d x %d unsupported: the FFT kernels implement N, M in {" QFFT_SIDES_TEXT "}, chosen independently", N, M);
        return QMRI_ERR_UNSUPPORTED;
    }
    if (s > 10 || T > 65535 || M > 65535) { qmri_set_error(ctx, "s <= 10 and T, M <= 65535 required (got s=%d T=%d)", s, T); return QMRI_ERR_UNSUPPORTED; }
    QMRI_CHECK_ARG(ctx, frame_ptr[0] == 0, "frame_ptr[0] must be 0");
    const int m = frame_ptr[T];
    QMRI_CHECK_ARG(ctx, m > 0, "empty measurement set");
    for (int t = 0; t < T; ++t) QMRI_CHECK_ARG(ctx, frame_ptr[t + 1] >= frame_ptr[t], "frame_ptr must be non-decreasing");
    for (int i = 0; i < m; ++i) QMRI_CHECK_ARG(ctx, kidx[i] >= 0 && kidx[i] < N * M, "kidx out of range");

    // ---- 2. wait for the stream, free the old operator
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    qmri_free_operator(ctx);
    OpHost& o = ctx->op;
    o.N = N; o.M = M; o.s = s; o.T = T; o.m = m; o.maxB = max_batch;
    o.V.assign(V, V + (size_t)T * s);
    o.frame_ptr.assign(frame_ptr, frame_ptr + T + 1);
    o.kidx.assign(kidx, kidx + m);

    // ---- 3. sort the samples by k location
    KSorted sorted = op_sort_samples(N, M, T, frame_ptr, kidx);
    const std::vector<int32_t> sptr = ks_slot_ptr(sorted);
    const std::vector<int32_t> kslot = std::move(sorted.kslot);
    o.kptr_h = std::move(sorted.kptr_h); o.ent_h = std::move(sorted.ent_h); o.perm_h = std::move(sorted.perm_h); o.nsampled = sorted.nsampled;

    // ---- 4. plan the work units of the k-space LSQR (op_plan.h ks_plan_units).  Whether V fits the LDS of each unit shape's kernels is asked for
    // all four shapes up front: host-only attribute queries, once per qmri_set_operator.  (ks_lds_fits also raises the dynamic-LDS limit of the
    // kernels it asks about, so a few instantiations that are never launched get it too; ks_attrs sets the same value on the ones that are
    // launched before their first launch, so no launch differs.)
    KsPlanIn pin;
    pin.m = m; pin.ns = o.nsampled; pin.s = s; pin.T = T; pin.max_batch = max_batch;
    pin.sptr = sptr.data(); pin.ent = o.ent_h.data();
    pin.one_launch = ctx->ks_persist != 0 && (ctx->ks_persist > 0 || qmri_knob(K_LSQR_PERSIST));
    pin.ncu = ctx->ncu;
    const int vcap = ((T * s + 10 + 15) / 16) * 16;      // (= KsPlan::vcap)
    for (int c = 0; c < KS_NCAPS; ++c) QMRI_TRY(ks_lds_fits(ctx, N, s, M, vcap, c, &pin.lds_fits[c]));
    const KsPlan plan = ks_plan_units(pin);

    // ---- 5. a refused operator leaves nothing allocated
    if (plan.status == KS_PLAN_BUSY_K) {
        qmri_set_error(ctx, "a k location is sampled %d times; at most %d are supported%s", plan.n, plan.tried,
                       plan.tried < KS_CAPS[2].ecap ? " with several slices per launch and the two-launch LSQR iteration (one slice per launch: 2560)" : "");
        return QMRI_ERR_UNSUPPORTED;
    }
    if (plan.status == KS_PLAN_V_TOO_LARGE) {
        qmri_set_error(ctx, "V (T=%d x s=%d) does not fit the on-chip budget of the LSQR kernels", T, s);
        return QMRI_ERR_UNSUPPORTED;
    }

    // ---- 6. upload the tables
    std::vector<double> Vt((size_t)T * s);
    for (int t = 0; t < T; ++t)
        for (int c = 0; c < s; ++c) Vt[(size_t)t * s + c] = V[t + (size_t)T * c];
    std::vector<double2> tw((size_t)N + M);           // the h plan's twiddles, then the w plan's (OpDev::tw_h, tw_w)
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < N; ++j) { const double a = 2.0 * pi * j / N; tw[j] = make_double2(std::cos(a), -std::sin(a)); }
    for (int j = 0; j < M; ++j) { const double a = 2.0 * pi * j / M; tw[(size_t)N + j] = make_double2(std::cos(a), -std::sin(a)); }
    QMRI_TRY(o.pool.upload(ctx, &o.d_Vt, Vt.data(), Vt.size()));
    QMRI_TRY(o.pool.upload(ctx, &o.d_ent, o.ent_h.data(), o.ent_h.size()));
    QMRI_TRY(o.pool.upload(ctx, &o.d_perm, o.perm_h.data(), o.perm_h.size()));
    QMRI_TRY(o.pool.upload(ctx, &o.d_kptr, o.kptr_h.data(), o.kptr_h.size()));
    QMRI_TRY(o.pool.upload(ctx, &o.d_tw, tw.data(), tw.size()));
    QMRI_TRY(o.pool.upload(ctx, &o.d_kslot, kslot.data(), kslot.size()));
    QMRI_TRY(o.pool.alloc(ctx, &o.d_ginv, (size_t)o.nsampled * s * s));       // (filled by qmri_prepare_direct)
    KsDev& ks = o.ks;
    ks.ns = o.nsampled; ks.G = plan.G; ks.caps = plan.caps; ks.vcap = plan.vcap; ks.b0 = 0;
    QMRI_TRY(o.pool.upload(ctx, &ks.sgrp, plan.sgrp.data(), plan.sgrp.size()));
    QMRI_TRY(o.pool.upload(ctx, &ks.es, plan.es.data(), plan.es.size()));
    QMRI_TRY(o.pool.upload(ctx, &ks.grp, plan.grp.data(), plan.grp.size()));
    QMRI_TRY(o.pool.upload(ctx, &ks.unit, plan.units.data(), plan.units.size()));
    ctx->ks_lds_attr[0] = ctx->ks_lds_attr[1] = false;

    // ---- 7. allocate the workspaces
    QMRI_TRY(op_alloc_workspaces(ctx, o));
    // ---- 8. synchronise the device once
    // Round 6: every table above went to the device by blocking copies on the NULL stream, and the kernels that read them run on this context's
    // NON-BLOCKING stream, which is not ordered with it.  hipMemcpy returns once the host buffer has been consumed; beside another process on the
    // device the transfer itself was seen to land AFTER kernels of a later call had started (tools/probe_under_contention.py: a set-up probe reading
    // weights that had not arrived).  One device-wide synchronisation per plan closes that for every later launch.
    QMRI_HIP(ctx, hipDeviceSynchronize());
    o.ready = true;
    return QMRI_OK;
}

extern "C" int qmri_operator_m(const qmri_ctx* ctx, int* m_out) {
    if (!ctx || !m_out) return QMRI_ERR_INVALID_ARG;
    if (!ctx->op.ready) return QMRI_ERR_STATE;
    *m_out = ctx->op.m;
    return QMRI_OK;
}

extern "C" int qmri_forward_dev(qmri_ctx* ctx, const void* d_x, void* d_y, int batch) {
    REQUIRE_OP(ctx);
    QMRI_CHECK_ARG(ctx, d_x && d_y && batch >= 1 && batch <= ctx->op.maxB, "qmri_forward_dev arguments / batch > max_batch");
    if (ctx->op.kind == OP_NUFFT) return nufft_launch_fwd(ctx, batch, (const double2*)d_x, (double2*)d_y);
    return dc_launch_fwd(ctx, qmri_opdev(ctx), ctx->op.ls, DC_PLAIN, batch, (const double2*)d_x, ctx->op.d_tmp,
                         (double2*)d_y, nullptr);
}

extern "C" int qmri_adjoint_dev(qmri_ctx* ctx, const void* d_y, void* d_x, int batch) {
    REQUIRE_OP(ctx);
    QMRI_CHECK_ARG(ctx, d_x && d_y && batch >= 1 && batch <= ctx->op.maxB, "qmri_adjoint_dev arguments / batch > max_batch");
    if (ctx->op.kind == OP_NUFFT) return nufft_launch_adj(ctx, batch, (const double2*)d_y, (double2*)d_x);
    return dc_launch_adj(ctx, qmri_opdev(ctx), batch, (const double2*)d_y, ctx->op.d_tmp, (double2*)d_x);
}

extern "C" int qmri_forward(qmri_ctx* ctx, const void* x, int x_is_complex, void* y) {
    REQUIRE_OP(ctx);
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    if (x_is_complex) {
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_xa, x, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    } else {
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_xb, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(ew_launch_real_to_complex(ctx, n, (const double*)o.d_xb, o.d_xa));
    }
    QMRI_TRY(qmri_forward_dev(ctx, o.d_xa, o.d_ya, 1));
    QMRI_HIP(ctx, hipMemcpyAsync(y, o.d_ya, (size_t)o.m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_adjoint(qmri_ctx* ctx, const void* y, void* x) {
    REQUIRE_OP(ctx);
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s;
    QMRI_HIP(ctx, hipMemcpyAsync(o.d_ya, y, (size_t)o.m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(qmri_adjoint_dev(ctx, o.d_ya, o.d_xa, 1));
    QMRI_HIP(ctx, hipMemcpyAsync(x, o.d_xa, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// ---------------------------------------------------------------------------------------------------
// Multi-coil extension (BASELINE.json configs[4]: "complex-valued multi-coil forward op").  NO counterpart in the reference -- it simulates a
// single coil (README.md:63) -- so there is nothing to be a drop-in for and nothing that pins it: parity unpinned, checked by adjointness,
// closed forms and a restatement in the oracle (oracle.py Operator.forward_mc / adjoint_mc).  A_mc x = [A (C_1 .* x); ...; A (C_nc .* x)] with A the
// single-coil operator of qmri_set_operator and C_j the sensitivity maps; A_mc^H y = sum_j conj(C_j) .* A^H y_j.  The coils of a call go through
// the batched transforms max_batch at a time.
// ---------------------------------------------------------------------------------------------------
extern "C" int qmri_set_coils(qmri_ctx* ctx, int ncoil, const void* maps) {
    REQUIRE_OP(ctx);
    OpHost& o = ctx->op;
    QMRI_CHECK_ARG(ctx, ncoil >= 0 && ncoil <= 1024 && (ncoil == 0 || maps), "0 <= ncoil <= 1024, maps must not be NULL");
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    o.d_coils.reset();
    o.ncoil = 0;
    if (ncoil == 0) return QMRI_OK;
    const size_t count = (size_t)ncoil * o.N * o.M;
    QMRI_TRY(o.d_coils.ensure(ctx, count));
    QMRI_HIP(ctx, hipMemcpy(o.d_coils, maps, count * sizeof(double2), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipDeviceSynchronize());                        // (as in qmri_set_operator: the copy must have landed before this context's stream reads it)
    o.ncoil = ncoil;
    return QMRI_OK;
}

extern "C" int qmri_forward_mc(qmri_ctx* ctx, const void* x, int x_is_complex, void* y) {
    REQUIRE_OP(ctx);
    OpHost& o = ctx->op;
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    if (!o.ncoil) { qmri_set_error(ctx, "no coil maps set: call qmri_set_coils first"); return QMRI_ERR_STATE; }
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    if (x_is_complex) {
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_xa, x, n * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    } else {
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_xb, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(ew_launch_real_to_complex(ctx, n, (const double*)o.d_xb, o.d_xa));
    }
    for (int j0 = 0; j0 < o.ncoil; j0 += o.maxB) {
        const int cnt = std::min(o.maxB, o.ncoil - j0);
        QMRI_TRY(ew_launch_coil_mul(ctx, n, plane, cnt, o.d_xa, o.d_coils + (size_t)j0 * plane, o.d_x));          // (o.d_x: [max_batch][n], free outside a reconstruction)
        if (o.kind == OP_NUFFT) QMRI_TRY(nufft_launch_fwd(ctx, cnt, o.d_x, o.d_ya));
        else QMRI_TRY(dc_launch_fwd(ctx, qmri_opdev(ctx), o.ls, DC_PLAIN, cnt, o.d_x, o.d_tmp, o.d_ya, nullptr));
        QMRI_HIP(ctx, hipMemcpyAsync((double2*)y + (size_t)j0 * o.m, o.d_ya, (size_t)cnt * o.m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    }
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_adjoint_mc(qmri_ctx* ctx, const void* y, void* x) {
    REQUIRE_OP(ctx);
    OpHost& o = ctx->op;
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    if (!o.ncoil) { qmri_set_error(ctx, "no coil maps set: call qmri_set_coils first"); return QMRI_ERR_STATE; }
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    for (int j0 = 0; j0 < o.ncoil; j0 += o.maxB) {
        const int cnt = std::min(o.maxB, o.ncoil - j0);
        QMRI_HIP(ctx, hipMemcpyAsync(o.d_ya, (const double2*)y + (size_t)j0 * o.m, (size_t)cnt * o.m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
        if (o.kind == OP_NUFFT) QMRI_TRY(nufft_launch_adj(ctx, cnt, o.d_ya, o.d_x));
        else QMRI_TRY(dc_launch_adj(ctx, qmri_opdev(ctx), cnt, o.d_ya, o.d_tmp, o.d_x));
        QMRI_TRY(ew_launch_coil_sum(ctx, n, plane, cnt, o.d_x, o.d_coils + (size_t)j0 * plane, o.d_xa, j0 > 0));
    }
    QMRI_HIP(ctx, hipMemcpyAsync(x, o.d_xa, n * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// single-precision boundary (MATLAB `single` arrays): widened on the host, computed in double, rounded once on the way out
extern "C" int qmri_forward_f32(qmri_ctx* ctx, const float* x, int x_is_complex, float* y) {
    REQUIRE_OP(ctx);
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    const OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s * (x_is_complex ? 2 : 1);
    std::vector<double> xd(x, x + n), yd((size_t)2 * o.m);
    QMRI_TRY(qmri_forward(ctx, xd.data(), x_is_complex, yd.data()));
    for (size_t i = 0; i < yd.size(); ++i) y[i] = (float)yd[i];
    return QMRI_OK;
}

extern "C" int qmri_adjoint_f32(qmri_ctx* ctx, const float* y, float* x) {
    REQUIRE_OP(ctx);
    QMRI_CHECK_ARG(ctx, x && y, "x / y must not be NULL");
    const OpHost& o = ctx->op;
    const size_t n2 = (size_t)2 * o.N * o.M * o.s;
    std::vector<double> yd(y, y + (size_t)2 * o.m), xd(n2);
    QMRI_TRY(qmri_adjoint(ctx, yd.data(), xd.data()));
    for (size_t i = 0; i < n2; ++i) x[i] = (float)xd[i];
    return QMRI_OK;
}
