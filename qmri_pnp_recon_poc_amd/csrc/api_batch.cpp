// api_batch.cpp -- slice batches over several GPUs (qmri_recon_batch*): one host thread + one context per device, static round-robin of launches
// (slices are independent, no collective).  No reference counterpart: main_recon_tsmis_FFT.m reconstructs one slice.
#include "qmri_internal.h"

#include <algorithm>
#include <cstring>
#include <thread>

// Round 4: the worker no longer waits for its copies.  Every launch (slices_per_launch slices) has one of two sets of device and PINNED host
// buffers.  After the reconstruction of launch k (qmri_pnp_admm_dev returns synchronised) the dictionary matches of its slices are queued on the
// compute stream and the results (x, maps) are copied to the pinned set on a COPY stream behind an event; the host then moves the PREVIOUS launch's
// results from its pinned set into the caller's (pageable) arrays while the device works, and goes on to launch k + 1, whose kernels overlap the
// copies of launch k.  Before: pageable hipMemcpy of 8 MB per slice plus a synchronise and two small copies per slice, all in series with the compute.
// shared_device (round 6): another worker of this call uses the same GPU.  The launches that need the device to themselves -- the one-launch LSQR
// iteration (one workgroup per CU, every unit resident at once) and the resident-tile convolution launch -- would then be partially resident
// side by side, both would wait to their time-outs and the reconstruction would be repeated: such a worker starts on the two-launch iteration
// and one launch per layer (same bits, tested).
// ncoil > 0 (multi-coil extension, qmri_recon_batch_mc): Y holds ncoil x m samples per slice and `cmaps` ncoil x N*M maps per slice; each launch is
// one qmri_pnp_admm_mc_dev call.  ncoil = 0 is the single-coil path, unchanged.
// cc (qmri_recon_batch_mc_cc; nullptr on every other path): each launch's uploaded slices are first compressed on the device to cc->nv virtual coils
// (qmri_coil_compress_dev, one W per slice, whitened with `psi` when given) and the reconstruction runs on the compressed stack.
static int recon_worker(int device, bool shared_device, int widx, int nworkers, int nslices, const qmri_problem* pb, const char* Y, char* X_out,
                        float* qmap_out, float* pd_out, std::string* err, int ncoil = 0, const char* cmaps = nullptr,
                        const qmri_cc_params* cc = nullptr, const void* psi = nullptr) {
    qmri_ctx* ctx = nullptr;
    int st = qmri_create(device, &ctx);
    if (st != QMRI_OK) { *err = qmri_last_error(nullptr); return st; }
    const int spl = std::max(1, pb->slices_per_launch);
    const size_t n = (size_t)pb->N * pb->M * pb->s, npix = (size_t)pb->N * pb->M;
    const int m = pb->frame_ptr[pb->T] * std::max(ncoil, 1);       // samples per slice (all coils)
    const int Q = std::max(pb->Q, 1);
    const bool maps = pb->K > 0 && (qmap_out || pd_out);
    const size_t by = (size_t)spl * m * sizeof(double2), bx = (size_t)spl * n * sizeof(double2);
    const size_t bq = (size_t)spl * npix * Q * sizeof(float), bp = (size_t)spl * npix * 2 * sizeof(float);
    const size_t bm = (size_t)spl * ncoil * npix * sizeof(double2);
    const int nv = cc ? cc->nv : ncoil;                             // coils the reconstruction sees
    const size_t byc = (size_t)spl * pb->frame_ptr[pb->T] * nv * sizeof(double2), bmc = (size_t)spl * nv * npix * sizeof(double2);
    // (locals release themselves in reverse order: the buffer sets, the copy stream and Psi behind the synchronisation at the end, the context last)
    struct CtxGuard { qmri_ctx* c; ~CtxGuard() { qmri_destroy(c); } } ctx_guard{ctx};
    DevBuf<double2> d_psi;
    Stream cs;
    struct Set { DevBuf<double2> dY, dX, dM, dYc, dMc; DevBuf<float> dq, dp;
                 PinnedArr<char> hY, hX, hM;
                 PinnedArr<float> hq, hp;
                 Event matched, copied; int s0 = -1, cnt = 0; } set[2];
    auto bail = [&](int code) { *err = qmri_last_error(ctx); return code; };
    auto hipfail = [&](const char* what) { *err = std::string(what) + " failed in qmri_recon_batch"; return QMRI_ERR_HIP; };
    // launch held by set `S` -> the caller's arrays (its copies have been queued; wait for them, then plain host copies)
    auto drain = [&](Set& S) -> int {
        if (S.s0 < 0) return QMRI_OK;
        if (hipEventSynchronize(S.copied) != hipSuccess) return hipfail("hipEventSynchronize");
        std::memcpy(X_out + (size_t)S.s0 * n * sizeof(double2), S.hX, (size_t)S.cnt * n * sizeof(double2));
        if (maps && qmap_out) std::memcpy(qmap_out + (size_t)S.s0 * npix * pb->Q, S.hq, (size_t)S.cnt * npix * pb->Q * sizeof(float));
        if (maps && pd_out) std::memcpy(pd_out + (size_t)S.s0 * npix * 2, S.hp, (size_t)S.cnt * npix * 2 * sizeof(float));
        S.s0 = -1;
        return QMRI_OK;
    };
    st = [&]() -> int {
        int rc;
        if ((rc = qmri_set_operator(ctx, pb->N, pb->M, pb->s, pb->T, pb->V, pb->frame_ptr, pb->kidx, spl)) != QMRI_OK) return bail(rc);
        if ((rc = qmri_set_denoiser(ctx, pb->net, pb->weights, pb->weights_nbytes, pb->N, pb->M, spl)) != QMRI_OK) return bail(rc);
        if (pb->K > 0 && (rc = qmri_set_dictionary(ctx, pb->K, pb->s, pb->Q, pb->D, pb->normD, pb->lut)) != QMRI_OK) return bail(rc);
        if (shared_device) {
            if ((rc = qmri_debug_lsqr_persist(ctx, 0)) != QMRI_OK) return bail(rc);
            if ((rc = qmri_debug_conv_resident(ctx, 0, nullptr)) != QMRI_OK) return bail(rc);
        }
        bool ok = hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking) == hipSuccess;
        for (int j = 0; j < 2 && ok; ++j) {
            Set& S = set[j];
            const auto dev = [&](DevBuf<double2>& d, size_t bytes) { return d.ensure(ctx, bytes / sizeof(double2)) == QMRI_OK; };
            ok = dev(S.dY, by) && dev(S.dX, bx) && S.hY.ensure(ctx, by) == QMRI_OK && S.hX.ensure(ctx, bx) == QMRI_OK &&
                 hipEventCreateWithFlags(&S.matched.e, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&S.copied.e, hipEventDisableTiming) == hipSuccess;
            if (ok && ncoil) ok = dev(S.dM, bm) && S.hM.ensure(ctx, bm) == QMRI_OK;
            if (ok && cc) ok = dev(S.dYc, byc) && dev(S.dMc, bmc);
            if (ok && maps) ok = S.dq.ensure(ctx, bq / sizeof(float)) == QMRI_OK && S.dp.ensure(ctx, bp / sizeof(float)) == QMRI_OK &&
                                 S.hq.ensure(ctx, bq / sizeof(float)) == QMRI_OK && S.hp.ensure(ctx, bp / sizeof(float)) == QMRI_OK;
        }
        if (ok && cc && psi) ok = d_psi.ensure(ctx, (size_t)ncoil * ncoil) == QMRI_OK;
        if (!ok) { *err = "allocation failed in qmri_recon_batch"; return QMRI_ERR_NOMEM; }
        if (d_psi && hipMemcpy(d_psi, psi, (size_t)ncoil * ncoil * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess) return hipfail("H2D copy");
        const int nlaunch = (nslices + spl - 1) / spl;
        int k = 0;
        for (int l = widx; l < nlaunch; l += nworkers, ++k) {
            Set& S = set[k & 1];
            QMRI_TRY(drain(S));                                    // (its previous launch, two launches ago: long since copied)
            const int s0 = l * spl, cnt = std::min(spl, nslices - s0);
            std::memcpy(S.hY, Y + (size_t)s0 * m * sizeof(double2), (size_t)cnt * m * sizeof(double2));
            if (hipMemcpyAsync(S.dY, S.hY, (size_t)cnt * m * sizeof(double2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return hipfail("H2D copy");
            if (ncoil) {
                const size_t mb = (size_t)ncoil * npix * sizeof(double2);
                std::memcpy(S.hM, cmaps + (size_t)s0 * mb, (size_t)cnt * mb);
                if (hipMemcpyAsync(S.dM, S.hM, (size_t)cnt * mb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return hipfail("H2D copy");
                if (cc) {
                    int got = 0;
                    if ((rc = qmri_coil_compress_dev(ctx, cnt, ncoil, S.dY, S.dM, d_psi, cc, &got, S.dYc, S.dMc, nullptr, nullptr)) != QMRI_OK) return bail(rc);
                    if ((rc = qmri_pnp_admm_mc_dev(ctx, cnt, nv, S.dMc, S.dYc, &pb->admm, nullptr, S.dX, nullptr)) != QMRI_OK) return bail(rc);
                } else if ((rc = qmri_pnp_admm_mc_dev(ctx, cnt, ncoil, S.dM, S.dY, &pb->admm, nullptr, S.dX, nullptr)) != QMRI_OK) return bail(rc);
            } else if ((rc = qmri_pnp_admm_dev(ctx, cnt, S.dY, &pb->admm, nullptr, nullptr, S.dX, nullptr, nullptr)) != QMRI_OK) return bail(rc);
            if (maps) {
                for (int i = 0; i < cnt; ++i)
                    if ((rc = qmri_dict_match_dev(ctx, S.dX + (size_t)i * n, (int)npix, qmap_out ? S.dq + (size_t)i * npix * Q : nullptr,
                                                  pd_out ? S.dp + (size_t)i * npix * 2 : nullptr, nullptr, nullptr)) != QMRI_OK) return bail(rc);
            }
            if (hipEventRecord(S.matched, ctx->stream) != hipSuccess || hipStreamWaitEvent(cs, S.matched, 0) != hipSuccess) return hipfail("event");
            if (hipMemcpyAsync(S.hX, S.dX, (size_t)cnt * n * sizeof(double2), hipMemcpyDeviceToHost, cs) != hipSuccess) return hipfail("D2H copy");
            if (maps && qmap_out && hipMemcpyAsync(S.hq, S.dq, (size_t)cnt * npix * Q * sizeof(float), hipMemcpyDeviceToHost, cs) != hipSuccess) return hipfail("D2H copy");
            if (maps && pd_out && hipMemcpyAsync(S.hp, S.dp, (size_t)cnt * npix * 2 * sizeof(float), hipMemcpyDeviceToHost, cs) != hipSuccess) return hipfail("D2H copy");
            if (hipEventRecord(S.copied, cs) != hipSuccess) return hipfail("event");
            S.s0 = s0; S.cnt = cnt;
            QMRI_TRY(drain(set[(k & 1) ^ 1]));                     // the previous launch's results, while the device matches and copies this one's
        }
        QMRI_TRY(drain(set[0]));
        return drain(set[1]);
    }();
    (void)hipDeviceSynchronize();
    return st;
}

static int recon_batch_impl(const char* name, int ndev, const int* devs, int nslices, const qmri_problem* prob, int ncoil, const void* maps, const void* Y,
                            void* X_out, float* qmap_out, float* pd_out, char* errbuf, size_t errbuf_len, const qmri_cc_params* cc = nullptr,
                            const void* psi = nullptr) {
    auto report = [&](const std::string& s) { if (errbuf && errbuf_len) { snprintf(errbuf, errbuf_len, "%s", s.c_str()); } };
    if (ndev <= 0 || !devs || nslices <= 0 || !prob || !Y || !X_out || !prob->V || !prob->frame_ptr || !prob->kidx || !prob->net ||
        !prob->weights || (ncoil && (ncoil < 0 || ncoil > 1024 || !maps))) {
        report(std::string(name) + ": invalid arguments");
        return QMRI_ERR_INVALID_ARG;
    }
    std::vector<std::thread> th;
    std::vector<int> status(ndev, QMRI_OK);
    std::vector<std::string> errs(ndev);
    for (int w = 0; w < ndev; ++w) {
        bool shared = false;
        for (int v = 0; v < ndev; ++v) shared = shared || (v != w && devs[v] == devs[w]);
        th.emplace_back([&, w, shared]() {
            status[w] = recon_worker(devs[w], shared, w, ndev, nslices, prob, (const char*)Y, (char*)X_out, qmap_out, pd_out, &errs[w], ncoil,
                                     (const char*)maps, cc, psi);
        });
    }
    for (auto& t : th) t.join();
    for (int w = 0; w < ndev; ++w)
        if (status[w] != QMRI_OK) { report("device " + std::to_string(devs[w]) + ": " + errs[w]); return status[w]; }
    return QMRI_OK;
}

extern "C" int qmri_recon_batch(int ndev, const int* devs, int nslices, const qmri_problem* prob, const void* Y, void* X_out,
                                float* qmap_out, float* pd_out, char* errbuf, size_t errbuf_len) {
    return recon_batch_impl("qmri_recon_batch", ndev, devs, nslices, prob, 0, nullptr, Y, X_out, qmap_out, pd_out, errbuf, errbuf_len);
}

extern "C" int qmri_recon_batch_mc(int ndev, const int* devs, int nslices, const qmri_problem* prob, int ncoil, const void* maps, const void* Y_mc,
                                   void* X_out, float* qmap_out, float* pd_out, char* errbuf, size_t errbuf_len) {
    if (ncoil < 1) {
        if (errbuf && errbuf_len) snprintf(errbuf, errbuf_len, "qmri_recon_batch_mc: invalid arguments (ncoil >= 1)");
        return QMRI_ERR_INVALID_ARG;
    }
    return recon_batch_impl("qmri_recon_batch_mc", ndev, devs, nslices, prob, ncoil, maps, Y_mc, X_out, qmap_out, pd_out, errbuf, errbuf_len);
}

extern "C" int qmri_recon_batch_mc_cc(int ndev, const int* devs, int nslices, const qmri_problem* prob, int ncoil, const void* maps, const void* Y_mc,
                                      void* X_out, float* qmap_out, float* pd_out, char* errbuf, size_t errbuf_len, const void* noise_cov,
                                      const qmri_cc_params* cc) {
    std::string msg = "invalid arguments (ncoil >= 1)";
    const int code = ncoil < 1 ? QMRI_ERR_INVALID_ARG : cc_batch_param_error(ncoil, cc, &msg);
    if (code != QMRI_OK) {
        if (errbuf && errbuf_len) snprintf(errbuf, errbuf_len, "qmri_recon_batch_mc_cc: %s", msg.c_str());
        return code;
    }
    return recon_batch_impl("qmri_recon_batch_mc_cc", ndev, devs, nslices, prob, ncoil, maps, Y_mc, X_out, qmap_out, pd_out, errbuf, errbuf_len, cc, noise_cov);
}
