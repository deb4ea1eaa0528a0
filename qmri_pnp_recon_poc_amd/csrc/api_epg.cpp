// api_epg.cpp -- C ABI of the FISP dictionary simulation by extended phase graphs, plain, over a slice profile, with derivatives and over a schedule of
// prepared, repeated trains (include/qmri.h; kernels:
// epg_kernels.hip).  An EXTENSION with no reference counterpart.  Every refusal is decided here, on the host, before the device is selected; with ctx == NULL the message of the first
// failing check is left in qmri_last_error(NULL), so the argument rules can be exercised on a machine without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "epg_seq_plan.h"
#include "qmri_internal.h"

namespace {
constexpr int EPG_MAX_T = 1024, EPG_MAX_S = 256, EPG_MAX_Q = 64;

// QMRI_OK, or the code of the first failing check with its message set on ctx (ctx may be NULL; ctx_check comes after
// these).  host_atoms: t1 / t2 / b1 can be read here; need_F: F_out is the call's one output (the derivative calls have their own output rules)
int epg_checks(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2, const double* b1,
               const qmri_epg_params* p, const void* F_out, bool host_atoms, bool need_F = true) {
    QMRI_CHECK_ARG(ctx, p, "simulation params must not be NULL");
    QMRI_CHECK_ARG(ctx, alpha && tr && te && t1 && t2 && (F_out || !need_F), "alpha / tr / te / t1 / t2 / F_out must not be NULL");
    QMRI_CHECK_ARG(ctx, K >= 1 && K <= (1 << 30), "K must satisfy 1 <= K <= 2^30");
    QMRI_CHECK_ARG(ctx, T >= 1 && T <= EPG_MAX_T, "T must satisfy 1 <= T <= 1024");
    QMRI_CHECK_ARG(ctx, p->nstates >= 1 && p->nstates <= EPG_MAX_S, "nstates must satisfy 1 <= nstates <= 256");
    QMRI_CHECK_ARG(ctx, p->inversion == 0 || p->inversion == 1, "inversion must be 0 or 1");
    QMRI_CHECK_ARG(ctx, p->out_is_f64 == 0 || p->out_is_f64 == 1, "out_is_f64 must be 0 or 1");
    if (p->inversion) {
        QMRI_CHECK_ARG(ctx, std::isfinite(p->ti) && p->ti >= 0.0, "ti must be finite and >= 0");
        QMRI_CHECK_ARG(ctx, p->inv_eff > 0.0 && p->inv_eff <= 1.0, "inv_eff must be in (0, 1]");
    }
    for (int t = 0; t < T; ++t) {
        QMRI_CHECK_ARG(ctx, std::isfinite(alpha[t]) && alpha[t] >= 0.0, "alpha must be finite and >= 0 in every frame");
        QMRI_CHECK_ARG(ctx, std::isfinite(tr[t]) && tr[t] > 0.0, "tr must be finite and > 0 in every frame");
        QMRI_CHECK_ARG(ctx, std::isfinite(te[t]) && te[t] >= 0.0, "te must be finite and >= 0 in every frame");
        QMRI_CHECK_ARG(ctx, te[t] <= tr[t], "te must not exceed tr in any frame");
    }
    if (host_atoms)
        for (int k = 0; k < K; ++k) {
            QMRI_CHECK_ARG(ctx, std::isfinite(t1[k]) && t1[k] > 0.0, "t1 must be finite and > 0 for every atom");
            QMRI_CHECK_ARG(ctx, std::isfinite(t2[k]) && t2[k] > 0.0, "t2 must be finite and > 0 for every atom");
            QMRI_CHECK_ARG(ctx, !b1 || (std::isfinite(b1[k]) && b1[k] >= 0.0), "b1 must be finite and >= 0 for every atom");
        }
    return QMRI_OK;
}

// the rules of a slice profile (ctx may be NULL)
int epg_profile_checks(qmri_ctx* ctx, int T, const qmri_epg_profile* sp) {
    QMRI_CHECK_ARG(ctx, sp, "slice profile must not be NULL");
    QMRI_CHECK_ARG(ctx, sp->nq >= 1 && sp->nq <= EPG_MAX_Q, "nq must satisfy 1 <= nq <= 64");
    QMRI_CHECK_ARG(ctx, sp->per_frame == 0 || sp->per_frame == 1, "per_frame must be 0 or 1");
    QMRI_CHECK_ARG(ctx, sp->prof && sp->weight, "prof / weight must not be NULL");
    const size_t np = (size_t)sp->nq * (sp->per_frame ? (size_t)T : 1);
    for (size_t i = 0; i < np; ++i) QMRI_CHECK_ARG(ctx, std::isfinite(sp->prof[i]) && sp->prof[i] >= 0.0, "prof must be finite and >= 0 in every entry");
    double sum = 0.0;
    for (int q = 0; q < sp->nq; ++q) {
        QMRI_CHECK_ARG(ctx, std::isfinite(sp->weight[q]) && sp->weight[q] >= 0.0, "weight must be finite and >= 0 in every entry");
        sum += sp->weight[q];
    }
    QMRI_CHECK_ARG(ctx, sum > 0.0, "the weights must sum to more than 0");
    return QMRI_OK;
}

// the rules of the derivative call's own arguments (ctx may be NULL)
int epg_grad_checks(qmri_ctx* ctx, int T, const qmri_epg_grad_params* gp, const void* F_out, const void* dF_out, const double* crb_out,
                    const int32_t* flags_out) {
    QMRI_CHECK_ARG(ctx, gp, "grad params must not be NULL");
    QMRI_CHECK_ARG(ctx, F_out || dF_out || crb_out || flags_out, "at least one of F_out / dF_out / crb_out must be given");
    QMRI_CHECK_ARG(ctx, !crb_out == !flags_out, "crb_out and flags_out go together");
    QMRI_CHECK_ARG(ctx, gp->nparams == 2 || gp->nparams == 3, "nparams must be 2 or 3");
    QMRI_CHECK_ARG(ctx, gp->s >= 0 && gp->s <= 16, "s must satisfy 0 <= s <= 16");
    for (int32_t r : gp->reserved) QMRI_CHECK_ARG(ctx, r == 0, "reserved must be zero");
    if (gp->s > 0) {
        QMRI_CHECK_ARG(ctx, gp->V, "V must not be NULL when s > 0");
        const size_t n = (size_t)T * (size_t)gp->s;
        for (size_t i = 0; i < n; ++i) QMRI_CHECK_ARG(ctx, std::isfinite(gp->V[i]), "V must be finite in every entry");
    }
    return QMRI_OK;
}

// the rules of a block schedule (ctx may be NULL); they follow the rules of the plain call, whose T bounds the sum
int epg_seq_checks(qmri_ctx* ctx, int T, const qmri_epg_params* p, const qmri_epg_seq* seq) {
    QMRI_CHECK_ARG(ctx, p->inversion == 0, "inversion must be 0 in this call: inversions are stated in the blocks");
    QMRI_CHECK_ARG(ctx, seq && seq->blocks, "seq / blocks must not be NULL");
    QMRI_CHECK_ARG(ctx, seq->nblocks >= 1 && seq->nblocks <= epgseq::MAX_BLOCKS, "nblocks must satisfy 1 <= nblocks <= 64");
    QMRI_CHECK_ARG(ctx, seq->ncycles >= 1 && seq->ncycles <= epgseq::MAX_CYCLES, "ncycles must satisfy 1 <= ncycles <= 16");
    for (int32_t r : seq->reserved) QMRI_CHECK_ARG(ctx, r == 0, "reserved must be zero");
    long long sum = 0;
    for (int b = 0; b < seq->nblocks; ++b) {
        const qmri_epg_block& bl = seq->blocks[b];
        QMRI_CHECK_ARG(ctx, bl.nframes >= 1, "nframes must be >= 1 in every block");
        QMRI_CHECK_ARG(ctx, bl.prep >= 0 && bl.prep <= 2, "prep must be 0 (none), 1 (inversion) or 2 (T2 preparation) in every block");
        QMRI_CHECK_ARG(ctx, std::isfinite(bl.wait) && bl.wait >= 0.0, "wait must be finite and >= 0 in every block");
        QMRI_CHECK_ARG(ctx, std::isfinite(bl.prep_time) && bl.prep_time >= 0.0, "prep_time must be finite and >= 0 in every block");
        QMRI_CHECK_ARG(ctx, bl.prep_eff > 0.0 && bl.prep_eff <= 1.0, "prep_eff must be in (0, 1] in every block");
        QMRI_CHECK_ARG(ctx, bl.prep != 0 || (bl.prep_time == 0.0 && bl.prep_eff == 1.0), "a block without a preparation must have prep_time 0 and prep_eff 1");
        sum += bl.nframes;
    }
    QMRI_CHECK_ARG(ctx, sum == T, "the nframes of the blocks must sum to T");
    return QMRI_OK;
}

int ctx_check(qmri_ctx* ctx) {
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

// the schedule on the device and the launch; the stream is idle on return.  Without a profile: alpha [T], tr [T], te [T].  With one: T frame
// records (alpha_t, tr_t, te_t, prof[t, 0 .. Q-1]; a per_frame = 0 profile repeated in every record), then weight [Q]: (3 + Q) T + Q doubles
int epg_run(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1, const double* d_t2,
            const double* d_b1, const qmri_epg_params& p, const qmri_epg_profile* sp, void* d_F) {
    const int Q = sp ? sp->nq : 0, FR = 3 + Q;
    std::vector<double> sched(sp ? (size_t)FR * T + Q : (size_t)3 * T);
    bool const_timing = true;
    for (int t = 0; t < T; ++t) {
        const_timing = const_timing && tr[t] == tr[0] && te[t] == te[0];
        if (!sp) { sched[t] = alpha[t]; sched[T + t] = tr[t]; sched[2 * T + t] = te[t]; continue; }
        double* fr = sched.data() + (size_t)t * FR;
        fr[0] = alpha[t]; fr[1] = tr[t]; fr[2] = te[t];
        std::copy_n(sp->prof + (sp->per_frame ? (size_t)t * Q : 0), Q, fr + 3);
    }
    if (sp) std::copy_n(sp->weight, Q, sched.data() + (size_t)FR * T);
    DevBuf<double> ds;
    QMRI_TRY(ds.ensure(ctx, sched.size()));
    QMRI_HIP(ctx, hipMemcpyAsync(ds.p, sched.data(), sched.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (sp) QMRI_TRY(epg_simulate_sp_dev(ctx, K, T, Q, ds, d_t1, d_t2, d_b1, p, const_timing, d_F));
    else QMRI_TRY(epg_simulate_dev(ctx, K, T, ds, d_t1, d_t2, d_b1, p, const_timing, d_F));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// the block schedule: alpha, tr, te followed by the segment records of epg_seq_plan.h on the device, and the launch; the stream is idle on return
int epg_seq_run(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1, const double* d_t2,
                const double* d_b1, const qmri_epg_params& p, const qmri_epg_seq& seq, void* d_F) {
    const std::vector<epgseq::Segment> segs = epgseq::plan(seq.nblocks, seq.blocks);
    constexpr size_t SD = sizeof(epgseq::Segment) / sizeof(double);
    std::vector<double> sched((size_t)3 * T + segs.size() * SD);
    bool const_timing = true;
    for (int t = 0; t < T; ++t) {
        const_timing = const_timing && tr[t] == tr[0] && te[t] == te[0];
        sched[t] = alpha[t]; sched[T + t] = tr[t]; sched[2 * T + t] = te[t];
    }
    std::memcpy(sched.data() + (size_t)3 * T, segs.data(), segs.size() * sizeof(epgseq::Segment));
    DevBuf<double> ds;
    QMRI_TRY(ds.ensure(ctx, sched.size()));
    QMRI_HIP(ctx, hipMemcpyAsync(ds.p, sched.data(), sched.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(epg_simulate_seq_dev(ctx, K, T, (int)segs.size(), seq.ncycles, ds, ds.p + (size_t)3 * T, d_t1, d_t2, d_b1, p, const_timing, d_F));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// the derivative call: the schedule followed by V on the device and the launch; the stream is idle on return
int epg_grad_run(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1, const double* d_t2,
                 const double* d_b1, const qmri_epg_params& p, const qmri_epg_grad_params& gp, void* d_F, void* d_dF, double* d_crb, int32_t* d_flags) {
    std::vector<double> sched((size_t)3 * T + (size_t)T * gp.s);
    bool const_timing = true;
    for (int t = 0; t < T; ++t) {
        const_timing = const_timing && tr[t] == tr[0] && te[t] == te[0];
        sched[t] = alpha[t]; sched[T + t] = tr[t]; sched[2 * T + t] = te[t];
    }
    if (gp.s > 0) std::copy_n(gp.V, (size_t)T * gp.s, sched.data() + (size_t)3 * T);
    DevBuf<double> ds;
    QMRI_TRY(ds.ensure(ctx, sched.size()));
    QMRI_HIP(ctx, hipMemcpyAsync(ds.p, sched.data(), sched.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(epg_simulate_grad_dev(ctx, K, T, gp.nparams, gp.s, ds, d_t1, d_t2, d_b1, p, const_timing, d_F, d_dF, d_crb, d_flags));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// the checks of both derivative entry points: the derivative arguments first (T bounds the read of V), then the rules of the plain call
int epg_grad_all_checks(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2,
                        const double* b1, const qmri_epg_params* p, const qmri_epg_grad_params* gp, const void* F_out, const void* dF_out,
                        const double* crb_out, const int32_t* flags_out, bool host_atoms) {
    QMRI_CHECK_ARG(ctx, p, "simulation params must not be NULL");
    QMRI_CHECK_ARG(ctx, T >= 1 && T <= EPG_MAX_T, "T must satisfy 1 <= T <= 1024");
    QMRI_TRY(epg_grad_checks(ctx, T, gp, F_out, dF_out, crb_out, flags_out));
    return epg_checks(ctx, K, T, alpha, tr, te, t1, t2, b1, p, F_out, host_atoms, false);
}

// the device-array and the host-array route behind all four entry points.  with_profile: the _sp calls, whose sp is checked (a NULL one is a
// refusal); the plain calls pass sp == NULL and run k_epg as before
int simulate_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1, const double* d_t2,
                 const double* d_b1, const qmri_epg_params* p, const qmri_epg_profile* sp, bool with_profile, void* d_F_out) {
    QMRI_TRY(epg_checks(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, p, d_F_out, false));
    if (with_profile) QMRI_TRY(epg_profile_checks(ctx, T, sp));
    QMRI_TRY(ctx_check(ctx));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return epg_run(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, *p, sp, d_F_out);
}

int simulate_host(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2, const double* b1,
                  const qmri_epg_params* p, const qmri_epg_profile* sp, bool with_profile, void* F_out) {
    QMRI_TRY(epg_checks(ctx, K, T, alpha, tr, te, t1, t2, b1, p, F_out, true));
    if (with_profile) QMRI_TRY(epg_profile_checks(ctx, T, sp));
    QMRI_TRY(ctx_check(ctx));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nF = (size_t)K * T * (p->out_is_f64 ? sizeof(double) : sizeof(float));
    DevBuf<double> d1, d2, db;
    DevBuf<unsigned char> dF;
    QMRI_TRY(d1.ensure(ctx, (size_t)K));
    QMRI_TRY(d2.ensure(ctx, (size_t)K));
    if (b1) QMRI_TRY(db.ensure(ctx, (size_t)K));
    QMRI_TRY(dF.ensure(ctx, nF));
    QMRI_HIP(ctx, hipMemcpyAsync(d1.p, t1, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(d2.p, t2, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (b1) QMRI_HIP(ctx, hipMemcpyAsync(db.p, b1, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(epg_run(ctx, K, T, alpha, tr, te, d1, d2, db, *p, sp, dF.p));
    QMRI_HIP(ctx, hipMemcpyAsync(F_out, dF.p, nF, hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_dict_simulate_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1,
                                      const double* d_t2, const double* d_b1, const qmri_epg_params* p, void* d_F_out) {
    return simulate_dev(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, p, nullptr, false, d_F_out);
}

extern "C" int qmri_dict_simulate(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2,
                                  const double* b1, const qmri_epg_params* p, void* F_out) {
    return simulate_host(ctx, K, T, alpha, tr, te, t1, t2, b1, p, nullptr, false, F_out);
}

extern "C" int qmri_dict_simulate_sp_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1,
                                         const double* d_t2, const double* d_b1, const qmri_epg_params* p, const qmri_epg_profile* sp, void* d_F_out) {
    return simulate_dev(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, p, sp, true, d_F_out);
}

extern "C" int qmri_dict_simulate_sp(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1,
                                     const double* t2, const double* b1, const qmri_epg_params* p, const qmri_epg_profile* sp, void* F_out) {
    return simulate_host(ctx, K, T, alpha, tr, te, t1, t2, b1, p, sp, true, F_out);
}

extern "C" int qmri_dict_simulate_seq_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1,
                                          const double* d_t2, const double* d_b1, const qmri_epg_params* p, const qmri_epg_seq* seq, void* d_F_out) {
    QMRI_TRY(epg_checks(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, p, d_F_out, false));
    QMRI_TRY(epg_seq_checks(ctx, T, p, seq));
    QMRI_TRY(ctx_check(ctx));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return epg_seq_run(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, *p, *seq, d_F_out);
}

extern "C" int qmri_dict_simulate_seq(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1,
                                      const double* t2, const double* b1, const qmri_epg_params* p, const qmri_epg_seq* seq, void* F_out) {
    QMRI_TRY(epg_checks(ctx, K, T, alpha, tr, te, t1, t2, b1, p, F_out, true));
    QMRI_TRY(epg_seq_checks(ctx, T, p, seq));
    QMRI_TRY(ctx_check(ctx));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nF = (size_t)K * T * (p->out_is_f64 ? sizeof(double) : sizeof(float));
    DevBuf<double> d1, d2, db;
    DevBuf<unsigned char> dF;
    QMRI_TRY(d1.ensure(ctx, (size_t)K));
    QMRI_TRY(d2.ensure(ctx, (size_t)K));
    if (b1) QMRI_TRY(db.ensure(ctx, (size_t)K));
    QMRI_TRY(dF.ensure(ctx, nF));
    QMRI_HIP(ctx, hipMemcpyAsync(d1.p, t1, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(d2.p, t2, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (b1) QMRI_HIP(ctx, hipMemcpyAsync(db.p, b1, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(epg_seq_run(ctx, K, T, alpha, tr, te, d1, d2, db, *p, *seq, dF.p));
    QMRI_HIP(ctx, hipMemcpyAsync(F_out, dF.p, nF, hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_dict_simulate_grad_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1,
                                           const double* d_t2, const double* d_b1, const qmri_epg_params* p, const qmri_epg_grad_params* gp, void* d_F_out,
                                           void* d_dF_out, double* d_crb_out, int32_t* d_flags_out) {
    QMRI_TRY(epg_grad_all_checks(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, p, gp, d_F_out, d_dF_out, d_crb_out, d_flags_out, false));
    QMRI_TRY(ctx_check(ctx));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return epg_grad_run(ctx, K, T, alpha, tr, te, d_t1, d_t2, d_b1, *p, *gp, d_F_out, d_dF_out, d_crb_out, d_flags_out);
}

extern "C" int qmri_dict_simulate_grad(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1,
                                       const double* t2, const double* b1, const qmri_epg_params* p, const qmri_epg_grad_params* gp, void* F_out,
                                       void* dF_out, double* crb_out, int32_t* flags_out) {
    QMRI_TRY(epg_grad_all_checks(ctx, K, T, alpha, tr, te, t1, t2, b1, p, gp, F_out, dF_out, crb_out, flags_out, true));
    QMRI_TRY(ctx_check(ctx));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const int NS = 1 + gp->nparams;
    const size_t nF = (size_t)K * T * (p->out_is_f64 ? sizeof(double) : sizeof(float)), ndF = nF * (size_t)gp->nparams;
    DevBuf<double> d1, d2, db, dcrb;
    DevBuf<unsigned char> dF, ddF;
    DevBuf<int32_t> dfl;
    QMRI_TRY(d1.ensure(ctx, (size_t)K));
    QMRI_TRY(d2.ensure(ctx, (size_t)K));
    if (b1) QMRI_TRY(db.ensure(ctx, (size_t)K));
    if (F_out) QMRI_TRY(dF.ensure(ctx, nF));
    if (dF_out) QMRI_TRY(ddF.ensure(ctx, ndF));
    if (crb_out) {
        QMRI_TRY(dcrb.ensure(ctx, (size_t)K * NS));
        QMRI_TRY(dfl.ensure(ctx, (size_t)K));
    }
    QMRI_HIP(ctx, hipMemcpyAsync(d1.p, t1, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(d2.p, t2, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (b1) QMRI_HIP(ctx, hipMemcpyAsync(db.p, b1, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(epg_grad_run(ctx, K, T, alpha, tr, te, d1, d2, db, *p, *gp, F_out ? dF.p : nullptr, dF_out ? ddF.p : nullptr, crb_out ? dcrb.p : nullptr,
                          crb_out ? dfl.p : nullptr));
    if (F_out) QMRI_HIP(ctx, hipMemcpyAsync(F_out, dF.p, nF, hipMemcpyDeviceToHost, ctx->stream));
    if (dF_out) QMRI_HIP(ctx, hipMemcpyAsync(dF_out, ddF.p, ndF, hipMemcpyDeviceToHost, ctx->stream));
    if (crb_out) {
        QMRI_HIP(ctx, hipMemcpyAsync(crb_out, dcrb.p, (size_t)K * NS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        QMRI_HIP(ctx, hipMemcpyAsync(flags_out, dfl.p, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_debug_epg_shift(qmri_ctx* ctx, int S, int nshift, const double* in, double* out) {
    QMRI_CHECK_ARG(ctx, in && out, "in / out must not be NULL");
    QMRI_CHECK_ARG(ctx, S >= 1 && S <= EPG_MAX_S, "S must satisfy 1 <= S <= 256");
    QMRI_CHECK_ARG(ctx, nshift >= 0 && nshift <= 4096, "nshift must satisfy 0 <= nshift <= 4096");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<double> di, dout;
    QMRI_TRY(di.ensure(ctx, (size_t)3 * S));
    QMRI_TRY(dout.ensure(ctx, (size_t)3 * S));
    QMRI_HIP(ctx, hipMemcpyAsync(di.p, in, (size_t)3 * S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(epg_shift_dev(ctx, S, nshift, di, dout));
    QMRI_HIP(ctx, hipMemcpyAsync(out, dout.p, (size_t)3 * S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
