// sms_kernels.hip -- simultaneous multi-slice (SMS) groups: the coupled operator and the joint x-update of PnP-ADMM.  An EXTENSION (DESIGN.md
// section 31) with no reference counterpart: PARITY UNPINNED, stated in include/qmri.h.  Z slices are excited together, so a coil sees their sum,
// each slice under a known phase per frame:
//     A_sms x   = [ sum_b E[t(i), b] (A (C_{g,b,j} . x_{g,b}))_i ]_{g,j}
//     A_sms^H y = [ sum_j conj(C_{g,b,j}) . A^H (conj(E[t(.), b]) . y_{g,j}) ]_{g,b}
// with A the context's gridded or trajectory operator.  The x-update is the image-domain LSQR of mc_kernels.hip, recurrence for recurrence, on the
// Z n elements of a group as ONE vector: one LsqrState per group, frozen once the group stops.
//
// What is reused: the image-side vector kernels of mc_kernels.hip (k_mcl_ub / dupd / vupd / coil_sum) run unchanged on the G Z slice vectors, each
// reading a COPY of its group's state (McWork::st) that k_sms_scalar refreshes whenever it changes the group's.  What is new: the coil product in
// the forward order, the COMBINE kernel (the phase-weighted sum over the slices of a group in k-space, fused with the update of u as k_mcl_ulin
// fuses it), the EXPAND kernel (its transpose: conj(E) u into the staging buffer the adjoint transform reads) and the per-group scalar kernel.
//
// Orders (sms_plan.h): forward q = (g ncoil + j) Z + b, adjoint q = (g Z + b) ncoil + j -- the multi-coil order with B = G Z.  A chunk of max_batch
// images may begin inside a sum; slice b is added after slice b - 1 and coil j after coil j - 1 in fp64 whichever chunk holds them (SmsWork::acc
// carries the sum over slices between chunks), and the |u|^2 partials are written once slice Z - 1 is in.
//
// Reductions: fixed partials, PC per (g, j) and PS per slice vector, added in one order by k_sms_scalar (coils ascending, then slices ascending).
// No floating-point atomics, no spin waits, no hand-offs between workgroups.  So a group's x-update is the same bits alone, at any position of
// any call, at any G and any max_batch; and with Z = 1, E = 1 it is qmri_lsqr_mc_batch_dev's bits: the products with (1, 0) are exact and the sums
// run in the same order.
#include <cfloat>
#include <cmath>
#include <vector>
#include "qmri_internal.h"

namespace {
constexpr int NT = 256;          // threads per workgroup of the streaming kernels
constexpr int PS = sms::PS, PC = sms::PC;
static_assert(PS == MC_PS && PC == MC_PC, "the slice-vector partials are written by mc_kernels.hip's kernels");
enum { SMS_INIT = 0, SMS_ITER = 1, SMS_PLAIN = 2 };
enum { SC_BETA0 = 0, SC_BETA = 1, SC_STOP = 2, SC_ALPHA = 3 };

__device__ __forceinline__ double block_sum(double v, double* sh) {          // fixed order: lanes by shuffle tree, waves in index order
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int w = 0; w < NT / 64; ++w) t += sh[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ double wave_sum(const double* p, int cnt) {        // one wave: lane l adds p[l], p[l + 64], ..., then a shuffle tree
    double v = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 64) v += p[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ bool frozen(const LsqrState* st, int g) { return st && st[g].done; }
__device__ __forceinline__ double2 cmul(double2 c, double2 v) { return make_double2(c.x * v.x - c.y * v.y, c.x * v.y + c.y * v.x); }

// forward order: out[q - q0][i] = maps[g][b][j][i % plane] * x[g][b][i],  q = (g ncoil + j) Z + b    (grid: n / NT x cnt)
__global__ __launch_bounds__(NT) void k_sms_coil_mul(size_t n, size_t plane, int ncoil, int Z, int q0, const double2* __restrict__ x,
                                                     const double2* __restrict__ maps, const LsqrState* __restrict__ st, double2* __restrict__ out) {
    const int q = q0 + blockIdx.y, a = q / Z, b = q - a * Z, g = a / ncoil, j = a - g * ncoil;
    if (frozen(st, g)) return;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const size_t sv = (size_t)g * Z + b;
    out[(size_t)blockIdx.y * n + i] = cmul(maps[(sv * ncoil + j) * plane + i % plane], x[sv * n + i]);
}
// COMBINE: the measurement half of u for the (g, j) a forward chunk touches, one per blockIdx.y (grid: PC x units), m complex each.  With
// s_i = sum over the chunk's slices b of (g, j), ascending, of E[t(i), b] ya_b[i], continued from acc when the chunk enters (g, j) after slice 0:
//   slice Z - 1 not in yet:  acc = s
//   INIT   u = y - s,  partials |u|^2 and |y|^2          ITER   u = s - (alpha / beta) u,  partial |u|^2          PLAIN  u = s   (qmri_forward_sms)
__global__ __launch_bounds__(NT) void k_sms_combine(int mode, size_t m, int ncoil, int Z, int T, int q0, int cnt, const double2* __restrict__ ya,
                                                    const double2* __restrict__ y, const int32_t* __restrict__ frame, const double2* __restrict__ E,
                                                    const LsqrState* __restrict__ st, double2* __restrict__ ut, double2* __restrict__ acc,
                                                    double* __restrict__ pu, double* __restrict__ py) {
    __shared__ double sh[NT / 64];
    const int a = q0 / Z + blockIdx.y, g = a / ncoil;
    if (frozen(st, g)) return;
    const int lo = max(q0, a * Z), hi = min(q0 + cnt, (a + 1) * Z);
    const bool last = hi == (a + 1) * Z;
    const double coef = mode == SMS_ITER ? st[g].sc[0].alpha * st[g].sc[0].ub : 0.0;
    double2* u = ut + (size_t)a * m;
    double2* ac = acc + (size_t)a * m;
    double su = 0.0, sy = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < m; i += (size_t)PC * NT) {
        const double2* e = E + frame[i];
        double2 s = make_double2(0.0, 0.0);
        for (int q = lo; q < hi; ++q) {
            const double2 p = cmul(e[(size_t)(q - a * Z) * T], ya[(size_t)(q - q0) * m + i]);
            if (q == a * Z) s = p;                                     // slice 0 starts the sum
            else {
                if (q == lo) s = ac[i];                                // an earlier chunk began it
                s.x += p.x; s.y += p.y;
            }
        }
        if (!last) { ac[i] = s; continue; }
        double2 w;
        if (mode == SMS_INIT) {
            const double2 yv = y[(size_t)a * m + i];
            w = make_double2(yv.x - s.x, yv.y - s.y);
            sy += yv.x * yv.x + yv.y * yv.y;
        } else if (mode == SMS_ITER) {
            const double2 uv = u[i];
            w = make_double2(s.x - coef * uv.x, s.y - coef * uv.y);
        } else w = s;
        u[i] = w;
        su += w.x * w.x + w.y * w.y;
    }
    if (!last || mode == SMS_PLAIN) return;
    su = block_sum(su, sh);
    if (mode == SMS_INIT) sy = block_sum(sy, sh);
    if (threadIdx.x == 0) {
        pu[(size_t)a * PC + blockIdx.x] = su;
        if (mode == SMS_INIT) py[(size_t)a * PC + blockIdx.x] = sy;
    }
}
// EXPAND: adjoint order q = (g Z + b) ncoil + j: out[q - q0][i] = conj(E[t(i), b]) u[g][j][i]    (grid: m / NT x cnt)
__global__ __launch_bounds__(NT) void k_sms_expand(size_t m, int ncoil, int Z, int T, int q0, const double2* __restrict__ ut,
                                                   const int32_t* __restrict__ frame, const double2* __restrict__ E, const LsqrState* __restrict__ st,
                                                   double2* __restrict__ out) {
    const int q = q0 + blockIdx.y, sv = q / ncoil, j = q - sv * ncoil, g = sv / Z, b = sv - g * Z;
    if (frozen(st, g)) return;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= m) return;
    const double2 e = E[(size_t)b * T + frame[i]], v = ut[((size_t)g * ncoil + j) * m + i];
    out[(size_t)blockIdx.y * m + i] = make_double2(e.x * v.x + e.y * v.y, e.x * v.y - e.y * v.x);      // conj(e) * v
}

struct ScalarArgs { LsqrState* st; LsqrState* sv; LsqrState* hst; const double *pu, *py, *pb, *pz, *pd, *px, *pv; int ncoil, Z, ii, maxit; double tol, r; };
// what follows every change of a group's state: its copies for the slice vectors' kernels, and iter / done / flag to the pinned host copy
__device__ void sms_publish(const ScalarArgs& a, int g, const LsqrState& S, bool tell) {
    if (threadIdx.x) return;
    for (int b = 0; b < a.Z; ++b) a.sv[(size_t)g * a.Z + b] = S;
    if (tell && a.hst) { LsqrState* h = a.hst + g; h->iter = S.iter; h->flag = S.flag; h->done = S.done; }
}
__device__ double sms_slices_sum(const double* p, int g, int Z) {             // slices ascending
    double t = 0.0;
    for (int b = 0; b < Z; ++b) t += wave_sum(p + ((size_t)g * Z + b) * PS, PS);
    return t;
}
// the recurrences of orc_lsqr.c between the vector kernels as k_mcl_scalar states them, one wave per group (grid: G x 64)
__global__ __launch_bounds__(64) void k_sms_scalar(int stage, ScalarArgs a) {
    const int g = blockIdx.x;
    LsqrState& S = a.st[g];
    LsqrScalars& q = S.sc[0];
    if (stage != SC_BETA0 && S.done) return;
    double su = 0.0;
    if (stage == SC_BETA0 || stage == SC_BETA)
        for (int j = 0; j < a.ncoil; ++j) su += wave_sum(a.pu + ((size_t)g * a.ncoil + j) * PC, PC);
    if (stage == SC_BETA0) {
        double sy = 0.0;
        for (int j = 0; j < a.ncoil; ++j) sy += wave_sum(a.py + ((size_t)g * a.ncoil + j) * PC, PC);
        const double sz = sms_slices_sum(a.pz, g, a.Z), sb = sms_slices_sum(a.pb, g, a.Z);
        if (threadIdx.x) return;
        S.n2b = sqrt(sy + a.r * sz);
        S.tolb = a.tol * S.n2b;
        S.ny2 = sy;
        q.beta = sqrt(su + sb);
        q.normr = q.beta;
        q.ub = q.beta != 0.0 ? 1.0 / q.beta : 1.0;
        q.c = 1.0; q.s = 0.0; q.phibar = q.beta; q.norma = 0.0; q.phi = 0.0; q.thet = 0.0; q.rho = 1.0; q.alpha = 0.0;
        S.pad = 0; S.iter = a.maxit; S.flag = 1; S.done = 0;
        sms_publish(a, g, S, true);
    } else if (stage == SC_BETA) {
        const double sb = sms_slices_sum(a.pb, g, a.Z);
        if (threadIdx.x) return;
        const double beta = sqrt(su + sb), alpha = q.alpha;
        q.beta = beta;
        q.ub = 1.0 / beta;
        q.norma = sqrt(q.norma * q.norma + alpha * alpha + beta * beta);
        const double thet = -q.s * alpha, rhot = q.c * alpha, rho = sqrt(rhot * rhot + beta * beta);
        q.thet = thet; q.rho = rho;
        q.c = rhot / rho;
        q.s = -beta / rho;
        q.phi = q.c * q.phibar;
        if (q.phi == 0.0) S.pad = 1;
        q.phibar = q.s * q.phibar;
        sms_publish(a, g, S, false);
    } else if (stage == SC_STOP) {
        const double sd = sms_slices_sum(a.pd, g, a.Z), sx = sms_slices_sum(a.px, g, a.Z);
        if (threadIdx.x) return;
        if (fabs(q.phi) * sqrt(sd) < DBL_EPSILON * sqrt(sx)) S.pad++; else S.pad = 0;
        if (q.factor / (q.norma * q.normr) <= a.tol || q.normr <= S.tolb) { S.done = 1; S.iter = a.ii - 1; S.flag = 0; }
        else if (S.pad >= 3) { S.done = 1; S.iter = a.ii - 1; S.flag = 3; }
        else q.normr = fabs(q.s) * q.normr;
        sms_publish(a, g, S, S.done != 0);
    } else {   // SC_ALPHA
        const double sv = sms_slices_sum(a.pv, g, a.Z);
        if (threadIdx.x) return;
        const double alpha = sqrt(sv);
        q.alpha = alpha;
        if (a.ii == 0) {
            q.ua = alpha != 0.0 ? 1.0 / alpha : 1.0;
            q.factor = alpha * q.beta;
            if (q.factor == 0.0 || S.n2b == 0.0) { S.done = 1; S.iter = 0; S.flag = 0; }
            else if (a.maxit == 0) { S.done = 1; S.iter = 0; S.flag = 1; }
        } else {
            q.ua = 1.0 / alpha;
            q.factor = alpha * fabs(q.s * q.phi);
            if (a.ii == a.maxit) { S.done = 1; S.iter = a.maxit; S.flag = 1; }
        }
        sms_publish(a, g, S, S.done != 0);
    }
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + NT - 1) / NT); }

// E and the frame table go to the device at the first call that needs them (qmri_set_sms itself is host work)
int sms_upload(qmri_ctx* ctx) {
    OpHost& o = ctx->op;
    SmsWork& w = o.sms;
    if (w.on_device) return QMRI_OK;
    const std::vector<int32_t> frame = sms::frame_table(o.T, o.frame_ptr.data());
    QMRI_TRY(w.d_E.ensure(ctx, w.E.size()));
    QMRI_TRY(w.d_frame.ensure(ctx, frame.size()));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    QMRI_HIP(ctx, hipMemcpy(w.d_E, w.E.data(), w.E.size() * sizeof(double2), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(w.d_frame, frame.data(), frame.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipDeviceSynchronize());                        // (as in qmri_set_operator: the copies must have landed before this context's stream reads them)
    w.on_device = true;
    return QMRI_OK;
}

// the buffers of G groups of ncoil coils, each grown only when its own need grows: the transform chunks' images and the sum over slices for the
// operator calls, and with `solve` the LSQR's vectors, partials and states
int sms_ensure_work(qmri_ctx* ctx, int G, int ncoil, bool solve) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    SmsWork& sw = o.sms;
    const size_t units = (size_t)G * ncoil, sl = (size_t)G * sw.Z, n = (size_t)o.N * o.M * o.s;
    const int st = [&]() -> int {
        QMRI_TRY(sms_upload(ctx));
        QMRI_TRY(w.scr.ensure(ctx, (size_t)o.maxB * n));
        QMRI_TRY(sw.ex.ensure(ctx, (size_t)o.maxB * o.m));
        QMRI_TRY(sw.acc.ensure(ctx, units * o.m));
        if (!solve) return QMRI_OK;
        QMRI_TRY(w.ut.ensure(ctx, units * o.m));
        for (DevArr<double2>* a : {&w.ub, &w.v, &w.d, &w.t}) QMRI_TRY(a->ensure(ctx, sl * n));
        QMRI_TRY(w.part.ensure(ctx, sms::parts(G, sw.Z, ncoil).total));
        QMRI_TRY(w.st.ensure(ctx, sl));
        QMRI_TRY(sw.st.ensure(ctx, (size_t)G));
        return sw.hst.ensure(ctx, (size_t)G);
    }();
    if (st == QMRI_ERR_NOMEM) qmri_set_error(ctx, "out of device memory for %d simultaneous multi-slice groups of %d slices x %d coils", G, sw.Z, ncoil);
    return st;
}

// A_sms x chunk by chunk, each chunk's measurements straight into k_sms_combine (y: INIT only; st: ITER only; pu / py: not PLAIN)
int sms_forward_chunks(qmri_ctx* ctx, int mode, int G, int ncoil, const double2* maps, const double2* x, const double2* y, const LsqrState* st,
                       double2* ut, double* pu, double* py) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    const SmsWork& sw = o.sms;
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    for (const sms::Chunk& c : sms::chunk_schedule(G * ncoil, sw.Z, o.maxB)) {
        k_sms_coil_mul<<<dim3(blocks_of(n), c.cnt), dim3(NT), 0, ctx->stream>>>(n, plane, ncoil, sw.Z, c.q0, x, maps, st, w.scr);
        QMRI_HIP(ctx, hipGetLastError());
        if (o.kind == OP_NUFFT) QMRI_TRY(nufft_launch_fwd(ctx, c.cnt, w.scr, o.d_ya));
        else QMRI_TRY(dc_launch_fwd(ctx, qmri_opdev(ctx), o.ls, DC_PLAIN, c.cnt, w.scr, o.d_tmp, o.d_ya, nullptr));
        k_sms_combine<<<dim3(PC, c.nu), dim3(NT), 0, ctx->stream>>>(mode, (size_t)o.m, ncoil, sw.Z, o.T, c.q0, c.cnt, o.d_ya, y, sw.d_frame, sw.d_E, st, ut,
                                                                    sw.acc, pu, py);
        QMRI_HIP(ctx, hipGetLastError());
    }
    return QMRI_OK;
}
// A_sms' (one row of u per (g, j)) into t [G Z][n], chunk by chunk.  st: the groups' states (k_sms_expand); sv: their copies per slice vector (k_mcl_coil_sum)
int sms_adjoint_chunks(qmri_ctx* ctx, int G, int ncoil, const double2* maps, const double2* ut, const LsqrState* st, const LsqrState* sv, double2* t) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    const SmsWork& sw = o.sms;
    for (const sms::Chunk& c : sms::chunk_schedule(G * sw.Z, ncoil, o.maxB)) {
        k_sms_expand<<<dim3(blocks_of((size_t)o.m), c.cnt), dim3(NT), 0, ctx->stream>>>((size_t)o.m, ncoil, sw.Z, o.T, c.q0, ut, sw.d_frame, sw.d_E, st, sw.ex);
        QMRI_HIP(ctx, hipGetLastError());
        if (o.kind == OP_NUFFT) QMRI_TRY(nufft_launch_adj(ctx, c.cnt, sw.ex, w.scr));
        else QMRI_TRY(dc_launch_adj(ctx, qmri_opdev(ctx), c.cnt, sw.ex, o.d_tmp, w.scr));
        QMRI_TRY(mc_launch_coil_sum(ctx, ncoil, c.q0, c.cnt, w.scr, maps, sv, t));
    }
    return QMRI_OK;
}
int sms_scalar(qmri_ctx* ctx, int stage, int G, const ScalarArgs& a) {
    k_sms_scalar<<<dim3(G), dim3(64), 0, ctx->stream>>>(stage, a);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
}  // namespace

int sms_forward_dev(qmri_ctx* ctx, int G, int ncoil, const double2* d_maps, const double2* d_x, double2* d_y) {
    QMRI_TRY(sms_ensure_work(ctx, G, ncoil, false));
    return sms_forward_chunks(ctx, SMS_PLAIN, G, ncoil, d_maps, d_x, nullptr, nullptr, d_y, nullptr, nullptr);
}

int sms_adjoint_dev(qmri_ctx* ctx, int G, int ncoil, const double2* d_maps, const double2* d_y, double2* d_x) {
    QMRI_TRY(sms_ensure_work(ctx, G, ncoil, false));
    return sms_adjoint_chunks(ctx, G, ncoil, d_maps, d_y, nullptr, nullptr, d_x);
}

// d_maps: [G][Z][ncoil][N*M], d_y: [G][ncoil][m] (the ABI's frame-major order), d_z / d_x: [G][Z][n].  iters_out / flags_out: [G] (nullable).  The
// event-chunked driver of qmri_lsqr_mc_batch_dev: one wait after the initial step, then one per chunk of iterations.
int sms_lsqr_dev(qmri_ctx* ctx, int G, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                 double2* d_x, int32_t* iters_out, int32_t* flags_out) {
    OpHost& o = ctx->op;
    QMRI_TRY(sms_ensure_work(ctx, G, ncoil, true));
    McWork& w = o.mc;
    SmsWork& sw = o.sms;
    const int Z = sw.Z, B = G * Z;
    const double sr = std::sqrt(r);
    const sms::Parts po = sms::parts(G, Z, ncoil);
    double* const base = w.part;
    double *pu = base + po.pu, *py = base + po.py, *pb = base + po.pb, *pz = base + po.pz, *pd = base + po.pd, *px = base + po.px, *pv = base + po.pv;
    ScalarArgs a{sw.st, w.st, sw.hst, pu, py, pb, pz, pd, px, pv, ncoil, Z, 0, maxit, tol, r};
    // u = b - B x0, v = B' u
    QMRI_TRY(mc_launch_ub(ctx, 0, B, sr, d_z, d_x, w.st, w.ub, w.v, w.d, pb, pz));
    QMRI_TRY(sms_forward_chunks(ctx, SMS_INIT, G, ncoil, d_maps, d_x, d_y, nullptr, w.ut, pu, py));
    QMRI_TRY(sms_scalar(ctx, SC_BETA0, G, a));
    QMRI_TRY(sms_adjoint_chunks(ctx, G, ncoil, d_maps, w.ut, sw.st, w.st, w.t));
    QMRI_TRY(mc_launch_vupd(ctx, 0, B, sr, w.t, w.ub, w.d, w.st, d_x, w.v, pv));
    QMRI_TRY(sms_scalar(ctx, SC_ALPHA, G, a));
    if (!ctx->ev_state) QMRI_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_state, hipEventDisableTiming));
    QMRI_HIP(ctx, hipEventRecord(ctx->ev_state, ctx->stream));
    QMRI_HIP(ctx, hipEventSynchronize(ctx->ev_state));
    bool any = false;
    for (int g = 0; g < G; ++g) any |= !sw.hst[g].done;
    int ii = 1, chunk = std::max(1, std::min(maxit, sw.pred));
    for (; any;) {
        const int last = std::min(maxit, ii + chunk - 1);
        for (; ii <= last; ++ii) {
            a.ii = ii;
            QMRI_TRY(mc_launch_ub(ctx, 1, B, sr, nullptr, nullptr, w.st, w.ub, w.v, nullptr, pb, nullptr));
            QMRI_TRY(sms_forward_chunks(ctx, SMS_ITER, G, ncoil, d_maps, w.v, nullptr, sw.st, w.ut, pu, py));
            QMRI_TRY(sms_scalar(ctx, SC_BETA, G, a));
            QMRI_TRY(mc_launch_dupd(ctx, B, w.v, d_x, w.st, w.d, pd, px));
            QMRI_TRY(sms_scalar(ctx, SC_STOP, G, a));
            QMRI_TRY(sms_adjoint_chunks(ctx, G, ncoil, d_maps, w.ut, sw.st, w.st, w.t));
            QMRI_TRY(mc_launch_vupd(ctx, 1, B, sr, w.t, w.ub, w.d, w.st, d_x, w.v, pv));
            QMRI_TRY(sms_scalar(ctx, SC_ALPHA, G, a));
        }
        QMRI_HIP(ctx, hipEventRecord(ctx->ev_state, ctx->stream));
        QMRI_HIP(ctx, hipEventSynchronize(ctx->ev_state));
        bool active = false;
        for (int g = 0; g < G; ++g) active |= !sw.hst[g].done;
        if (!active || ii > maxit) break;
        chunk = std::max(2, sw.pred / 4);
    }
    int most = 0;
    for (int g = 0; g < G; ++g) {
        if (iters_out) iters_out[g] = sw.hst[g].iter;
        if (flags_out) flags_out[g] = sw.hst[g].flag;
        most = std::max(most, (int)sw.hst[g].iter);
    }
    sw.pred = std::max(1, most + 1);
    return QMRI_OK;
}
