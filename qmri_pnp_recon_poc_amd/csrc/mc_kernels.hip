// mc_kernels.hip -- multi-coil x-update of PnP-ADMM: an EXTENSION (BASELINE.json configs[4] names a "complex-valued multi-coil forward op").
//
// The reference simulates a single coil (README.md:63) and has no multi-coil operator, so nothing here has a reference counterpart and nothing can pin
// it: PARITY UNPINNED, stated in include/qmri.h and in the oracle's restatement.  What it generalises is the one line PnP_ADMM.m:102
//     x = lsqr(@afun, [y; sqrt(r) z], cg_tol, cg_iter, [], [], x0),   afun: B = [A; sqrt(r) I]  (PnP_ADMM.m:153-171)
// with A replaced by the SENSE operator of api_operator.cpp (qmri_forward_mc / qmri_adjoint_mc):  A_mc x = [A (C_j . x)]_j,  A_mc' y = sum_j conj(C_j) . A' y_j.
// Coil maps act in image space, so A_mc'A_mc is no longer block-diagonal in k-space and the k-space iteration of kslsqr_kernels.hip does not apply:
// this is the image-domain LSQR, the recurrences, stop rules and their order exactly as oracle/orc_lsqr.c restates MATLAB's lsqr.
//
// B slices per call, each with its own maps ([B][ncoil][N*M]).  The "coil images" of all slices (g = b * ncoil + j) go through the batched transforms
// of dc_kernels.hip max_batch at a time; a chunk may span slices.  Every LSQR scalar lives on the device, in one LsqrState per slice (sc[0] only):
//     sc[0].c, s, phibar, normr, norma, thet, rho, phi, alpha, beta   the recurrences
//     sc[0].factor = normar,  sc[0].ua = 1 / alpha,  sc[0].ub = 1 / beta,  pad = stagnation counter,  iter / done / flag as the k-space solver's
// u and v are kept UNSCALED: the 1 / beta and 1 / alpha of lsqr's normalisations are multiplied in by the next kernel that reads them.  The small
// k_mcl_scalar launches (one wave per slice) do the recurrences and the stop tests and mirror iter / done / flag to pinned host memory; the host
// enqueues a predicted number of iterations, waits on ONE event and reads the flags (qmri_lsqr_mc_batch_dev).  A slice that has stopped is frozen: every
// kernel tests its slice's done flag (uniform per workgroup) and leaves x, u, v, d alone.
//
// Reductions: every norm is summed from fixed per-vector partials -- PS workgroups per slice vector, PC per coil image, whatever B or the chunking --
// added in one fixed order by k_mcl_scalar.  No floating-point atomics.  So a slice's x-update is bit-identical alone or at any position in any batch,
// with any max_batch.  (The conjugate coil sum accumulates coil j after coil j - 1 in fp64 whichever chunk holds them: the same bits too.)
#include <cfloat>
#include <cmath>
#include <vector>
#include "qmri_internal.h"

namespace {
constexpr int NT = 256;          // threads per workgroup of the streaming kernels
constexpr int PS = MC_PS;        // partial sums per slice vector (n complex)
constexpr int PC = MC_PC;        // partial sums per coil image (m complex)
enum { MCL_INIT = 0, MCL_ITER = 1 };
enum { SC_BETA0 = 0, SC_BETA = 1, SC_STOP = 2, SC_ALPHA = 3 };

// partial-sum slots of one solve (McWork::part): [img][PC] |u_j|^2, [img][PC] |y_j|^2, then [B][PS] each of |u2|^2, |z|^2, |d|^2, |x|^2, |v|^2
struct McParts {
    double *pu, *py, *pb, *pz, *pd, *px, *pv;
};
McParts mc_parts(double* base, int B, int ncoil) {
    McParts p;
    const size_t img = (size_t)B * ncoil * PC, sl = (size_t)B * PS;
    p.pu = base; p.py = p.pu + img; p.pb = p.py + img; p.pz = p.pb + sl; p.pd = p.pz + sl; p.px = p.pd + sl; p.pv = p.px + sl;
    return p;
}

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
__device__ __forceinline__ bool frozen(const LsqrState* st, int b) { return st && st[b].done; }
__device__ __forceinline__ double2 cmul(double2 c, double2 v) { return make_double2(c.x * v.x - c.y * v.y, c.x * v.y + c.y * v.x); }

// out[j][i] = maps[g0 + j][i % plane] * x[b][i],  b = (g0 + j) / ncoil    (grid: n / NT x cnt)
__global__ __launch_bounds__(NT) void k_mcl_coil_mul(size_t n, size_t plane, int ncoil, int g0, const double2* __restrict__ x,
                                                     const double2* __restrict__ maps, const LsqrState* __restrict__ st, double2* __restrict__ out) {
    const int g = g0 + blockIdx.y, b = g / ncoil;
    if (frozen(st, b)) return;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    out[(size_t)blockIdx.y * n + i] = cmul(maps[(size_t)g * plane + i % plane], x[(size_t)b * n + i]);
}
// t[b][i] (+)= sum over the chunk's coils j of slice b, ascending, of conj(maps[g][px]) * xj[g - g0][i]   (grid: n / NT x slices the chunk touches)
__global__ __launch_bounds__(NT) void k_mcl_coil_sum(size_t n, size_t plane, int ncoil, int g0, int cnt, const double2* __restrict__ xj,
                                                     const double2* __restrict__ maps, const LsqrState* __restrict__ st, double2* __restrict__ t) {
    const int b = g0 / ncoil + blockIdx.y;
    if (frozen(st, b)) return;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int lo = max(g0, b * ncoil), hi = min(g0 + cnt, (b + 1) * ncoil);
    const size_t px = i % plane;
    double2 a = lo > b * ncoil ? t[(size_t)b * n + i] : make_double2(0.0, 0.0);
    for (int g = lo; g < hi; ++g) {
        const double2 c = maps[(size_t)g * plane + px], v = xj[(size_t)(g - g0) * n + i];
        a.x += c.x * v.x + c.y * v.y;                              // conj(c) * v
        a.y += c.x * v.y - c.y * v.x;
    }
    t[(size_t)b * n + i] = a;
}
// measurement half of u, one coil image per blockIdx.y (grid: PC x cnt), m complex each:
//   INIT  u_j = y_j - (A C_j x0),  partials |u_j|^2 and |y_j|^2
//   ITER  u_j = (A C_j v) - (alpha / beta) u_j
__global__ __launch_bounds__(NT) void k_mcl_ulin(int mode, size_t m, int ncoil, int g0, const double2* __restrict__ ya, const double2* __restrict__ y,
                                                 const LsqrState* __restrict__ st, double2* __restrict__ ut, double* __restrict__ pu, double* __restrict__ py) {
    __shared__ double sh[NT / 64];
    const int g = g0 + blockIdx.y, b = g / ncoil;
    if (frozen(st, b)) return;
    const double coef = mode == MCL_ITER ? st[b].sc[0].alpha * st[b].sc[0].ub : 0.0;
    const double2* a = ya + (size_t)blockIdx.y * m;
    double2* u = ut + (size_t)g * m;
    double su = 0.0, sy = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < m; i += (size_t)PC * NT) {
        const double2 av = a[i];
        double2 w;
        if (mode == MCL_INIT) {
            const double2 yv = y[(size_t)g * m + i];
            w = make_double2(yv.x - av.x, yv.y - av.y);
            sy += yv.x * yv.x + yv.y * yv.y;
        } else {
            const double2 uv = u[i];
            w = make_double2(av.x - coef * uv.x, av.y - coef * uv.y);
        }
        u[i] = w;
        su += w.x * w.x + w.y * w.y;
    }
    su = block_sum(su, sh);
    if (mode == MCL_INIT) sy = block_sum(sy, sh);
    if (threadIdx.x == 0) {
        pu[(size_t)g * PC + blockIdx.x] = su;
        if (mode == MCL_INIT) py[(size_t)g * PC + blockIdx.x] = sy;
    }
}
// image half of u, per slice (grid: PS x B):
//   INIT  u2 = sr z - sr x0,  d = 0,  partials |u2|^2 and |z|^2
//   ITER  v = v / alpha (stored scaled from here on),  u2 = sr v - (alpha / beta) u2,  partial |u2|^2
__global__ __launch_bounds__(NT) void k_mcl_ub(int mode, size_t n, double sr, const double2* __restrict__ z, const double2* __restrict__ x,
                                               const LsqrState* __restrict__ st, double2* __restrict__ ub, double2* __restrict__ v, double2* __restrict__ d,
                                               double* __restrict__ pb, double* __restrict__ pz) {
    __shared__ double sh[NT / 64];
    const int b = blockIdx.y;
    if (mode == MCL_ITER && frozen(st, b)) return;
    const size_t o = (size_t)b * n;
    double ia = 0.0, coef = 0.0;
    if (mode == MCL_ITER) { ia = st[b].sc[0].ua; coef = st[b].sc[0].alpha * st[b].sc[0].ub; }
    double sb = 0.0, szz = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        double2 w;
        if (mode == MCL_INIT) {
            const double2 zv = z[o + i], xv = x[o + i];
            w = make_double2(zv.x * sr - xv.x * sr, zv.y * sr - xv.y * sr);
            d[o + i] = make_double2(0.0, 0.0);
            szz += zv.x * zv.x + zv.y * zv.y;
        } else {
            double2 vv = v[o + i];
            vv = make_double2(vv.x * ia, vv.y * ia);
            v[o + i] = vv;
            const double2 uv = ub[o + i];
            w = make_double2(vv.x * sr - coef * uv.x, vv.y * sr - coef * uv.y);
        }
        ub[o + i] = w;
        sb += w.x * w.x + w.y * w.y;
    }
    sb = block_sum(sb, sh);
    if (mode == MCL_INIT) szz = block_sum(szz, sh);
    if (threadIdx.x == 0) {
        pb[(size_t)b * PS + blockIdx.x] = sb;
        if (mode == MCL_INIT) pz[(size_t)b * PS + blockIdx.x] = szz;
    }
}
// d = (v - thet d) / rho, partials |d|^2 and |x|^2 (x before this iteration's update: the stagnation test)   (grid: PS x B)
__global__ __launch_bounds__(NT) void k_mcl_dupd(size_t n, const double2* __restrict__ v, const double2* __restrict__ x, const LsqrState* __restrict__ st,
                                                 double2* __restrict__ d, double* __restrict__ pd, double* __restrict__ px) {
    __shared__ double sh[NT / 64];
    const int b = blockIdx.y;
    if (frozen(st, b)) return;
    const size_t o = (size_t)b * n;
    const double thet = st[b].sc[0].thet, rho = st[b].sc[0].rho;
    double a = 0.0, c = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        const double2 vv = v[o + i], dv = d[o + i], xv = x[o + i];
        const double2 w = make_double2((vv.x - thet * dv.x) / rho, (vv.y - thet * dv.y) / rho);
        d[o + i] = w;
        a += w.x * w.x + w.y * w.y;
        c += xv.x * xv.x + xv.y * xv.y;
    }
    a = block_sum(a, sh);
    c = block_sum(c, sh);
    if (threadIdx.x == 0) { pd[(size_t)b * PS + blockIdx.x] = a; px[(size_t)b * PS + blockIdx.x] = c; }
}
// the x update of the iteration that passed its stop tests, fused with the next v (grid: PS x B):
//   INIT  v = t / beta + sr u2 / beta
//   ITER  x += phi d,  v = t / beta + sr u2 / beta - beta v
// partial |v|^2 (v unscaled: the next k_mcl_ub divides by alpha)
__global__ __launch_bounds__(NT) void k_mcl_vupd(int mode, size_t n, double sr, const double2* __restrict__ t, const double2* __restrict__ ub,
                                                 const double2* __restrict__ d, const LsqrState* __restrict__ st, double2* __restrict__ x,
                                                 double2* __restrict__ v, double* __restrict__ pv) {
    __shared__ double sh[NT / 64];
    const int b = blockIdx.y;
    if (frozen(st, b)) return;
    const size_t o = (size_t)b * n;
    const double ib = st[b].sc[0].ub, beta = st[b].sc[0].beta, phi = st[b].sc[0].phi;
    double a = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)PS * NT) {
        const double2 tv = t[o + i], uv = ub[o + i];
        double2 w = make_double2(tv.x * ib + uv.x * ib * sr, tv.y * ib + uv.y * ib * sr);
        if (mode == MCL_ITER) {
            const double2 dv = d[o + i], xv = x[o + i], vv = v[o + i];
            x[o + i] = make_double2(xv.x + phi * dv.x, xv.y + phi * dv.y);
            w = make_double2(w.x - beta * vv.x, w.y - beta * vv.y);
        }
        v[o + i] = w;
        a += w.x * w.x + w.y * w.y;
    }
    a = block_sum(a, sh);
    if (threadIdx.x == 0) pv[(size_t)b * PS + blockIdx.x] = a;
}

struct ScalarArgs { LsqrState* st; LsqrState* hst; McParts p; int ncoil, ii, maxit; double tol, r; };
__device__ void mcl_tell(const ScalarArgs& a, int b, const LsqrState& s) {
    if (threadIdx.x == 0 && a.hst) { LsqrState* h = a.hst + b; h->iter = s.iter; h->flag = s.flag; h->done = s.done; }
}
// the recurrences of orc_lsqr.c between the vector kernels, one wave per slice (grid: B x 64)
__global__ __launch_bounds__(64) void k_mcl_scalar(int stage, ScalarArgs a) {
    const int b = blockIdx.x;
    LsqrState& S = a.st[b];
    LsqrScalars& q = S.sc[0];
    if (stage != SC_BETA0 && S.done) return;
    double su = 0.0;
    if (stage == SC_BETA0 || stage == SC_BETA)
        for (int j = 0; j < a.ncoil; ++j) su += wave_sum(a.p.pu + ((size_t)b * a.ncoil + j) * PC, PC);
    if (stage == SC_BETA0) {
        double sy = 0.0;
        for (int j = 0; j < a.ncoil; ++j) sy += wave_sum(a.p.py + ((size_t)b * a.ncoil + j) * PC, PC);
        const double sz = wave_sum(a.p.pz + (size_t)b * PS, PS), sb = wave_sum(a.p.pb + (size_t)b * PS, PS);
        if (threadIdx.x) return;
        S.n2b = sqrt(sy + a.r * sz);
        S.tolb = a.tol * S.n2b;
        S.ny2 = sy;
        q.beta = sqrt(su + sb);
        q.normr = q.beta;
        q.ub = q.beta != 0.0 ? 1.0 / q.beta : 1.0;
        q.c = 1.0; q.s = 0.0; q.phibar = q.beta; q.norma = 0.0; q.phi = 0.0; q.thet = 0.0; q.rho = 1.0; q.alpha = 0.0;
        S.pad = 0; S.iter = a.maxit; S.flag = 1; S.done = 0;
        mcl_tell(a, b, S);
    } else if (stage == SC_BETA) {
        const double sb = wave_sum(a.p.pb + (size_t)b * PS, PS);
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
    } else if (stage == SC_STOP) {
        const double sd = wave_sum(a.p.pd + (size_t)b * PS, PS), sx = wave_sum(a.p.px + (size_t)b * PS, PS);
        if (threadIdx.x) return;
        if (fabs(q.phi) * sqrt(sd) < DBL_EPSILON * sqrt(sx)) S.pad++; else S.pad = 0;
        if (q.factor / (q.norma * q.normr) <= a.tol || q.normr <= S.tolb) { S.done = 1; S.iter = a.ii - 1; S.flag = 0; }
        else if (S.pad >= 3) { S.done = 1; S.iter = a.ii - 1; S.flag = 3; }
        else q.normr = fabs(q.s) * q.normr;
        if (S.done) mcl_tell(a, b, S);
    } else {   // SC_ALPHA
        const double sv = wave_sum(a.p.pv + (size_t)b * PS, PS);
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
        if (S.done) mcl_tell(a, b, S);
    }
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + NT - 1) / NT); }

// A_mc' (one coil image per row of u) into t, chunk by chunk
int mc_adjoint_chunks(qmri_ctx* ctx, int B, int ncoil, const double2* maps, const double2* ut, const LsqrState* st, double2* t) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    for (int g0 = 0; g0 < B * ncoil; g0 += o.maxB) {
        const int cnt = std::min(o.maxB, B * ncoil - g0), nb = (g0 + cnt - 1) / ncoil - g0 / ncoil + 1;
        if (o.kind == OP_NUFFT) QMRI_TRY(nufft_launch_adj(ctx, cnt, ut + (size_t)g0 * o.m, w.scr));
        else QMRI_TRY(dc_launch_adj(ctx, qmri_opdev(ctx), cnt, ut + (size_t)g0 * o.m, o.d_tmp, w.scr));
        k_mcl_coil_sum<<<dim3(blocks_of(n), nb), dim3(NT), 0, ctx->stream>>>(n, plane, ncoil, g0, cnt, w.scr, maps, st, t);
        QMRI_HIP(ctx, hipGetLastError());
    }
    return QMRI_OK;
}
// A_mc x chunk by chunk, each chunk's measurements straight into k_mcl_ulin
int mc_forward_chunks(qmri_ctx* ctx, int mode, int B, int ncoil, const double2* maps, const double2* x, const double2* y, const LsqrState* st, const McParts& p) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    for (int g0 = 0; g0 < B * ncoil; g0 += o.maxB) {
        const int cnt = std::min(o.maxB, B * ncoil - g0);
        k_mcl_coil_mul<<<dim3(blocks_of(n), cnt), dim3(NT), 0, ctx->stream>>>(n, plane, ncoil, g0, x, maps, st, w.scr);
        QMRI_HIP(ctx, hipGetLastError());
        if (o.kind == OP_NUFFT) QMRI_TRY(nufft_launch_fwd(ctx, cnt, w.scr, o.d_ya));
        else QMRI_TRY(dc_launch_fwd(ctx, qmri_opdev(ctx), o.ls, DC_PLAIN, cnt, w.scr, o.d_tmp, o.d_ya, nullptr));
        k_mcl_ulin<<<dim3(PC, cnt), dim3(NT), 0, ctx->stream>>>(mode, (size_t)o.m, ncoil, g0, o.d_ya, y, st, w.ut, p.pu, p.py);
        QMRI_HIP(ctx, hipGetLastError());
    }
    return QMRI_OK;
}
int mc_scalar(qmri_ctx* ctx, int stage, int B, const ScalarArgs& a) {
    k_mcl_scalar<<<dim3(B), dim3(64), 0, ctx->stream>>>(stage, a);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
}  // namespace

int mc_launch_coil_mul(qmri_ctx* ctx, int ncoil, int g0, int cnt, const double2* x, const double2* maps, const LsqrState* st, double2* out) {
    const OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    k_mcl_coil_mul<<<dim3(blocks_of(n), cnt), dim3(NT), 0, ctx->stream>>>(n, plane, ncoil, g0, x, maps, st, out);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
int mc_launch_coil_sum(qmri_ctx* ctx, int ncoil, int g0, int cnt, const double2* xj, const double2* maps, const LsqrState* st, double2* t) {
    const OpHost& o = ctx->op;
    const size_t n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    const int nb = (g0 + cnt - 1) / ncoil - g0 / ncoil + 1;
    k_mcl_coil_sum<<<dim3(blocks_of(n), nb), dim3(NT), 0, ctx->stream>>>(n, plane, ncoil, g0, cnt, xj, maps, st, t);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
// the image-side vector kernels on B slice vectors, one state per vector (mode 0: the initial step, 1: an iteration).  sms_kernels.hip runs them on
// the G Z slice vectors of its groups: the same kernels, so the same bits.
int mc_launch_ub(qmri_ctx* ctx, int mode, int B, double sr, const double2* z, const double2* x, const LsqrState* st, double2* ub, double2* v, double2* d,
                 double* pb, double* pz) {
    const OpHost& o = ctx->op;
    k_mcl_ub<<<dim3(PS, B), dim3(NT), 0, ctx->stream>>>(mode, (size_t)o.N * o.M * o.s, sr, z, x, st, ub, v, d, pb, pz);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
int mc_launch_dupd(qmri_ctx* ctx, int B, const double2* v, const double2* x, const LsqrState* st, double2* d, double* pd, double* px) {
    const OpHost& o = ctx->op;
    k_mcl_dupd<<<dim3(PS, B), dim3(NT), 0, ctx->stream>>>((size_t)o.N * o.M * o.s, v, x, st, d, pd, px);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
int mc_launch_vupd(qmri_ctx* ctx, int mode, int B, double sr, const double2* t, const double2* ub, const double2* d, const LsqrState* st, double2* x,
                   double2* v, double* pv) {
    const OpHost& o = ctx->op;
    k_mcl_vupd<<<dim3(PS, B), dim3(NT), 0, ctx->stream>>>(mode, (size_t)o.N * o.M * o.s, sr, t, ub, d, st, x, v, pv);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

// work buffers of a B-slice, ncoil-coil solve: allocated on first use, each grown only when its own need grows (they go with the operator)
int mc_ensure_work(qmri_ctx* ctx, int B, int ncoil) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    const size_t sl = (size_t)B, img = sl * ncoil, n = (size_t)o.N * o.M * o.s;
    const int st = [&]() -> int {
        QMRI_TRY(w.ut.ensure(ctx, img * o.m));
        for (DevArr<double2>* a : {&w.ub, &w.v, &w.d, &w.t}) QMRI_TRY(a->ensure(ctx, sl * n));
        QMRI_TRY(w.scr.ensure(ctx, (size_t)o.maxB * n));
        QMRI_TRY(w.part.ensure(ctx, 2 * img * PC + 5 * sl * PS));
        QMRI_TRY(w.st.ensure(ctx, sl));
        return w.hst.ensure(ctx, sl);
    }();
    if (st == QMRI_ERR_NOMEM) qmri_set_error(ctx, "out of device memory for the multi-coil LSQR of %d slices x %d coils", B, ncoil);
    return st;
}

// staging of host-array calls: maps, y, x, z (or x0) for B slices of ncoil coils, each grown only when its own need grows
int mc_ensure_staging(qmri_ctx* ctx, int B, int ncoil) {
    OpHost& o = ctx->op;
    McWork& w = o.mc;
    const size_t sl = (size_t)B, img = sl * ncoil, n = (size_t)o.N * o.M * o.s, plane = (size_t)o.N * o.M;
    const int st = [&]() -> int {
        QMRI_TRY(w.sy.ensure(ctx, img * o.m));
        QMRI_TRY(w.sm.ensure(ctx, img * plane));
        QMRI_TRY(w.sx.ensure(ctx, sl * n));
        return w.sz.ensure(ctx, sl * n);
    }();
    if (st == QMRI_ERR_NOMEM) qmri_set_error(ctx, "out of device memory for the staging of %d slices x %d coils", B, ncoil);
    return st;
}

// x = A_mc' y for B slices (the ADMM loop's start, PnP_ADMM.m:84)
int mc_adjoint_batch_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_maps, const double2* d_y, double2* d_x) {
    QMRI_TRY(mc_ensure_work(ctx, B, ncoil));                   // (the chunks' coil images go through McWork::scr)
    return mc_adjoint_chunks(ctx, B, ncoil, d_maps, d_y, nullptr, d_x);
}

// LSQR on [A_mc; sqrt(r) I] x = [y; sqrt(r) z] for B slices from x0 = d_x (device, overwritten with the solutions).  d_maps: [B][ncoil][N*M],
// d_y: [B][ncoil][m] (the ABI's frame-major order), d_z / d_x: [B][n].  iters_out / flags_out: [B] (nullable).
int qmri_lsqr_mc_batch_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                           double2* d_x, int32_t* iters_out, int32_t* flags_out) {
    OpHost& o = ctx->op;
    QMRI_TRY(mc_ensure_work(ctx, B, ncoil));
    McWork& w = o.mc;
    const size_t n = (size_t)o.N * o.M * o.s;
    const double sr = std::sqrt(r);
    const McParts p = mc_parts(w.part, B, ncoil);
    ScalarArgs a{w.st, w.hst, p, ncoil, 0, maxit, tol, r};
    const dim3 gs(PS, B);
    // u = b - B x0, v = B' u
    k_mcl_ub<<<gs, dim3(NT), 0, ctx->stream>>>(MCL_INIT, n, sr, d_z, d_x, w.st, w.ub, w.v, w.d, p.pb, p.pz);
    QMRI_HIP(ctx, hipGetLastError());
    QMRI_TRY(mc_forward_chunks(ctx, MCL_INIT, B, ncoil, d_maps, d_x, d_y, nullptr, p));
    QMRI_TRY(mc_scalar(ctx, SC_BETA0, B, a));
    QMRI_TRY(mc_adjoint_chunks(ctx, B, ncoil, d_maps, w.ut, w.st, w.t));
    k_mcl_vupd<<<gs, dim3(NT), 0, ctx->stream>>>(MCL_INIT, n, sr, w.t, w.ub, w.d, w.st, d_x, w.v, p.pv);
    QMRI_HIP(ctx, hipGetLastError());
    QMRI_TRY(mc_scalar(ctx, SC_ALPHA, B, a));
    // iterations in chunks: the first as many as the last solve needed, then a quarter of that (>= 2) at a time; one event wait per chunk.  The
    // transforms run on every coil image of a chunk whether or not its slice is still active, so the host first waits for the initial step: a
    // batch that stops at iteration 0 (y = 0, or z = x0 with A x0 = y) queues no iteration at all.
    if (!ctx->ev_state) QMRI_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_state, hipEventDisableTiming));
    QMRI_HIP(ctx, hipEventRecord(ctx->ev_state, ctx->stream));
    QMRI_HIP(ctx, hipEventSynchronize(ctx->ev_state));
    bool any = false;
    for (int b = 0; b < B; ++b) any |= !w.hst[b].done;
    int ii = 1, chunk = std::max(1, std::min(maxit, w.pred));
    for (; any;) {
        const int last = std::min(maxit, ii + chunk - 1);
        for (; ii <= last; ++ii) {
            a.ii = ii;
            k_mcl_ub<<<gs, dim3(NT), 0, ctx->stream>>>(MCL_ITER, n, sr, nullptr, nullptr, w.st, w.ub, w.v, nullptr, p.pb, nullptr);
            QMRI_HIP(ctx, hipGetLastError());
            QMRI_TRY(mc_forward_chunks(ctx, MCL_ITER, B, ncoil, d_maps, w.v, nullptr, w.st, p));
            QMRI_TRY(mc_scalar(ctx, SC_BETA, B, a));
            k_mcl_dupd<<<gs, dim3(NT), 0, ctx->stream>>>(n, w.v, d_x, w.st, w.d, p.pd, p.px);
            QMRI_HIP(ctx, hipGetLastError());
            QMRI_TRY(mc_scalar(ctx, SC_STOP, B, a));
            QMRI_TRY(mc_adjoint_chunks(ctx, B, ncoil, d_maps, w.ut, w.st, w.t));
            k_mcl_vupd<<<gs, dim3(NT), 0, ctx->stream>>>(MCL_ITER, n, sr, w.t, w.ub, w.d, w.st, d_x, w.v, p.pv);
            QMRI_HIP(ctx, hipGetLastError());
            QMRI_TRY(mc_scalar(ctx, SC_ALPHA, B, a));
        }
        QMRI_HIP(ctx, hipEventRecord(ctx->ev_state, ctx->stream));
        QMRI_HIP(ctx, hipEventSynchronize(ctx->ev_state));
        bool active = false;
        for (int b = 0; b < B; ++b) active |= !w.hst[b].done;
        if (!active || ii > maxit) break;
        chunk = std::max(2, w.pred / 4);
    }
    int most = 0;
    for (int b = 0; b < B; ++b) {
        if (iters_out) iters_out[b] = w.hst[b].iter;
        if (flags_out) flags_out[b] = w.hst[b].flag;
        most = std::max(most, (int)w.hst[b].iter);
    }
    w.pred = std::max(1, most + 1);
    return QMRI_OK;
}
