// dcf_kernels.hip -- density compensation weights of a trajectory operator (qmri_nufft_dcf), fp64 throughout, gfx950.
//
// The iteration of Pipe & Menon on the operator's own kernel psi = nu_phi (nufft_device.h) and the plan's spreading lists, all samples one set:
//   w_i = 1;   g[k] = sum_j w_j psi(u_j1 - k1) psi(u_j2 - k2);   d_i = sum_k g[k] psi(u_i1 - k1) psi(u_i2 - k2);   w_i <- w_i / d_i
//   k_dcf_spread      the tile / segment walk of k_nu_spread on ONE real channel: per staged sample one weight and the two 16-entry axis rows in
//                     LDS -- no V, no phase, no complex arithmetic.  Split tiles go through k_dcf_reduce (k_nu_reduce's real twin), in segment order.
//   k_dcf_interp_div  one lane per sample in plan order: the w x w gather from g, the division, and the workgroup's partial of max |d - 1|
//   k_dcf_scale       w <- kappa w, permuted to ABI order; the call's iteration count and deviation
// No floating-point atomics and every sum in a fixed order: the weights are the same bits on every call.
// The stop test of iteration k (dev_k <= tol) is read at the START of iteration k + 1, by every workgroup of k_dcf_spread, from the per-workgroup
// partials iteration k left (a maximum: exact in any order); the decision goes to stop[k + 1] for the launches behind it.  A launch reads only what
// an EARLIER launch wrote, so the host enqueues all niter iterations without waiting (the discipline of k_tv_iter, lrtv_kernels.hip).
#include "dc_device.h"
#include "nufft_device.h"

using namespace dcdev;
using namespace nudev;

namespace {

constexpr int DCF_CH = 64;       // samples staged in LDS at a time (as NU_CH)

struct DcfRes { double dev; int32_t iters, clamped; };
struct DcfDev {
    double* w;                   // [m] the weights, plan (sorted) order
    double* g;                   // [2N][2M] the spread weights
    double* part;                // [nslot][256] partial tiles of the split tiles
    double* pd[2];               // [nblk] per-workgroup max |d - 1| of k_dcf_interp_div, by iteration parity
    int32_t* pc;                 // [nblk] samples clamped so far (d <= 0 or non-finite)
    int32_t* stop;               // [niter + 2] stop[k] != 0: iteration k does not run (an earlier one met tol); zeroed by the host
    DcfRes* res;
    int nblk;
};

// max of p[0 .. n) in every thread of the workgroup (values >= 0; a maximum does not depend on the order it is taken in)
__device__ __forceinline__ double block_max(const double* __restrict__ p, int n, double* red) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) v = fmax(v, p[i]);
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(NT) void k_dcf_init(DcfDev d, int m) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e < m) d.w[e] = 1.0;
    if (e < d.nblk) d.pc[e] = 0;
}

// iteration k (1-based): one workgroup per segment; thread (r1, r2) owns grid point (16 t1 + r1, 16 t2 + r2)
__global__ __launch_bounds__(NT) void k_dcf_spread(NufftDev nu, DcfDev d, int k, double tol) {
    __shared__ double wv[DCF_CH];                     // the staged samples' weights
    __shared__ double wl[DCF_CH][2 * NU_TB];          // their kernel values along both axes at the tile's 16 + 16 grid lines (0 outside the window)
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    if (k >= 2) {                                     // the stop test of iteration k - 1 (uniform over the workgroup and over the launch)
        const int was = d.stop[k - 1];
        const double dev = block_max(d.pd[(k - 1) & 1], d.nblk, red);
        const bool skip = was != 0 || dev <= tol;
        if (blockIdx.x == 0 && tid == 0) {
            d.stop[k] = skip;
            if (!was && dev <= tol) { d.res->iters = k - 1; d.res->dev = dev; }
        }
        if (skip) return;
    }
    const NuSeg sg = nu.seg[blockIdx.x];
    const int N = nu.N, M = nu.M;
    const int t1 = sg.tile / nu.ntile2, t2 = sg.tile - t1 * nu.ntile2;
    const int r1 = tid >> 4, r2 = tid & 15;
    const double inv_hw = 1.0 / nu.hw;
    double acc = 0.0;
    for (int i0 = sg.b; i0 < sg.e; i0 += DCF_CH) {
        const int cnt = min(DCF_CH, sg.e - i0);
        __syncthreads();
        if (tid < cnt) wv[tid] = d.w[nu.list[i0 + tid]];
        for (int it = tid; it < cnt * 2 * NU_TB; it += NT) {
            const int j = it / (2 * NU_TB), r = it - j * (2 * NU_TB), ax = r >= NU_TB, rr = r - ax * NU_TB;
            const double2 u = nu.u[nu.list[i0 + j]];
            const double uu = ax ? u.y : u.x;
            const int G = ax ? 2 * M : 2 * N;
            const int k0 = nu_k0(uu, nu.hw);
            const int off = nu_wrap((ax ? t2 : t1) * NU_TB + rr - k0, G);
            wl[j][r] = off < nu.w ? nu_phi(uu - (double)(k0 + off), inv_hw, nu.beta) : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) acc = fma(wl[j][r1] * wl[j][NU_TB + r2], wv[j], acc);
    }
    if (sg.slot >= 0) { d.part[(size_t)sg.slot * NT + tid] = acc; return; }
    d.g[(size_t)(t1 * NU_TB + r1) * 2 * M + (t2 * NU_TB + r2)] = acc;
}

// the partial tiles of a split tile, added in segment order; one workgroup per split tile
__global__ __launch_bounds__(NT) void k_dcf_reduce(NufftDev nu, DcfDev d, int k) {
    if (d.stop[k]) return;
    const NuRed rd = nu.red[blockIdx.x];
    const int tid = threadIdx.x, M = nu.M;
    const int t1 = rd.tile / nu.ntile2, t2 = rd.tile - t1 * nu.ntile2;
    double a = 0.0;
    for (int q = 0; q < rd.nslot; ++q) a += d.part[(size_t)(rd.slot0 + q) * NT + tid];
    d.g[(size_t)(t1 * NU_TB + (tid >> 4)) * 2 * M + (t2 * NU_TB + (tid & 15))] = a;
}

// iteration k: d_e over the sample's w x w window of g (the window and the kernel values of k_nu_interp), w_e <- w_e / d_e
template <int W>
__global__ __launch_bounds__(NT) void k_dcf_interp_div(NufftDev nu, DcfDev d, int k) {
    __shared__ double red[NT];
    __shared__ int redc[NT];
    if (d.stop[k]) return;
    const int tid = threadIdx.x, e = blockIdx.x * NT + tid;
    double dv = 0.0;
    int cl = 0;
    if (e < nu.m) {
        const int N = nu.N, M = nu.M;
        const double2 u = nu.u[e];
        const double inv_hw = 1.0 / nu.hw;
        const int k01 = nu_k0(u.x, nu.hw), k02 = nu_k0(u.y, nu.hw);
        double w1[W], w2[W];
#pragma unroll
        for (int i = 0; i < W; ++i) { w1[i] = nu_phi(u.x - (double)(k01 + i), inv_hw, nu.beta); w2[i] = nu_phi(u.y - (double)(k02 + i), inv_hw, nu.beta); }
        double a = 0.0;
#pragma unroll
        for (int i1 = 0; i1 < W; ++i1) {
            const double* row = d.g + (size_t)nu_wrap(k01 + i1, 2 * N) * 2 * M;
#pragma unroll
            for (int i2 = 0; i2 < W; ++i2) a = fma(w1[i1] * w2[i2], row[nu_wrap(k02 + i2, 2 * M)], a);
        }
        // psi > 0 on a sample's own window, so a > 0 for finite input; guarded all the same: a zero weight and a count, never a NaN written out
        const double q = d.w[e] / a;
        if (a > 0.0 && isfinite(a) && isfinite(q)) { d.w[e] = q; dv = fabs(a - 1.0); }
        else { d.w[e] = 0.0; cl = 1; }
    }
    red[tid] = dv; redc[tid] = cl;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) { red[tid] = fmax(red[tid], red[tid + h]); redc[tid] += redc[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { d.pd[k & 1][blockIdx.x] = red[0]; d.pc[blockIdx.x] += redc[0]; }
}

// w_out (ABI order) = kappa * w; workgroup 0 also closes the call's report
__global__ __launch_bounds__(NT) void k_dcf_scale(NufftDev nu, DcfDev d, int niter, double kappa, double* __restrict__ w_out) {
    __shared__ double red[NT];
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e < nu.m) w_out[nu.perm[e]] = kappa * d.w[e];
    if (blockIdx.x != 0) return;
    const bool ran_all = d.stop[niter] == 0;
    const double dev = block_max(d.pd[niter & 1], d.nblk, red);
    if (threadIdx.x == 0) {
        if (ran_all) { d.res->iters = niter; d.res->dev = dev; }
        int c = 0;
        for (int i = 0; i < d.nblk; ++i) c += d.pc[i];
        d.res->clamped = c;
    }
}

template <int W> int launch_interp_div_t(qmri_ctx* ctx, const NufftDev& nu, const DcfDev& d, int k) {
    k_dcf_interp_div<W><<<dim3(d.nblk), dim3(NT), 0, ctx->stream>>>(nu, d, k);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int launch_interp_div(qmri_ctx* ctx, const NufftDev& nu, const DcfDev& d, int k) {
    switch (nu.w) {
#define DCF_W_CASE_(w_) case w_: return launch_interp_div_t<w_>(ctx, nu, d, k);
        DCF_W_CASE_(2) DCF_W_CASE_(3) DCF_W_CASE_(4) DCF_W_CASE_(5) DCF_W_CASE_(6) DCF_W_CASE_(7) DCF_W_CASE_(8) DCF_W_CASE_(9)
        DCF_W_CASE_(10) DCF_W_CASE_(11) DCF_W_CASE_(12) DCF_W_CASE_(13) DCF_W_CASE_(14) DCF_W_CASE_(15) DCF_W_CASE_(16)
#undef DCF_W_CASE_
        default: qmri_set_error(ctx, "NUFFT kernel width %d unsupported (2..%d)", nu.w, NU_WMAX); return QMRI_ERR_UNSUPPORTED;
    }
}

}  // namespace

int dcf_weights_dev(qmri_ctx* ctx, int niter, double tol, double kappa, double* d_w_out, qmri_dcf_info* info) {
    OpHost& o = ctx->op;
    if (o.kind != OP_NUFFT || niter < 1 || niter > 200 || !d_w_out) { qmri_set_error(ctx, "dcf_weights_dev: no trajectory operator / niter out of range (internal)"); return QMRI_ERR_STATE; }
    const NufftDev nu = nufft_dev_view(ctx);
    DcfDev d{};
    d.nblk = (nu.m + NT - 1) / NT;
    // g and the partial tiles live in the plan's own scratch: d_grid holds 4 max_batch N M s complex doubles (>= 4 N M doubles), d_part
    // max_batch nslot s 256 complex doubles (>= nslot 256 doubles); both are free outside a transform
    d.g = (double*)o.nu.d_grid;
    d.part = (double*)o.nu.d_part;
    DevBuf<double> w, pd;
    DevBuf<int32_t> ints;
    DevBuf<DcfRes> res;
    QMRI_TRY(w.ensure(ctx, (size_t)nu.m));
    QMRI_TRY(pd.ensure(ctx, (size_t)2 * d.nblk));
    QMRI_TRY(ints.ensure(ctx, (size_t)d.nblk + niter + 2));
    QMRI_TRY(res.ensure(ctx, 1));
    d.w = w; d.pd[0] = pd; d.pd[1] = pd.p + d.nblk; d.pc = ints; d.stop = ints.p + d.nblk; d.res = res;
    QMRI_HIP(ctx, hipMemsetAsync(ints.p, 0, ((size_t)d.nblk + niter + 2) * sizeof(int32_t), ctx->stream));
    QMRI_HIP(ctx, hipMemsetAsync(res.p, 0, sizeof(DcfRes), ctx->stream));
    QMRI_HIP(ctx, hipMemsetAsync(pd.p, 0, (size_t)2 * d.nblk * sizeof(double), ctx->stream));
    k_dcf_init<<<dim3(d.nblk), dim3(NT), 0, ctx->stream>>>(d, nu.m);
    QMRI_HIP(ctx, hipGetLastError());
    const double tol_k = tol > 0.0 ? tol : -1.0;      // tol = 0: never (a deviation is >= 0)
    for (int k = 1; k <= niter; ++k) {
        k_dcf_spread<<<dim3(nu.nseg), dim3(NT), 0, ctx->stream>>>(nu, d, k, tol_k);
        QMRI_HIP(ctx, hipGetLastError());
        if (nu.nred > 0) {
            k_dcf_reduce<<<dim3(nu.nred), dim3(NT), 0, ctx->stream>>>(nu, d, k);
            QMRI_HIP(ctx, hipGetLastError());
        }
        QMRI_TRY(launch_interp_div(ctx, nu, d, k));
    }
    k_dcf_scale<<<dim3(d.nblk), dim3(NT), 0, ctx->stream>>>(nu, d, niter, kappa, d_w_out);
    QMRI_HIP(ctx, hipGetLastError());
    DcfRes h{};
    QMRI_HIP(ctx, hipMemcpyAsync(&h, res.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) { info->iters = h.iters; info->dev = h.dev; info->clamped = h.clamped; info->split_tiles = nu.nred; }
    return QMRI_OK;
}
