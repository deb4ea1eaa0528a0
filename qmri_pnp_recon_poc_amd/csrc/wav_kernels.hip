// wav_kernels.hip -- joint wavelet soft-thresholding of a stack of coefficient images (include/qmri.h qmri_wavelet_prox): a
// multi-level, halo-tiled, separable fp64 filter bank with periodic boundaries (Haar, Daubechies-2), the shrink of the detail coefficients
// jointly over the channels, and the inverse.  The geometry -- corners, sub-band places, tiles, halos, buffers, launches -- is wav_plan.h's.
//
// k_wav_fwd<T>: one analysis level, both axes, in one launch.  A workgroup takes a tile (at most 32 x 32 inputs, T - 2 wrapped halo rows and
//   columns) of the level's input corner of one channel plane of one slice into LDS, runs the N-axis pass and then the M-axis pass there and
//   writes its four half-size sub-band tiles.  Lanes run along N in the load, in both passes and in the stores.  The tile's rows are stored
//   de-interleaved (even rows, then odd rows of a column), so the 16 lanes that produce consecutive outputs k read consecutive 16-byte elements
//   at every tap instead of every second one.  Level 1 reads x (+ u) with the circular shift in its index arithmetic and the real-mode
//   projection in its load.
// k_wav_shrink: one lane per position of a plane; m over the channels in ascending order, f = m > tau ? 1 - tau / m : 0 (a NaN m gives a NaN f),
//   the coefficients rescaled in place in the buffer of their level; the workgroup's largest m goes through a fixed-order LDS tree to a partials
//   array, of which k_wav_cmax takes the slice's maximum when it is asked for (a maximum has no summation order; NaN wins).
// k_wav_inv<T>: one synthesis level on the same tiling, M axis first; level 1 writes v with the inverse shift in its index arithmetic.
// All fp64, no atomics, every sum in one fixed order that depends on the output's own taps only: a slice has the same bits alone, anywhere in a
// stack and for any number of slices.
#include <cmath>
#include <cstdint>
#include "qmri_internal.h"

namespace {

using namespace wav;

// the doubles numpy computes from h = [1, 1] / sqrt(2) and h = [1 + sqrt 3, 3 + sqrt 3, 3 - sqrt 3, 1 - sqrt 3] / (4 sqrt 2), g[j] = (-1)^j h[T-1-j]
template <int T> struct Filt;
template <> struct Filt<2> {
    static __device__ __forceinline__ double h(int j) { return 0.70710678118654746; }
    static __device__ __forceinline__ double g(int j) { return j ? -0.70710678118654746 : 0.70710678118654746; }
};
template <> struct Filt<4> {
    static __device__ __forceinline__ double h(int j) {
        return j == 0 ? 0.4829629131445341 : j == 1 ? 0.83651630373780772 : j == 2 ? 0.22414386804201339 : -0.12940952255126034;
    }
    static __device__ __forceinline__ double g(int j) {
        return j == 0 ? -0.12940952255126034 : j == 1 ? -0.22414386804201339 : j == 2 ? 0.83651630373780772 : -0.4829629131445341;
    }
};

struct WavArgs {
    int N, M, s, L, o1, o2, real, joint;
    int level, n, m, tn, tm;                 // this launch (wav::Launch)
    long long gps;                           // shrink: workgroups per slice
    double tau;
    const double2* src; const double2* u; double2* dst;      // analysis / synthesis
    double2* s0; double2* s1; double* part;                  // shrink
};

__device__ __forceinline__ double nanmax(double a, double b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }

template <int T>
__global__ __launch_bounds__(NT) void k_wav_fwd(const WavArgs a) {
    constexpr int HALO = T - 2, HS = FWD_IN_SIDE / 2;           // HS: where the odd rows of a column start
    __shared__ double2 in[FWD_IN_SIDE * FWD_IN_STRIDE];
    __shared__ double2 mid[FWD_IN_SIDE * FWD_MID_STRIDE];
    long long g = blockIdx.x;
    const int t1 = (int)(g % a.tn); g /= a.tn;
    const int t2 = (int)(g % a.tm);
    const long long pc = g / a.tm;                              // slice * s + channel
    const int len1 = tile_len(a.n, t1), len2 = tile_len(a.m, t2), h1 = len1 / 2, h2 = len2 / 2;
    const size_t base = (size_t)pc * a.N * a.M;
    const int tid = threadIdx.x;
    // ---- load: tile and halo, wrapped inside the corner ----
    const int w1 = len1 + HALO, w2 = len2 + HALO;
    for (int idx = tid; idx < w1 * w2; idx += NT) {
        const int i = idx % w1, j = idx / w1;
        const int r = wrap(t1 * TILE + i, a.n), c = wrap(t2 * TILE + j, a.m);
        double2 v;
        if (a.level == 1) {
            int rr = r + a.o1, cc = c + a.o2;
            if (rr >= a.N) rr -= a.N;
            if (cc >= a.M) cc -= a.M;
            const size_t at = base + (size_t)rr + (size_t)a.N * cc;
            v = a.src[at];
            if (a.u) { const double2 w = a.u[at]; v.x += w.x; v.y += w.y; }
            if (a.real) v.y = 0.0;
        } else {
            v = a.src[base + (size_t)r + (size_t)a.N * c];
        }
        in[j * FWD_IN_STRIDE + (i & 1) * HS + (i >> 1)] = v;
    }
    __syncthreads();
    // ---- N axis: column j, output k1 -> a at row k1, d at row h1 + k1 of mid ----
    for (int idx = tid; idx < h1 * w2; idx += NT) {
        const int k1 = idx % h1, j = idx / h1;
        const double2* col = in + j * FWD_IN_STRIDE;
        double2 x = col[k1];
        double2 lo = make_double2(Filt<T>::h(0) * x.x, Filt<T>::h(0) * x.y), hi = make_double2(Filt<T>::g(0) * x.x, Filt<T>::g(0) * x.y);
#pragma unroll
        for (int t = 1; t < T; ++t) {
            x = col[(t & 1) * HS + k1 + (t >> 1)];
            lo.x = fma(Filt<T>::h(t), x.x, lo.x); lo.y = fma(Filt<T>::h(t), x.y, lo.y);
            hi.x = fma(Filt<T>::g(t), x.x, hi.x); hi.y = fma(Filt<T>::g(t), x.y, hi.y);
        }
        mid[j * FWD_MID_STRIDE + k1] = lo;
        mid[j * FWD_MID_STRIDE + h1 + k1] = hi;
    }
    __syncthreads();
    // ---- M axis: row r of mid, output k2 -> the four sub-band tiles ----
    const int hn = a.n / 2, hm = a.m / 2;
    for (int idx = tid; idx < len1 * h2; idx += NT) {
        const int r = idx % len1, k2 = idx / len1;
        double2 x = mid[(2 * k2) * FWD_MID_STRIDE + r];
        double2 lo = make_double2(Filt<T>::h(0) * x.x, Filt<T>::h(0) * x.y), hi = make_double2(Filt<T>::g(0) * x.x, Filt<T>::g(0) * x.y);
#pragma unroll
        for (int t = 1; t < T; ++t) {
            x = mid[(2 * k2 + t) * FWD_MID_STRIDE + r];
            lo.x = fma(Filt<T>::h(t), x.x, lo.x); lo.y = fma(Filt<T>::h(t), x.y, lo.y);
            hi.x = fma(Filt<T>::g(t), x.x, hi.x); hi.y = fma(Filt<T>::g(t), x.y, hi.y);
        }
        const int p1 = r >= h1 ? 1 : 0;
        const int row = p1 * hn + t1 * HALF + (r - p1 * h1), col = t2 * HALF + k2;
        a.dst[base + (size_t)row + (size_t)a.N * col] = lo;
        a.dst[base + (size_t)row + (size_t)a.N * (hm + col)] = hi;
    }
}

template <int T>
__global__ __launch_bounds__(NT) void k_wav_inv(const WavArgs a) {
    constexpr int HH = T / 2 - 1;
    __shared__ double2 cin[INV_IN_SIDE * INV_IN_STRIDE];
    __shared__ double2 mid[TILE * INV_MID_STRIDE];
    long long g = blockIdx.x;
    const int t1 = (int)(g % a.tn); g /= a.tn;
    const int t2 = (int)(g % a.tm);
    const long long pc = g / a.tm;
    const int len1 = tile_len(a.n, t1), len2 = tile_len(a.m, t2), c1 = len1 / 2 + HH, c2 = len2 / 2 + HH;
    const int hn = a.n / 2, hm = a.m / 2;
    const size_t base = (size_t)pc * a.N * a.M;
    const int tid = threadIdx.x;
    // ---- load: both sub-bands of each axis with HH wrapped coefficients in front ----
    for (int idx = tid; idx < 4 * c1 * c2; idx += NT) {
        const int ii = idx % (2 * c1), jj = idx / (2 * c1);
        const int p1 = ii >= c1 ? 1 : 0, p2 = jj >= c2 ? 1 : 0;
        const int row = p1 * hn + wrap(t1 * HALF - HH + (ii - p1 * c1), hn), col = p2 * hm + wrap(t2 * HALF - HH + (jj - p2 * c2), hm);
        cin[jj * INV_IN_STRIDE + ii] = a.src[base + (size_t)row + (size_t)a.N * col];
    }
    __syncthreads();
    // ---- M axis: output column j = 2 q + p takes the taps t = p + 2 u of the coefficients q - u ----
    for (int idx = tid; idx < 2 * c1 * len2; idx += NT) {
        const int ii = idx % (2 * c1), j = idx / (2 * c1), q = j >> 1, p = j & 1;
        double2 acc = make_double2(0.0, 0.0);
#pragma unroll
        for (int u = 0; u < T / 2; ++u) {
            const double hh = p ? Filt<T>::h(2 * u + 1) : Filt<T>::h(2 * u), gg = p ? Filt<T>::g(2 * u + 1) : Filt<T>::g(2 * u);
            const double2 lo = cin[(q - u + HH) * INV_IN_STRIDE + ii], hi = cin[(c2 + q - u + HH) * INV_IN_STRIDE + ii];
            acc.x = fma(hh, lo.x, fma(gg, hi.x, acc.x));
            acc.y = fma(hh, lo.y, fma(gg, hi.y, acc.y));
        }
        mid[j * INV_MID_STRIDE + ii] = acc;
    }
    __syncthreads();
    // ---- N axis ----
    for (int idx = tid; idx < len1 * len2; idx += NT) {
        const int i = idx % len1, j = idx / len1, q = i >> 1, p = i & 1;
        const double2* col = mid + j * INV_MID_STRIDE;
        double2 acc = make_double2(0.0, 0.0);
#pragma unroll
        for (int u = 0; u < T / 2; ++u) {
            const double hh = p ? Filt<T>::h(2 * u + 1) : Filt<T>::h(2 * u), gg = p ? Filt<T>::g(2 * u + 1) : Filt<T>::g(2 * u);
            const double2 lo = col[q - u + HH], hi = col[c1 + q - u + HH];
            acc.x = fma(hh, lo.x, fma(gg, hi.x, acc.x));
            acc.y = fma(hh, lo.y, fma(gg, hi.y, acc.y));
        }
        const int r = t1 * TILE + i, c = t2 * TILE + j;
        if (a.level == 1) {
            int rr = r + a.o1, cc = c + a.o2;
            if (rr >= a.N) rr -= a.N;
            if (cc >= a.M) cc -= a.M;
            if (a.real) acc.y = 0.0;
            a.dst[base + (size_t)rr + (size_t)a.N * cc] = acc;
        } else {
            a.dst[base + (size_t)r + (size_t)a.N * c] = acc;
        }
    }
}

__device__ __forceinline__ double shrink_factor(double m, double tau) { return m > tau ? 1.0 - tau / m : (m == m ? 0.0 : m); }

__global__ __launch_bounds__(NT) void k_wav_shrink(const WavArgs a) {
    __shared__ double red[NT];
    const long long g = blockIdx.x, b = g / a.gps;
    const size_t plane = (size_t)a.N * a.M;
    const size_t pos = (size_t)(g - b * a.gps) * SHRINK_POS + threadIdx.x;
    double wmax = 0.0;
    if (pos < plane) {
        const int n1 = (int)(pos % a.N), n2 = (int)(pos / a.N);
        const int l = level_of(n1, n2, a.N, a.M, a.L);
        if (l > 0) {                                             // (the final approximation corner is never thresholded)
            double2* p = (buf_of_level(l) ? a.s1 : a.s0) + (size_t)b * a.s * plane + pos;
            if (a.joint) {
                double acc = 0.0;
                for (int c = 0; c < a.s; ++c) { const double2 v = p[c * plane]; acc = fma(v.x, v.x, fma(v.y, v.y, acc)); }
                wmax = sqrt(acc);
                const double f = shrink_factor(wmax, a.tau);
                for (int c = 0; c < a.s; ++c) { const double2 v = p[c * plane]; p[c * plane] = make_double2(f * v.x, f * v.y); }
            } else {
                for (int c = 0; c < a.s; ++c) {
                    const double2 v = p[c * plane];
                    const double m = sqrt(fma(v.x, v.x, v.y * v.y)), f = shrink_factor(m, a.tau);
                    p[c * plane] = make_double2(f * v.x, f * v.y);
                    wmax = nanmax(wmax, m);
                }
            }
        }
    }
    red[threadIdx.x] = wmax;
    for (int off = NT / 2; off > 0; off >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < off) red[threadIdx.x] = nanmax(red[threadIdx.x], red[threadIdx.x + off]);
    }
    if (threadIdx.x == 0) a.part[g] = red[0];
}

// the slice's largest partial (NaN wins); one wave per slice
__global__ __launch_bounds__(64) void k_wav_cmax(const double* __restrict__ part, long long gps, double* __restrict__ out) {
    const double* p = part + (size_t)blockIdx.x * gps;
    double m = 0.0;
    for (long long i = threadIdx.x; i < gps; i += 64) m = nanmax(m, p[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = nanmax(m, __shfl_down(m, off, 64));
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

template <int T> int wav_launches(qmri_ctx* ctx, WavArgs a, const WavPlan& pl, int B, const double2* d_x, const double2* d_u, double2* d_out) {
    Launch ls[MAX_LAUNCHES];
    const int nl = launch_list(pl.N, pl.M, pl.s, B, pl.levels, ls);
    double2* const s[2] = {ctx->wav_s[0].p, ctx->wav_s[1].p};
    for (int i = 0; i < nl; ++i) {
        const Launch& l = ls[i];
        if (l.groups > 0x7fffffffLL) { qmri_set_error(ctx, "invalid argument: too many wavelet tiles in one launch"); return QMRI_ERR_INVALID_ARG; }
        a.level = l.level; a.n = l.n; a.m = l.m; a.tn = l.tn; a.tm = l.tm;
        a.src = l.src == BUF_X ? d_x : s[l.src];
        a.u = l.src == BUF_X ? d_u : nullptr;
        a.dst = l.dst == BUF_OUT ? d_out : s[l.dst];
        if (l.kind == FWD) k_wav_fwd<T><<<dim3((unsigned)l.groups), dim3(NT), 0, ctx->stream>>>(a);
        else if (l.kind == INV) k_wav_inv<T><<<dim3((unsigned)l.groups), dim3(NT), 0, ctx->stream>>>(a);
        else k_wav_shrink<<<dim3((unsigned)l.groups), dim3(NT), 0, ctx->stream>>>(a);
        QMRI_HIP(ctx, hipGetLastError());
    }
    return QMRI_OK;
}

}  // namespace

int wav_prox_dev(qmri_ctx* ctx, const WavPlan& pl, int B, const double2* d_x, const double2* d_u, double2* d_out, double* d_cmax) {
    QMRI_TRY(ctx->wav_s[0].ensure(ctx, scratch_elems(pl.N, pl.M, pl.s, B)));
    if (pl.levels > 1) QMRI_TRY(ctx->wav_s[1].ensure(ctx, scratch_elems(pl.N, pl.M, pl.s, B)));
    QMRI_TRY(ctx->wav_part.ensure(ctx, partial_elems(pl.N, pl.M, B)));
    WavArgs a{};
    a.N = pl.N; a.M = pl.M; a.s = pl.s; a.L = pl.levels; a.o1 = pl.o1; a.o2 = pl.o2; a.real = pl.real; a.joint = pl.joint;
    a.gps = shrink_groups_per_slice(pl.N, pl.M);
    a.tau = pl.tau;
    a.s0 = ctx->wav_s[0].p; a.s1 = ctx->wav_s[1].p; a.part = ctx->wav_part.p;
    if (taps(pl.filter) == 2) QMRI_TRY(wav_launches<2>(ctx, a, pl, B, d_x, d_u, d_out));
    else QMRI_TRY(wav_launches<4>(ctx, a, pl, B, d_x, d_u, d_out));
    if (d_cmax) {
        k_wav_cmax<<<dim3(B), dim3(64), 0, ctx->stream>>>(ctx->wav_part.p, a.gps, d_cmax);
        QMRI_HIP(ctx, hipGetLastError());
    }
    return QMRI_OK;
}
