// fmap_kernels.hip -- field map from multi-echo images in fp64: an EXTENSION with no reference counterpart.  Definition: include/qmri.h, DESIGN.md
// section 24.  Planes are [n1 + N n2]; phi and w are [slice][pair][pixel], f is [slice][pixel].
//   k_fmap_pairs        one pass over Y: phi_ab, |s_ab| and the start per pixel; per block the maximum of sum_ab |s_ab| and a non-finite flag
//   k_fmap_wmax         the slice's W and flag from the block partials (a maximum: exact in any order)
//   k_fmap_scale        w_ab = |s_ab| / W and the trust plane sum_ab w_ab
//   k_fmap_iter         one iteration per launch, a pixel per lane (the default: the faster form as measured)
//   k_fmap_iter_halo    (knob fmap_fuse = 1) up to FH iterations per launch: a workgroup loads its FT x FT tile of f with a halo of FH pixels into LDS, runs the iterations on
//                       the shrinking valid region ping-pong between two LDS planes and writes the tile.  Jacobi with a recomputed halo IS the
//                       one-iteration-per-launch result, and both kernels call fmap_update, so the two forms agree bit for bit.  w and phi are
//                       streamed from global memory per pixel and iteration (P <= 28 pairs do not fit LDS beside f at this tile; the tile's share of
//                       them, 2 P (FT + 2 FH)^2 doubles, stays in L2 between the iterations of a launch).
//   k_fmap_cost(+_fin)  Psi, min f and max f by fixed partials: a block's 256 values through a fixed tree, the blocks' partials in block order
//   k_fmap_finish       the result plane, NaN for a flagged slice
// No atomics, vector stores only, fused multiply-adds only where written (the file is compiled with -ffp-contract=off): a slice's bits do not depend
// on the launch geometry, on its position in the stack or on nslices.
#include <cmath>
#include <cstdint>
#include <limits>
#include "qmri_internal.h"

namespace {
constexpr int NT = 256;                  // threads per workgroup
constexpr int FT = 32;                   // tile side of the fused iteration
constexpr int FH = 8;                    // halo = iterations per fused launch
constexpr int FE = FT + 2 * FH;          // extended tile side; 2 FE^2 doubles = 36 KiB of LDS: 4 workgroups (16 waves) per CU
constexpr double TWO_PI = 6.283185307179586476925286766559;

struct FmapK {                           // what every iteration launch needs, by value
    int N, M, P;
    double beta;
    double d[FMAP_MAX_PAIRS];
};

// f^{k+1} of one pixel.  phi, w: the pixel's first pair; stride: pixels per plane.  hu/hd/hl/hr: neighbour n1-1 / n1+1 / n2-1 / n2+1 is inside the grid.
__device__ __forceinline__ double fmap_update(double f, double fu, double fd, double fl, double fr, bool hu, bool hd, bool hl, bool hr,
                                              const double* __restrict__ phi, const double* __restrict__ w, size_t stride, const FmapK& k) {
    double g = 0.0, c = 0.0;
    for (int p = 0; p < k.P; ++p) {
        const double d = k.d[p];
        double u = fma(-d, f, phi[(size_t)p * stride]);
        u = fma(-TWO_PI, rint(u / TWO_PI), u);
        const double s = sin(u);
        const double kap = fabs(u) < 1e-8 ? 1.0 : s / u;
        const double wd = w[(size_t)p * stride] * d;
        g = fma(-wd, s, g);
        c = fma(wd * d, kap, c);
    }
    double nb = 0.0, ns = 0.0;
    if (hu) { nb += 1.0; ns += fu; }
    if (hd) { nb += 1.0; ns += fd; }
    if (hl) { nb += 1.0; ns += fl; }
    if (hr) { nb += 1.0; ns += fr; }
    const double lap = fma(nb, f, -ns);
    const double den = fma(2.0 * k.beta, nb, c);
    return den > 0.0 ? f - fma(k.beta, lap, g) / den : f;
}

struct FmapPairs { int L, C, P, sign; double d01; int pa[FMAP_MAX_PAIRS], pb[FMAP_MAX_PAIRS]; };

__device__ __forceinline__ bool finite2(double2 v) { return isfinite(v.x) && isfinite(v.y); }

__global__ void __launch_bounds__(NT) k_fmap_pairs(FmapPairs q, int npix, const double2* __restrict__ Y, const double* __restrict__ finit,
                                                    double* __restrict__ phi, double* __restrict__ mag, double* __restrict__ f0,
                                                    double* __restrict__ pmax, int* __restrict__ pbad) {
    __shared__ double smax[NT];
    __shared__ int sbad[NT];
    const int tid = threadIdx.x, sl = blockIdx.y;
    const int n = blockIdx.x * NT + tid;
    double tot = 0.0;
    int bad = 0;
    if (n < npix) {
        const double2* Ys = Y + (size_t)sl * q.L * q.C * npix + n;
        double phi0 = 0.0;
        for (int p = 0; p < q.P; ++p) {
            const double2* ya = Ys + (size_t)q.pa[p] * q.C * npix;
            const double2* yb = Ys + (size_t)q.pb[p] * q.C * npix;
            double re = 0.0, im = 0.0;
            for (int c = 0; c < q.C; ++c) {                  // coils ascending
                const double2 a = ya[(size_t)c * npix], b = yb[(size_t)c * npix];
                bad |= !(finite2(a) && finite2(b));
                re = fma(a.x, b.x, re);
                re = fma(a.y, b.y, re);
                if (q.sign < 0) { im = fma(a.y, b.x, im); im = fma(-a.x, b.y, im); }     // a conj(b)
                else            { im = fma(a.x, b.y, im); im = fma(-a.y, b.x, im); }     // conj(a) b
            }
            const double ph = atan2(im, re), mg = sqrt(fma(re, re, im * im));
            const size_t o = ((size_t)sl * q.P + p) * npix + n;
            phi[o] = ph;
            mag[o] = mg;
            tot += mg;
            if (p == 0) phi0 = ph;
        }
        double f = phi0 / q.d01;
        if (finit) {
            f = finit[(size_t)sl * npix + n];
            bad |= !isfinite(f);
        }
        f0[(size_t)sl * npix + n] = f;
        if (!isfinite(tot)) { bad = 1; tot = 0.0; }
    }
    smax[tid] = tot;
    sbad[tid] = bad;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) { smax[tid] = fmax(smax[tid], smax[tid + s]); sbad[tid] |= sbad[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { pmax[(size_t)sl * gridDim.x + blockIdx.x] = smax[0]; pbad[(size_t)sl * gridDim.x + blockIdx.x] = sbad[0]; }
}

__global__ void __launch_bounds__(NT) k_fmap_wmax(int nblk, const double* __restrict__ pmax, const int* __restrict__ pbad, double* __restrict__ W,
                                                   int* __restrict__ badsl) {
    __shared__ double smax[NT];
    __shared__ int sbad[NT];
    const int tid = threadIdx.x, sl = blockIdx.x;
    double m = 0.0;
    int bad = 0;
    for (int i = tid; i < nblk; i += NT) { m = fmax(m, pmax[(size_t)sl * nblk + i]); bad |= pbad[(size_t)sl * nblk + i]; }
    smax[tid] = m;
    sbad[tid] = bad;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) { smax[tid] = fmax(smax[tid], smax[tid + s]); sbad[tid] |= sbad[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { W[sl] = smax[0]; badsl[sl] = sbad[0]; }
}

__global__ void __launch_bounds__(NT) k_fmap_scale(int P, int npix, const double* __restrict__ W, const int* __restrict__ badsl, double* __restrict__ w,
                                                    double* __restrict__ trust) {
    const int sl = blockIdx.y;
    const int n = blockIdx.x * NT + threadIdx.x;
    if (n >= npix) return;
    const double Ws = W[sl];
    double tot = 0.0;
    for (int p = 0; p < P; ++p) {
        const size_t o = ((size_t)sl * P + p) * npix + n;
        const double v = Ws > 0.0 ? w[o] / Ws : 0.0;
        w[o] = v;
        tot += v;
    }
    if (trust) trust[(size_t)sl * npix + n] = badsl[sl] ? std::numeric_limits<double>::quiet_NaN() : tot;
}

__global__ void __launch_bounds__(NT) k_fmap_iter(FmapK k, const double* __restrict__ phi, const double* __restrict__ w, const double* __restrict__ fin,
                                                   double* __restrict__ fout) {
    const int npix = k.N * k.M, sl = blockIdx.y;
    const int n = blockIdx.x * NT + threadIdx.x;
    if (n >= npix) return;
    const int n1 = n % k.N, n2 = n / k.N;
    const double* fs = fin + (size_t)sl * npix;
    const bool hu = n1 > 0, hd = n1 + 1 < k.N, hl = n2 > 0, hr = n2 + 1 < k.M;
    const double fu = hu ? fs[n - 1] : 0.0, fd = hd ? fs[n + 1] : 0.0, fl = hl ? fs[n - k.N] : 0.0, fr = hr ? fs[n + k.N] : 0.0;
    const size_t o = (size_t)sl * k.P * npix + n;
    fout[(size_t)sl * npix + n] = fmap_update(fs[n], fu, fd, fl, fr, hu, hd, hl, hr, phi + o, w + o, (size_t)npix, k);
}

// nit <= FH iterations on the tile (blockIdx.x % tiles1, blockIdx.x / tiles1) of slice blockIdx.y
__global__ void __launch_bounds__(NT) k_fmap_iter_halo(FmapK k, int tiles1, int nit, const double* __restrict__ phi, const double* __restrict__ w,
                                                        const double* __restrict__ fin, double* __restrict__ fout) {
    __shared__ double buf[2][FE * FE];
    const int npix = k.N * k.M, sl = blockIdx.y, tid = threadIdx.x;
    const int o1 = (int)(blockIdx.x % tiles1) * FT - FH, o2 = (int)(blockIdx.x / tiles1) * FT - FH;     // grid position of the extended tile's corner
    const double* fs = fin + (size_t)sl * npix;
    for (int e = tid; e < FE * FE; e += NT) {
        const int g1 = o1 + e % FE, g2 = o2 + e / FE;
        const bool in = g1 >= 0 && g1 < k.N && g2 >= 0 && g2 < k.M;
        buf[0][e] = in ? fs[g1 + k.N * g2] : 0.0;
    }
    __syncthreads();
    const size_t so = (size_t)sl * k.P * npix;
    int cur = 0;
    for (int it = 1; it <= nit; ++it) {
        const int side = FE - 2 * it;                        // valid after `it` iterations: [it, FE - it) in both directions
        const double* b = buf[cur];
        double* bn = buf[cur ^ 1];
        for (int e = tid; e < side * side; e += NT) {
            const int i = it + e % side, j = it + e / side;
            const int g1 = o1 + i, g2 = o2 + j;
            if (g1 < 0 || g1 >= k.N || g2 < 0 || g2 >= k.M) continue;
            const int li = i + FE * j;
            const bool hu = g1 > 0, hd = g1 + 1 < k.N, hl = g2 > 0, hr = g2 + 1 < k.M;
            const double fu = hu ? b[li - 1] : 0.0, fd = hd ? b[li + 1] : 0.0, fl = hl ? b[li - FE] : 0.0, fr = hr ? b[li + FE] : 0.0;
            const size_t o = so + (size_t)(g1 + k.N * g2);
            bn[li] = fmap_update(b[li], fu, fd, fl, fr, hu, hd, hl, hr, phi + o, w + o, (size_t)npix, k);
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int e = tid; e < FT * FT; e += NT) {
        const int i = FH + e % FT, j = FH + e / FT;
        const int g1 = o1 + i, g2 = o2 + j;
        if (g1 < k.N && g2 < k.M) fout[(size_t)sl * npix + g1 + k.N * g2] = buf[cur][i + FE * j];
    }
}

// per block: Psi's share of its 256 pixels (data term, then the edges to n1 + 1 and n2 + 1), min f, max f
__global__ void __launch_bounds__(NT) k_fmap_cost(FmapK k, const double* __restrict__ phi, const double* __restrict__ w, const double* __restrict__ f,
                                                   double* __restrict__ part) {
    __shared__ double sc[NT], smin[NT], smax[NT];
    const int npix = k.N * k.M, sl = blockIdx.y, tid = threadIdx.x;
    const int n = blockIdx.x * NT + tid;
    const double inf = std::numeric_limits<double>::infinity();
    double v = 0.0, lo = inf, hi = -inf;
    if (n < npix) {
        const double* fs = f + (size_t)sl * npix;
        const double fn = fs[n];
        const size_t o = (size_t)sl * k.P * npix + n;
        for (int p = 0; p < k.P; ++p) v = fma(w[o + (size_t)p * npix], 1.0 - cos(fma(-k.d[p], fn, phi[o + (size_t)p * npix])), v);
        const int n1 = n % k.N, n2 = n / k.N;
        double e = 0.0;
        if (n1 + 1 < k.N) { const double t = fs[n + 1] - fn; e = fma(t, t, e); }
        if (n2 + 1 < k.M) { const double t = fs[n + k.N] - fn; e = fma(t, t, e); }
        v = fma(0.5 * k.beta, e, v);
        lo = hi = fn;
    }
    sc[tid] = v; smin[tid] = lo; smax[tid] = hi;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) { sc[tid] += sc[tid + s]; smin[tid] = fmin(smin[tid], smin[tid + s]); smax[tid] = fmax(smax[tid], smax[tid + s]); }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = part + ((size_t)sl * gridDim.x + blockIdx.x) * 3;
        o[0] = sc[0]; o[1] = smin[0]; o[2] = smax[0];
    }
}

// res[slice][3]: the partials of a slice in block order (lane t takes blocks t, t + 256, ...; then the fixed tree)
__global__ void __launch_bounds__(NT) k_fmap_cost_fin(int nblk, const double* __restrict__ part, const int* __restrict__ badsl, double* __restrict__ res) {
    __shared__ double sc[NT], smin[NT], smax[NT];
    const int tid = threadIdx.x, sl = blockIdx.x;
    const double inf = std::numeric_limits<double>::infinity();
    double v = 0.0, lo = inf, hi = -inf;
    for (int i = tid; i < nblk; i += NT) {
        const double* o = part + ((size_t)sl * nblk + i) * 3;
        v += o[0]; lo = fmin(lo, o[1]); hi = fmax(hi, o[2]);
    }
    sc[tid] = v; smin[tid] = lo; smax[tid] = hi;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) { sc[tid] += sc[tid + s]; smin[tid] = fmin(smin[tid], smin[tid + s]); smax[tid] = fmax(smax[tid], smax[tid + s]); }
        __syncthreads();
    }
    if (tid == 0) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const bool bad = badsl[sl] != 0;
        res[sl * 3 + 0] = bad ? nan : sc[0]; res[sl * 3 + 1] = bad ? nan : smin[0]; res[sl * 3 + 2] = bad ? nan : smax[0];
    }
}

__global__ void __launch_bounds__(NT) k_fmap_finish(int npix, const int* __restrict__ badsl, const double* __restrict__ f, double* __restrict__ out) {
    const int sl = blockIdx.y;
    const int n = blockIdx.x * NT + threadIdx.x;
    if (n < npix) out[(size_t)sl * npix + n] = badsl[sl] ? std::numeric_limits<double>::quiet_NaN() : f[(size_t)sl * npix + n];
}
}  // namespace

int fmap_halo() { return FH; }

int fmap_estimate_dev(qmri_ctx* ctx, const FmapPlan& pl, const double2* d_Y, const double* d_f_init, double* d_f_out, double* d_trust_out,
                      qmri_fieldmap_info* info) {
    const int S = pl.nslices, P = pl.P, npix = pl.N * pl.M, nblk = (npix + NT - 1) / NT;
    const size_t plane = (size_t)npix;
    DevBuf<double> phi, w, fa, fb, pmax, W, part, res;
    DevBuf<int> pbad, badsl;
    QMRI_TRY(phi.ensure(ctx, (size_t)S * P * plane));
    QMRI_TRY(w.ensure(ctx, (size_t)S * P * plane));
    QMRI_TRY(fa.ensure(ctx, (size_t)S * plane));
    QMRI_TRY(fb.ensure(ctx, (size_t)S * plane));
    QMRI_TRY(pmax.ensure(ctx, (size_t)S * nblk));
    QMRI_TRY(pbad.ensure(ctx, (size_t)S * nblk));
    QMRI_TRY(W.ensure(ctx, (size_t)S));
    QMRI_TRY(badsl.ensure(ctx, (size_t)S));
    QMRI_TRY(part.ensure(ctx, (size_t)S * nblk * 3));
    QMRI_TRY(res.ensure(ctx, (size_t)S * 6));

    FmapPairs q{};
    q.L = pl.L; q.C = pl.C; q.P = P; q.sign = pl.sign; q.d01 = pl.d[0];
    FmapK k{};
    k.N = pl.N; k.M = pl.M; k.P = P; k.beta = pl.beta;
    for (int p = 0; p < P; ++p) { q.pa[p] = pl.pa[p]; q.pb[p] = pl.pb[p]; k.d[p] = pl.d[p]; }

    const dim3 gpix((unsigned)nblk, (unsigned)S);
    hipStream_t st = ctx->stream;
    k_fmap_pairs<<<gpix, NT, 0, st>>>(q, npix, d_Y, d_f_init, phi.p, w.p, fa.p, pmax.p, pbad.p);
    k_fmap_wmax<<<S, NT, 0, st>>>(nblk, pmax.p, pbad.p, W.p, badsl.p);
    k_fmap_scale<<<gpix, NT, 0, st>>>(P, npix, W.p, badsl.p, w.p, d_trust_out);
    k_fmap_cost<<<gpix, NT, 0, st>>>(k, phi.p, w.p, fa.p, part.p);
    k_fmap_cost_fin<<<S, NT, 0, st>>>(nblk, part.p, badsl.p, res.p);
    QMRI_HIP(ctx, hipGetLastError());

    double *cur = fa.p, *nxt = fb.p;
    const int iters = qmri_knob(K_FMAP_START) ? 0 : pl.iters;
    if (qmri_knob(K_FMAP_FUSE)) {
        const int tiles1 = (pl.N + FT - 1) / FT, tiles2 = (pl.M + FT - 1) / FT;
        for (int done = 0; done < iters; done += FH) {
            k_fmap_iter_halo<<<dim3((unsigned)(tiles1 * tiles2), (unsigned)S), NT, 0, st>>>(k, tiles1, std::min(FH, iters - done), phi.p, w.p, cur, nxt);
            std::swap(cur, nxt);
        }
    } else {
        for (int it = 0; it < iters; ++it) {
            k_fmap_iter<<<gpix, NT, 0, st>>>(k, phi.p, w.p, cur, nxt);
            std::swap(cur, nxt);
        }
    }
    k_fmap_cost<<<gpix, NT, 0, st>>>(k, phi.p, w.p, cur, part.p);
    k_fmap_cost_fin<<<S, NT, 0, st>>>(nblk, part.p, badsl.p, res.p + (size_t)S * 3);
    k_fmap_finish<<<gpix, NT, 0, st>>>(npix, badsl.p, cur, d_f_out);
    QMRI_HIP(ctx, hipGetLastError());
    std::vector<double> h((size_t)S * 6);
    QMRI_HIP(ctx, hipMemcpyAsync(h.data(), res.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    QMRI_HIP(ctx, hipStreamSynchronize(st));
    if (info)
        for (int s = 0; s < S; ++s) {
            info[s] = qmri_fieldmap_info{};
            info[s].cost0 = h[(size_t)s * 3];
            info[s].cost = h[(size_t)(S + s) * 3];
            info[s].f_min = h[(size_t)(S + s) * 3 + 1];
            info[s].f_max = h[(size_t)(S + s) * 3 + 2];
            info[s].iters = iters;
            info[s].unwrap_limit_hz = pl.unwrap_limit_hz;
        }
    return QMRI_OK;
}
