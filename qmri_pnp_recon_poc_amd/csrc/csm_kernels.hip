// csm_kernels.hip -- coil sensitivity maps from calibration data (adaptive combine: Walsh, Gmitro & Marcellin, MRM 2000): an EXTENSION with no
// reference counterpart (the reference is single-coil, README.md:63), like cc_kernels.hip whose output it follows.  Definition: include/qmri.h and
// DESIGN.md section 17.  All fp64 complex.
//
// Per slice, with the calibration images I_j (N x M, ncoil <= 128) and a patch half-width p <= 4:
//     R(r) = sum_{d in [-p, p]^2} I(r + d) I(r + d)^H  (terms outside the grid dropped),   lambda_1(r), u(r) its dominant eigenpair,
//     C(r) = u(r) times the phase of the chosen reference, zero where lambda_1(r) < thresh^2 max_r lambda_1.
//
// Kernels (launch order):
//   k_csm_pad     (KSPACE input) taper, zero-pad, shift and conjugate a chunk of <= max_batch coil blocks onto the N x M grid; the dense
//                 spectrum passes of dc_kernels.hip (DC_SPECTRUM, one channel per "slice") then give conj(I_j): a forward DFT of conj(X) is the
//                 conjugate of the inverse DFT of X, and the passes' 1 / sqrt(NM) leaves exactly the sqrt(NM) ifft2 of the definition
//   k_csm_unpack  conjugates and transposes that spectrum ([n1][n2], n2 contiguous) into the image layout of `maps` (n1 + N n2)
//   k_csm_eig     the hot path: power iteration on R(r) WITHOUT forming it, v <- sum_d I(r + d) (I(r + d)^H v)
//   k_csm_energy  (PHASE_COIL) sum_r |I_j(r)|^2 per coil: one workgroup per (coil, slice), one fixed tree
//   k_csm_scalar  per slice: max_r lambda_1 from the tiles' maxima, the reference coil (largest energy, lowest index on ties), iteration statistics
//   k_csm_finish  phase, mask and combine in one elementwise pass: C in place of u, C^H I, lambda_1
//
// k_csm_eig.  Why power iteration and not R + Jacobi: R(r) is ncoil^2 complex per pixel (16 KB at 32 coils, 256 KB at 128), which neither
// registers nor LDS hold for more than a handful of coils, while the matrix-free product needs only the coil images of the pixel's patch -- and those
// are shared by the neighbouring pixels.  A workgroup (256 threads) owns a 4 x 4 tile of pixels, 16 lanes per pixel.  LDS (64 KB per workgroup, so
// that two share a CU's 160 KB): the iterate v [16 pixels][ncoil] (256 B per coil), the patch products s_d = I(r + d)^H v [16][(2p + 1)^2]
// (<= 20.3 KB), and the coil images of the tile plus its halo, [coils][(4 + 2p)^2] (1.6 KB per coil at p = 3), in the room that is left: all coils
// when they fit (8 or 16 coils stay resident for the whole iteration), else in chunks of as many coils as fit, staged again from global memory
// (L2) in ascending order twice per iteration (32 coils at p = 3: 27 + 5; 128 coils at p = 4: 26 chunks of 5).
//   pass 1: the lane g of a pixel owns the offsets d = g, g + 16, .. (<= 6, accumulators in registers): s_d = sum_j conj(I_j(r + d)) v_j, coils ascending
//   pass 2: the lane owns the coils j = g, g + 16, .. (<= 8, in registers):                        w_j = sum_d I_j(r + d) s_d,       d ascending
//   then |w|^2 and max_j |w_j / |w| - v_j| by a butterfly over the pixel's 16 lanes (commutative at every stage: all lanes hold the same bits), and
//   v <- w / |w|, lambda_1 = |w| (= |R v| with |v| = 1).  R is Hermitian positive semi-definite, so v^H R v >= 0 and consecutive iterates need no
//   phase alignment.  A pixel stops when the largest real or imaginary change of an entry is <= 1e-13, or after 256 iterations (counted in
//   qmri_csm_info); a pixel that has stopped is left alone while its tile's other pixels finish.  Start: I(r) / |I(r)|, or e_0 where I(r) = 0;
//   a patch of zeros gives lambda_1 = 0 and keeps e_0.
// Every sum has one order that depends on (ncoil, p, N, M) alone, there are no floating-point atomics, and a workgroup touches one slice: a slice's
// bits are the same alone, at any position of a stack and at any max_batch.
// Arithmetic (MI355X_MICROARCH.md): an iteration is 2 (2p + 1)^2 ncoil complex FMAs per pixel, each with one 16-byte LDS read of an image value (the
// v_j / s_d operand is read once per 6 / 8 of them).  At 128 B / clock / CU of LDS against 256 fp64 FMA / clock / CU (4 per complex FMA) the LDS
// read bounds the kernel at about 1 / 4 of the vector fp64 rate -- the same bound as k_cc_cov_part's.
#include <algorithm>
#include <cmath>
#include <vector>
#include "qmri_internal.h"

namespace {
constexpr int NT = 256;
constexpr int CSM_T = 4;                 // tile side (every supported grid side is a multiple of 16)
constexpr int CSM_PX = CSM_T * CSM_T;    // pixels per workgroup
constexpr int CSM_G = NT / CSM_PX;       // lanes per pixel (16: a quarter wave)
constexpr int CSM_PMAX = 4;
constexpr int CSM_DQ = ((2 * CSM_PMAX + 1) * (2 * CSM_PMAX + 1) + CSM_G - 1) / CSM_G;   // offsets per lane (6)
constexpr int CSM_JQ = 128 / CSM_G;      // coils per lane (8)
constexpr int CSM_LDS = 65536 - 512;     // bytes of dynamic LDS per workgroup (the static arrays of k_csm_eig take the rest of 64 KB)
constexpr int CSM_MAXIT = 256;
constexpr double CSM_TOL = 1e-13;

struct CsmScalar { double lmax; int32_t ref, itmax, bad, pad; };

// block index a of an axis of c block entries that lands on DFT bin k of a side-n axis (block index c / 2 is k = 0), or -1
__device__ __forceinline__ int csm_block_index(int k, int c, int n) {
    const int a = k + c / 2 < n ? k + c / 2 : k + c / 2 - n;
    return a < c ? a : -1;
}

// out[g][n1 + N n2] = conj(w1[a1] w2[a2] calib[g][a1 + cN a2]) at the bin (n1, n2) the block entry (a1, a2) shifts to, zero elsewhere
__global__ void __launch_bounds__(NT) k_csm_pad(const double2* __restrict__ calib, int cN, int cM, int N, int M, const double* __restrict__ taper,
                                                double2* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x, g = blockIdx.y;
    if (i >= N * M) return;
    const int n1 = i % N, n2 = i / N;
    const int a1 = csm_block_index(n1, cN, N), a2 = csm_block_index(n2, cM, M);
    double2 v = make_double2(0.0, 0.0);
    if (a1 >= 0 && a2 >= 0) {
        const double2 z = calib[(size_t)g * cN * cM + a1 + (size_t)cN * a2];
        const double w = taper[a1] * taper[cN + a2];
        v = make_double2(w * z.x, -(w * z.y));
    }
    out[(size_t)g * N * M + i] = v;
}

// img[g][n1 + N n2] = conj(spec[g][n1 M + n2])
__global__ void __launch_bounds__(NT) k_csm_unpack(const double2* __restrict__ spec, int N, int M, double2* __restrict__ img) {
    const int i = blockIdx.x * NT + threadIdx.x, g = blockIdx.y;
    if (i >= N * M) return;
    const int n1 = i % N, n2 = i / N;
    const double2 z = spec[(size_t)g * N * M + (size_t)n1 * M + n2];
    img[(size_t)g * N * M + i] = make_double2(z.x, -z.y);
}

__device__ __forceinline__ double group_sum(double x) {      // over the 16 lanes of a pixel; the same bits in every lane
#pragma unroll
    for (int k = CSM_G / 2; k > 0; k >>= 1) x += __shfl_xor(x, k, CSM_G);
    return x;
}
__device__ __forceinline__ double group_max(double x) {
#pragma unroll
    for (int k = CSM_G / 2; k > 0; k >>= 1) x = fmax(x, __shfl_xor(x, k, CSM_G));
    return x;
}

struct CsmEig {
    int N, M, ncoil, p, ch;                  // ch: coils per LDS chunk (>= ncoil: everything resident)
    const double2* img;                      // [B][ncoil][N M]
    double2* u;                              // [B][ncoil][N M]
    double* lam;                             // [B][N M]
    double* tmax; int32_t* tit; int32_t* tbad;   // [B][tiles]
};

// the coil images j0 .. j0 + cnt - 1 of the tile and its halo: stage[jj][a + S b] = I_{j0 + jj}(n1_0 - p + a, n2_0 - p + b), zero outside the grid
__device__ __forceinline__ void csm_stage(const CsmEig& a, const double2* __restrict__ ib, int n10, int n20, int j0, int cnt, double2* stage) {
    const int S = CSM_T + 2 * a.p, S2 = S * S;
    for (int e = threadIdx.x; e < cnt * S2; e += NT) {
        const int jj = e / S2, q = e - jj * S2;
        const int n1 = n10 - a.p + q % S, n2 = n20 - a.p + q / S;
        stage[e] = (n1 >= 0 && n1 < a.N && n2 >= 0 && n2 < a.M) ? ib[(size_t)(j0 + jj) * a.N * a.M + n1 + (size_t)a.N * n2] : make_double2(0.0, 0.0);
    }
}

__global__ void __launch_bounds__(NT) k_csm_eig(CsmEig a) {
    extern __shared__ double2 lds[];
    __shared__ double plam[CSM_PX];
    __shared__ int pit[CSM_PX], pbad[CSM_PX];
    const int W = 2 * a.p + 1, P = W * W, S = CSM_T + 2 * a.p, S2 = S * S, nc = a.ncoil;
    double2* v = lds;                        // [PX][nc]
    double2* sd = v + CSM_PX * nc;           // [PX][P]
    double2* stage = sd + CSM_PX * P;        // [ch][S2]
    const int tid = threadIdx.x, px = tid / CSM_G, g = tid % CSM_G, b = blockIdx.y;
    const int tiles1 = a.N / CSM_T;
    const int n10 = (blockIdx.x % tiles1) * CSM_T, n20 = (blockIdx.x / tiles1) * CSM_T;
    const int tx = px % CSM_T, ty = px / CSM_T;
    const size_t plane = (size_t)a.N * a.M, pix = (size_t)(n10 + tx) + (size_t)a.N * (n20 + ty);
    const double2* ib = a.img + (size_t)b * nc * plane;
    const int base = tx + S * ty;            // stage offset of the patch's first entry (offset -p, -p)
    const bool resident = a.ch >= nc;
    int doff[CSM_DQ];
#pragma unroll
    for (int q = 0; q < CSM_DQ; ++q) { const int d = g + CSM_G * q; doff[q] = d < P ? base + d % W + S * (d / W) : -1; }

    // start: I(r) / |I(r)|, or e_0
    {
        double2 w[CSM_JQ];
        double nn = 0.0;
#pragma unroll
        for (int q = 0; q < CSM_JQ; ++q) {
            const int j = g + CSM_G * q;
            w[q] = j < nc ? ib[(size_t)j * plane + pix] : make_double2(0.0, 0.0);
            nn = fma(w[q].x, w[q].x, fma(w[q].y, w[q].y, nn));
        }
        const double nrm = sqrt(group_sum(nn));
#pragma unroll
        for (int q = 0; q < CSM_JQ; ++q) {
            const int j = g + CSM_G * q;
            if (j < nc) v[px * nc + j] = nrm > 0.0 ? make_double2(w[q].x / nrm, w[q].y / nrm) : make_double2(j == 0 ? 1.0 : 0.0, 0.0);
        }
    }
    if (resident) csm_stage(a, ib, n10, n20, 0, nc, stage);
    __syncthreads();

    bool active = true, conv = false;
    int it = 0;
    double lam = 0.0;
    for (;;) {
        // pass 1: s_d = sum_j conj(I_j(r + d)) v_j
        double2 acc[CSM_DQ];
#pragma unroll
        for (int q = 0; q < CSM_DQ; ++q) acc[q] = make_double2(0.0, 0.0);
        for (int j0 = 0; j0 < nc; j0 += a.ch) {
            const int cnt = min(a.ch, nc - j0);
            if (!resident) { __syncthreads(); csm_stage(a, ib, n10, n20, j0, cnt, stage); __syncthreads(); }
            if (active)
                for (int jj = 0; jj < cnt; ++jj) {
                    const double2 vj = v[px * nc + j0 + jj];
                    const double2* im = stage + jj * S2;
#pragma unroll
                    for (int q = 0; q < CSM_DQ; ++q)
                        if (doff[q] >= 0) {
                            const double2 z = im[doff[q]];
                            acc[q].x = fma(z.x, vj.x, fma(z.y, vj.y, acc[q].x));
                            acc[q].y = fma(z.x, vj.y, fma(-z.y, vj.x, acc[q].y));
                        }
                }
        }
        if (active) {
#pragma unroll
            for (int q = 0; q < CSM_DQ; ++q)
                if (doff[q] >= 0) sd[px * P + g + CSM_G * q] = acc[q];
        }
        __syncthreads();
        // pass 2: w_j = sum_d I_j(r + d) s_d
        double2 w[CSM_JQ];
#pragma unroll
        for (int q = 0; q < CSM_JQ; ++q) w[q] = make_double2(0.0, 0.0);
        for (int j0 = 0; j0 < nc; j0 += a.ch) {
            const int cnt = min(a.ch, nc - j0);
            if (!resident) { __syncthreads(); csm_stage(a, ib, n10, n20, j0, cnt, stage); __syncthreads(); }
            if (active) {
                int joff[CSM_JQ];
#pragma unroll
                for (int q = 0; q < CSM_JQ; ++q) { const int j = g + CSM_G * q; joff[q] = (j >= j0 && j < j0 + cnt) ? (j - j0) * S2 + base : -1; }
                for (int d2 = 0; d2 < W; ++d2)
                    for (int d1 = 0; d1 < W; ++d1) {
                        const double2 s = sd[px * P + d1 + W * d2];
                        const int o = d1 + S * d2;
#pragma unroll
                        for (int q = 0; q < CSM_JQ; ++q)
                            if (joff[q] >= 0) {
                                const double2 z = stage[joff[q] + o];
                                w[q].x = fma(z.x, s.x, fma(-z.y, s.y, w[q].x));
                                w[q].y = fma(z.x, s.y, fma(z.y, s.x, w[q].y));
                            }
                    }
            }
        }
        if (active) {
            double nn = 0.0;
#pragma unroll
            for (int q = 0; q < CSM_JQ; ++q) nn = fma(w[q].x, w[q].x, fma(w[q].y, w[q].y, nn));
            const double nrm = sqrt(group_sum(nn));
            double dm = 0.0;
            if (nrm > 0.0) {
#pragma unroll
                for (int q = 0; q < CSM_JQ; ++q) {
                    const int j = g + CSM_G * q;
                    if (j < nc) {
                        const double2 vn = make_double2(w[q].x / nrm, w[q].y / nrm), vo = v[px * nc + j];
                        dm = fmax(dm, fmax(fabs(vn.x - vo.x), fabs(vn.y - vo.y)));
                        v[px * nc + j] = vn;           // (this lane alone reads or writes entry j of its pixel between the barriers)
                    }
                }
            }
            dm = group_max(dm);
            lam = nrm;
            ++it;
            if (!(nrm > 0.0) ? nrm == 0.0 : dm <= CSM_TOL) { conv = true; active = false; }
            else if (it >= CSM_MAXIT) active = false;
        }
        if (!__syncthreads_or(active ? 1 : 0)) break;
    }
#pragma unroll
    for (int q = 0; q < CSM_JQ; ++q) {
        const int j = g + CSM_G * q;
        if (j < nc) a.u[((size_t)b * nc + j) * plane + pix] = v[px * nc + j];
    }
    if (g == 0) { a.lam[(size_t)b * plane + pix] = lam; plam[px] = lam; pit[px] = it; pbad[px] = conv ? 0 : 1; }
    __syncthreads();
    if (tid == 0) {
        double lm = plam[0];
        int im = pit[0], nb = pbad[0];
        for (int k = 1; k < CSM_PX; ++k) { lm = fmax(lm, plam[k]); im = max(im, pit[k]); nb += pbad[k]; }
        const size_t t = (size_t)b * gridDim.x + blockIdx.x;
        a.tmax[t] = lm; a.tit[t] = im; a.tbad[t] = nb;
    }
}

// en[b][j] = sum_r |I_j(r)|^2: thread t adds r = t, t + 256, .. ascending, then one fixed tree
__global__ void __launch_bounds__(NT) k_csm_energy(const double2* __restrict__ img, size_t plane, double* __restrict__ en) {
    __shared__ double red[NT];
    const double2* p = img + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * plane;
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < plane; i += NT) { const double2 z = p[i]; acc = fma(z.x, z.x, fma(z.y, z.y, acc)); }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int k = NT / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) en[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// max, integer max and integer sum do not depend on the order: lane t takes the tiles t, t + 64, .., lane 0 combines the 64 partials
__global__ void __launch_bounds__(64) k_csm_scalar(int ntiles, int ncoil, const double* __restrict__ tmax, const int32_t* __restrict__ tit,
                                                   const int32_t* __restrict__ tbad, const double* __restrict__ en, CsmScalar* __restrict__ sc) {
    __shared__ double lm[64];
    __shared__ int im[64], nb[64];
    const int b = blockIdx.x, l = threadIdx.x;
    double m = 0.0;
    int i = 0, n = 0;
    for (int t = l; t < ntiles; t += 64) {
        const size_t k = (size_t)b * ntiles + t;
        m = fmax(m, tmax[k]); i = max(i, tit[k]); n += tbad[k];
    }
    lm[l] = m; im[l] = i; nb[l] = n;
    __syncthreads();
    if (l) return;
    CsmScalar s{0.0, 0, 0, 0, 0};
    for (int t = 0; t < 64; ++t) { s.lmax = fmax(s.lmax, lm[t]); s.itmax = max(s.itmax, im[t]); s.bad += nb[t]; }
    if (en) {
        double best = en[(size_t)b * ncoil];
        for (int j = 1; j < ncoil; ++j) if (en[(size_t)b * ncoil + j] > best) { best = en[(size_t)b * ncoil + j]; s.ref = j; }
    }
    sc[b] = s;
}

// C = u * phase (in place), zero below the threshold; img = C^H I (coils ascending); lambda_1 is already where k_csm_eig wrote it
__global__ void __launch_bounds__(NT) k_csm_finish(int ncoil, size_t plane, int phase_coil, double thresh, const double2* __restrict__ I,
                                                   const double* __restrict__ lam, const CsmScalar* __restrict__ sc, double2* maps,
                                                   double2* __restrict__ img_out) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= plane) return;
    const CsmScalar s = sc[b];
    const double l = lam[(size_t)b * plane + i];
    const double2* ib = I + (size_t)b * ncoil * plane + i;
    double2* mb = maps + (size_t)b * ncoil * plane + i;
    const bool keep = !(thresh > 0.0 && l < thresh * thresh * s.lmax);
    double2 ph = make_double2(1.0, 0.0);
    if (keep) {
        double2 z = make_double2(0.0, 0.0);
        if (phase_coil) { const double2 r = mb[(size_t)s.ref * plane]; z = make_double2(r.x, -r.y); }
        else
            for (int j = 0; j < ncoil; ++j) {                                   // u^H I
                const double2 u = mb[(size_t)j * plane], x = ib[(size_t)j * plane];
                z.x = fma(u.x, x.x, fma(u.y, x.y, z.x));
                z.y = fma(u.x, x.y, fma(-u.y, x.x, z.y));
            }
        const double m = sqrt(z.x * z.x + z.y * z.y);
        if (m > 0.0) ph = make_double2(z.x / m, z.y / m);
    }
    double2 acc = make_double2(0.0, 0.0);
    for (int j = 0; j < ncoil; ++j) {
        double2 c = make_double2(0.0, 0.0);
        if (keep) {
            const double2 u = mb[(size_t)j * plane], x = ib[(size_t)j * plane];
            c = make_double2(u.x * ph.x - u.y * ph.y, u.x * ph.y + u.y * ph.x);
            acc.x = fma(c.x, x.x, fma(c.y, x.y, acc.x));
            acc.y = fma(c.x, x.y, fma(-c.y, x.x, acc.y));
        }
        mb[(size_t)j * plane] = c;
    }
    if (img_out) img_out[(size_t)b * plane + i] = acc;
}
}  // namespace

// coils per LDS chunk of k_csm_eig: all of them when they fit beside v and s_d, else as many as fit (a function of ncoil and p alone)
int csm_chunk_coils(int ncoil, int p) {
    const int P = (2 * p + 1) * (2 * p + 1), S = CSM_T + 2 * p;
    const int room = CSM_LDS - (int)sizeof(double2) * CSM_PX * (ncoil + P);
    const int fit = room / ((int)sizeof(double2) * S * S);
    return fit >= ncoil ? ncoil : fit;
}

// The whole estimate on device arrays (api_csm.cpp checks the arguments; N, M are the operator's).  d_calib: [B][ncoil][cM][cN] (KSPACE) or
// [B][ncoil][N M] (IMAGES); d_maps [B][ncoil][N M]; d_img [B][N M] and d_lam [B][N M] nullable; info nullable.  Returns after its kernels have finished.
int csm_maps_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_calib, const qmri_csm_params& prm, double2* d_maps, double2* d_img, double* d_lam,
                 qmri_csm_info* info) {
    OpHost& o = ctx->op;
    const int N = o.N, M = o.M;
    const size_t plane = (size_t)N * M, nimg = (size_t)B * ncoil;
    const int ntiles = (N / CSM_T) * (M / CSM_T);
    const unsigned gp = (unsigned)((plane + NT - 1) / NT);
    DevBuf<double2> I, pad, tmp, spec;
    DevBuf<double> lam, tmax, en, taper;
    DevBuf<int32_t> tit, tbad;
    DevBuf<CsmScalar> sc;
    const double2* d_I = d_calib;
    if (prm.kind == QMRI_CSM_KSPACE) {
        const int cN = prm.cN, cM = prm.cM;
        QMRI_TRY(I.ensure(ctx, nimg * plane));
        QMRI_TRY(pad.ensure(ctx, (size_t)o.maxB * plane));
        QMRI_TRY(tmp.ensure(ctx, (size_t)o.maxB * plane));
        QMRI_TRY(spec.ensure(ctx, (size_t)o.maxB * plane));
        QMRI_TRY(taper.ensure(ctx, (size_t)cN + cM));
        std::vector<double> w((size_t)cN + cM, 1.0);
        if (prm.window) {
            const double pi = 3.14159265358979323846;
            for (int k = 0; k < cN; ++k) w[k] = 0.5 * (1.0 + std::cos(2.0 * pi * (k - cN / 2) / cN));
            for (int k = 0; k < cM; ++k) w[(size_t)cN + k] = 0.5 * (1.0 + std::cos(2.0 * pi * (k - cM / 2) / cM));
        }
        QMRI_HIP(ctx, hipMemcpyAsync(taper.p, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));                       // (w leaves scope)
        OpDev op = qmri_opdev(ctx);
        op.s = 1;                                                               // one coil image per "slice" of the dense passes
        for (size_t g0 = 0; g0 < nimg; g0 += o.maxB) {
            const int cnt = (int)std::min<size_t>(o.maxB, nimg - g0);
            k_csm_pad<<<dim3(gp, cnt), dim3(NT), 0, ctx->stream>>>(d_calib + g0 * cN * cM, cN, cM, N, M, taper, pad);
            QMRI_HIP(ctx, hipGetLastError());
            QMRI_TRY(dc_launch_fwd(ctx, op, o.ls, DC_SPECTRUM, cnt, pad, tmp, spec, nullptr));
            k_csm_unpack<<<dim3(gp, cnt), dim3(NT), 0, ctx->stream>>>(spec, N, M, I + g0 * plane);
            QMRI_HIP(ctx, hipGetLastError());
        }
        d_I = I;
    }
    if (!d_lam) { QMRI_TRY(lam.ensure(ctx, (size_t)B * plane)); }
    double* lamw = d_lam ? d_lam : lam.p;
    QMRI_TRY(tmax.ensure(ctx, (size_t)B * ntiles));
    QMRI_TRY(tit.ensure(ctx, (size_t)B * ntiles));
    QMRI_TRY(tbad.ensure(ctx, (size_t)B * ntiles));
    QMRI_TRY(sc.ensure(ctx, (size_t)B));
    CsmEig a{N, M, ncoil, prm.patch, csm_chunk_coils(ncoil, prm.patch), d_I, d_maps, lamw, tmax, tit, tbad};
    const int P = (2 * prm.patch + 1) * (2 * prm.patch + 1), S = CSM_T + 2 * prm.patch;
    const size_t ldsb = sizeof(double2) * ((size_t)CSM_PX * (ncoil + P) + (size_t)std::min(a.ch, ncoil) * S * S);
    if (a.ch < 1 || ldsb > (size_t)CSM_LDS) { qmri_set_error(ctx, "k_csm_eig: %d coils at patch %d do not fit the LDS plan (internal)", ncoil, prm.patch); return QMRI_ERR_UNSUPPORTED; }
    k_csm_eig<<<dim3(ntiles, B), dim3(NT), ldsb, ctx->stream>>>(a);
    QMRI_HIP(ctx, hipGetLastError());
    const bool coil = prm.phase_ref == QMRI_CSM_PHASE_COIL;
    if (coil) {
        QMRI_TRY(en.ensure(ctx, nimg));
        k_csm_energy<<<dim3(ncoil, B), dim3(NT), 0, ctx->stream>>>(d_I, plane, en);
        QMRI_HIP(ctx, hipGetLastError());
    }
    k_csm_scalar<<<dim3(B), dim3(64), 0, ctx->stream>>>(ntiles, ncoil, tmax, tit, tbad, coil ? en.p : nullptr, sc);
    QMRI_HIP(ctx, hipGetLastError());
    k_csm_finish<<<dim3(gp, B), dim3(NT), 0, ctx->stream>>>(ncoil, plane, coil ? 1 : 0, prm.thresh, d_I, lamw, sc, d_maps, d_img);
    QMRI_HIP(ctx, hipGetLastError());
    std::vector<CsmScalar> hs((size_t)B);
    QMRI_HIP(ctx, hipMemcpyAsync(hs.data(), sc.p, (size_t)B * sizeof(CsmScalar), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));                           // (the scratch is released on return)
    if (info) {
        info->max_iters = 0; info->not_converged = 0;
        for (const CsmScalar& s : hs) { info->max_iters = std::max(info->max_iters, s.itmax); info->not_converged += s.bad; }
    }
    return QMRI_OK;
}
