// dictb_kernels.hip -- the B1 map estimated from the fingerprints themselves (extension, no reference counterpart; include/qmri.h
// qmri_dict_group_scores / qmri_b1_pool / qmri_b1_estimate).  Two stages:
//   1. group scores: score[g][p] = max over the atoms k of group g of abs(ip(k, p)) -- the mt of a grouped match of pixel p against group g, for
//      EVERY group.  The exact single-precision products of dict_kernels.hip (v_mfma_f32_32x32x2_f32 over the group-padded pack d_gpack; a f32
//      MFMA accumulates k in order with one fma per product, so ip is the oracle's fmaf chain over c = 0 .. s-1), but no incumbent: only the
//      largest |ip|^2 = fma(im, im, re * re) of the group is kept, one float per lane, and one square root is taken at the end (sqrtf is
//      correctly rounded and monotone, so sqrtf(max m2) == max sqrtf(m2)).  A NaN magnitude never wins, as in the oracle's `mag > best`; a pixel
//      whose magnitudes are all NaN scores the oracle's -1.  Zero-padded rows give 0 (or NaN for a non-finite pixel) and change no maximum.
//      No f16 filter: every product is needed.  A maximum does not depend on the order, so the atoms of a group may be split over workgroups
//      (parts go to a scratch array and k_dictb_finish takes their maximum; no floating-point atomics).  The runs of groups and the atom parts
//      of a launch: dict_plan_scores and dict_group_part, dict_plan.h.
//   2. pooled argmax (fp64): E = score^2 on foreground pixels with a finite positive score, box sums over (2h+1) x (2h+1) windows as two passes
//      of direct left-to-right sums, the lowest group with the largest pooled energy per pixel.
#include <algorithm>
#include <cmath>

#include "qmri_internal.h"
#include "dict_device.h"
#include "dict_plan.h"

namespace {

constexpr int NT = 256;
constexpr int MAXPAIR = 8;      // s <= 16

// One 32-atom tile: the exact products of dict_kernels.hip's exact_tile, then the tile's largest |ip|^2 into the lane's running maximum.
// `tm > run` is false for a NaN: a tile whose 16 rows are all NaN leaves the maximum alone (fmaxf drops a NaN beside a number).
template <int NPAIR, int NV>
__device__ __forceinline__ void score_tile(const f32x4 (&av)[NV], const float (&bre)[NPAIR], const float (&bim)[NPAIR], float& run) {
    f32x16 are, aim;
    exact_products<NPAIR, NV>(av, bre, bim, are, aim);
    const float tm = tile_max2(are, aim);
    if (tm > run) run = tm;
}

// Work unit: (four 32-pixel tiles, one per wave; a run of groups blockIdx.y * grun ..; atom part blockIdx.z of nparts).  A wave reads its pixels
// once, keeps them as MFMA B fragments and walks the groups of its run one after the other, all tiles of each (or its part of them).
// X: the pixels p0 .. p0 + n - 1 of an Npix x s column-major complex-double array (xstride = Npix).  out[g * n + i], i the pixel within the
// range: the score when nparts == 1, else the part's largest |ip|^2 at out[(z * G + g) * n + i] (-1: nothing, an empty part included).
template <int NPAIR>
__global__ __launch_bounds__(NT) void k_dictb_scores(const double2* __restrict__ X, size_t xstride, int n, int s, const float* __restrict__ pack,
                                                     const int* __restrict__ gtile, int G, int grun, float* __restrict__ out) {
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const int i = ((int)blockIdx.x * 4 + wave) * 32 + j;
    const bool valid = i < n;
    float bre[NPAIR], bim[NPAIR];
    load_b_frags<NPAIR>(X, i, xstride, s, valid, h, bre, bim);
    constexpr int NV = (NPAIR <= 4) ? 1 : 2;
    const int nparts = (int)gridDim.z, z = (int)blockIdx.z;
    const int g0 = (int)blockIdx.y * grun, g1 = min(G, g0 + grun);
    for (int g = g0; g < g1; ++g) {
        // this workgroup's part of the group's tiles (dict_plan.h); a part beyond the group's own is empty
        const dplan::TileRange part_r = dplan::dict_group_part(gtile[g], gtile[g + 1], nparts, z, dplan::MIN_TILES, 1);
        const int tbeg = part_r.tbeg, tend = part_r.tend;
        float run = -1.0f;
        f32x4 av[NV], avn[NV];
        auto request = [&](int t, f32x4 (&dst)[NV]) __attribute__((always_inline)) { request_tile<NV>(pack, t, lane, dst); };
        // (the fragments of the next tile are requested before the products of this one: register double buffer, as in k_dict_match)
        if (tbeg < tend) request(tbeg, av);
        for (int t = tbeg; t < tend; t += 2) {
            if (t + 1 < tend) request(t + 1, avn);
            score_tile<NPAIR, NV>(av, bre, bim, run);
            if (t + 1 >= tend) break;
            if (t + 2 < tend) request(t + 2, av);
            score_tile<NPAIR, NV>(avn, bre, bim, run);
        }
        // the two lane halves hold the same pixel and interleaved atom rows
        const float o = __shfl(run, lane ^ 32, 64);
        if (o > run) run = o;
        if (h == 0 && valid) {
            if (nparts == 1) out[(size_t)g * n + i] = (run >= 0.f) ? sqrtf(run) : -1.0f;
            else out[((size_t)z * G + g) * n + i] = run;
        }
    }
}

// score[g][i] from the parts' largest |ip|^2
__global__ __launch_bounds__(256) void k_dictb_finish(const float* __restrict__ part, int P, size_t gn, float* __restrict__ score) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= gn) return;
    float run = part[e];
    for (int k = 1; k < P; ++k) {
        const float o = part[(size_t)k * gn + e];
        if (o > run) run = o;
    }
    score[e] = (run >= 0.f) ? sqrtf(run) : -1.0f;
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------------------------
// Pixels i + N j of a slice, slices stacked; a launch covers the slices sl0 .. sl0 + nsl - 1.  score[g * sstride + (pixel - soff)], mask by pixel.
// E = S * S in fp64 (exact: two singles) where the pixel is foreground and S is finite and > 0, else 0.
__device__ __forceinline__ double b1_energy(float S, bool fg) { return (fg && S > 0.f && S <= 3.402823466e38f) ? (double)S * (double)S : 0.0; }

// pass 1, along N: T[g][i, j] = sum over d = -h .. h ascending of E[g][i + d, j], terms outside the row skipped, plain additions left to right
// (a contraction of E's product into the addition gives the same bits: the product is exact).  T[g * npl + local pixel], npl = nsl N M.
__global__ __launch_bounds__(256) void k_b1_rows(const float* __restrict__ score, size_t sstride, size_t soff, const uint8_t* __restrict__ mask, int N, size_t p0,
                                                 size_t npl, int hw, double* __restrict__ T) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;             // local pixel of the launch
    if (l >= npl) return;
    const int g = blockIdx.y;
    const int i = (int)(l % (size_t)N);
    const size_t row = l - i;                                            // first local pixel of the row
    const int d0 = max(-hw, -i), d1 = min(hw, N - 1 - i);
    const float* sg = score + (size_t)g * sstride + (p0 - soff) + row;
    const uint8_t* mg = mask ? mask + p0 + row : nullptr;
    double t = 0.0;
    for (int d = d0; d <= d1; ++d) t += b1_energy(sg[i + d], mg ? mg[i + d] != 0 : true);
    T[(size_t)g * npl + l] = t;
}

// pass 2, along M, and the argmax: P[g][i, j] = sum over d ascending of T[g][i, j + d] inside the slice; the lowest g with the largest P;
// conf = (P_best - P_second) / P_best (1 for G = 1).  Background, or P_best not > 0: grp 0, b1 NaN, conf 0.
__global__ __launch_bounds__(256) void k_b1_cols(const double* __restrict__ T, int G, const double* __restrict__ gval, const uint8_t* __restrict__ mask, int N,
                                                 int M, size_t p0, size_t npl, int hw, double* __restrict__ b1, int32_t* __restrict__ grp,
                                                 double* __restrict__ conf) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= npl) return;
    const int j = (int)((l / (size_t)N) % (size_t)M);
    const int d0 = max(-hw, -j), d1 = min(hw, M - 1 - j);
    const bool fg = mask ? mask[p0 + l] != 0 : true;
    double best = 0.0, second = -1.0;
    int bg = 0;
    if (fg)
        for (int g = 0; g < G; ++g) {
            const double* tg = T + (size_t)g * npl + l;
            double pg = 0.0;
            for (int d = d0; d <= d1; ++d) pg += tg[(ptrdiff_t)d * N];
            if (g == 0) { best = pg; continue; }
            if (pg > best) { second = best; best = pg; bg = g; }
            else if (pg > second) second = pg;
        }
    const bool ok = fg && best > 0.0;
    if (grp) grp[p0 + l] = ok ? bg + 1 : 0;
    if (b1) b1[p0 + l] = ok ? gval[bg] : __builtin_nan("");
    if (conf) conf[p0 + l] = ok ? (G == 1 ? 1.0 : (best - second) / best) : 0.0;
}

}  // namespace

// Stage 1 on the pixels p0 .. p0 + n - 1 of X (Npix x s): d_score[g * n + i].  The dictionary is narrow and has groups (api_b1.cpp checks).
int dictb_launch_scores(qmri_ctx* ctx, const double2* d_X, size_t Npix, size_t p0, int n, float* d_score) {
    DictHost& D = ctx->dict;
    const int npair = (D.s + 1) / 2;
    if (npair < 1 || npair > MAXPAIR) {
        qmri_set_error(ctx, "group scores support s <= %d channels (got %d)", 2 * MAXPAIR, D.s);
        return QMRI_ERR_UNSUPPORTED;
    }
    QMRI_TRY(dict_resident_slots(ctx, k_dictb_scores<5>, NT, D.slots_b));
    const dplan::ScoresPlan pl = dplan::dict_plan_scores(n, D.G, D.gtiles_max, D.slots_b);
    float* out = d_score;
    const size_t gn = (size_t)D.G * n;
    if (pl.P > 1) {
        QMRI_TRY(D.d_bpart.ensure(ctx, (size_t)pl.P * gn));
        out = D.d_bpart;
    }
    const dim3 grid(pl.ptiles, pl.nruns, pl.P), blk(NT);
    const double2* x = d_X + p0;
    dict_dispatch_npair(npair, [&](auto np) {
        k_dictb_scores<decltype(np)::value><<<grid, blk, 0, ctx->stream>>>(x, Npix, n, D.s, D.d_gpack, D.d_gtile, D.G, pl.grun, out);
    });
    QMRI_HIP(ctx, hipGetLastError());
    if (pl.P > 1) {
        k_dictb_finish<<<dim3((unsigned)((gn + 255) / 256)), dim3(256), 0, ctx->stream>>>(out, pl.P, gn, d_score);
        QMRI_HIP(ctx, hipGetLastError());
    }
    return QMRI_OK;
}

// Stage 2 on the slices sl0 .. sl0 + nsl - 1: d_score[g * sstride + (pixel - soff)], the mask and the outputs by pixel of the whole stack (nullable).
// T (G x nsl N M doubles) is the context's scratch.
int b1_launch_pool(qmri_ctx* ctx, int G, const double* d_gval, int N, int M, int sl0, int nsl, const float* d_score, size_t sstride, size_t soff,
                   const uint8_t* d_mask, int hw, double* d_b1, int32_t* d_grp, double* d_conf) {
    const size_t nm = (size_t)N * M, p0 = (size_t)sl0 * nm, npl = (size_t)nsl * nm;
    QMRI_TRY(ctx->dict.d_bT.ensure(ctx, (size_t)G * npl));
    double* T = ctx->dict.d_bT;
    const unsigned nb = (unsigned)((npl + 255) / 256);
    k_b1_rows<<<dim3(nb, G), dim3(256), 0, ctx->stream>>>(d_score, sstride, soff, d_mask, N, p0, npl, hw, T);
    k_b1_cols<<<dim3(nb), dim3(256), 0, ctx->stream>>>(T, G, d_gval, d_mask, N, M, p0, npl, hw, d_b1, d_grp, d_conf);
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
