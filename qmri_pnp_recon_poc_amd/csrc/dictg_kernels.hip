// dictg_kernels.hip -- groups of a dictionary and the grouped match (extension, no reference counterpart; include/qmri.h
// qmri_set_dictionary_groups / qmri_dict_match_grouped): every pixel is matched against the atoms of ONE group, chosen by a
// per-pixel selector value (a measured B1) -- 1/G of the products of a match over all atoms.
//
// Two pieces live here; the match itself is dict_kernels.hip's, instantiated with GRP = true:
//   * qmri_set_dictionary_groups: a second copy of the packed dictionary (exact fragments and f16 pieces) in which every group starts on a
//     32-atom tile, made on the device from the packs qmri_set_dictionary left there (the host copy of D is gone by then);
//   * per call, the pixel bucketing: group of each pixel, per-group counts, a scan over the counts padded to the workgroup's pixel width, and a
//     slot -> pixel table.  The match reads X and writes its outputs THROUGH that table (a gathered copy of X would cost a pass of 16 s bytes per
//     pixel each way for nothing: a lane reads its pixel's s values once, at the start of the workgroup).  Slots are handed out by an integer
//     atomic; no result depends on which slot a pixel got.  Unmatched pixels (non-finite selector) get no slot and their zeros here.
//     The layout of the bucketing scratch (DictgWork) and the atom parts of the match are dict_plan.h's.
#include <cfloat>
#include <cmath>

#include "qmri_internal.h"
#include "dict_device.h"
#include "dict_plan.h"

// g(b), 1-based: the lowest g that minimises fabs(b - group_val[g]) in fp64; 0 (unmatched) for a non-finite b.  One subtraction and one fabs per
// group -- nothing a compiler may contract or reorder -- so the host and the device give the same integers.
__host__ __device__ static inline int dictg_group_of(double b, const double* __restrict__ gval, int G) {
    if (!(fabs(b) <= DBL_MAX)) return 0;
    int best = 0;
    double bd = fabs(b - gval[0]);
    for (int g = 1; g < G; ++g) {
        const double d = fabs(b - gval[g]);
        if (d < bd) { bd = d; best = g; }
    }
    return best + 1;
}

namespace {

// pack / pack16 of the dictionary -> the group-padded ones: tile t of those holds atoms atom0[t] .. min(atom0[t] + 32, atom1[t]) - 1, zeros after
__global__ __launch_bounds__(256) void k_dictg_repack(const float4* __restrict__ pack, float4* __restrict__ gpack, int nv, const uint4* __restrict__ pack16,
                                                       uint4* __restrict__ gpack16, const int* __restrict__ atom0, const int* __restrict__ atom1, int gtiles) {
    const int i = blockIdx.x * 256 + threadIdx.x;                      // (tile, lane)
    if (i >= gtiles * 64) return;
    const int t = i >> 6, lane = i & 63;
    const int a = atom0[t] + (lane & 31);
    const bool real = a < atom1[t];
    const size_t src = (size_t)(a >> 5) * 64 + (a & 31) + 32 * (lane >> 5);
    for (int v = 0; v < nv; ++v) gpack[(size_t)i * nv + v] = real ? pack[src * nv + v] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (pack16)
        for (int hl = 0; hl < 2; ++hl)                                  // [tile][hi | lo][lane]
            gpack16[(size_t)t * 128 + hl * 64 + lane] = real ? pack16[(size_t)(a >> 5) * 128 + hl * 64 + (a & 31) + 32 * (lane >> 5)] : make_uint4(0, 0, 0, 0);
}

// group of every pixel (1-based, 0 unmatched) and the pixels per group
__global__ __launch_bounds__(256) void k_dictg_assign(const double* __restrict__ sel, int Npix, const double* __restrict__ gval, int G, int* __restrict__ grp,
                                                       int* __restrict__ count) {
    __shared__ int s_cnt[256];
    __shared__ double s_val[256];
    s_cnt[threadIdx.x] = 0;
    if ((int)threadIdx.x < G) s_val[threadIdx.x] = gval[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < Npix) {
        const int g = dictg_group_of(sel[p], s_val, G);
        grp[p] = g;
        if (g > 0) atomicAdd(&s_cnt[g - 1], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < G && s_cnt[threadIdx.x]) atomicAdd(&count[threadIdx.x], s_cnt[threadIdx.x]);
}

// slot_beg[g] = first slot of group g with every count padded to padw (slot_beg[G]: slots in use); cursor[g] = slot_beg[g].  One workgroup, G <= 256.
__global__ __launch_bounds__(256) void k_dictg_scan(const int* __restrict__ count, int G, int padw, int* __restrict__ slot_beg, int* __restrict__ cursor) {
    __shared__ int s[256];
    const int g = threadIdx.x;
    const int mine = (g < G) ? (count[g] + padw - 1) / padw * padw : 0;
    s[g] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = (g >= d) ? s[g - d] : 0;
        __syncthreads();
        s[g] += v;
        __syncthreads();
    }
    if (g < G) { slot_beg[g] = s[g] - mine; cursor[g] = s[g] - mine; }
    if (g == G - 1) slot_beg[G] = s[g];
}

// every slot empty; the group of every slot tile in use (the LAST g with slot_beg[g] <= the tile's first slot: groups without pixels have no slots)
__global__ __launch_bounds__(256) void k_dictg_fill(int* __restrict__ slot_pix, int* __restrict__ tile_grp, int slot_cap, int padw, const int* __restrict__ slot_beg,
                                                     int G) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < slot_cap) slot_pix[i] = -1;
    if (i < slot_cap / padw) {
        const int first = i * padw;
        int lo = 0, hi = G;                                             // slot_beg[lo] <= first always (slot_beg[0] = 0)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (slot_beg[mid] <= first) lo = mid; else hi = mid;
        }
        tile_grp[i] = lo;
    }
}

// a matched pixel takes the next slot of its group; an unmatched one gets its outputs here: zeros, and atom -1 for k_dict_xfit.  A workgroup
// ranks its pixels per group in LDS and reserves each group's run of slots with ONE global atomic: with a smooth selector map neighbouring pixels
// share a group, and one returning global atomic per pixel on G addresses serialises in the L2 (DESIGN.md section 20 has the figures).
__global__ __launch_bounds__(256) void k_dictg_place(const int* __restrict__ grp, int Npix, int* __restrict__ cursor, int* __restrict__ slot_pix, int Q,
                                                      float* __restrict__ qmap, float* __restrict__ pd, float* __restrict__ mt, int32_t* __restrict__ dm,
                                                      int32_t* __restrict__ grp_out, float4* __restrict__ win) {
    __shared__ int s_cnt[256], s_base[256];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int g = (p < Npix) ? grp[p] : 0;
    const int rank = (g > 0) ? atomicAdd(&s_cnt[g - 1], 1) : 0;
    __syncthreads();
    if (s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], s_cnt[threadIdx.x]);      // (G <= 256: one thread per group)
    __syncthreads();
    if (p >= Npix) return;
    if (grp_out) grp_out[p] = g;
    if (g > 0) { slot_pix[s_base[g - 1] + rank] = p; return; }
    if (dm) dm[p] = 0;
    if (mt) mt[p] = 0.f;
    if (pd) { pd[2 * (size_t)p] = 0.f; pd[2 * (size_t)p + 1] = 0.f; }
    if (qmap) for (int q = 0; q < Q; ++q) qmap[(size_t)p + (size_t)Npix * q] = 0.f;
    if (win) win[p] = make_float4(0.f, 0.f, __int_as_float(-1), 0.f);
}

}  // namespace

extern "C" int qmri_dict_group_assign(int G, const double* group_val, int n, const double* sel, int32_t* grp_out) {
    QMRI_CHECK_ARG(nullptr, G >= 1 && G <= 256, "1 <= G <= 256 groups");
    QMRI_CHECK_ARG(nullptr, group_val && n >= 0 && (n == 0 || (sel && grp_out)), "group_val / sel / grp_out must not be NULL, n >= 0");
    for (int g = 0; g < G; ++g)
        QMRI_CHECK_ARG(nullptr, std::isfinite(group_val[g]) && (g == 0 || group_val[g] > group_val[g - 1]), "group_val must be finite and strictly ascending");
    for (int i = 0; i < n; ++i) grp_out[i] = dictg_group_of(sel[i], group_val, G);
    return QMRI_OK;
}

void dictg_free(qmri_ctx* ctx) {
    DictHost& d = ctx->dict;
    d.d_gpack.reset(); d.d_gpack16.reset(); d.d_gptr.reset(); d.d_gtile.reset(); d.d_gval.reset(); d.d_gwork.reset();
    d.G = 0; d.gtiles_max = 0; d.gtile_h.clear();
}

// the arguments are checked (api_dict.cpp); the dictionary is set and narrow.  The new groups are built beside the current ones and take their
// place only when every allocation, copy and the repack launch has succeeded: a failure leaves the groups as they were.
int dictg_set_groups(qmri_ctx* ctx, int G, const int32_t* group_ptr, const double* group_val) {
    DictHost& d = ctx->dict;
    std::vector<int> gtile(G + 1, 0), atom0, atom1;
    int tmax = 0;
    for (int g = 0; g < G; ++g) {
        const int nt = (group_ptr[g + 1] - group_ptr[g] + 31) / 32;
        gtile[g + 1] = gtile[g] + nt;
        tmax = std::max(tmax, nt);
        for (int t = 0; t < nt; ++t) { atom0.push_back(group_ptr[g] + 32 * t); atom1.push_back(group_ptr[g + 1]); }
    }
    const int gtiles = gtile[G], npl = ((d.s + 1) / 2 <= 4) ? 4 : 8;
    DevBuf<int> a0, a1, gptr, gtl;
    DevBuf<float> gpack; DevBuf<uint4> gpack16; DevBuf<double> gval;
    QMRI_TRY(a0.ensure(ctx, (size_t)gtiles));
    QMRI_TRY(a1.ensure(ctx, (size_t)gtiles));
    QMRI_TRY(gpack.ensure(ctx, (size_t)gtiles * 64 * npl));
    if (d.d_pack16) QMRI_TRY(gpack16.ensure(ctx, (size_t)gtiles * 128));
    QMRI_TRY(gptr.ensure(ctx, (size_t)G + 1));
    QMRI_TRY(gtl.ensure(ctx, (size_t)G + 1));
    QMRI_TRY(gval.ensure(ctx, (size_t)G));
    QMRI_HIP(ctx, hipMemcpy(a0.p, atom0.data(), (size_t)gtiles * sizeof(int), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(a1.p, atom1.data(), (size_t)gtiles * sizeof(int), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(gptr.p, group_ptr, ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(gtl.p, gtile.data(), ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice));
    QMRI_HIP(ctx, hipMemcpy(gval.p, group_val, (size_t)G * sizeof(double), hipMemcpyHostToDevice));
    k_dictg_repack<<<dim3((gtiles * 64 + 255) / 256), dim3(256), 0, ctx->stream>>>((const float4*)d.d_pack, (float4*)gpack.p, npl / 4, d.d_pack16, gpack16.p,
                                                                                    a0.p, a1.p, gtiles);
    QMRI_HIP(ctx, hipGetLastError());
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));            // (also drains a grouped match still reading the old groups)
    dictg_free(ctx);
    d.d_gpack = std::move(gpack); d.d_gpack16 = std::move(gpack16);
    d.d_gptr = std::move(gptr); d.d_gtile = std::move(gtl); d.d_gval = std::move(gval);
    d.G = G; d.gtiles_max = tmax; d.gtile_h = gtile;
    return QMRI_OK;
}

int dictg_launch(qmri_ctx* ctx, const double2* d_X, int Npix, const double* d_sel, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm, int32_t* d_grp,
                 float2* d_xfit) {
    DictHost& D = ctx->dict;
    const int padw = dict_group_pixel_width(ctx);
    const dplan::DictgWork w = dplan::dictg_work(Npix, D.G, padw);           // the bucketing scratch (dict_plan.h)
    QMRI_TRY(D.d_gwork.ensure(ctx, w.total));
    float4* win = nullptr;
    if (d_xfit) {
        QMRI_TRY(D.d_win.ensure(ctx, (size_t)Npix));
        win = D.d_win;
    }
    int* base = D.d_gwork;
    int *grp = base + w.grp, *count = base + w.count, *cursor = base + w.cursor, *slot_beg = base + w.slot_beg, *tile_grp = base + w.tile_grp,
        *slot_pix = base + w.slot_pix;
    const dim3 blk(256), gpix((Npix + 255) / 256);
    QMRI_HIP(ctx, hipMemsetAsync(count, 0, 256 * sizeof(int), ctx->stream));
    k_dictg_assign<<<gpix, blk, 0, ctx->stream>>>(d_sel, Npix, D.d_gval, D.G, grp, count);
    k_dictg_scan<<<dim3(1), blk, 0, ctx->stream>>>(count, D.G, padw, slot_beg, cursor);
    k_dictg_fill<<<dim3((w.slot_cap + 255) / 256), blk, 0, ctx->stream>>>(slot_pix, tile_grp, w.slot_cap, padw, slot_beg, D.G);
    k_dictg_place<<<gpix, blk, 0, ctx->stream>>>(grp, Npix, cursor, slot_pix, D.Q, d_qmap, d_pd, d_mt, d_dm, d_grp, win);
    QMRI_HIP(ctx, hipGetLastError());
    const DictGroupView gv = {slot_pix, tile_grp, slot_beg, D.d_gtile, D.d_gptr, D.G, w.slot_cap};
    QMRI_TRY(dict_launch_grouped(ctx, d_X, Npix, gv, w.ntiles, d_qmap, d_pd, d_mt, d_dm, win));
    if (d_xfit) QMRI_TRY(dict_launch_xfit(ctx, win, Npix, d_xfit));
    return QMRI_OK;
}
