// dict_plan.h -- how the dictionary match cuts its atom tiles into parts over workgroups, and which tiles a workgroup or a wave then walks: the
// launch plans of the narrow, grouped and wide match and of the group scores (host), and the functions the kernels and the host must agree on
// (DP_HD: part of a tile range, a wave's share, the bit-reversed visiting order, the seed rule, the wide kernel's workgroup order).  No HIP, no
// context: plain C++17 of integers, so that tests/cpp/dict_plan_test.cpp runs the functions the library and its kernels call under the host
// sanitizers on a machine without a GPU.  dict_kernels.hip, dictw_kernels.hip, dictb_kernels.hip and dictg_kernels.hip query the resident
// workgroups (`slots`), call these, size their scratch and launch; nothing else decides.
#ifndef QMRI_DICT_PLAN_H           // (a guard, not #pragma once: the header is also compiled on its own)
#define QMRI_DICT_PLAN_H

#include <cstddef>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DP_HD __host__ __device__ __forceinline__
#else
#define DP_HD inline
#endif

namespace dplan {

constexpr int LCAP = 128;       // tiles a wave collects for the exact products before it works them off
constexpr int FSTEP = 8;        // tiles per LDS step: 16 KB of f16 pieces, [tile][hi | lo][lane] of 16 bytes
// atom parts: none if the pixel tiles fill the device's resident workgroups at least four times over (a ragged last round then
// costs little), else as many as give ~8 rounds, each part keeping >= 64 atom tiles per wave
constexpr int ROUNDS_WHOLE = 4, ROUNDS_SPLIT = 8;
constexpr int MIN_TILES = 64, MIN_TILES_EXACT = 4 * MIN_TILES;     // per part: the filter's waves walk all tiles of a part, the exact kernel's four share them
// seed launch: ~12 steps of the whole dictionary per pixel, spread over as many workgroups as give one round of the device
// (skipped for a dictionary, or a group, of fewer than 48 steps)
constexpr int SEED_MIN_STEPS = 48, SEED_STEPS = 12;
// wide match, atom parts: ~20 rounds of the device's resident workgroups (a ragged last round then costs < 5 %), whole groups of 16 for the XCD super-tiles
constexpr int WIDE_ROUNDS = 20, WIDE_PART_GROUP = 16;
constexpr int SCORE_MAX_PARTS = 1024;                               // group scores: most atom parts of a launch (grid z)

DP_HD int imin(int a, int b) { return a < b ? a : b; }
DP_HD int imax(int a, int b) { return a > b ? a : b; }

// ---- shared by the host and the kernels ------------------------------------------------------------------------------------------------------
// The part of a tile range.  ntl tiles are cut into as many of the launched parts as keep >= min_tiles tiles each (at least one), every part
// `tper` tiles: whole steps of `step` tiles.  Part `part` of [t0, tall) is [tbeg, tend); a part beyond the range's own is empty (tbeg == tend).
// k_dict_match cuts a group with (MIN_TILES_EXACT, 1), k_dict_match_f with (MIN_TILES, FSTEP), k_dictb_scores with (MIN_TILES, 1); where the
// host has cut (the narrow match: tper an argument, or all launched parts in use) the kernels go through dict_part alone.
struct TileRange { int tbeg, tend; };
DP_HD int dict_nparts(int ntl, int launched, int min_tiles) { return imax(1, imin(launched, ntl / min_tiles)); }
DP_HD int dict_tper(int ntl, int nparts, int step) { return ((ntl + nparts - 1) / nparts + step - 1) / step * step; }
DP_HD TileRange dict_part(int t0, int tall, int tper, int part) {
    const int tbeg = t0 + part * tper;
    return {tbeg, imax(tbeg, imin(tall, tbeg + tper))};
}
DP_HD TileRange dict_group_part(int t0, int tall, int launched, int part, int min_tiles, int step) {
    return dict_part(t0, tall, dict_tper(tall - t0, dict_nparts(tall - t0, launched, min_tiles), step), part);
}

// The filter lists the FIRST tile of its dictionary (of its group) whatever it finds: part 0 does, when it has tiles (k_dict_match_f has the reason).
DP_HD bool dict_lists_first_tile(TileRange r, int part) { return part == 0 && r.tend > r.tbeg; }

// The exact kernel's waves share a part: wave w of 4 takes the tiles tbeg + w + 4 i, i = 0 .. n-1 (n <= 0: none).
DP_HD int dict_wave_count(TileRange r, int wave) { return (r.tend - r.tbeg - wave + 3) / 4; }
DP_HD int dict_wave_tile(TileRange r, int wave, int i) { return r.tbeg + wave + 4 * i; }

// Visiting order: i = 0 .. n-1 in BIT-REVERSED order -- coarse to fine over the whole range (k_dict_match has the reason).  The counter k
// starts at 0; brev_next gives the next valid i at or after it (n when exhausted) and moves k past it.
struct BrevOrder { int n, nb; unsigned kend; };
DP_HD unsigned brev32(unsigned v) {
#if defined(__clang__)
    return __builtin_bitreverse32(v);                                   // (s_brev_b32)
#else
    unsigned r = 0;
    for (int b = 0; b < 32; ++b) r |= ((v >> b) & 1u) << (31 - b);
    return r;
#endif
}
DP_HD BrevOrder brev_order(int n) {
    int nb = 0;
    while ((1 << nb) < n) ++nb;
    return {n, nb, 1u << nb};
}
DP_HD int brev_next(const BrevOrder& o, unsigned& k) {
    while (k < o.kend) {
        const int i = o.nb ? (int)(brev32(k) >> (32 - o.nb)) : 0;
        ++k;
        if (i < o.n) return i;
    }
    return o.n;
}

// The seed launch samples every stride-th step of a range of nsteps steps, workgroup y of ny taking the steps (y + ny k) stride, k = 0, 1, ..
// (nsteps when exhausted); ranges of fewer than SEED_MIN_STEPS steps are not seeded.
DP_HD bool dict_seed_on(int nsteps) { return nsteps >= SEED_MIN_STEPS; }
DP_HD int dict_seed_stride(int nsteps) { return imax(1, nsteps / SEED_STEPS); }
DP_HD int dict_seed_step(unsigned y, unsigned ny, unsigned k, int stride, int nsteps) {
    const long i = ((long)y + (long)ny * k) * stride;
    return i < nsteps ? (int)i : nsteps;
}

// Wide match, workgroup order: id % 8 is the XCD under round-robin placement (speed only); an XCD walks super-tiles of 2^lsp pixel tiles x
// 2^(6 - lsp) atom parts (64 workgroups = what it holds at once).  dictw_decode: the (pixel tile, atom part) of workgroup id, false for an id
// of the padded grid that has none.
DP_HD int dictw_nsuper(int PT, int P, int lsp) {
    const int lsa = 6 - lsp;
    return ((PT + (1 << lsp) - 1) >> lsp) * ((P + (1 << lsa) - 1) >> lsa);
}
DP_HD unsigned dictw_grid(int PT, int P, int lsp) { return 8u * 64u * (unsigned)((dictw_nsuper(PT, P, lsp) + 7) / 8); }
DP_HD bool dictw_decode(int id, int PT, int P, int lsp, int& pt, int& prt) {
    const int xcd = id & 7, kk = id >> 3;
    const int lsa = 6 - lsp;
    const int SPT = (PT + (1 << lsp) - 1) >> lsp;
    const int sidx = xcd + 8 * (kk >> 6), within = kk & 63;
    if (sidx >= dictw_nsuper(PT, P, lsp)) return false;
    pt = ((sidx % SPT) << lsp) + (within & ((1 << lsp) - 1));
    prt = ((sidx / SPT) << lsa) + (within >> lsp);
    return pt < PT && prt < P;
}

// ---- host plans ------------------------------------------------------------------------------------------------------------------------------
// `slots`: workgroups of the launch's kernel the device holds at once (occupancy query).

// Narrow and grouped match: grid (gx, P); seed: a first launch of grid (gx, Ps) (k_dict_match_f).  npart / ngmax: elements of the parts'
// candidates (0: no parts, no merge) and of the filter's running maxima (0: no filter).
struct MatchPlan { int ptiles, gx, P, tper; bool seed; int Ps, seed_stride; size_t npart, ngmax; };

inline int dict_match_parts(int ptiles, int slots, int tiles, bool filt) {
    int P = 1;
    if (ptiles < ROUNDS_WHOLE * slots) {
        P = (ROUNDS_SPLIT * slots + ptiles - 1) / ptiles;
        P = imax(1, imin(P, tiles / (filt ? MIN_TILES : MIN_TILES_EXACT)));
    }
    return P;
}
inline int dict_pixel_tiles(int Npix, bool filt) { return filt ? (Npix + 127) / 128 : (Npix + 31) / 32; }

// ntiles: 32-atom tiles of the dictionary.  tper is the filter kernel's argument (the exact kernel cuts its P parts itself, dict_tper(.., 1)).
inline MatchPlan dict_plan_narrow(int Npix, int ntiles, bool filt, int slots) {
    MatchPlan p{};
    p.ptiles = p.gx = dict_pixel_tiles(Npix, filt);
    p.P = dict_match_parts(p.ptiles, slots, ntiles, filt);
    p.tper = ntiles;
    if (filt) {                                                         // whole LDS steps per part, no empty part
        p.tper = dict_tper(ntiles, p.P, FSTEP);
        p.P = (ntiles + p.tper - 1) / p.tper;
    }
    const int nsteps_all = (ntiles + FSTEP - 1) / FSTEP;
    p.seed_stride = dict_seed_stride(nsteps_all);
    const int nseed = (nsteps_all + p.seed_stride - 1) / p.seed_stride;
    p.seed = filt && p.P > 1 && dict_seed_on(nsteps_all);
    p.Ps = p.seed ? imax(1, imin(nseed, (slots + p.ptiles - 1) / p.ptiles)) : 0;
    p.npart = p.P > 1 ? (size_t)p.P * Npix : 0;
    p.ngmax = filt ? (size_t)Npix : 0;
    return p;
}

// The grouped match: nslot_tiles is the largest number of slot tiles the call can have, slot_cap its slots (DictgWork); atom parts as in the
// narrow match, from the largest group's tiles (gtiles_max): a smaller group uses fewer of them (dict_group_part) and picks its own seed stride.
inline MatchPlan dict_plan_grouped(int Npix, int nslot_tiles, int slot_cap, int gtiles_max, bool filt, int slots) {
    MatchPlan p{};
    p.ptiles = dict_pixel_tiles(Npix, filt);
    p.gx = nslot_tiles;
    p.P = dict_match_parts(p.ptiles, slots, gtiles_max, filt);
    p.seed = filt && p.P > 1 && dict_seed_on((gtiles_max + FSTEP - 1) / FSTEP);
    p.Ps = p.seed ? imax(1, imin(SEED_STEPS, (slots + p.ptiles - 1) / p.ptiles)) : 0;
    p.npart = p.P > 1 ? (size_t)p.P * slot_cap : 0;
    p.ngmax = filt ? (size_t)slot_cap : 0;
    return p;
}

// The wide match: PT pixel tiles of 128, AT atom tiles of 128 (ntiles: 32-atom tiles) in P parts of tper, no empty part; the flat grid covers
// nsuper super-tiles.  nxp: float4 of the packed pixels (half as many threads pack them), npart: the parts' candidates.
struct WidePlan { int PT, AT, P, tper, lsp, nsuper; unsigned grid; size_t nxp, npart; };
inline WidePlan dict_plan_wide(int Npix, int ntiles, int G8, int slots, int lsp) {
    WidePlan p{};
    p.PT = (Npix + 127) / 128; p.AT = ntiles / 4;
    p.P = imax(1, imin(p.AT, (WIDE_ROUNDS * slots + p.PT - 1) / p.PT));
    if (p.P < p.AT) p.P = imin(p.AT, (p.P + WIDE_PART_GROUP - 1) / WIDE_PART_GROUP * WIDE_PART_GROUP);
    p.tper = (p.AT + p.P - 1) / p.P;
    p.P = (p.AT + p.tper - 1) / p.tper;                                 // no empty part
    p.lsp = imax(0, imin(6, lsp));
    p.nsuper = dictw_nsuper(p.PT, p.P, p.lsp);
    p.grid = dictw_grid(p.PT, p.P, p.lsp);
    p.nxp = (size_t)p.PT * 4 * G8 * 2 * 64;
    p.npart = (size_t)p.P * Npix;
    return p;
}

// Group scores of n pixels against G groups, grid (ptiles, nruns, P).
// Units: pixel tiles x groups fill the device's resident workgroups about eight times over.  More than that: a workgroup takes a run of groups
// (its pixels are read once per run); fewer than four times: the atoms of a group are split into parts of >= 64 tiles.
struct ScoresPlan { int ptiles, grun, nruns, P; };
inline ScoresPlan dict_plan_scores(int n, int G, int gtiles_max, int slots) {
    ScoresPlan p{};
    p.ptiles = (n + 127) / 128;
    const long long units = (long long)p.ptiles * G, whole = units / ((long long)ROUNDS_SPLIT * slots);
    p.grun = (int)(whole < 1 ? 1 : whole > G ? G : whole);
    p.nruns = (G + p.grun - 1) / p.grun;
    p.P = 1;
    if (p.grun == 1 && units < (long long)ROUNDS_WHOLE * slots) {
        p.P = (int)(((long long)ROUNDS_SPLIT * slots + units - 1) / units);
        p.P = imax(1, imin(imin(p.P, gtiles_max / MIN_TILES), SCORE_MAX_PARTS));
    }
    return p;
}

// Layout of the bucketing scratch for Npix pixels, G groups, pixel width padw (ints): the most slots a call can use is every pixel plus less than
// one width of padding per group.
struct DictgWork { int slot_cap, ntiles; size_t grp, count, cursor, slot_beg, tile_grp, slot_pix, total; };
inline DictgWork dictg_work(int Npix, int G, int padw) {
    DictgWork w;
    w.ntiles = (Npix + padw - 1) / padw + G;
    w.slot_cap = w.ntiles * padw;
    w.grp = 0; w.count = w.grp + (size_t)Npix; w.cursor = w.count + 256; w.slot_beg = w.cursor + 256; w.tile_grp = w.slot_beg + 257;
    w.slot_pix = w.tile_grp + (size_t)w.ntiles; w.total = w.slot_pix + (size_t)w.slot_cap;
    return w;
}

}  // namespace dplan

#endif  // QMRI_DICT_PLAN_H
