// Stand-alone check of csrc/dict_plan.h (tests/test_dict_plan_host.py builds it with the address and undefined-behaviour sanitizers): what must
// hold of the dictionary match's work split whatever its thresholds are, through the functions the library and its kernels call.  Then it prints
// the plans at the shapes the GPU tests and the benchmark reach, which the Python side compares with recorded ones.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dict_plan.h"

using namespace dplan;

#define REQUIRE(cond, ...)                                                          \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #cond);  \
            std::fprintf(stderr, __VA_ARGS__);                                      \
            std::fprintf(stderr, "\n");                                             \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static const int NPIX[] = {1, 31, 32, 33, 127, 128, 129, 300, 1600, 4096, 50176, 65536};
static const int SLOTS[] = {256, 512, 768, 1024, 1280, 1536, 1792, 2048, 777, 1301};
static const int SLOTS_FEW[] = {256, 1280, 2048, 777, 1301};                       // for the sweeps that walk every tile

// The launched parts of [t0, tall): every tile in exactly one part; with `exact`, the four waves' tiles of all parts likewise; filter parts are
// whole steps and only part 0 lists the range's first tile; `own` parts have tiles, the parts beyond them none.
static void check_parts(int t0, int tall, int launched, int own, bool filt, bool grouped, int tper_host) {
    std::vector<int> seen(tall - t0, 0), wseen(tall - t0, 0);
    int listed = 0;
    for (int y = 0; y < launched; ++y) {
        const TileRange r = grouped ? dict_group_part(t0, tall, launched, y, filt ? MIN_TILES : MIN_TILES_EXACT, filt ? FSTEP : 1)
                                    : dict_part(t0, tall, filt ? tper_host : dict_tper(tall - t0, launched, 1), y);
        REQUIRE(r.tbeg <= r.tend, "part %d of %d, tiles %d", y, launched, tall - t0);
        REQUIRE((y < own) == (r.tend > r.tbeg), "part %d of %d (own %d), tiles %d: [%d, %d)", y, launched, own, tall - t0, r.tbeg, r.tend);
        if (r.tend == r.tbeg) continue;
        REQUIRE(r.tbeg >= t0 && r.tend <= tall, "part %d outside the range", y);
        for (int t = r.tbeg; t < r.tend; ++t) ++seen[t - t0];
        if (filt) {
            REQUIRE((r.tbeg - t0) % FSTEP == 0, "part %d starts off a step", y);
            REQUIRE((r.tend - r.tbeg) % FSTEP == 0 || r.tend == tall, "part %d is not whole steps", y);
            if (dict_lists_first_tile(r, y)) { ++listed; REQUIRE(r.tbeg == t0, "the listed tile is not the range's first"); }
        } else {
            for (int w = 0; w < 4; ++w)
                for (int i = 0; i < dict_wave_count(r, w); ++i) {
                    const int t = dict_wave_tile(r, w, i);
                    REQUIRE(t >= r.tbeg && t < r.tend, "wave %d tile %d outside its part", w, t);
                    ++wseen[t - t0];
                }
        }
    }
    for (int t = 0; t < tall - t0; ++t) {
        REQUIRE(seen[t] == 1, "tile %d of %d covered %d times by %d parts", t, tall - t0, seen[t], launched);
        if (!filt) REQUIRE(wseen[t] == 1, "tile %d of %d walked by %d waves", t, tall - t0, wseen[t]);
    }
    if (filt) REQUIRE(listed == 1, "first tile listed by %d parts", listed);
}

static void narrow_and_grouped() {
    for (int npix : NPIX)
        for (int slots : SLOTS_FEW)
            for (int filt = 0; filt < 2; ++filt) {
                for (int nt = 1; nt <= 6000; nt += (nt < 300 ? 1 : 97)) {
                    const MatchPlan p = dict_plan_narrow(npix, nt, filt, slots);
                    REQUIRE(p.P >= 1 && p.gx == p.ptiles && p.ptiles >= 1, "narrow plan");
                    REQUIRE(p.npart == (p.P > 1 ? (size_t)p.P * npix : 0) && p.ngmax == (filt ? (size_t)npix : 0), "narrow scratch");
                    check_parts(0, nt, p.P, p.P, filt, false, p.tper);               // the host's cut: no empty part
                    if (p.seed) {
                        const int nsteps = (nt + FSTEP - 1) / FSTEP;
                        REQUIRE(filt && p.P > 1 && dict_seed_on(nsteps) && p.Ps >= 1 && p.seed_stride >= 1, "seed launch");
                        for (int y = 0; y < p.Ps; ++y)
                            for (unsigned k = 0; k < 40; ++k) {
                                const int st = dict_seed_step(y, p.Ps, k, p.seed_stride, nsteps);
                                REQUIRE(st >= 0 && st <= nsteps, "seed step %d of %d", st, nsteps);
                            }
                    } else REQUIRE(p.Ps == 0, "no seed launch, Ps = %d", p.Ps);
                }
                // groups: the plan comes from the largest one; each group cuts itself on the device
                const int padw = filt ? 128 : 32;
                for (int gmax = 1; gmax <= 1000; gmax += (gmax < 130 ? 1 : 13)) {
                    MatchPlan p{};
                    for (int G : {1, 3, 5, 64, 256}) {                              // (G moves the slot tiles, not the parts)
                        const DictgWork w = dictg_work(npix, G, padw);
                        p = dict_plan_grouped(npix, w.ntiles, w.slot_cap, gmax, filt, slots);
                        REQUIRE(p.P >= 1 && p.gx == w.ntiles && p.tper == 0 && p.seed_stride == 0, "grouped plan");
                        REQUIRE(p.npart == (p.P > 1 ? (size_t)p.P * w.slot_cap : 0) && p.ngmax == (filt ? (size_t)w.slot_cap : 0), "grouped scratch");
                    }
                    for (int ntl : {gmax, (gmax + 1) / 2, 1 + gmax / 3, 1}) {
                        const int own = dict_nparts(ntl, p.P, filt ? MIN_TILES : MIN_TILES_EXACT);
                        const int tper = dict_tper(ntl, own, filt ? FSTEP : 1);
                        check_parts(1000, 1000 + ntl, p.P, (ntl + tper - 1) / tper, filt, true, 0);
                        if (p.seed) {                                           // the group's own seed steps
                            const int nsteps = (ntl + FSTEP - 1) / FSTEP;
                            if (dict_seed_on(nsteps))
                                for (int y = 0; y < p.Ps; ++y)
                                    for (unsigned k = 0; k < 40; ++k) {
                                        const int st = dict_seed_step(y, p.Ps, k, dict_seed_stride(nsteps), nsteps);
                                        REQUIRE(st >= 0 && st <= nsteps, "group seed step %d of %d", st, nsteps);
                                    }
                        }
                    }
                }
            }
}

static void visiting_order() {
    for (int n = 0; n <= 300; ++n) {
        const BrevOrder o = brev_order(n);
        std::vector<int> seen(n, 0);
        unsigned k = 0;
        for (int it = 0; it < n; ++it) {
            const int i = brev_next(o, k);
            REQUIRE(i >= 0 && i < n, "n = %d: i = %d", n, i);
            ++seen[i];
        }
        for (int i = 0; i < n; ++i) REQUIRE(seen[i] == 1, "n = %d: i = %d visited %d times", n, i, seen[i]);
        REQUIRE(brev_next(o, k) == n && brev_next(o, k) == n, "n = %d: not exhausted", n);
    }
}

static void wide() {
    for (int npix : NPIX)
        for (int slots : SLOTS_FEW)
            for (int lsp = 0; lsp <= 6; ++lsp)
                for (int AT : {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 100, 768, 1600}) {
                    const WidePlan p = dict_plan_wide(npix, 4 * AT, 4, slots, lsp);
                    REQUIRE(p.PT == (npix + 127) / 128 && p.AT == AT && p.P >= 1 && p.P <= AT && p.lsp == lsp, "wide plan");
                    REQUIRE(p.grid % 512 == 0 && p.grid >= 64u * (unsigned)p.nsuper, "wide grid");
                    std::vector<int> seen((size_t)p.PT * p.P, 0), tiles(AT, 0);
                    for (unsigned id = 0; id < p.grid; ++id) {
                        int pt = -1, prt = -1;
                        if (!dictw_decode((int)id, p.PT, p.P, p.lsp, pt, prt)) continue;
                        REQUIRE(pt >= 0 && pt < p.PT && prt >= 0 && prt < p.P, "id %u -> (%d, %d)", id, pt, prt);
                        ++seen[(size_t)pt * p.P + prt];
                    }
                    for (size_t i = 0; i < seen.size(); ++i) REQUIRE(seen[i] == 1, "pair %zu reached by %d workgroups (PT %d, P %d, lsp %d)", i, seen[i], p.PT, p.P, lsp);
                    for (int prt = 0; prt < p.P; ++prt) {
                        const TileRange r = dict_part(0, AT, p.tper, prt);
                        REQUIRE(r.tend > r.tbeg, "wide part %d of %d is empty (AT %d)", prt, p.P, AT);
                        for (int t = r.tbeg; t < r.tend; ++t) ++tiles[t];
                    }
                    for (int t = 0; t < AT; ++t) REQUIRE(tiles[t] == 1, "wide tile %d covered %d times", t, tiles[t]);
                }
    for (int lsp : {-3, 9}) REQUIRE(dict_plan_wide(4096, 128, 4, 1024, lsp).lsp == (lsp < 0 ? 0 : 6), "lsp is clamped");
}

static void scores_and_layout() {
    for (int n : NPIX)
        for (int slots : SLOTS)
            for (int G : {1, 3, 5, 64, 256}) {
                for (int gmax = 1; gmax <= 1000; gmax += 9) {
                    const ScoresPlan p = dict_plan_scores(n, G, gmax, slots);
                    REQUIRE(p.grun >= 1 && p.grun <= G && p.P >= 1 && p.P <= SCORE_MAX_PARTS, "scores plan");
                    REQUIRE(p.P == 1 || p.grun == 1, "atom parts (%d) with runs of %d groups", p.P, p.grun);
                    std::vector<int> seen(G, 0);
                    for (int y = 0; y < p.nruns; ++y)
                        for (int g = y * p.grun; g < imin(G, (y + 1) * p.grun); ++g) ++seen[g];
                    for (int g = 0; g < G; ++g) REQUIRE(seen[g] == 1, "group %d in %d runs", g, seen[g]);
                    const int own = dict_nparts(gmax, p.P, MIN_TILES), tper = dict_tper(gmax, own, 1);
                    std::vector<int> tiles(gmax, 0);
                    for (int z = 0; z < p.P; ++z) {
                        const TileRange r = dict_group_part(5, 5 + gmax, p.P, z, MIN_TILES, 1);
                        REQUIRE((z < (gmax + tper - 1) / tper) == (r.tend > r.tbeg), "scores part %d", z);
                        for (int t = r.tbeg; t < r.tend; ++t) ++tiles[t - 5];
                    }
                    for (int t = 0; t < gmax; ++t) REQUIRE(tiles[t] == 1, "scores tile %d covered %d times", t, tiles[t]);
                }
                for (int padw : {32, 128}) {
                    const DictgWork w = dictg_work(n, G, padw);
                    REQUIRE(w.slot_cap % padw == 0 && w.slot_cap == w.ntiles * padw, "slot_cap %d", w.slot_cap);
                    REQUIRE(w.slot_cap >= n + G * (padw - 1), "slot_cap %d < %d pixels + padding of %d groups", w.slot_cap, n, G);
                    // grp [Npix], count [256], cursor [256], slot_beg [G + 1 <= 257], tile_grp [ntiles], slot_pix [slot_cap]
                    REQUIRE(w.grp + (size_t)n <= w.count && w.count + 256 <= w.cursor && w.cursor + 256 <= w.slot_beg && w.slot_beg + (size_t)G + 1 <= w.tile_grp &&
                                w.tile_grp + (size_t)w.ntiles <= w.slot_pix && w.slot_pix + (size_t)w.slot_cap <= w.total,
                            "regions overlap (Npix %d, G %d, padw %d)", n, G, padw);
                }
            }
}

static void print_plans() {
    for (int k = 1; k <= 8; ++k) {
        const int slots = 256 * k;
        const struct { const char* name; int nt, npix; } nar[] = {{"narrow_3072_50176", 3072, 50176}, {"narrow_1250_1600", 1250, 1600}, {"narrow_1024_50176", 1024, 50176}};
        for (const auto& c : nar)
            for (int filt = 0; filt < 2; ++filt) {
                const MatchPlan p = dict_plan_narrow(c.npix, c.nt, filt, slots);
                std::printf("%s/f%d/k%d P=%d tper=%d seed=%d Ps=%d seed_stride=%d\n", c.name, filt, k, p.P, p.tper, (int)p.seed, p.Ps, p.seed_stride);
            }
        for (int filt = 0; filt < 2; ++filt) {
            const DictgWork w = dictg_work(1600, 3, filt ? 128 : 32);
            const MatchPlan p = dict_plan_grouped(1600, w.ntiles, w.slot_cap, 625, filt, slots);
            std::printf("grouped_407_625_219_1600/f%d/k%d P=%d tper=%d seed=%d Ps=%d seed_stride=%d", filt, k, p.P, p.tper, (int)p.seed, p.Ps, p.seed_stride);
            int g = 0;
            for (int ntl : {407, 625, 219}) {                               // each group's own parts and tiles per part
                const int np = dict_nparts(ntl, p.P, filt ? MIN_TILES : MIN_TILES_EXACT);
                std::printf(" g%d=%d/%d", g++, np, dict_tper(ntl, np, filt ? FSTEP : 1));
            }
            std::printf("\n");
        }
        for (int n : {301, 6}) {
            const ScoresPlan s = dict_plan_scores(n, 3, 407, slots);
            std::printf("scores_%d_3_407/k%d grun=%d nruns=%d P=%d\n", n, k, s.grun, s.nruns, s.P);
        }
        const WidePlan w1 = dict_plan_wide(50176, 4 * 768, 126, slots, 2), w2 = dict_plan_wide(4096, 4 * 32, 4, slots, 2);
        std::printf("wide_768_392/k%d P=%d tper=%d grid=%u\n", k, w1.P, w1.tper, w1.grid);
        std::printf("wide_32_32/k%d P=%d tper=%d grid=%u\n", k, w2.P, w2.tper, w2.grid);
    }
}

int main() {
    narrow_and_grouped();
    visiting_order();
    wide();
    scores_and_layout();
    print_plans();
    return 0;
}
