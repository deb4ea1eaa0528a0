// nufft_plan_test.cpp -- the host planning of a trajectory operator (csrc/nufft_plan.h): the functions qmri_set_operator_nufft, qmri_build_spiral_traj
// and qmri_nufft_dcf call, on a machine without a GPU and under the address and undefined-behaviour sanitizers.  Built and run by
// tests/test_nufft_plan_host.py, which compares the lines printed here with the values the planner gave before it was moved into the header.
//   stdout: per case  "<name> m=<m> nseg=<segments> nred=<split tiles> nslot=<partial slots> list=<list entries> digest=<FNV-1a of perm, t, list, segs, reds>"
//           then the float tables of case A at width 12 ("dump <table> <values, %.17g>") and the kernel sums ("ksum <w> <I>", "kappa <T> <w> <kappa>")
// For every case the program itself checks what holds whatever the segment length is (check_plan), and once the Gauss-Legendre rule and the spiral
// builder's capacity rule.  Exit status 1: a check failed (named on stderr).
#include <cinttypes>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include "nufft_plan.h"

using namespace nuplan;

static int g_failed = 0;
static std::string g_case = "-";
#define EXPECT(cond) do { if (!(cond)) { if (++g_failed <= 20) fprintf(stderr, "nufft_plan_test: %s: line %d: %s is false\n", g_case.c_str(), __LINE__, #cond); } } while (0)

// ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
struct Traj { int N = 0, M = 0, T = 0; std::vector<int32_t> fp; std::vector<double> om; };
// omega in [-pi, pi) from a fixed 64-bit linear congruential recurrence (no library generator: the same values everywhere)
static void fill_random(std::vector<double>& om, uint64_t seed) {
    uint64_t x = seed;
    for (double& v : om) { x = x * 6364136223846793005ull + 1442695040888963407ull; v = PI * (2.0 * ((double)(x >> 11) / 9007199254740992.0) - 1.0); }
}
static Traj case_a() {             // 16 x 24, 3 frames, 64 samples; the first eight are the corners and edges of [-pi, pi]^2 (tests/test_nufft_host.py gridding_case)
    Traj k; k.N = 16; k.M = 24; k.T = 3; k.fp = {0, 20, 45, 64}; k.om.resize(128);
    fill_random(k.om, 14);
    const double edge[16] = {PI, PI, -PI, -PI, PI, -PI, -PI, PI, 0.0, 0.0, -PI, 1e-9, 1e-12, PI, PI, 0.3};
    std::copy(edge, edge + 16, k.om.begin());
    return k;
}
static Traj case_b() {             // 32 x 32, the library's own spiral, S = 60, T = 48
    Traj k; k.N = k.M = 32; k.T = 48; k.fp.assign(49, -1); k.om.assign(2 * 60 * 48, 0.0);
    EXPECT(spiral_traj_build(60, 48, k.fp.data(), k.om.data(), 60 * 48) == 60 * 48);
    return k;
}
static Traj case_c() {             // 32 x 64, 700 samples in 7 frames: the rectangular case
    Traj k; k.N = 32; k.M = 64; k.T = 7; k.om.resize(1400);
    for (int t = 0; t <= 7; ++t) k.fp.push_back(100 * t);
    fill_random(k.om, 5);
    return k;
}
static Traj case_d() {             // one sample at (pi, -pi) on 16 x 16
    Traj k; k.N = k.M = 16; k.T = 1; k.fp = {0, 1}; k.om = {PI, -PI};
    return k;
}
static Traj case_e() {             // 1100 samples all at (0, 0) on 16 x 16: every reached tile is cut into 3 segments
    Traj k; k.N = k.M = 16; k.T = 2; k.fp = {0, 600, 1100}; k.om.assign(2200, 0.0);
    return k;
}
// calls f(name, trajectory, width, seg) for every case
template <class F> static void for_each_case(F f) {
    auto run = [&](const char* name, const Traj& k, std::vector<int> widths, std::vector<int> segs) {
        for (int w : widths)
            for (int seg : segs) f(std::string(name) + "/w" + std::to_string(w) + "/seg" + std::to_string(seg), k, w, seg);
    };
    run("A_16x24", case_a(), {2, 7, 12, 16}, {512, 32});
    run("B_spiral32", case_b(), {12}, {512, 32});
    run("C_32x64", case_c(), {12}, {512});
    run("D_corner16", case_d(), {2, 16}, {512});
    run("E_pile16", case_e(), {12}, {512});
}

// ---- what holds whatever the segment length is ---------------------------------------------------------------------------------------------------
static int wrap_ref(int k, int G) { return ((k % G) + G) % G; }
static void check_plan(const Traj& k, const NufftPlan& p, int w, int seg) {
    const int N = k.N, M = k.M, m = k.fp[k.T], G1 = 2 * N, G2 = 2 * M, nt1 = G1 / NU_TB, nt2 = G2 / NU_TB, ntile = nt1 * nt2;
    EXPECT(p.u.size() == 2 * (size_t)m && p.ph.size() == 2 * (size_t)m && p.t.size() == (size_t)m && p.perm.size() == (size_t)m);
    EXPECT(p.dp.size() == (size_t)N + M && p.ramp.size() == 2 * ((size_t)N + M));
    if (g_failed) return;
    // perm is a permutation; tiles of floor(u) ascend along the sorted order, ABI order inside a tile; t is the frame of perm
    std::vector<uint8_t> seen(m, 0);
    int last_tile = -1;
    for (int e = 0; e < m; ++e) {
        const int i = p.perm[e];
        EXPECT(i >= 0 && i < m && !seen[i]);
        if (g_failed) return;
        seen[i] = 1;
        EXPECT(p.u[2 * e] == k.om[2 * i] * N / PI && p.u[2 * e + 1] == k.om[2 * i + 1] * M / PI);
        const int tile = (wrap_ref((int)std::floor(p.u[2 * e]), G1) / NU_TB) * nt2 + wrap_ref((int)std::floor(p.u[2 * e + 1]), G2) / NU_TB;
        EXPECT(tile >= last_tile);
        if (tile == last_tile) EXPECT(i > p.perm[e - 1]);
        last_tile = tile;
        EXPECT(p.t[e] >= 0 && p.t[e] < k.T && k.fp[p.t[e]] <= i && i < k.fp[p.t[e] + 1]);
    }
    // segments: ordered by non-increasing length (ties keep the order they were cut in), lengths sum to the list
    size_t total = 0;
    std::map<int, std::vector<NuSeg>> by_tile;
    for (size_t q = 0; q < p.segs.size(); ++q) {
        const NuSeg& s = p.segs[q];
        EXPECT(s.tile >= 0 && s.tile < ntile && s.b >= 0 && s.b <= s.e && (size_t)s.e <= p.list.size() && s.e - s.b <= seg);
        if (g_failed) return;
        if (q > 0) {
            const NuSeg& r = p.segs[q - 1];
            EXPECT(r.e - r.b >= s.e - s.b);
            if (r.e - r.b == s.e - s.b) EXPECT(r.tile < s.tile || (r.tile == s.tile && r.b < s.b));
        }
        total += (size_t)(s.e - s.b);
        by_tile[s.tile].push_back(s);
    }
    EXPECT(total == p.list.size() && by_tile.size() == (size_t)ntile);
    std::map<int, NuRed> red_of;
    for (const NuRed& r : p.reds) { EXPECT(r.pad == 0 && !red_of.count(r.tile)); red_of[r.tile] = r; }
    // every tile's segments tile its list range (tile after tile) without gap or overlap; the slots
    std::vector<uint8_t> slot_seen((size_t)std::max(p.nslot, 0), 0);
    std::vector<std::pair<int, int>> range(ntile);
    int at = 0;
    for (int tile = 0; tile < ntile && !g_failed; ++tile) {
        std::vector<NuSeg>& v = by_tile[tile];
        std::sort(v.begin(), v.end(), [](const NuSeg& a, const NuSeg& b) { return a.b < b.b; });
        const int b0 = at;
        for (const NuSeg& s : v) { EXPECT(s.b == at); at = s.e; }
        range[tile] = {b0, at};
        EXPECT((int)v.size() == std::max(1, (at - b0 + seg - 1) / seg));
        if (v.size() == 1) { EXPECT(v[0].slot == -1 && !red_of.count(tile)); continue; }
        EXPECT(red_of.count(tile) == 1);
        if (g_failed) return;
        const NuRed r = red_of[tile];
        EXPECT(r.nslot == (int)v.size() && r.slot0 >= 0 && r.slot0 + r.nslot <= p.nslot);
        if (g_failed) return;
        for (size_t q = 0; q < v.size(); ++q) { EXPECT(v[q].slot == r.slot0 + (int)q && !slot_seen[v[q].slot]); slot_seen[v[q].slot] = 1; }
    }
    EXPECT((size_t)at == p.list.size());
    for (uint8_t s : slot_seen) EXPECT(s == 1);
    if (g_failed) return;
    // the tiles whose list holds a sample are the tiles its w x w window touches, recomputed here from k0 = ceil(u - w/2) with wrap-around; once each
    std::vector<std::set<int>> holds(m);
    for (int tile = 0; tile < ntile; ++tile)
        for (int q = range[tile].first; q < range[tile].second; ++q) {
            const int e = p.list[q];
            EXPECT(e >= 0 && e < m);
            if (g_failed) return;
            EXPECT(holds[e].insert(tile).second);
        }
    for (int e = 0; e < m; ++e) {
        std::set<int> touched;
        const int k01 = (int)std::ceil(p.u[2 * e] - 0.5 * w), k02 = (int)std::ceil(p.u[2 * e + 1] - 0.5 * w);
        for (int a = 0; a < w; ++a)
            for (int b = 0; b < w; ++b) touched.insert((wrap_ref(k01 + a, G1) / NU_TB) * nt2 + wrap_ref(k02 + b, G2) / NU_TB);
        EXPECT(touched == holds[e]);
    }
}

// Gauss-Legendre with n = 200 integrates polynomials up to degree 399 exactly: 200 terms of an ulp each, a decade of margin -> 1e-13
static void check_gauss_legendre() {
    g_case = "gauss_legendre";
    std::vector<double> x, wt;
    gauss_legendre(200, x, wt);
    EXPECT(x.size() == 200 && wt.size() == 200);
    if (g_failed) return;
    double s0 = 0.0, s2 = 0.0, s4 = 0.0, s8 = 0.0;
    for (int i = 0; i < 200; ++i) {
        const double x2 = x[i] * x[i];
        s0 += wt[i]; s2 += wt[i] * x2; s4 += wt[i] * x2 * x2; s8 += wt[i] * x2 * x2 * x2 * x2;
        EXPECT(x[i] == -x[199 - i] && wt[i] == wt[199 - i] && wt[i] > 0.0);
        if (i > 0) EXPECT(x[i] > x[i - 1]);
    }
    EXPECT(std::fabs(s0 - 2.0) <= 1e-13 && std::fabs(s2 - 2.0 / 3.0) <= 1e-13 && std::fabs(s4 - 2.0 / 5.0) <= 1e-13 && std::fabs(s8 - 2.0 / 9.0) <= 1e-13);
}

static uint64_t digest(const NufftPlan& p) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* q, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)q)[i]; h *= 1099511628211ull; } };
    mix(p.perm.data(), p.perm.size() * sizeof(int32_t)); mix(p.t.data(), p.t.size() * sizeof(int32_t)); mix(p.list.data(), p.list.size() * sizeof(int32_t));
    mix(p.segs.data(), p.segs.size() * sizeof(NuSeg)); mix(p.reds.data(), p.reds.size() * sizeof(NuRed));
    return h;
}
static void dump(const char* name, const double* v, size_t n) {
    printf("dump %s", name);
    for (size_t i = 0; i < n; ++i) printf(" %.17g", v[i]);
    printf("\n");
}

int main() {
    static_assert(sizeof(NuSeg) == 16 && sizeof(NuRed) == 16, "the device reads these layouts");
    static_assert(NU_WMAX <= NU_TB, "a window reaches at most two tiles per axis");
    {   // the capacity rule of the spiral builder: the count comes back whatever the capacity, and nothing is written past it
        g_case = "spiral_capacity";
        const Traj b = case_b();
        std::vector<int32_t> fp(49, -1);
        std::vector<double> part(2 * 100 + 2, -7.0);
        EXPECT(spiral_traj_build(60, 48, fp.data(), part.data(), 100) == 2880 && fp == b.fp && part[200] == -7.0 && std::equal(part.begin(), part.begin() + 200, b.om.begin()));
        EXPECT(spiral_traj_build(60, 48, fp.data(), nullptr, 0) == 2880 && fp[48] == 2880 && fp[1] == 60);
        for (double v : b.om) EXPECT(std::fabs(v) <= PI);
    }
    check_gauss_legendre();
    EXPECT(nufft_kernel_ok(2) && nufft_kernel_ok(NU_WMAX) && nufft_kernel_ok(NU_WDEF) && !nufft_kernel_ok(1) && !nufft_kernel_ok(NU_WMAX + 1));
    for_each_case([&](const std::string& name, const Traj& k, int w, int seg) {
        g_case = name;
        const NufftPlan p = nu_plan(k.N, k.M, k.T, k.fp.data(), k.om.data(), w, seg);
        check_plan(k, p, w, seg);
        printf("%s m=%d nseg=%zu nred=%zu nslot=%d list=%zu digest=%016" PRIx64 "\n", name.c_str(), (int)k.fp[k.T], p.segs.size(), p.reds.size(), p.nslot,
               p.list.size(), digest(p));
        if (name == "A_16x24/w12/seg512") {
            std::vector<double> perm(p.perm.begin(), p.perm.end());
            dump("omega", k.om.data(), k.om.size()); dump("perm", perm.data(), perm.size());
            dump("u", p.u.data(), p.u.size()); dump("ph", p.ph.data(), p.ph.size()); dump("dp", p.dp.data(), p.dp.size()); dump("ramp", p.ramp.data(), p.ramp.size());
        }
        if (name == "E_pile16/w12/seg512") EXPECT(p.reds.size() == 4 && p.nslot == 12 && p.segs.size() == 12);   // the window wraps: all 2 x 2 tiles are reached, 3 segments each
    });
    for (int w = 2; w <= NU_WMAX; ++w) { printf("ksum %d %.17g\n", w, kernel_sum(w, nu_beta(w))); printf("kappa 48 %d %.17g\n", w, dcf_kappa(48, w, nu_beta(w))); }
    if (g_failed) fprintf(stderr, "nufft_plan_test: %d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
