// refine_plan_test.cpp -- the lines of a gridded dictionary (csrc/refine_plan.h) on the host, under the address and
// undefined-behaviour sanitizers: a full tensor grid, a grid with the T2 > T1 atoms removed (ragged lines), a 3-column lut, duplicates, NaN lut rows,
// zero and non-finite normD, every refusal, and the table of unnormalised atoms.  Every case is compared with a direct O(K^2) statement of the rule.
// Built and run by tests/test_refine_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "refine_plan.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

struct Dict { int K, Q; std::vector<float> lut, normD; };     // lut column-major

static Dict grid(const std::vector<std::vector<float>>& axes) {
    Dict d; d.Q = (int)axes.size(); d.K = 1;
    for (auto& a : axes) d.K *= (int)a.size();
    d.lut.assign((size_t)d.K * d.Q, 0.f); d.normD.assign(d.K, 1.5f);
    for (int k = 0; k < d.K; ++k) {
        int r = k;
        for (int c = d.Q - 1; c >= 0; --c) { d.lut[k + (size_t)d.K * c] = axes[c][r % axes[c].size()]; r /= (int)axes[c].size(); }
    }
    return d;
}
static Dict keep(const Dict& d, const std::vector<char>& on) {
    Dict o; o.Q = d.Q; o.K = 0;
    for (char v : on) o.K += v ? 1 : 0;
    o.lut.assign((size_t)o.K * o.Q, 0.f); o.normD.assign(o.K, 0.f);
    for (int k = 0, j = 0; k < d.K; ++k)
        if (on[k]) { for (int c = 0; c < d.Q; ++c) o.lut[j + (size_t)o.K * c] = d.lut[k + (size_t)d.K * c]; o.normD[j] = d.normD[k]; ++j; }
    return o;
}

// the rule, directly
static void direct(const Dict& d, int P, const int32_t* cols, std::vector<int32_t>& nbr) {
    nbr.assign((size_t)d.K * P * 2, -1);
    auto at = [&](int k, int c) { return d.lut[k + (size_t)d.K * c]; };
    auto ok = [&](int k) { return rplan::atom_valid(d.K, d.Q, d.lut.data(), d.normD.data(), k); };
    for (int q = 0; q < P; ++q)
        for (int k = 0; k < d.K; ++k) {
            if (!ok(k)) continue;
            int up = -1, dn = -1;
            for (int b = 0; b < d.K; ++b) {
                if (b == k || !ok(b)) continue;
                bool line = true;
                for (int o = 0; o < d.Q; ++o) line = line && (o == cols[q] || at(b, o) == at(k, o));
                if (!line) continue;
                const float v = at(b, cols[q]), v0 = at(k, cols[q]);
                if (v > v0 && (up < 0 || v < at(up, cols[q]))) up = b;          // (b ascending: the lowest index of a value is met first)
                if (v < v0 && (dn < 0 || v > at(dn, cols[q]))) dn = b;
            }
            nbr[((size_t)k * P + q) * 2] = dn; nbr[((size_t)k * P + q) * 2 + 1] = up;
        }
}

static void check(const Dict& d, int P, const int32_t* cols, const char* name, int32_t* count_out = nullptr) {
    std::vector<int32_t> nbr((size_t)d.K * P * 2, 7), want;
    int32_t count[9] = {};
    const std::string msg = rplan::dict_lines(d.K, d.Q, d.lut.data(), d.normD.data(), P, cols, nbr.data(), count);
    EXPECT(msg.empty());
    direct(d, P, cols, want);
    if (nbr != want) { std::fprintf(stderr, "%s: lines differ from the direct statement\n", name); ++fails; }
    for (int q = 0; q < P; ++q) {
        int32_t c[3] = {0, 0, 0};
        for (int k = 0; k < d.K; ++k) ++c[(want[((size_t)k * P + q) * 2] >= 0) + (want[((size_t)k * P + q) * 2 + 1] >= 0)];
        EXPECT(c[0] == count[3 * q] && c[1] == count[3 * q + 1] && c[2] == count[3 * q + 2]);
        EXPECT(c[0] + c[1] + c[2] == d.K);
    }
    // neighbours are mutual along a line: the upper neighbour's lower neighbour has k's value
    for (int q = 0; q < P; ++q)
        for (int k = 0; k < d.K; ++k) {
            const int up = nbr[((size_t)k * P + q) * 2 + 1];
            if (up < 0) continue;
            const int back = nbr[((size_t)up * P + q) * 2];
            EXPECT(back >= 0 && d.lut[back + (size_t)d.K * cols[q]] == d.lut[k + (size_t)d.K * cols[q]] && back <= k);
        }
    if (count_out) std::memcpy(count_out, count, sizeof count);
    std::printf("%s K=%d", name, d.K);
    for (int q = 0; q < P; ++q) std::printf(" col%d=%d/%d/%d", cols[q], count[3 * q], count[3 * q + 1], count[3 * q + 2]);
    std::printf("\n");
}

int main() {
    const std::vector<float> t1 = {0.1f, 0.2f, 0.4f, 0.8f, 1.6f, 3.2f}, t2 = {0.05f, 0.1f, 0.3f, 0.5f}, b1 = {0.8f, 1.0f, 1.2f};
    const int32_t c01[2] = {0, 1}, c10[2] = {1, 0}, c0[1] = {0}, c1[1] = {1}, c012[3] = {0, 1, 2}, c2[1] = {2};
    int32_t count[9];
    // a full tensor grid: every line has 2 ends and n - 2 interior atoms
    Dict full = grid({t1, t2});
    check(full, 2, c01, "full", count);
    EXPECT(count[0] == 0 && count[1] == 2 * 4 && count[2] == 4 * 4 && count[3] == 0 && count[4] == 2 * 6 && count[5] == 2 * 6);
    check(full, 2, c10, "full_swapped");
    check(full, 1, c1, "full_t2_only");
    {                                                           // atom (i, j) = i * 4 + j: its T1 neighbours are 4 away, its T2 neighbours 1 away
        std::vector<int32_t> nbr((size_t)full.K * 4);
        EXPECT(rplan::dict_lines(full.K, 2, full.lut.data(), full.normD.data(), 2, c01, nbr.data(), count).empty());
        const int k = 2 * 4 + 1;
        EXPECT(nbr[k * 4 + 0] == k - 4 && nbr[k * 4 + 1] == k + 4 && nbr[k * 4 + 2] == k - 1 && nbr[k * 4 + 3] == k + 1);
        EXPECT(nbr[0] == -1 && nbr[1] == 4 && nbr[2] == -1 && nbr[3] == 1);
    }
    // ragged: the atoms with T2 > T1 removed
    std::vector<char> on(full.K);
    for (int k = 0; k < full.K; ++k) on[k] = full.lut[k + (size_t)full.K] <= full.lut[k];
    Dict rag = keep(full, on);
    EXPECT(rag.K < full.K);
    check(rag, 2, c01, "ragged", count);
    // T1 lines (one per T2) hold 6, 6, 4, 3 atoms, T2 lines (one per T1) 2, 2, 3, 4, 4, 4
    EXPECT(rag.K == 19 && count[0] == 0 && count[1] == 8 && count[2] == 11 && count[3] == 0 && count[4] == 12 && count[5] == 7);
    // three columns; cols (0, 1) never leave a b1 group
    Dict g3 = grid({t1, t2, b1});
    check(g3, 3, c012, "three");
    check(g3, 2, c01, "three_t1t2");
    check(g3, 1, c2, "three_b1");
    {
        std::vector<int32_t> nbr((size_t)g3.K * 4);
        EXPECT(rplan::dict_lines(g3.K, 3, g3.lut.data(), g3.normD.data(), 2, c01, nbr.data(), count).empty());
        for (int k = 0; k < g3.K; ++k)
            for (int e = 0; e < 4; ++e)
                if (nbr[k * 4 + e] >= 0) EXPECT(g3.lut[nbr[k * 4 + e] + (size_t)g3.K * 2] == g3.lut[k + (size_t)g3.K * 2]);
    }
    // duplicates: the whole grid twice, interleaved with a shuffled copy: the lowest index of a value is the neighbour
    {
        Dict dup = full; dup.K = 2 * full.K;
        dup.lut.assign((size_t)dup.K * 2, 0.f); dup.normD.assign(dup.K, 2.f);
        for (int k = 0; k < full.K; ++k)
            for (int c = 0; c < 2; ++c) {
                dup.lut[k + (size_t)dup.K * c] = full.lut[k + (size_t)full.K * c];
                dup.lut[full.K + (full.K - 1 - k) + (size_t)dup.K * c] = full.lut[k + (size_t)full.K * c];
            }
        check(dup, 2, c01, "duplicates");
        std::vector<int32_t> nbr((size_t)dup.K * 4);
        EXPECT(rplan::dict_lines(dup.K, 2, dup.lut.data(), dup.normD.data(), 2, c01, nbr.data(), count).empty());
        for (int k = 0; k < dup.K; ++k)
            for (int e = 0; e < 4; ++e) EXPECT(nbr[k * 4 + e] < full.K);       // the first copy holds every lowest index
        EXPECT(nbr[(size_t)(full.K + full.K - 1) * 4 + 1] == 4);                // the copy of atom 0 has atom 0's upper neighbour
    }
    // NaN / Inf lut rows, zero and non-finite normD: no neighbours, nobody's neighbour; the line closes over them
    {
        Dict bad = full;
        bad.lut[(2 * 4 + 1)] = NAN;                              // atom (2, 1): T1 NaN
        bad.lut[(3 * 4 + 2) + (size_t)bad.K] = INFINITY;         // atom (3, 2): T2 Inf
        bad.normD[1 * 4 + 1] = 0.f; bad.normD[4 * 4 + 0] = NAN; bad.normD[4 * 4 + 3] = -INFINITY; bad.normD[1 * 4 + 2] = -2.f;     // (a negative normD is fine)
        check(bad, 2, c01, "invalid_atoms");
        std::vector<int32_t> nbr((size_t)bad.K * 4);
        EXPECT(rplan::dict_lines(bad.K, 2, bad.lut.data(), bad.normD.data(), 2, c01, nbr.data(), count).empty());
        const int dead[5] = {2 * 4 + 1, 3 * 4 + 2, 1 * 4 + 1, 4 * 4 + 0, 4 * 4 + 3};
        for (int dk : dead) {
            for (int e = 0; e < 4; ++e) EXPECT(nbr[dk * 4 + e] == -1);
            for (size_t i = 0; i < nbr.size(); ++i) EXPECT(nbr[i] != dk);
        }
        EXPECT(nbr[(0 * 4 + 1) * 4 + 1] == 3 * 4 + 1);           // (0, 1) -> up T1: (1, 1) and (2, 1) are out, (3, 1) is next
        EXPECT(nbr[(3 * 4 + 1) * 4 + 0] == 0 * 4 + 1);
    }
    // refusals
    {
        std::vector<int32_t> nbr((size_t)full.K * 6);
        const int32_t rep[2] = {1, 1}, hi[2] = {0, 2}, neg[1] = {-1};
        auto run = [&](const Dict& d, int P, const int32_t* cols) { return rplan::dict_lines(d.K, d.Q, d.lut.data(), d.normD.data(), P, cols, nbr.data(), count); };
        EXPECT(run(full, 0, c0).find("1 <= P <= 3") != std::string::npos);
        EXPECT(run(full, 4, c012).find("1 <= P <= 3") != std::string::npos);
        EXPECT(run(full, 2, rep).find("twice") != std::string::npos);
        EXPECT(run(full, 2, hi).find("outside 0..1") != std::string::npos);
        EXPECT(run(full, 1, neg).find("outside 0..1") != std::string::npos);
        Dict one = grid({t1, {0.1f}});                           // a single T2: column 1 has no lines, column 0 has
        EXPECT(run(one, 1, c0).empty());
        EXPECT(run(one, 1, c1) == "lut column 1 has no lines");
        EXPECT(run(one, 2, c01) == "lut column 1 has no lines");
        Dict dead = full; dead.normD.assign(dead.K, 0.f);        // no valid atom at all
        EXPECT(run(dead, 1, c0) == "lut column 0 has no lines");
        Dict single = grid({{1.f}, {2.f}});                      // K = 1
        EXPECT(run(single, 1, c0) == "lut column 0 has no lines");
    }
    // the table of unnormalised atoms
    {
        const int K = 5, s = 3;
        std::vector<float> D((size_t)K * s), nd(K);
        for (int k = 0; k < K; ++k) { nd[k] = 0.5f + k; for (int j = 0; j < s; ++j) D[k + (size_t)K * j] = 0.1f * (k + 1) - 0.3f * j; }
        std::vector<double> arow((size_t)K * rplan::ROW, -1.0);
        rplan::atom_rows(K, s, D.data(), nd.data(), arow.data());
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < rplan::ROW; ++j) EXPECT(arow[(size_t)k * rplan::ROW + j] == (j < s ? (double)nd[k] * (double)D[k + (size_t)K * j] : 0.0));
    }
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("REFINE_PLAN_OK\n");
    return 0;
}
