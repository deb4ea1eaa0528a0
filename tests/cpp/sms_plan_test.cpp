// sms_plan_test.cpp -- the host plan of a simultaneous multi-slice solve (csrc/sms_plan.h) swept over ncoil 1 .. 13, Z 1 .. 8,
// G 1 .. 3 and max_batch 1 .. 20, in both image orders: every image appears exactly once, ascending, no chunk holds more than max_batch; every unit's
// sum begins exactly once (at its member 0), is continued in order and finishes exactly once (after its last member), and a chunk's first and last
// unit are what k_sms_combine / k_mcl_coil_sum derive from (q0, cnt); the partial-sum slots tile their buffer without overlap; the frame table
// inverts frame_ptr.  Plain C++17, built with -fsanitize=address,undefined and run by tests/test_sms_host.py.
#include <cstdio>
#include <vector>

#include "sms_plan.h"

static long fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { if (fails < 20) std::fprintf(stderr, "check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

static void sweep_order(int units, int unit, int max_batch) {
    const std::vector<sms::Chunk> sch = sms::chunk_schedule(units, unit, max_batch);
    std::vector<int> next((size_t)units, 0);       // members of each unit summed so far
    std::vector<int> begun((size_t)units, 0), finished((size_t)units, 0);
    long q = 0;
    for (const sms::Chunk& c : sch) {
        EXPECT(c.q0 == q && c.cnt >= 1 && c.cnt <= max_batch);
        EXPECT(c.u0 == c.q0 / unit && c.nu == (c.q0 + c.cnt - 1) / unit - c.q0 / unit + 1);      // what the kernels' grids are sized by
        long seen = 0;
        for (int k = 0; k < c.nu; ++k) {
            const int u = c.u0 + k;
            EXPECT(u >= 0 && u < units);
            if (u < 0 || u >= units) return;
            int lo, hi;
            sms::members(c, k, unit, &lo, &hi);
            // the device's own arithmetic (k_sms_combine, k_mcl_coil_sum)
            EXPECT(lo == std::max(c.q0, u * unit) - u * unit && hi == std::min(c.q0 + c.cnt, (u + 1) * unit) - u * unit);
            EXPECT(0 <= lo && lo < hi && hi <= unit);
            EXPECT(lo == next[(size_t)u]);                            // continued where the last chunk left it
            EXPECT(sms::begins(c, k) == (lo == 0) && sms::finishes(c, k, unit) == (hi == unit));
            if (sms::begins(c, k)) begun[(size_t)u] += 1;
            if (sms::finishes(c, k, unit)) finished[(size_t)u] += 1;
            EXPECT(finished[(size_t)u] <= begun[(size_t)u]);          // never finished before begun
            for (int mem = lo; mem < hi; ++mem) { EXPECT((long)u * unit + mem == q + seen); ++seen; }     // ascending, exactly once
            next[(size_t)u] = hi;
        }
        EXPECT(seen == c.cnt);
        q += c.cnt;
    }
    EXPECT(q == (long)units * unit);
    for (int u = 0; u < units; ++u) EXPECT(begun[(size_t)u] == 1 && finished[(size_t)u] == 1 && next[(size_t)u] == unit);
    EXPECT((long)sch.size() == ((long)units * unit + max_batch - 1) / max_batch);
}

static void check_parts(int G, int Z, int ncoil) {
    const sms::Parts p = sms::parts(G, Z, ncoil);
    const size_t img = (size_t)G * ncoil * sms::PC, sl = (size_t)G * Z * sms::PS;
    const size_t start[7] = {p.pu, p.py, p.pb, p.pz, p.pd, p.px, p.pv}, len[7] = {img, img, sl, sl, sl, sl, sl};
    size_t at = 0;
    for (int i = 0; i < 7; ++i) { EXPECT(start[i] == at); at += len[i]; }     // back to back: no overlap, no gap
    EXPECT(p.total == at);
}

int main() {
    long swept = 0;
    for (int ncoil = 1; ncoil <= 13; ++ncoil)
        for (int Z = 1; Z <= sms::MAX_Z; ++Z)
            for (int G = 1; G <= 3; ++G) {
                check_parts(G, Z, ncoil);
                for (int mb = 1; mb <= 20; ++mb) {
                    sweep_order(G * ncoil, Z, mb);        // forward: q = (g ncoil + j) Z + b
                    sweep_order(G * Z, ncoil, mb);        // adjoint: q = (g Z + b) ncoil + j
                    swept += 2;
                }
            }
    // the frame table: empty frames, one-sample frames
    const int32_t fp[] = {0, 3, 3, 4, 9, 9};
    const std::vector<int32_t> f = sms::frame_table(5, fp);
    EXPECT(f.size() == 9);
    for (int t = 0; t < 5; ++t)
        for (int32_t i = fp[t]; i < fp[t + 1]; ++i) EXPECT(f[(size_t)i] == t);
    EXPECT(sms::MAX_Z == 8 && sms::MAX_E == 8192 && sms::PS == 256 && sms::PC == 64);
    if (fails) { std::fprintf(stderr, "%ld checks failed\n", fails); return 1; }
    std::printf("SMS_PLAN_OK swept %ld\n", swept);
    return 0;
}
