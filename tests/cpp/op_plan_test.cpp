// op_plan_test.cpp -- the host planning of a gridded operator (csrc/op_plan.h): the functions qmri_set_operator and qmri_prepare_direct call, on a
// machine without a GPU and under the address and undefined-behaviour sanitizers.  Built and run by tests/test_op_plan_host.py, which compares
// the lines printed here with the values the planner gave before it was moved into the header (and, for the masks of the GPU sweep, as it stands).
//   stdout: per case  "<name> status=<KsPlanStatus> caps=<shape> units=<G> n=<n> tried=<tried> digest=<FNV-1a of sgrp, es, grp, units>"
// For every case the program itself checks what holds whatever the planner's thresholds are (check_plan), and once the mask builders' capacity
// rule, the sorted sample list and the DIRECT solver's tables (a product check).  Exit status 1: a check failed (named on stderr).
#include <cinttypes>
#include <cstdio>
#include <string>
#include "op_plan.h"

static int g_failed = 0;
#define EXPECT(cond) do { if (!(cond)) { if (++g_failed <= 20) fprintf(stderr, "op_plan_test: %s: line %d: %s is false\n", g_case.c_str(), __LINE__, #cond); } } while (0)
static std::string g_case = "-";

// ---- masks ---------------------------------------------------------------------------------------------------------------------------------------
struct Mask { int N = 0, M = 0, T = 0; std::vector<int32_t> fp, kidx; };
static Mask spiral(int N, int S, int T) {
    Mask k; k.N = k.M = N; k.T = T; k.fp.assign(T + 1, -1);
    const long m = mask_build_spiral(N, S, T, k.fp.data(), nullptr, 0);                  // capacity 0: nothing is written, the count comes back
    k.kidx.assign(m, -1);
    EXPECT(mask_build_spiral(N, S, T, k.fp.data(), k.kidx.data(), (int)m) == m && k.fp[T] == m);
    return k;
}
static Mask epi(int N, int M, double pct, int T) {
    Mask k; k.N = N; k.M = M; k.T = T; k.fp.assign(T + 1, -1);
    const long m = mask_build_epi(N, M, pct, T, k.fp.data(), nullptr, 0);
    k.kidx.assign(m, -1);
    EXPECT(mask_build_epi(N, M, pct, T, k.fp.data(), k.kidx.data(), (int)m) == m && k.fp[T] == m);
    return k;
}
// every k of the N x N grid in every frame but the last, which samples the first `last` k
static Mask full_with_short_last_frame(int N, int T, int last) {
    Mask k; k.N = k.M = N; k.T = T; k.fp.assign(T + 1, 0);
    for (int t = 0; t < T; ++t) {
        k.fp[t] = (int32_t)k.kidx.size();
        for (int i = 0; i < (t == T - 1 ? last : N * N); ++i) k.kidx.push_back(i);
    }
    k.fp[T] = (int32_t)k.kidx.size();
    return k;
}
// every k of the N x N grid in each of the first `full` frames, then k = 0 alone in the other frames
static Mask full_then_k0(int N, int T, int full) {
    Mask k; k.N = k.M = N; k.T = T; k.fp.assign(T + 1, 0);
    for (int t = 0; t < T; ++t) {
        k.fp[t] = (int32_t)k.kidx.size();
        if (t < full) for (int i = 0; i < N * N; ++i) k.kidx.push_back(i);
        else k.kidx.push_back(0);
    }
    k.fp[T] = (int32_t)k.kidx.size();
    return k;
}
// one sample in all: frame t samples k, the other frames are empty
static Mask single_sample(int N, int T, int t, int k) {
    Mask q; q.N = q.M = N; q.T = T; q.fp.assign(T + 1, 0);
    for (int f = t + 1; f <= T; ++f) q.fp[f] = 1;
    q.kidx.push_back(k);
    return q;
}

// ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
struct Setting { const char* tag = ""; int s = 10, max_batch = 1; bool one_launch = true; int ncu = 256; bool fits[KS_NCAPS] = {true, true, true, true}; };
static Setting setting(const char* tag, int max_batch = 1, bool one_launch = true, int ncu = 256) {
    Setting g; g.tag = tag; g.max_batch = max_batch; g.one_launch = one_launch; g.ncu = ncu;
    return g;
}
static Setting without(const char* tag, int c0, int c1 = -1) {
    Setting g; g.tag = tag; g.fits[c0] = false; if (c1 >= 0) g.fits[c1] = false;
    return g;
}

// calls f(name, mask, sorted list, planner input) for every case: the branches of ks_plan_units, each at the smallest mask found that reaches it
template <class F> static void for_each_case(F f) {
    auto run = [&](const std::string& mname, const Mask& k, std::vector<Setting> settings) {
        const KSorted ks = op_sort_samples(k.N, k.M, k.T, k.fp.data(), k.kidx.data());
        const std::vector<int32_t> sptr = ks_slot_ptr(ks);
        for (const Setting& g : settings) {
            KsPlanIn in;
            in.m = k.fp[k.T]; in.ns = ks.nsampled; in.s = g.s; in.T = k.T; in.max_batch = g.max_batch;
            in.sptr = sptr.data(); in.ent = ks.ent_h.data(); in.one_launch = g.one_launch; in.ncu = g.ncu;
            for (int c = 0; c < KS_NCAPS; ++c) in.lds_fits[c] = g.fits[c];
            f(mname + (g.tag[0] ? "/" : "") + g.tag, k, ks, in);
        }
    };
    Setting s6 = setting("s6"); s6.s = 6;
    run("spiral32_S400_T24", spiral(32, 400, 24), {setting(""), without("v_too_large", 0)});                  // dense, one attempt | the chosen shape's V does not fit
    run("spiral32_S57_T9", spiral(32, 57, 9), {setting("")});                                                 // sparse
    run("full16_T8_last255", full_with_short_last_frame(16, 8, 255), {setting("")});                          // 7.996 samples per k: sparse
    run("full16_T8", full_with_short_last_frame(16, 8, 256), {setting("")});                                  // 8 samples per k: dense
    run("spiral224_S771_T200", spiral(224, 771, 200), {setting("B1"), setting("B15", 15)});                   // the headline operator: 250 after three attempts
    run("epi128_5th_T100", epi(128, 128, 0.2, 100), {setting("")});                                           // the 251..320 band: all 8 attempts, no upgrade
    run("epi160_5th_T9", epi(160, 160, 0.2, 9), {setting("B1"), setting("B4_off", 4, false), setting("ncu64", 1, true, 64),    // upgrade | none | refused, re-cut
                                                 without("no1", 1), without("no12", 1, 2), s6});              // shape 1 does not fit: 2, or the base again | s != 10
    run("epi128_5th_T30", epi(128, 128, 0.2, 30), {setting("B1"), without("no1", 1)});                        // shape 1 | it does not fit: the sparse mask on shape 2
    run("epi224_65th_T200", epi(224, 224, 1.0 / 65, 200), {setting("B1")});
    run("epi256_65th_T200", epi(256, 256, 1.0 / 65, 200), {setting("B1")});                                   // 256 units: all 8 attempts of the upgrade
    run("full32_T300", full_then_k0(32, 300, 300), {setting("B1"), setting("B4_off", 4, false), setting("ncu100", 1, true, 100)});   // dense upgrade to shape 2
    run("cut0_spiral224_S771_T1000", spiral(224, 771, 1000), {setting("B1")});
    run("busy16_T300", full_then_k0(16, 300, 1), {setting("")});                                              // sparse on average, shape 3 refuses k = 0 (300 > 256)
    run("busy16_T1100", full_then_k0(16, 1100, 1), {setting("B1"), setting("B4_off", 4, false)});             // shapes 3, 0, 1 refuse | refusal with the long tail
    run("k0_T2600", full_then_k0(16, 2600, 0), {setting("B1")});                                              // refusal: no shape holds 2600
    // the 32-sided masks tests/test_gpu_gridded_sweep.py runs on the device (with spiral32_* and full32_T300 above): the shape each one reaches
    run("busy32_T300", full_then_k0(32, 300, 1), {setting("")});                                              // as busy16_T300
    run("busy32_T1100", full_then_k0(32, 1100, 1), {setting("")});                                            // as busy16_T1100: only shape 2 holds k = 0
    run("full32_T8", full_with_short_last_frame(32, 8, 1024), {setting("")});                                 // 8 samples per k: dense
    run("full32_T8_last1023", full_with_short_last_frame(32, 8, 1023), {setting("")});                        // 7.999 samples per k: sparse
    run("single_sample32", single_sample(32, 3, 1, 5 + 32 * 7), {setting("")});                               // m = 1: one slot, one group, one unit
}

// ---- what holds whatever the thresholds are ----------------------------------------------------------------------------------------------------------
static void check_plan(const KsPlanIn& in, const KsPlan& p) {
    const KsCapsHost cp = KS_CAPS[p.caps];
    const int ns = in.ns;
    EXPECT(p.vcap == (in.T * in.s + 10 + 15) / 16 * 16 && p.vcap >= in.T * in.s + 10 && p.vcap % 16 == 0);
    EXPECT(p.caps >= 0 && p.caps < KS_NCAPS && p.G >= 1 && (size_t)p.G == p.units.size());
    EXPECT(p.sgrp.size() == (size_t)ns + 1 && p.es.size() == (size_t)in.m);
    if (g_failed) return;
    // sgrp: the prefix sum of ceil(samples / gcap) over the slots -- what the kernels index
    EXPECT(p.sgrp[0] == 0 && (size_t)p.sgrp[ns] == p.grp.size());
    for (int j = 0; j < ns; ++j) EXPECT(p.sgrp[j + 1] - p.sgrp[j] == (in.sptr[j + 1] - in.sptr[j] + cp.gcap - 1) / cp.gcap);
    if (g_failed) return;
    int slot = 0, group = 0;
    for (const KsUnit& u : p.units) {
        // units tile the slots, the samples and the groups without gap or overlap, inside the shape's capacities
        EXPECT(u.s0 == slot && u.s1 > u.s0 && u.s1 <= ns && u.g0 == group && u.pad0 == 0 && u.pad1 == 0);
        if (g_failed) return;
        EXPECT(u.e0 == in.sptr[u.s0] && u.e1 == in.sptr[u.s1] && u.g0 == p.sgrp[u.s0] && u.g1 == p.sgrp[u.s1]);
        EXPECT(u.s1 - u.s0 <= cp.scap && u.e1 - u.e0 <= cp.ecap && u.g1 - u.g0 <= cp.gcapb);
        for (int j = u.s0; j < u.s1; ++j) {
            // a slot's groups tile its samples, <= gcap each; every 16-bit offset is relative to the unit and holds the value it was narrowed from
            int e = in.sptr[j];
            for (int g = p.sgrp[j]; g < p.sgrp[j + 1]; ++g) {
                const KsGroup& q = p.grp[g];
                const int end = std::min(e + cp.gcap, in.sptr[j + 1]);
                EXPECT((int)q.ls == j - u.s0 && (int)q.b == e - u.e0 && (int)q.e == end - u.e0 && q.pad == 0 && end > e);
                e = end;
            }
            EXPECT(e == in.sptr[j + 1]);
            for (e = in.sptr[j]; e < in.sptr[j + 1]; ++e) EXPECT((int)p.es[e].ls == j - u.s0 && p.es[e].t == in.ent[e].t);
        }
        slot = u.s1; group = u.g1;
    }
    EXPECT(slot == ns && (size_t)group == p.grp.size() && p.units.back().e1 == in.m);
}

static void check_sorted(const Mask& k, const KSorted& o) {
    const int NM = k.N * k.M, m = k.fp[k.T];
    EXPECT(o.kptr_h.size() == (size_t)NM + 1 && o.kptr_h[0] == 0 && o.kptr_h[NM] == m && o.ent_h.size() == (size_t)m && o.perm_h.size() == (size_t)m);
    std::vector<uint8_t> seen(m, 0);
    int slots = 0;
    for (int kp = 0; kp < NM; ++kp) {
        const bool sampled = o.kptr_h[kp + 1] > o.kptr_h[kp];
        EXPECT(o.kslot[kp] == (sampled ? slots : -1));
        slots += sampled;
        for (int e = o.kptr_h[kp]; e < o.kptr_h[kp + 1]; ++e) {
            const int i = o.perm_h[e];
            EXPECT(i >= 0 && i < m && !seen[i]);
            if (g_failed) return;
            seen[i] = 1;
            EXPECT((k.kidx[i] % k.N) * k.M + k.kidx[i] / k.N == kp && o.ent_h[e].kw == k.kidx[i] / k.N);
            EXPECT(k.fp[o.ent_h[e].t] <= i && i < k.fp[o.ent_h[e].t + 1]);
            if (e > o.kptr_h[kp]) EXPECT(o.ent_h[e].t >= o.ent_h[e - 1].t && i > o.perm_h[e - 1]);
        }
    }
    EXPECT(slots == o.nsampled);
}

// (G_k + r I) * inv = I within 1e-12 entrywise.  V has orthonormal columns, so the eigenvalues of G_k + r I lie in [r, 1 + r]: with r = 0.05 a
// condition number <= 21, and 1e-12 is about 10^3 ulps of the unit diagonal.
static void check_direct() {
    g_case = "direct_inverse";
    const int N = 32, T = 24, s = 10;
    const double r = 0.05;
    const Mask k = spiral(N, 400, T);
    const KSorted o = op_sort_samples(N, N, T, k.fp.data(), k.kidx.data());
    std::vector<double> V((size_t)T * s);                           // column-major; a fixed pseudo-random matrix, orthonormalised (modified Gram-Schmidt)
    uint64_t x = 88172645463325252ull;
    for (double& v : V) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (double)(x >> 11) / 9007199254740992.0 - 0.5; }
    for (int c = 0; c < s; ++c) {
        for (int p = 0; p < c; ++p) {
            double d = 0.0;
            for (int t = 0; t < T; ++t) d += V[t + (size_t)T * c] * V[t + (size_t)T * p];
            for (int t = 0; t < T; ++t) V[t + (size_t)T * c] -= d * V[t + (size_t)T * p];
        }
        double n2 = 0.0;
        for (int t = 0; t < T; ++t) n2 += V[t + (size_t)T * c] * V[t + (size_t)T * c];
        for (int t = 0; t < T; ++t) V[t + (size_t)T * c] /= std::sqrt(n2);
    }
    const std::vector<double> ginv = direct_inverse_tables(V, o.kptr_h, o.ent_h, s, T, r);
    EXPECT(ginv.size() == (size_t)o.nsampled * s * s && o.nsampled > 0);
    if (g_failed) return;
    double worst = 0.0;
    for (int kp = 0; kp < N * N; ++kp) {
        if (o.kslot[kp] < 0) continue;
        const double* inv = ginv.data() + (size_t)o.kslot[kp] * s * s;
        std::vector<double> G(s * s, 0.0);
        for (int e = o.kptr_h[kp]; e < o.kptr_h[kp + 1]; ++e)
            for (int a = 0; a < s; ++a)
                for (int b = 0; b < s; ++b) G[a * s + b] += V[o.ent_h[e].t + (size_t)T * a] * V[o.ent_h[e].t + (size_t)T * b];
        for (int a = 0; a < s; ++a) G[a * s + a] += r;
        for (int a = 0; a < s; ++a)
            for (int b = 0; b < s; ++b) {
                double v = 0.0;
                for (int c = 0; c < s; ++c) v += G[a * s + c] * inv[c * s + b];
                worst = std::max(worst, std::fabs(v - (a == b ? 1.0 : 0.0)));
                EXPECT(inv[a * s + b] == inv[b * s + a]);
            }
    }
    EXPECT(worst <= 1e-12);
    printf("direct_inverse slots=%d worst=%.3g\n", o.nsampled, worst);
}

static uint64_t digest(const KsPlan& p) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* q, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)q)[i]; h *= 1099511628211ull; } };
    mix(p.sgrp.data(), p.sgrp.size() * sizeof(int32_t)); mix(p.es.data(), p.es.size() * sizeof(KSample));
    mix(p.grp.data(), p.grp.size() * sizeof(KsGroup)); mix(p.units.data(), p.units.size() * sizeof(KsUnit));
    return h;
}

int main() {
    static_assert(sizeof(KSample) == 4 && sizeof(KsGroup) == 8 && sizeof(KsUnit) == 32 && sizeof(KEntry) == 4, "the device reads these layouts");
    {   // the capacity rule of the mask builders: the count comes back whatever the capacity, and nothing is written past it
        g_case = "mask_capacity";
        const Mask a = spiral(32, 57, 9), b = epi(32, 16, 0.2, 9);
        std::vector<int32_t> fp(10), part(100, -7);
        EXPECT(mask_build_spiral(32, 57, 9, fp.data(), part.data(), 60) == a.fp[9] && fp == a.fp && part[60] == -7 && std::equal(part.begin(), part.begin() + 60, a.kidx.begin()));
        part.assign(100, -7);
        EXPECT(mask_build_epi(32, 16, 0.2, 9, fp.data(), part.data(), 50) == b.fp[9] && fp == b.fp && part[50] == -7 && std::equal(part.begin(), part.begin() + 50, b.kidx.begin()));
        EXPECT(b.fp[9] == 9 * 16 * 6 && a.fp[9] > 100);
    }
    for_each_case([&](const std::string& name, const Mask& k, const KSorted& o, const KsPlanIn& in) {
        g_case = name;
        check_sorted(k, o);
        const KsPlan p = ks_plan_units(in);
        if (p.status == KS_PLAN_OK) check_plan(in, p);
        else EXPECT(p.units.empty());
        if (p.status == KS_PLAN_BUSY_K) EXPECT(p.n > p.tried && p.tried >= KS_CAPS[0].ecap);
        printf("%s status=%d caps=%d units=%d n=%d tried=%d digest=%016" PRIx64 "\n", name.c_str(), (int)p.status, p.status == KS_PLAN_BUSY_K ? -1 : p.caps,
               p.status == KS_PLAN_BUSY_K ? 0 : p.G, p.n, p.tried, p.status == KS_PLAN_OK ? digest(p) : (uint64_t)0);
    });
    check_direct();
    if (g_failed) fprintf(stderr, "op_plan_test: %d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
