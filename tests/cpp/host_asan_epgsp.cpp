// host_asan_epgsp.cpp -- every refusal of qmri_dict_simulate_sp / qmri_dict_simulate_sp_dev (api_epg.cpp) under the host-only
// AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided
// before the device is selected and needs neither an operator nor a dictionary.  Run by tests/test_epgsp_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

typedef int (*entry_t)(qmri_ctx*, int, int, const double*, const double*, const double*, const double*, const double*, const double*, const qmri_epg_params*,
                       const qmri_epg_profile*, void*);

static void drive(entry_t f, bool host_atoms) {
    const int K = 3, T = 4, Q = 3, E = QMRI_ERR_INVALID_ARG;
    const double al[T] = {0.1, 0.2, 0.0, 0.4}, tr[T] = {0.012, 0.012, 0.013, 0.012}, te[T] = {0.002, 0.0, 0.013, 0.002};
    const double t1[K] = {1.0, 0.5, 2.0}, t2[K] = {0.1, 0.05, 0.2}, b1[K] = {1.0, 0.0, 1.2};
    const double w[Q] = {0.5, 0.0, 0.5}, pc[Q] = {1.0, 0.7, 0.0};
    double pf[T * Q];                                // exactly T Q entries: a read past them is an error here
    for (int i = 0; i < T * Q; ++i) pf[i] = 1.0 - 0.05 * i;
    double F[K * T];
    const qmri_epg_params ok = {32, 1, 0.0, 1.0, 1};
    const qmri_epg_profile sc = {Q, 0, pc, w}, sf = {Q, 1, pf, w};
    auto msg = [](qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; };
    for (int pass = 0; pass < 2; ++pass) {          // without a context (messages in qmri_last_error(NULL)), then with one
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        // the refusals of qmri_dict_simulate carry over, and come first
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, nullptr, &sc, F) == E && msg(c, "params"));
        EXPECT(f(c, K, T, nullptr, tr, te, t1, t2, b1, &ok, &sc, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, nullptr, te, t1, t2, b1, &ok, &sc, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, nullptr, t1, t2, b1, &ok, &sc, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, nullptr, t2, b1, &ok, &sc, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, t1, nullptr, b1, &ok, &sc, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &sc, nullptr) == E && msg(c, "F_out"));
        EXPECT(f(c, 0, T, al, tr, te, t1, t2, b1, &ok, &sc, F) == E && msg(c, "K must"));
        EXPECT(f(c, K, 0, al, tr, te, t1, t2, b1, &ok, nullptr, F) == E && msg(c, "T must"));
        EXPECT(f(c, K, 1025, al, tr, te, t1, t2, b1, &ok, &sf, F) == E && msg(c, "T must"));
        qmri_epg_params p = ok;
        const int bad_s[] = {0, -1, 257};
        for (int v : bad_s) { p = ok; p.nstates = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sc, F) == E && msg(c, "nstates")); }
        p = ok; p.inversion = 2;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sc, F) == E && msg(c, "inversion"));
        p = ok; p.out_is_f64 = -1;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sc, F) == E && msg(c, "out_is_f64"));
        const double bad_ti[] = {-1e-3, NAN, INFINITY};
        for (double v : bad_ti) { p = ok; p.ti = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sc, F) == E && msg(c, "ti must")); }
        const double bad_eff[] = {0.0, -0.5, 1.0001, NAN};
        for (double v : bad_eff) { p = ok; p.inv_eff = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sc, F) == E && msg(c, "inv_eff")); }
        const double bad_frame[] = {-0.1, NAN, INFINITY};
        for (double v : bad_frame) {
            double x[T];
            std::memcpy(x, al, sizeof x); x[2] = v;
            EXPECT(f(c, K, T, x, tr, te, t1, t2, b1, &ok, &sc, F) == E && msg(c, "alpha must"));
            std::memcpy(x, tr, sizeof x); x[3] = v;
            EXPECT(f(c, K, T, al, x, te, t1, t2, b1, &ok, &sc, F) == E && msg(c, "tr must"));
            std::memcpy(x, te, sizeof x); x[1] = v;
            EXPECT(f(c, K, T, al, tr, x, t1, t2, b1, &ok, &sc, F) == E && msg(c, "te must"));
        }
        {
            double x[T];
            std::memcpy(x, tr, sizeof x); x[1] = 0.0;
            EXPECT(f(c, K, T, al, x, te, t1, t2, b1, &ok, &sc, F) == E && msg(c, "tr must"));
            std::memcpy(x, te, sizeof x); x[0] = 0.0125;
            EXPECT(f(c, K, T, al, tr, x, t1, t2, b1, &ok, &sc, F) == E && msg(c, "te must not exceed tr"));
        }
        const double bad_atom[] = {0.0, -1.0, NAN, INFINITY};
        for (double v : bad_atom) {
            double x[K];
            if (!host_atoms) break;                                     // the device route cannot read its atoms here
            std::memcpy(x, t1, sizeof x); x[2] = v;
            EXPECT(f(c, K, T, al, tr, te, x, t2, b1, &ok, &sc, F) == E && msg(c, "t1 must"));
            std::memcpy(x, t2, sizeof x); x[0] = v;
            EXPECT(f(c, K, T, al, tr, te, t1, x, b1, &ok, &sc, F) == E && msg(c, "t2 must"));
            if (v != 0.0) {
                std::memcpy(x, b1, sizeof x); x[1] = v;
                EXPECT(f(c, K, T, al, tr, te, t1, t2, x, &ok, &sc, F) == E && msg(c, "b1 must"));
            }
        }
        // the profile's own
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, nullptr, F) == E && msg(c, "slice profile"));
        qmri_epg_profile s = sc;
        const int bad_q[] = {0, -3, 65};
        for (int v : bad_q) { s = sc; s.nq = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "nq must")); }
        const int bad_pf[] = {-1, 2};
        for (int v : bad_pf) { s = sc; s.per_frame = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "per_frame")); }
        s = sc; s.prof = nullptr;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "prof / weight"));
        s = sf; s.weight = nullptr;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "prof / weight"));
        const double bad_entry[] = {-0.1, NAN, INFINITY};
        for (double v : bad_entry) {
            double x[T * Q];
            std::memcpy(x, pc, sizeof pc); x[Q - 1] = v;
            s = sc; s.prof = x;
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "prof must"));
            std::memcpy(x, pf, sizeof pf); x[T * Q - 1] = v;                // the last entry of the last frame is read
            s = sf; s.prof = x;
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "prof must"));
            std::memcpy(x, w, sizeof w); x[1] = v;
            s = sc; s.weight = x;
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "weight must"));
        }
        const double w0[Q] = {0.0, 0.0, 0.0};
        s = sf; s.weight = w0;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "sum to more than 0"));
        p = ok; p.inversion = 0; p.ti = -1.0; p.inv_eff = 7.0;          // without an inversion its fields are ignored
        if (!pass) {
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &sc, F) == E && msg(c, "ctx"));
            EXPECT(f(c, K, T, al, tr, te, t1, t2, nullptr, &p, &sf, F) == E && msg(c, "ctx"));
            if (!host_atoms) {
                double x[K];
                std::memcpy(x, t1, sizeof x); x[2] = NAN;               // passes the host checks of the device route
                EXPECT(f(c, K, T, al, tr, te, x, t2, b1, &ok, &sc, F) == E && msg(c, "ctx"));
            }
        }
    }
}

int main() {
    drive(qmri_dict_simulate_sp, true);
    drive(qmri_dict_simulate_sp_dev, false);
    // the launch plan: Q <= the groups of a workgroup (16, 8, 4 at S <= 16, 32, above) shares it among floor(groups / Q) atoms, beyond one atom
    EXPECT(epg_sp_atoms_per_workgroup(16, 1) == 16 && epg_sp_atoms_per_workgroup(16, 5) == 3 && epg_sp_atoms_per_workgroup(16, 16) == 1);
    EXPECT(epg_sp_atoms_per_workgroup(16, 17) == 1 && epg_sp_atoms_per_workgroup(32, 1) == 8 && epg_sp_atoms_per_workgroup(32, 5) == 1);
    EXPECT(epg_sp_atoms_per_workgroup(32, 4) == 2 && epg_sp_atoms_per_workgroup(256, 2) == 2 && epg_sp_atoms_per_workgroup(256, 64) == 1);
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_EPGSP_OK\n");
    return 0;
}
