// host_asan_epg.cpp -- every refusal of qmri_dict_simulate / qmri_dict_simulate_dev (api_epg.cpp) under the host-only
// AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided
// before the device is selected and needs neither an operator nor a dictionary.  Run by tests/test_epg_host.py.
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
                       void*);

static void drive(entry_t f, bool host_atoms) {
    const int K = 3, T = 4, E = QMRI_ERR_INVALID_ARG;
    const double al[T] = {0.1, 0.2, 0.0, 0.4}, tr[T] = {0.012, 0.012, 0.013, 0.012}, te[T] = {0.002, 0.0, 0.013, 0.002};
    const double t1[K] = {1.0, 0.5, 2.0}, t2[K] = {0.1, 0.05, 0.2}, b1[K] = {1.0, 0.0, 1.2};
    double F[K * T];
    const qmri_epg_params ok = {32, 1, 0.0, 1.0, 1};
    auto msg = [](qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; };
    for (int pass = 0; pass < 2; ++pass) {          // without a context (messages in qmri_last_error(NULL)), then with one
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, nullptr, F) == E && msg(c, "params"));
        EXPECT(f(c, K, T, nullptr, tr, te, t1, t2, b1, &ok, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, nullptr, te, t1, t2, b1, &ok, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, nullptr, t1, t2, b1, &ok, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, nullptr, t2, b1, &ok, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, t1, nullptr, b1, &ok, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, nullptr) == E && msg(c, "F_out"));
        EXPECT(f(c, 0, T, al, tr, te, t1, t2, b1, &ok, F) == E && msg(c, "K must"));
        EXPECT(f(c, -2, T, al, tr, te, t1, t2, b1, &ok, F) == E && msg(c, "K must"));
        EXPECT(f(c, K, 0, al, tr, te, t1, t2, b1, &ok, F) == E && msg(c, "T must"));
        EXPECT(f(c, K, 1025, al, tr, te, t1, t2, b1, &ok, F) == E && msg(c, "T must"));
        qmri_epg_params p = ok;
        const int bad_s[] = {0, -1, 257};
        for (int v : bad_s) { p = ok; p.nstates = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, F) == E && msg(c, "nstates")); }
        p = ok; p.inversion = 2;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, F) == E && msg(c, "inversion"));
        p = ok; p.out_is_f64 = -1;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, F) == E && msg(c, "out_is_f64"));
        const double bad_ti[] = {-1e-3, NAN, INFINITY};
        for (double v : bad_ti) { p = ok; p.ti = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, F) == E && msg(c, "ti must")); }
        const double bad_eff[] = {0.0, -0.5, 1.0001, NAN};
        for (double v : bad_eff) { p = ok; p.inv_eff = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, F) == E && msg(c, "inv_eff")); }
        const double bad_frame[] = {-0.1, NAN, INFINITY};
        for (double v : bad_frame) {
            double x[T];
            std::memcpy(x, al, sizeof x); x[2] = v;
            EXPECT(f(c, K, T, x, tr, te, t1, t2, b1, &ok, F) == E && msg(c, "alpha must"));
            std::memcpy(x, tr, sizeof x); x[3] = v;
            EXPECT(f(c, K, T, al, x, te, t1, t2, b1, &ok, F) == E && msg(c, "tr must"));
            std::memcpy(x, te, sizeof x); x[1] = v;
            EXPECT(f(c, K, T, al, tr, x, t1, t2, b1, &ok, F) == E && msg(c, "te must"));
        }
        {
            double x[T];
            std::memcpy(x, tr, sizeof x); x[1] = 0.0;
            EXPECT(f(c, K, T, al, x, te, t1, t2, b1, &ok, F) == E && msg(c, "tr must"));
            std::memcpy(x, te, sizeof x); x[0] = 0.0125;
            EXPECT(f(c, K, T, al, tr, x, t1, t2, b1, &ok, F) == E && msg(c, "te must not exceed tr"));
        }
        const double bad_atom[] = {0.0, -1.0, NAN, INFINITY};
        for (double v : bad_atom) {
            double x[K];
            const char* after = host_atoms ? nullptr : "ctx";           // the device route cannot read its atoms here
            if (!host_atoms && pass) continue;                         // (with a context it would go on to the device)
            std::memcpy(x, t1, sizeof x); x[2] = v;
            EXPECT(f(c, K, T, al, tr, te, x, t2, b1, &ok, F) == E && msg(c, after ? after : "t1 must"));
            std::memcpy(x, t2, sizeof x); x[0] = v;
            EXPECT(f(c, K, T, al, tr, te, t1, x, b1, &ok, F) == E && msg(c, after ? after : "t2 must"));
            if (v != 0.0) {
                std::memcpy(x, b1, sizeof x); x[1] = v;
                EXPECT(f(c, K, T, al, tr, te, t1, t2, x, &ok, F) == E && msg(c, after ? after : "b1 must"));
            }
        }
        p = ok; p.inversion = 0; p.ti = -1.0; p.inv_eff = 7.0;          // without an inversion its fields are ignored
        if (!pass) {
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, F) == E && msg(c, "ctx"));
            EXPECT(f(c, K, T, al, tr, te, t1, t2, nullptr, &p, F) == E && msg(c, "ctx"));
        }
    }
}

int main() {
    drive(qmri_dict_simulate, true);
    drive(qmri_dict_simulate_dev, false);
    double in[6] = {0}, out[6];
    EXPECT(qmri_debug_epg_shift(nullptr, 2, 1, in, out) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(nullptr), "ctx"));
    EXPECT(qmri_debug_epg_shift(nullptr, 2, 1, nullptr, out) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(nullptr), "in / out"));
    EXPECT(qmri_debug_epg_shift(nullptr, 257, 1, in, out) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(nullptr), "S must"));
    EXPECT(qmri_debug_epg_shift(nullptr, 2, -1, in, out) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(nullptr), "nshift"));
    // the launch plan: at least 8 atoms (64 B of fp64) contiguous per frame at S = 32, a whole number of groups per workgroup everywhere
    EXPECT(epg_atoms_per_workgroup(1) == 16 && epg_atoms_per_workgroup(16) == 16 && epg_atoms_per_workgroup(17) == 8 && epg_atoms_per_workgroup(32) == 8);
    EXPECT(epg_atoms_per_workgroup(33) == 4 && epg_atoms_per_workgroup(64) == 4 && epg_atoms_per_workgroup(65) == 4 && epg_atoms_per_workgroup(256) == 4);
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_EPG_OK\n");
    return 0;
}
