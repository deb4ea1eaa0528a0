// host_asan_fieldmap.cpp -- every refusal of qmri_field_map_estimate / qmri_field_map_estimate_dev (api_fmap.cpp) under the
// host-only AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is
// decided before the device is selected and needs neither an operator nor a denoiser.  Run by tests/test_fieldmap_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

typedef int (*entry_t)(qmri_ctx*, int, int, int, int, int, const void*, const double*, const double*, const qmri_fieldmap_params*, double*, double*,
                       qmri_fieldmap_info*);

static void drive(entry_t f, bool host) {
    const int S = 2, L = 3, C = 2, N = 4, M = 5, E = QMRI_ERR_INVALID_ARG;
    std::vector<double> Y((size_t)2 * S * L * C * N * M, 0.25), fi((size_t)S * N * M, 1.0), fo((size_t)S * N * M), tr((size_t)S * N * M);
    const double t[L] = {0.0, 2e-3, 5e-3};
    qmri_fieldmap_info info[S];
    const qmri_fieldmap_params ok = {};
    auto msg = [](qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; };
    for (int pass = 0; pass < 2; ++pass) {          // without a context (messages in qmri_last_error(NULL)), then with one
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        EXPECT(f(c, S, L, C, N, M, nullptr, t, fi.data(), &ok, fo.data(), tr.data(), info) == E && msg(c, "Y / t_s"));
        EXPECT(f(c, S, L, C, N, M, Y.data(), nullptr, fi.data(), &ok, fo.data(), tr.data(), info) == E && msg(c, "Y / t_s"));
        EXPECT(f(c, S, L, C, N, M, Y.data(), t, fi.data(), &ok, nullptr, tr.data(), info) == E && msg(c, "f_out"));
        const int bad_s[] = {0, -1, 4097};
        for (int v : bad_s) EXPECT(f(c, v, L, C, N, M, Y.data(), t, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "nslices"));
        const int bad_l[] = {1, 0, 9, -3};
        for (int v : bad_l) EXPECT(f(c, S, v, C, N, M, Y.data(), t, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "nechoes"));
        EXPECT(f(c, S, L, 0, N, M, Y.data(), t, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "ncoil"));
        EXPECT(f(c, S, L, 129, N, M, Y.data(), t, nullptr, &ok, fo.data(), nullptr, nullptr) == QMRI_ERR_UNSUPPORTED && msg(c, "128 coils"));
        const int bad_n[] = {1, 0, -4, 4097};
        for (int v : bad_n) {
            EXPECT(f(c, S, L, C, v, M, Y.data(), t, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "N and M"));
            EXPECT(f(c, S, L, C, N, v, Y.data(), t, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "N and M"));
        }
        const double bad_t[] = {NAN, INFINITY, -INFINITY};
        for (double v : bad_t) {
            double x[L] = {t[0], v, t[2]};
            EXPECT(f(c, S, L, C, N, M, Y.data(), x, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "t_s must be finite"));
        }
        {
            double x[L] = {0.0, 2e-3, 2e-3};
            EXPECT(f(c, S, L, C, N, M, Y.data(), x, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "strictly increasing"));
            x[1] = -1e-3;
            EXPECT(f(c, S, L, C, N, M, Y.data(), x, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, "strictly increasing"));
        }
        qmri_fieldmap_params p = ok;
        const int bad_it[] = {-1, 100001};
        for (int v : bad_it) { p = ok; p.iters = v; EXPECT(f(c, S, L, C, N, M, Y.data(), t, nullptr, &p, fo.data(), nullptr, nullptr) == E && msg(c, "iters")); }
        const double bad_beta[] = {-0.01, NAN, INFINITY};
        for (double v : bad_beta) { p = ok; p.beta = v; EXPECT(f(c, S, L, C, N, M, Y.data(), t, nullptr, &p, fo.data(), nullptr, nullptr) == E && msg(c, "beta")); }
        const int bad_sign[] = {2, -2, 7};
        for (int v : bad_sign) { p = ok; p.phase_sign = v; EXPECT(f(c, S, L, C, N, M, Y.data(), t, nullptr, &p, fo.data(), nullptr, nullptr) == E && msg(c, "phase_sign")); }
        for (int k = 0; k < 4; ++k) { p = ok; p.reserved[k] = 1; EXPECT(f(c, S, L, C, N, M, Y.data(), t, nullptr, &p, fo.data(), nullptr, nullptr) == E && msg(c, "reserved")); }
        if (host || !pass) {                         // (the device route with a context would go on to the device)
            const double bad_v[] = {NAN, INFINITY};
            for (double v : bad_v) {
                std::vector<double> x = Y;
                x.back() = v;                         // the last value: the scan reads the whole array
                EXPECT(f(c, S, L, C, N, M, x.data(), t, nullptr, &ok, fo.data(), nullptr, nullptr) == E && msg(c, host ? "Y must be finite" : "ctx"));
                std::vector<double> g = fi;
                g.back() = v;
                EXPECT(f(c, S, L, C, N, M, Y.data(), t, g.data(), &ok, fo.data(), nullptr, nullptr) == E && msg(c, host ? "f_init must be finite" : "ctx"));
            }
        }
        if (!host) EXPECT(f(c, S, L, C, N, M, Y.data(), t, fo.data(), &ok, fo.data(), nullptr, nullptr) == E && msg(c, "alias"));
        if (!pass) {                                 // everything fine: refused for the missing context only
            EXPECT(f(c, S, L, C, N, M, Y.data(), t, fi.data(), &ok, fo.data(), tr.data(), info) == E && msg(c, "ctx"));
            EXPECT(f(c, S, L, C, N, M, Y.data(), t, nullptr, nullptr, fo.data(), nullptr, nullptr) == E && msg(c, "ctx"));
            p = ok; p.iters = 100000; p.beta = 0.5; p.phase_sign = 1;
            const std::vector<double> big((size_t)2 * 8 * 128 * 2 * 2, 1.0);        // the largest echo and coil counts on the smallest grid
            const double t8[8] = {0, 1, 2, 3, 4, 5, 6, 7};
            EXPECT(f(c, 1, 8, 128, 2, 2, big.data(), t8, nullptr, &p, fo.data(), nullptr, nullptr) == E && msg(c, "ctx"));
        }
    }
}

int main() {
    drive(qmri_field_map_estimate, true);
    drive(qmri_field_map_estimate_dev, false);
    EXPECT(fmap_halo() == 8);
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_FIELDMAP_OK\n");
    return 0;
}
