// host_asan_dsvd.cpp -- every refusal of qmri_dict_compress / qmri_dict_compress_dev (api_dsvd.cpp) under the host-only
// AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided
// before the device is selected and needs neither an operator nor a dictionary.  Run by tests/test_dict_svd_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

typedef int (*entry_t)(qmri_ctx*, int, int, const void*, int, const qmri_dsvd_params*, int*, double*, float*, float*, double*, qmri_dsvd_info*);

static void drive(entry_t f) {
    double F[64] = {0}, V[64], eig[16];
    float D[128], nd[8];
    int s = 0;
    qmri_dsvd_info info;
    const qmri_dsvd_params ok = {2, 16, 0.99, 0.0, 0};
    auto msg = [](qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; };
    const int E = QMRI_ERR_INVALID_ARG;
    for (int pass = 0; pass < 2; ++pass) {          // without a context (messages in qmri_last_error(NULL)), then with one
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        EXPECT(f(c, 8, 4, F, 1, nullptr, &s, V, D, nd, eig, &info) == E && msg(c, "params"));
        EXPECT(f(c, 8, 4, nullptr, 1, &ok, &s, V, D, nd, eig, &info) == E && msg(c, "F /"));
        EXPECT(f(c, 8, 4, F, 1, &ok, nullptr, V, D, nd, eig, &info) == E && msg(c, "s_out"));
        EXPECT(f(c, 8, 4, F, 1, &ok, &s, nullptr, D, nd, eig, &info) == E && msg(c, "V_out"));
        EXPECT(f(c, 8, 4, F, 1, &ok, &s, V, nullptr, nd, eig, &info) == E && msg(c, "D_out"));
        EXPECT(f(c, 8, 4, F, 1, &ok, &s, V, D, nullptr, eig, &info) == E && msg(c, "normD_out"));
        EXPECT(f(c, 0, 4, F, 1, &ok, &s, V, D, nd, eig, &info) == E && msg(c, "K must"));
        EXPECT(f(c, -3, 4, F, 1, &ok, &s, V, D, nd, eig, &info) == E && msg(c, "K must"));
        EXPECT(f(c, 8, 0, F, 1, &ok, &s, V, D, nd, eig, &info) == E && msg(c, "T must"));
        EXPECT(f(c, 8, 1025, F, 1, &ok, &s, V, D, nd, eig, &info) == E && msg(c, "T must"));
        EXPECT(f(c, 8, 4, F, 2, &ok, &s, V, D, nd, eig, &info) == E && msg(c, "f_is_f64"));
        qmri_dsvd_params p = ok;
        p.s = -1;
        EXPECT(f(c, 8, 4, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "s must"));
        p.s = 17;
        EXPECT(f(c, 8, 32, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "s must"));
        p.s = 5;
        EXPECT(f(c, 8, 4, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "min(T, K)"));
        EXPECT(f(c, 4, 8, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "min(T, K)"));
        const int bad_smax[] = {0, -1, 17};
        for (int v : bad_smax) {
            p = ok; p.s = 0; p.s_max = v;
            EXPECT(f(c, 8, 4, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "s_max"));
        }
        const double bad_energy[] = {0.0, -0.5, 1.0001, NAN, INFINITY};
        for (double v : bad_energy) {
            p = ok; p.s = 0; p.energy = v;
            EXPECT(f(c, 8, 4, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "energy"));
        }
        const double bad_tol[] = {-1e-9, 1.0, NAN, INFINITY};
        for (double v : bad_tol) {
            p = ok; p.tol = v;
            EXPECT(f(c, 8, 4, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "tol"));
        }
        p = ok; p.maxit = -1;
        EXPECT(f(c, 8, 4, F, 1, &p, &s, V, D, nd, eig, &info) == E && msg(c, "maxit"));
        p = ok; p.energy = -7.0; p.s_max = 99;           // a fixed rank ignores the energy fields
        if (!pass) {
            EXPECT(f(c, 8, 4, F, 1, &ok, &s, V, D, nd, nullptr, nullptr) == E && msg(c, "ctx"));
            EXPECT(f(c, 8, 4, F, 0, &p, &s, V, D, nd, nullptr, nullptr) == E && msg(c, "ctx"));
        }
    }
}

int main() {
    drive(qmri_dict_compress);
    drive(qmri_dict_compress_dev);
    double F[8] = {0}, G[16];
    EXPECT(qmri_debug_dsvd_gram(nullptr, 2, 4, F, 1, 0, G) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(nullptr), "ctx"));
    EXPECT(qmri_debug_dsvd_gram(nullptr, 2, 4, nullptr, 1, 0, G) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(nullptr), "G_out"));
    // the scratch plan of the Gram kernel: a function of (K, T) alone, whole 64 x 64 tiles of the upper triangle per chunk of atoms
    const size_t chunk = (size_t)dsvd_gram_chunk();
    EXPECT(chunk > 0 && chunk % 32 == 0);
    EXPECT(dsvd_gram_scratch(1, 1) == 4096 && dsvd_gram_scratch((int)chunk, 64) == 4096 && dsvd_gram_scratch((int)chunk + 1, 65) == 2 * 3 * 4096);
    EXPECT(dsvd_gram_scratch(98304, 1000) == (size_t)136 * ((98304 + chunk - 1) / chunk) * 4096);
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_DSVD_OK\n");
    return 0;
}
