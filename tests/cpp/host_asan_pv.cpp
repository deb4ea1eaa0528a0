// host_asan_pv.cpp -- every refusal of qmri_set_components / qmri_dict_unmix / qmri_dict_unmix_dev (api_pv.cpp) and the host
// code that forms the components, under the host-only AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a
// machine without a GPU.  Every refusal is decided before the device is selected; the dictionary a context needs is put into its host copy
// directly (qmri_set_dictionary itself uploads).  Run by tests/test_pv_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

static bool msg(qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; }

// K atoms of s channels, column-major: smooth, pairwise independent rows; atom 5 is zero, atom 6 = 2 x atom 1, atom 7 holds a NaN
static void fill_dictionary(DictHost& d, int K, int s) {
    d.ready = true; d.K = K; d.s = s; d.Q = 2; d.wide = 0;
    d.D_h.assign((size_t)K * s, 0.f); d.normD_h.assign(K, 1.f);
    for (int a = 0; a < K; ++a) {
        for (int j = 0; j < s; ++j) d.D_h[a + (size_t)K * j] = std::cos(0.37f * (a + 1) * (j + 1)) + (j == a % s ? 1.5f : 0.f);
        d.normD_h[a] = 1.f + 0.25f * a;
    }
    for (int j = 0; j < s; ++j) { d.D_h[4 + (size_t)K * j] = 0.f; d.D_h[5 + (size_t)K * j] = 2.f * d.D_h[0 + (size_t)K * j]; }
    d.D_h[6 + (size_t)K * 1] = NAN;
}

static void drive_set() {
    const int E = QMRI_ERR_INVALID_ARG;
    const int32_t ok[3] = {1, 2, 3};
    qmri_pv_info info;
    // without a context: the rules that need none, then the context itself
    EXPECT(qmri_set_components(nullptr, -1, ok, &info) == E && msg(nullptr, "0 <= C <= 8"));
    EXPECT(qmri_set_components(nullptr, 9, ok, &info) == E && msg(nullptr, "0 <= C <= 8"));
    EXPECT(qmri_set_components(nullptr, 3, nullptr, &info) == E && msg(nullptr, "atoms"));
    EXPECT(qmri_set_components(nullptr, 3, ok, &info) == E && msg(nullptr, "ctx"));
    EXPECT(qmri_set_components(nullptr, 0, nullptr, nullptr) == E && msg(nullptr, "ctx"));
    {
        qmri_ctx ctx;
        qmri_ctx* c = &ctx;
        EXPECT(qmri_set_components(c, 3, ok, &info) == QMRI_ERR_STATE && msg(c, "dictionary not set"));
        EXPECT(qmri_set_components(c, 0, nullptr, &info) == QMRI_OK && info.C == 0);          // clearing needs nothing
        EXPECT(qmri_set_components(c, 9, ok, nullptr) == E && qmri_set_components(c, 2, nullptr, nullptr) == E);
        ctx.dict.ready = true; ctx.dict.wide = 1; ctx.dict.K = 40; ctx.dict.s = 24;
        EXPECT(qmri_set_components(c, 3, ok, &info) == QMRI_ERR_UNSUPPORTED && msg(c, "s <= 16"));
        fill_dictionary(ctx.dict, 12, 4);
        ctx.dict.pv.C = 2; ctx.dict.pv.s = 4; ctx.dict.pv.min_pivot = 0.5;                    // "earlier components": a refused call leaves them
        const int32_t lo[2] = {0, 2}, hi[2] = {2, 13}, rep[3] = {2, 3, 2}, zero[2] = {1, 5}, col[2] = {1, 6}, nan[2] = {7, 2}, many[5] = {1, 2, 3, 4, 8};
        EXPECT(qmri_set_components(c, 2, lo, &info) == E && msg(c, "outside 1..12"));
        EXPECT(qmri_set_components(c, 2, hi, &info) == E && msg(c, "outside 1..12"));
        EXPECT(qmri_set_components(c, 3, rep, &info) == E && msg(c, "twice"));
        EXPECT(qmri_set_components(c, 2, zero, &info) == E && msg(c, "is zero"));
        EXPECT(qmri_set_components(c, 2, nan, &info) == E && msg(c, "not finite"));
        EXPECT(qmri_set_components(c, 5, many, &info) == E && msg(c, "than channels"));
        EXPECT(qmri_set_components(c, 2, col, &info) == E && msg(c, "collinear"));
        EXPECT(ctx.dict.pv.C == 2 && ctx.dict.pv.s == 4 && ctx.dict.pv.min_pivot == 0.5);
        EXPECT(qmri_set_components(c, 0, nullptr, nullptr) == QMRI_OK && ctx.dict.pv.C == 0);
        qmri_free_dict(c);                                                                    // what qmri_set_dictionary does first
        EXPECT(!ctx.dict.ready && ctx.dict.pv.C == 0 && ctx.dict.D_h.empty());
    }
}

typedef int (*unmix_t)(qmri_ctx*, const void*, int, int, double*, double*, double*, double*, int32_t*);

static void drive_unmix(unmix_t f) {
    const int E = QMRI_ERR_INVALID_ARG, n = 5;
    std::vector<double> X((size_t)2 * n * 4, 0.25), w((size_t)n * 8);
    for (int pass = 0; pass < 2; ++pass) {
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        EXPECT(f(c, X.data(), 0, 0, w.data(), nullptr, nullptr, nullptr, nullptr) == E && msg(c, "Npix"));
        EXPECT(f(c, X.data(), -3, 0, w.data(), nullptr, nullptr, nullptr, nullptr) == E && msg(c, "Npix"));
        EXPECT(f(c, nullptr, n, 0, w.data(), nullptr, nullptr, nullptr, nullptr) == E && msg(c, "X / w"));
        EXPECT(f(c, X.data(), n, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == E && msg(c, "X / w"));
        const int bad_mode[] = {-1, 2, 7};
        for (int m : bad_mode) EXPECT(f(c, X.data(), n, m, w.data(), nullptr, nullptr, nullptr, nullptr) == E && msg(c, "mode"));
        if (!pass) EXPECT(f(c, X.data(), n, 1, w.data(), nullptr, nullptr, nullptr, nullptr) == E && msg(c, "ctx"));
        else {
            EXPECT(f(c, X.data(), n, 0, w.data(), nullptr, nullptr, nullptr, nullptr) == QMRI_ERR_STATE && msg(c, "components not set"));
            fill_dictionary(ctx.dict, 12, 4);                                                 // a dictionary alone is not enough
            EXPECT(f(c, X.data(), n, 1, w.data(), nullptr, nullptr, nullptr, nullptr) == QMRI_ERR_STATE && msg(c, "components not set"));
        }
    }
}

// the table against a direct evaluation
static void form_components() {
    DictHost d;
    fill_dictionary(d, 12, 6);
    const int32_t atoms[4] = {9, 2, 12, 4};
    double tab[PV_TAB], piv = -1.0;
    std::string m;
    EXPECT(pv_form_components(d.D_h.data(), d.normD_h.data(), d.K, d.s, 4, atoms, tab, &piv, &m) == QMRI_OK && m.empty());
    EXPECT(piv > 1e-10 && piv <= 1.0);
    for (int c = 0; c < PV_MAX_C; ++c)
        for (int j = 0; j < PV_MAX_S; ++j) {
            const double want = (c < 4 && j < 6) ? (double)d.normD_h[atoms[c] - 1] * (double)d.D_h[(atoms[c] - 1) + (size_t)12 * j] : 0.0;
            EXPECT(tab[PV_TAB_A + j * PV_MAX_C + c] == want);
        }
    for (int a = 0; a < 4; ++a) {
        for (int b = 0; b < 4; ++b) {
            double g = 0.0;
            for (int j = 0; j < 6; ++j) g += tab[PV_TAB_A + j * PV_MAX_C + a] * tab[PV_TAB_A + j * PV_MAX_C + b];
            EXPECT(tab[PV_TAB_G + a * PV_MAX_C + b] == g && tab[PV_TAB_G + b * PV_MAX_C + a] == g);
        }
        EXPECT(tab[PV_TAB_NA + a] == std::sqrt(tab[PV_TAB_G + a * PV_MAX_C + a]));
    }
    for (int j = 0; j < 6; ++j) {
        double t = 0.0;
        for (int c = 0; c < 4; ++c) t += tab[PV_TAB_A + j * PV_MAX_C + c];
        EXPECT(tab[PV_TAB_ASUM + j] == t);
    }
    const int32_t one[1] = {3};                              // one component: pivot exactly 1
    EXPECT(pv_form_components(d.D_h.data(), d.normD_h.data(), d.K, d.s, 1, one, tab, &piv, &m) == QMRI_OK && piv == 1.0);
    const int32_t full[6] = {1, 2, 3, 4, 8, 9};              // C == s is allowed
    EXPECT(pv_form_components(d.D_h.data(), d.normD_h.data(), d.K, d.s, 6, full, tab, &piv, &m) == QMRI_OK && piv > 1e-10);
}

int main() {
    drive_set();
    drive_unmix(qmri_dict_unmix);
    drive_unmix(qmri_dict_unmix_dev);
    form_components();
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_PV_OK\n");
    return 0;
}
