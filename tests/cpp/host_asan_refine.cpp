// host_asan_refine.cpp -- every refusal of qmri_dict_lines / qmri_set_refine / qmri_dict_refine / qmri_dict_refine_dev (api_refine.cpp; DESIGN.md
// section 30) and the host code that builds the lines, under the host-only AddressSanitizer + UBSan build of libqmri
// (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided before the device is selected; the
// dictionary a context needs is put into its host copy directly (qmri_set_dictionary itself uploads).  Run by tests/test_refine_host.py.
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

// n1 x n2 grid of (T1, T2), K = n1 n2 atoms of s channels, column-major
static void fill_dictionary(DictHost& d, int n1, int n2, int s) {
    const int K = n1 * n2;
    d.ready = true; d.K = K; d.s = s; d.Q = 2; d.wide = 0;
    d.D_h.assign((size_t)K * s, 0.f); d.normD_h.assign(K, 1.f); d.lut_h.assign((size_t)K * 2, 0.f);
    for (int a = 0; a < K; ++a) {
        for (int j = 0; j < s; ++j) d.D_h[a + (size_t)K * j] = std::cos(0.37f * (a + 1) * (j + 1));
        d.normD_h[a] = 1.f + 0.25f * a;
        d.lut_h[a] = 0.1f * (1 + a / n2); d.lut_h[a + (size_t)K] = 0.01f * (1 + a % n2);
    }
}

static void drive_lines() {
    const int E = QMRI_ERR_INVALID_ARG;
    DictHost d;
    fill_dictionary(d, 5, 4, 3);
    std::vector<int32_t> nbr((size_t)d.K * 3 * 2);
    int32_t info[9];
    const int32_t c01[2] = {0, 1}, rep[2] = {0, 0}, hi[2] = {0, 2}, neg[1] = {-1};
    const float* lut = d.lut_h.data(); const float* nd = d.normD_h.data();
    EXPECT(qmri_dict_lines(d.K, 2, nullptr, nd, 2, c01, nbr.data(), info) == E && msg(nullptr, "must not be NULL"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nullptr, 2, c01, nbr.data(), info) == E && msg(nullptr, "must not be NULL"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 2, nullptr, nbr.data(), info) == E && msg(nullptr, "must not be NULL"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 2, c01, nullptr, info) == E && msg(nullptr, "must not be NULL"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 2, c01, nbr.data(), nullptr) == E && msg(nullptr, "must not be NULL"));
    EXPECT(qmri_dict_lines(0, 2, lut, nd, 2, c01, nbr.data(), info) == E && msg(nullptr, "K >= 1"));
    EXPECT(qmri_dict_lines(d.K, 0, lut, nd, 2, c01, nbr.data(), info) == E && msg(nullptr, "Q >= 1"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 0, c01, nbr.data(), info) == E && msg(nullptr, "1 <= P <= 3"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 4, c01, nbr.data(), info) == E && msg(nullptr, "1 <= P <= 3"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 2, rep, nbr.data(), info) == E && msg(nullptr, "twice"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 2, hi, nbr.data(), info) == E && msg(nullptr, "outside 0..1"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 1, neg, nbr.data(), info) == E && msg(nullptr, "outside 0..1"));
    EXPECT(qmri_dict_lines(d.K, 1, lut, nd, 1, c01, nbr.data(), info) == QMRI_OK);           // one column: every atom of a value on one line
    std::vector<float> flat((size_t)d.K * 2, 0.5f);
    EXPECT(qmri_dict_lines(d.K, 2, flat.data(), nd, 1, c01, nbr.data(), info) == E && msg(nullptr, "lut column 0 has no lines"));
    EXPECT(qmri_dict_lines(d.K, 2, lut, nd, 2, c01, nbr.data(), info) == QMRI_OK);
    EXPECT(info[0] == 0 && info[1] == 2 * 4 && info[2] == 3 * 4 && info[3] == 0 && info[4] == 2 * 5 && info[5] == 2 * 5);
    const int k = 2 * 4 + 1;
    EXPECT(nbr[k * 4] == k - 4 && nbr[k * 4 + 1] == k + 4 && nbr[k * 4 + 2] == k - 1 && nbr[k * 4 + 3] == k + 1);
}

static void drive_set() {
    const int E = QMRI_ERR_INVALID_ARG;
    const int32_t c01[2] = {0, 1};
    qmri_refine_info info;
    EXPECT(qmri_set_refine(nullptr, -1, c01, &info) == E && msg(nullptr, "0 <= P <= 3"));
    EXPECT(qmri_set_refine(nullptr, 4, c01, &info) == E && msg(nullptr, "0 <= P <= 3"));
    EXPECT(qmri_set_refine(nullptr, 2, nullptr, &info) == E && msg(nullptr, "cols"));
    EXPECT(qmri_set_refine(nullptr, 2, c01, &info) == E && msg(nullptr, "ctx"));
    EXPECT(qmri_set_refine(nullptr, 0, nullptr, nullptr) == E && msg(nullptr, "ctx"));
    {
        qmri_ctx ctx;
        qmri_ctx* c = &ctx;
        EXPECT(qmri_set_refine(c, 2, c01, &info) == QMRI_ERR_STATE && msg(c, "dictionary not set"));
        info.P = 7;
        EXPECT(qmri_set_refine(c, 0, nullptr, &info) == QMRI_OK && info.P == 0);               // clearing needs nothing
        EXPECT(qmri_set_refine(c, 4, c01, nullptr) == E && qmri_set_refine(c, 1, nullptr, nullptr) == E);
        ctx.dict.ready = true; ctx.dict.wide = 1; ctx.dict.K = 40; ctx.dict.s = 24;
        EXPECT(qmri_set_refine(c, 2, c01, &info) == QMRI_ERR_UNSUPPORTED && msg(c, "s <= 16"));
        fill_dictionary(ctx.dict, 5, 4, 3);
        ctx.dict.rf.P = 1; ctx.dict.rf.cols[0] = 1;                                            // "an earlier state": a refused call leaves it
        const int32_t rep[2] = {1, 1}, hi[2] = {0, 2}, neg[1] = {-1};
        EXPECT(qmri_set_refine(c, 2, rep, &info) == E && msg(c, "twice"));
        EXPECT(qmri_set_refine(c, 2, hi, &info) == E && msg(c, "outside 0..1"));
        EXPECT(qmri_set_refine(c, 1, neg, &info) == E && msg(c, "outside 0..1"));
        for (int a = 0; a < ctx.dict.K; ++a) ctx.dict.lut_h[a + (size_t)ctx.dict.K] = 0.25f;    // a single T2
        EXPECT(qmri_set_refine(c, 2, c01, &info) == E && msg(c, "lut column 1 has no lines"));
        EXPECT(ctx.dict.rf.P == 1 && ctx.dict.rf.cols[0] == 1 && !ctx.dict.rf.d_nbr.p);
        EXPECT(qmri_set_refine(c, 0, nullptr, nullptr) == QMRI_OK && ctx.dict.rf.P == 0);
        ctx.dict.rf.P = 2;
        qmri_free_dict(c);                                                                     // what qmri_set_dictionary does first
        EXPECT(!ctx.dict.ready && ctx.dict.rf.P == 0 && ctx.dict.lut_h.empty());
    }
}

typedef int (*refine_t)(qmri_ctx*, const void*, int, const int32_t*, double*, double*, double*, double*, int32_t*, int32_t*);

static void drive_refine(refine_t f) {
    const int E = QMRI_ERR_INVALID_ARG, n = 5;
    std::vector<double> X((size_t)2 * n * 3, 0.25), q((size_t)n * 2);
    std::vector<int32_t> dm(n, 1);
    for (int pass = 0; pass < 2; ++pass) {
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        EXPECT(f(c, X.data(), 0, dm.data(), q.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == E && msg(c, "Npix"));
        EXPECT(f(c, X.data(), -3, dm.data(), q.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == E && msg(c, "Npix"));
        EXPECT(f(c, nullptr, n, dm.data(), q.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == E && msg(c, "X / dm"));
        EXPECT(f(c, X.data(), n, nullptr, q.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == E && msg(c, "X / dm"));
        if (!pass) EXPECT(f(c, X.data(), n, dm.data(), q.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == E && msg(c, "ctx"));
        else {
            EXPECT(f(c, X.data(), n, dm.data(), q.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == QMRI_ERR_STATE && msg(c, "refinement not set"));
            fill_dictionary(ctx.dict, 5, 4, 3);                                                // a dictionary alone is not enough
            EXPECT(f(c, X.data(), n, dm.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == QMRI_ERR_STATE && msg(c, "refinement not set"));
        }
    }
}

int main() {
    drive_lines();
    drive_set();
    drive_refine(qmri_dict_refine);
    drive_refine(qmri_dict_refine_dev);
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_REFINE_OK\n");
    return 0;
}
