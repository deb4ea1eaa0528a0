// host_asan_dictg.cpp -- the assignment rule and the host-side refusals of the grouped dictionary match (dictg_kernels.hip, api_dict.cpp; DESIGN.md
// section 20) under the host-only AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine
// without a GPU.  Run by tests/test_dict_group_host.py.
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

int main() {
    const int E = QMRI_ERR_INVALID_ARG;
    auto msg = [](qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; };
    // the rule: exact midpoints to the lower group, outside values to the end groups, non-finite values unmatched
    const double gv[3] = {0.75, 1.0, 1.25};
    const double sel[8] = {0.875, 1.125, 0.1, 9.0, 1.0, NAN, INFINITY, -0.0};
    const int32_t want[8] = {1, 2, 1, 3, 2, 0, 0, 1};
    int32_t got[8];
    EXPECT(qmri_dict_group_assign(3, gv, 8, sel, got) == QMRI_OK && std::memcmp(got, want, sizeof want) == 0);
    EXPECT(qmri_dict_group_assign(3, gv, 0, nullptr, nullptr) == QMRI_OK);
    {
        std::vector<double> v(256), b(1000);
        std::vector<int32_t> g(1000);
        for (int i = 0; i < 256; ++i) v[i] = 0.5 + i / 256.0;
        for (int i = 0; i < 1000; ++i) b[i] = 0.4 + i * 1.3e-3;
        EXPECT(qmri_dict_group_assign(256, v.data(), 1000, b.data(), g.data()) == QMRI_OK && g[0] == 1 && g[999] == 256);
        for (int i = 1; i < 1000; ++i) EXPECT(g[i] >= g[i - 1]);
    }
    EXPECT(qmri_dict_group_assign(0, gv, 8, sel, got) == E && msg(nullptr, "G <= 256"));
    EXPECT(qmri_dict_group_assign(257, gv, 8, sel, got) == E && msg(nullptr, "G <= 256"));
    EXPECT(qmri_dict_group_assign(3, nullptr, 8, sel, got) == E && msg(nullptr, "NULL"));
    EXPECT(qmri_dict_group_assign(3, gv, 8, nullptr, got) == E && msg(nullptr, "NULL"));
    EXPECT(qmri_dict_group_assign(3, gv, 8, sel, nullptr) == E && msg(nullptr, "NULL"));
    EXPECT(qmri_dict_group_assign(3, gv, -1, sel, got) == E);
    const double bad[][3] = {{1.0, 0.75, 1.25}, {0.75, 0.75, 1.25}, {0.75, NAN, 1.25}, {0.75, 1.0, INFINITY}, {-INFINITY, 1.0, 1.25}};
    for (const auto& b : bad) EXPECT(qmri_dict_group_assign(3, b, 8, sel, got) == E && msg(nullptr, "ascending"));
    // the context calls: NULL context, then a context without a dictionary (argument refusals come first, then the state)
    const int32_t gp[4] = {0, 2, 5, 9};
    EXPECT(qmri_set_dictionary_groups(nullptr, 3, gp, gv) == E);
    EXPECT(qmri_dict_match_grouped(nullptr, sel, 8, sel, nullptr, nullptr, nullptr, nullptr, got, nullptr) == E);
    EXPECT(qmri_dict_match_grouped_dev(nullptr, sel, 8, sel, nullptr, nullptr, nullptr, nullptr, got, nullptr) == E);
    {
        qmri_ctx ctx;
        EXPECT(qmri_set_dictionary_groups(&ctx, 257, gp, gv) == E && msg(&ctx, "G <= 256"));
        EXPECT(qmri_set_dictionary_groups(&ctx, -1, gp, gv) == E);
        EXPECT(qmri_set_dictionary_groups(&ctx, 3, nullptr, gv) == E && msg(&ctx, "NULL"));
        EXPECT(qmri_set_dictionary_groups(&ctx, 3, gp, nullptr) == E && msg(&ctx, "NULL"));
        const int32_t empty[4] = {0, 2, 2, 9}, back[4] = {0, 5, 2, 9}, off[4] = {1, 2, 5, 9};
        EXPECT(qmri_set_dictionary_groups(&ctx, 3, empty, gv) == E && msg(&ctx, "strictly increasing"));
        EXPECT(qmri_set_dictionary_groups(&ctx, 3, back, gv) == E && msg(&ctx, "strictly increasing"));
        EXPECT(qmri_set_dictionary_groups(&ctx, 3, off, gv) == E && msg(&ctx, "group_ptr[0]"));
        for (const auto& b : bad) EXPECT(qmri_set_dictionary_groups(&ctx, 3, gp, b) == E && msg(&ctx, "ascending"));
        EXPECT(qmri_set_dictionary_groups(&ctx, 3, gp, gv) == QMRI_ERR_STATE && msg(&ctx, "dictionary not set"));
    }
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_DICTG_OK\n");
    return 0;
}
