// host_asan_coilmaps.cpp -- every refusal of qmri_coil_maps / qmri_coil_maps_dev (api_csm.cpp) under the host-only
// AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided
// before the device is selected, so a context in each state is made here by hand.  Run by tests/test_coil_maps_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

typedef int (*entry_t)(qmri_ctx*, int, int, int, int, const void*, const qmri_csm_params*, void*, void*, double*, qmri_csm_info*);

static void drive(entry_t f, bool dev) {
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    const qmri_csm_params ok = QMRI_CSM_PARAMS_DEFAULT(16, 16);
    qmri_csm_info info;
    auto msg = [](qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; };
    for (int pass = 0; pass < 2; ++pass) {          // without a context (messages in qmri_last_error(NULL)), then with one
        qmri_ctx ctx;
        ctx.op.ready = true; ctx.op.kind = OP_GRIDDED; ctx.op.N = 32; ctx.op.M = 64; ctx.op.s = 1; ctx.op.maxB = 2;
        qmri_ctx* c = pass ? &ctx : nullptr;
        EXPECT(f(c, 1, 8, 32, 64, a, nullptr, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "params"));
        EXPECT(f(c, 1, 8, 32, 64, nullptr, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "calib"));
        EXPECT(f(c, 1, 8, 32, 64, a, &ok, nullptr, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "maps_out"));
        EXPECT(f(c, 0, 8, 32, 64, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "nslices"));
        EXPECT(f(c, 1, 0, 32, 64, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "ncoil"));
        EXPECT(f(c, 1, 129, 32, 64, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_UNSUPPORTED && msg(c, "128"));
        EXPECT(f(c, 1, 8, 33, 64, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "supported sizes"));
        EXPECT(f(c, 1, 8, 32, 48, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "supported sizes"));
        qmri_csm_params p = ok;
        p.kind = 2;
        EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "kind"));
        const int badc[] = {15, 6, 34, -2};
        for (int v : badc) {
            p = ok; p.cN = v;
            EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "cN"));
            p = ok; p.cM = v == 34 ? 66 : v;
            EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "cM"));
        }
        p = ok; p.window = 2;
        EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "window"));
        p = ok; p.patch = -1;
        EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "patch"));
        p.patch = 5;
        EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "patch"));
        p = ok; p.phase_ref = 2;
        EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "phase_ref"));
        p = ok; p.thresh = -0.1;
        EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "thresh"));
        p.thresh = NAN;
        EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "thresh"));
        if (dev) EXPECT(f(c, 1, 8, 32, 64, a, &ok, a, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "alias"));
        p = ok; p.kind = QMRI_CSM_IMAGES; p.cN = p.cM = 0; p.window = 7;      // an IMAGES call ignores the block's fields
        if (!pass) {
            EXPECT(f(c, 1, 8, 32, 64, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "ctx"));
            EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "ctx"));
        } else {
            EXPECT(f(c, 1, 8, 64, 32, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_INVALID_ARG && msg(c, "operator's grid"));
            ctx.op.ready = false;
            EXPECT(f(c, 1, 8, 32, 64, a, &ok, b, nullptr, nullptr, &info) == QMRI_ERR_STATE && msg(c, "operator not set"));
            EXPECT(f(c, 1, 8, 32, 64, a, &p, b, nullptr, nullptr, &info) == QMRI_ERR_STATE);
        }
        ctx.op.ready = false;                     // (nothing was allocated: nothing for a destructor to release)
    }
}

int main() {
    drive(qmri_coil_maps, false);
    drive(qmri_coil_maps_dev, true);
    // the LDS plan of the eigen kernel: a function of (ncoil, patch) alone, at least one coil per chunk everywhere
    for (int n = 1; n <= 128; ++n)
        for (int p = 0; p <= 4; ++p) { const int ch = csm_chunk_coils(n, p); EXPECT(ch >= 1 && ch <= n); }
    EXPECT(csm_chunk_coils(8, 3) == 8 && csm_chunk_coils(32, 3) < 32);
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_COILMAPS_OK\n");
    return 0;
}
