// host_asan_devmem.cpp -- the failure contract of the memory owners (csrc/dev_mem.h: DevArr, PinnedArr, DevPool) under the host-only
// AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU: there every allocation
// fails, which is the path no GPU test reaches.  Run by tests/test_devmem_host.py::test_failure_contract_under_address_and_ub_sanitizer.
#include <cstdio>
#include <cstring>
#include <utility>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

static bool nothing_live() {
    qmri_mem_stats s;
    std::memset(&s, 0xff, sizeof s);
    return qmri_debug_mem_stats(&s) == QMRI_OK && s.dev_live == 0 && s.dev_bytes == 0 && s.dev_total == 0 && s.pinned_live == 0 && s.pinned_bytes == 0 &&
           s.pinned_total == 0;
}

template <typename Arr> static void array_contract(qmri_ctx* ctx, const char* api) {
    Arr a;
    EXPECT(a.p == nullptr && a.cap == 0);
    a.reset();                                                       // an empty owner
    EXPECT(a.p == nullptr && a.cap == 0);
    qmri_set_error(ctx, "untouched");
    EXPECT(a.ensure(ctx, 100) == QMRI_ERR_NOMEM);
    EXPECT(a.p == nullptr && a.cap == 0);
    EXPECT(std::strstr(qmri_last_error(ctx), api) && std::strstr(qmri_last_error(ctx), "bytes failed"));     // the library's own message
    EXPECT(a.ensure(ctx, 7, "the site's own text") == QMRI_ERR_NOMEM);
    EXPECT(a.p == nullptr && a.cap == 0 && std::strcmp(qmri_last_error(ctx), "the site's own text") == 0);
    EXPECT(a.ensure(ctx, 0) == QMRI_ERR_NOMEM && a.p == nullptr && a.cap == 0);                             // (at least one element is asked for)
    decltype(a.p) raw = a;                                           // converts to T*
    EXPECT(raw == nullptr);
    Arr b(std::move(a));                                             // move construction and assignment leave the source empty
    EXPECT(a.p == nullptr && a.cap == 0 && b.p == nullptr && b.cap == 0);
    a.reset();                                                       // a moved-from owner
    Arr c;
    c = std::move(b);
    EXPECT(b.p == nullptr && b.cap == 0 && c.p == nullptr && c.cap == 0);
    b.reset();
    Arr& same = c;
    c = std::move(same);                                             // self-assignment
    EXPECT(c.p == nullptr && c.cap == 0);
    EXPECT(nothing_live());
}

int main() {
    EXPECT(qmri_debug_mem_stats(nullptr) == QMRI_ERR_INVALID_ARG);
    EXPECT(nothing_live());
    qmri_ctx c;
    for (qmri_ctx* ctx : {&c, (qmri_ctx*)nullptr}) {                 // (without a context the message goes where qmri_create's goes)
        array_contract<DevArr<double2>>(ctx, "hipMalloc");
        array_contract<PinnedArr<LsqrState>>(ctx, "hipHostMalloc");
        {
            DevArr<void> v;                                          // capacity in bytes
            EXPECT(v.ensure(ctx, 64) == QMRI_ERR_NOMEM && v.p == nullptr && v.cap == 0);
        }
        {
            DevPool pool;
            pool.reset();                                            // an empty pool
            double* x = (double*)&c;                                 // (any non-null value: a failed alloc must null it)
            const float* y = (const float*)&c;
            EXPECT(pool.alloc(ctx, &x, 10) == QMRI_ERR_NOMEM && x == nullptr && pool.recs.empty());
            EXPECT(std::strstr(qmri_last_error(ctx), "hipMalloc of 80 bytes failed"));
            EXPECT(pool.alloc(ctx, &y, 3, "pool text") == QMRI_ERR_NOMEM && y == nullptr && pool.recs.empty());
            EXPECT(std::strcmp(qmri_last_error(ctx), "pool text") == 0);
            pool.free_one(nullptr);
            pool.free_one(&c);                                       // not one of its arrays: nothing happens
            pool.reset();                                            // after failed allocs: frees only what succeeded, which is nothing
            EXPECT(pool.recs.empty());
            DevPool q(std::move(pool));
            pool.reset();
            DevPool r;
            r = std::move(q);
            q.reset();
            EXPECT(r.recs.empty() && q.recs.empty() && pool.recs.empty());
        }
        EXPECT(nothing_live());
    }
    {   // the owners inside the context-owned structs: replacing a plan by a fresh value, as the qmri_free_* functions do
        c.op = OpHost();
        c.net = NetPlan();
        c.cc = CcWork();
        c.op.mc = McWork();
        qmri_free_operator(&c);
        qmri_free_net(&c);
        qmri_free_dict(&c);
        EXPECT(c.op.pool.recs.empty() && c.net.pool.recs.empty() && c.dict.pool.recs.empty() && c.op.h_state.p == nullptr && c.cc.hK.p == nullptr);
        // a grower of the library itself: the first allocation fails, the work buffers stay empty, the site's message is the one reported
        c.op.N = c.op.M = 32; c.op.s = 1; c.op.m = 16; c.op.maxB = 1;
        EXPECT(mc_ensure_work(&c, 2, 4) == QMRI_ERR_NOMEM && std::strstr(qmri_last_error(&c), "multi-coil LSQR of 2 slices x 4 coils"));
        EXPECT(c.op.mc.ut.p == nullptr && c.op.mc.ut.cap == 0 && c.op.mc.hst.p == nullptr);
        EXPECT(mc_ensure_staging(&c, 2, 4) == QMRI_ERR_NOMEM && std::strstr(qmri_last_error(&c), "staging of 2 slices x 4 coils"));
        EXPECT(cc_ensure_staging(&c, 8, 8, 8, 8) == QMRI_ERR_NOMEM && std::strstr(qmri_last_error(&c), "staging of the coil compression"));
        EXPECT(c.cc.sy.p == nullptr && c.cc.sy.cap == 0);
    }
    EXPECT(nothing_live());
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_DEVMEM_OK\n");
    return 0;
}
