// host_asan_epgseq.cpp -- every refusal of qmri_dict_simulate_seq / qmri_dict_simulate_seq_dev (api_epg.cpp) and the plan
// function of epg_seq_plan.h under the host-only AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a
// machine without a GPU.  Every refusal is decided before the device is selected and needs neither an operator nor a dictionary; the block array
// holds exactly nblocks entries, so a read past it is an error here.  Run by tests/test_epgseq_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "epg_seq_plan.h"
#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

typedef int (*entry_t)(qmri_ctx*, int, int, const double*, const double*, const double*, const double*, const double*, const double*, const qmri_epg_params*,
                       const qmri_epg_seq*, void*);

static void drive(entry_t f, bool host_atoms) {
    const int K = 3, T = 4, B = 3, E = QMRI_ERR_INVALID_ARG;
    const double al[T] = {0.1, 0.2, 0.0, 0.4}, tr[T] = {0.012, 0.012, 0.013, 0.012}, te[T] = {0.002, 0.0, 0.013, 0.002};
    const double t1[K] = {1.0, 0.5, 2.0}, t2[K] = {0.1, 0.05, 0.2}, b1[K] = {1.0, 0.0, 1.2};
    const qmri_epg_block blocks[B] = {{1, 1, 0.0, 0.021, 0.95}, {2, 0, 0.5, 0.0, 1.0}, {1, 2, 0.3, 0.040, 1.0}};
    const double canary = -7.0;
    double F[K * T];
    for (double& v : F) v = canary;
    const qmri_epg_params ok = {32, 0, 0.0, 1.0, 1};
    const qmri_epg_seq sq = {B, 2, blocks, {0, 0, 0, 0}};
    auto msg = [](qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; };
    for (int pass = 0; pass < 2; ++pass) {          // without a context (messages in qmri_last_error(NULL)), then with one
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        // the refusals of qmri_dict_simulate carry over, and come first
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, nullptr, &sq, F) == E && msg(c, "params"));
        EXPECT(f(c, K, T, nullptr, tr, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, nullptr, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, nullptr, t1, t2, b1, &ok, &sq, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, nullptr, t2, b1, &ok, &sq, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, t1, nullptr, b1, &ok, &sq, F) == E && msg(c, "alpha /"));
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &sq, nullptr) == E && msg(c, "F_out"));
        EXPECT(f(c, 0, T, al, tr, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "K must"));
        EXPECT(f(c, K, 0, al, tr, te, t1, t2, b1, &ok, nullptr, F) == E && msg(c, "T must"));
        EXPECT(f(c, K, 1025, al, tr, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "T must"));
        qmri_epg_params p = ok;
        const int bad_s[] = {0, -1, 257};
        for (int v : bad_s) { p = ok; p.nstates = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sq, F) == E && msg(c, "nstates")); }
        p = ok; p.inversion = 2;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sq, F) == E && msg(c, "inversion must be 0 or 1"));
        p = ok; p.out_is_f64 = -1;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sq, F) == E && msg(c, "out_is_f64"));
        const double bad_frame[] = {-0.1, NAN, INFINITY};
        for (double v : bad_frame) {
            double x[T];
            std::memcpy(x, al, sizeof x); x[2] = v;
            EXPECT(f(c, K, T, x, tr, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "alpha must"));
            std::memcpy(x, tr, sizeof x); x[3] = v;
            EXPECT(f(c, K, T, al, x, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "tr must"));
            std::memcpy(x, te, sizeof x); x[1] = v;
            EXPECT(f(c, K, T, al, tr, x, t1, t2, b1, &ok, &sq, F) == E && msg(c, "te must"));
        }
        {
            double x[T];
            std::memcpy(x, tr, sizeof x); x[1] = 0.0;
            EXPECT(f(c, K, T, al, x, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "tr must"));
            std::memcpy(x, te, sizeof x); x[0] = 0.0125;
            EXPECT(f(c, K, T, al, tr, x, t1, t2, b1, &ok, &sq, F) == E && msg(c, "te must not exceed tr"));
        }
        const double bad_atom[] = {0.0, -1.0, NAN, INFINITY};
        for (double v : bad_atom) {
            double x[K];
            if (!host_atoms) break;                                     // the device route cannot read its atoms here
            std::memcpy(x, t1, sizeof x); x[2] = v;
            EXPECT(f(c, K, T, al, tr, te, x, t2, b1, &ok, &sq, F) == E && msg(c, "t1 must"));
            std::memcpy(x, t2, sizeof x); x[0] = v;
            EXPECT(f(c, K, T, al, tr, te, t1, x, b1, &ok, &sq, F) == E && msg(c, "t2 must"));
            if (v != 0.0) {
                std::memcpy(x, b1, sizeof x); x[1] = v;
                EXPECT(f(c, K, T, al, tr, te, t1, t2, x, &ok, &sq, F) == E && msg(c, "b1 must"));
            }
        }
        // the schedule's own
        p = ok; p.inversion = 1;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &p, &sq, F) == E && msg(c, "stated in the blocks"));
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, nullptr, F) == E && msg(c, "seq / blocks"));
        qmri_epg_seq s = sq;
        s.blocks = nullptr;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "seq / blocks"));
        const int bad_nb[] = {0, -2, 65};
        for (int v : bad_nb) { s = sq; s.nblocks = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "nblocks must")); }
        const int bad_nc[] = {0, -1, 17};
        for (int v : bad_nc) { s = sq; s.ncycles = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "ncycles must")); }
        for (int i = 0; i < 4; ++i) { s = sq; s.reserved[i] = 1; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "reserved")); }
        qmri_epg_block bl[B];
        s = sq; s.blocks = bl;
        auto fresh = [&] { std::memcpy(bl, blocks, sizeof bl); };
        const int bad_nf[] = {0, -3};
        for (int v : bad_nf) { fresh(); bl[B - 1].nframes = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "nframes must")); }
        const int bad_prep[] = {-1, 3};
        for (int v : bad_prep) { fresh(); bl[B - 1].prep = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "prep must")); }
        const double bad_time[] = {-1e-3, NAN, INFINITY};
        for (double v : bad_time) {
            fresh(); bl[B - 1].wait = v;
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "wait must"));
            fresh(); bl[0].prep_time = v;
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "prep_time must"));
        }
        const double bad_eff[] = {0.0, -0.5, 1.0001, NAN};
        for (double v : bad_eff) { fresh(); bl[B - 1].prep_eff = v; EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "prep_eff must")); }
        fresh(); bl[1].prep_time = 0.01;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "without a preparation"));
        fresh(); bl[1].prep_eff = 0.9;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "without a preparation"));
        fresh(); bl[1].nframes = 3;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "sum to T"));
        fresh(); bl[1].nframes = 1;
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "sum to T"));
        fresh(); bl[0].nframes = 2147483647; bl[1].nframes = 2147483647;        // the sum is taken in 64 bits
        EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &s, F) == E && msg(c, "sum to T"));
        p = ok; p.ti = -1.0; p.inv_eff = 7.0;                            // without an inversion its fields are ignored
        if (!pass) {
            EXPECT(f(c, K, T, al, tr, te, t1, t2, b1, &ok, &sq, F) == E && msg(c, "ctx"));
            EXPECT(f(c, K, T, al, tr, te, t1, t2, nullptr, &p, &sq, F) == E && msg(c, "ctx"));
            if (!host_atoms) {
                double x[K];
                std::memcpy(x, t1, sizeof x); x[2] = NAN;               // passes the host checks of the device route
                EXPECT(f(c, K, T, al, tr, te, x, t2, b1, &ok, &sq, F) == E && msg(c, "ctx"));
            }
        }
    }
    for (double v : F) EXPECT(v == canary);                             // a refused call writes nothing
}

int main() {
    drive(qmri_dict_simulate_seq, true);
    drive(qmri_dict_simulate_seq_dev, false);
    // the plan: the fixture of the GPU tests (blocks of 5, 16, 17, 10 frames) in segments of at most 16 that never straddle a block
    const qmri_epg_block mix[4] = {{5, 0, 0.0, 0.0, 1.0}, {16, 1, 0.3, 0.021, 0.95}, {17, 2, 0.25, 0.040, 1.0}, {10, 2, 0.01, 0.080, 0.9}};
    const std::vector<epgseq::Segment> sg = epgseq::plan(4, mix);
    const int t0[5] = {0, 5, 21, 37, 38}, nf[5] = {5, 16, 16, 1, 10}, first[5] = {1, 1, 1, 0, 1}, prep[5] = {0, 1, 2, 0, 2};
    EXPECT(sg.size() == 5 && (int)sg.size() <= epgseq::max_segments(48, 4));
    for (size_t i = 0; i < sg.size() && i < 5; ++i)
        EXPECT(sg[i].t0 == t0[i] && sg[i].nf == nf[i] && sg[i].first == first[i] && sg[i].prep == prep[i]);
    EXPECT(sg.size() == 5 && sg[2].wait == 0.25 && sg[2].prep_time == 0.040 && sg[3].wait == 0.0 && sg[3].prep_time == 0.0 && sg[3].prep_eff == 1.0 &&
           sg[4].prep_eff == 0.9);
    std::vector<qmri_epg_block> many(64, qmri_epg_block{16, 2, 0.5, 0.04, 1.0});
    EXPECT(epgseq::plan(64, many.data()).size() == 64 && epgseq::max_segments(1024, 64) == 128);
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_EPGSEQ_OK\n");
    return 0;
}
