// host_asan_wav.cpp -- every refusal of qmri_wavelet_prox / qmri_wavelet_prox_dev / qmri_set_wavelet (api_wav.cpp), the mutual
// exclusion with qmri_set_llr and the offset rule of the ADMM loop under the host-only AddressSanitizer + UBSan build of libqmri
// (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided before the device is selected and needs
// neither an operator nor a denoiser.  Run by tests/test_wavelet_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

typedef int (*entry_t)(qmri_ctx*, int, int, int, int, const void*, int, const qmri_wavelet_params*, int, int, void*, double*);

static bool msg(qmri_ctx* c, const char* word) { return std::strstr(qmri_last_error(c), word) != nullptr; }

static void drive(entry_t f) {
    const int N = 16, M = 32, s = 3, S = 2, E = QMRI_ERR_INVALID_ARG;
    std::vector<double> x((size_t)2 * N * M * s * S, 0.5), out(x.size());
    double cm[S];
    qmri_wavelet_params ok = {};
    ok.tau = 0.1; ok.levels = 3; ok.filter = QMRI_WAVELET_DB2; ok.joint = 1;
    for (int pass = 0; pass < 2; ++pass) {          // without a context (messages in qmri_last_error(NULL)), then with one
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        EXPECT(f(c, N, M, s, S, nullptr, 1, &ok, 0, 0, out.data(), cm) == E && msg(c, "x / p / out"));
        EXPECT(f(c, N, M, s, S, x.data(), 1, nullptr, 0, 0, out.data(), cm) == E && msg(c, "x / p / out"));
        EXPECT(f(c, N, M, s, S, x.data(), 1, &ok, 0, 0, nullptr, cm) == E && msg(c, "x / p / out"));
        const int bad_S[] = {0, -1};
        for (int v : bad_S) EXPECT(f(c, N, M, s, v, x.data(), 1, &ok, 0, 0, out.data(), nullptr) == E && msg(c, "nslices"));
        const int bad_s[] = {0, -2, 17};
        for (int v : bad_s) EXPECT(f(c, N, M, v, S, x.data(), 1, &ok, 0, 0, out.data(), nullptr) == E && msg(c, "1 <= s <= 16"));
        qmri_wavelet_params p = ok;
        const double bad_tau[] = {-1e-9, NAN, INFINITY, -INFINITY};
        for (double v : bad_tau) { p = ok; p.tau = v; EXPECT(f(c, N, M, s, S, x.data(), 1, &p, 0, 0, out.data(), nullptr) == E && msg(c, "tau")); }
        const int bad_L[] = {-1, 5, 100};
        for (int v : bad_L) { p = ok; p.levels = v; EXPECT(f(c, N, M, s, S, x.data(), 1, &p, 0, 0, out.data(), nullptr) == E && msg(c, "levels must be")); }
        const int bad_f[] = {-1, 2, 97};
        for (int v : bad_f) { p = ok; p.filter = v; EXPECT(f(c, N, M, s, S, x.data(), 1, &p, 0, 0, out.data(), nullptr) == E && msg(c, "filter must be")); }
        const int bad_j[] = {-1, 2};
        for (int v : bad_j) { p = ok; p.joint = v; EXPECT(f(c, N, M, s, S, x.data(), 1, &p, 0, 0, out.data(), nullptr) == E && msg(c, "joint")); }
        for (int k = 0; k < 4; ++k) { p = ok; p.reserved[k] = k + 1; EXPECT(f(c, N, M, s, S, x.data(), 1, &p, 0, 0, out.data(), nullptr) == E && msg(c, "reserved")); }
        const int bad_n[] = {0, -8, 12, 20, 7, 32768};
        for (int v : bad_n) {
            EXPECT(f(c, v, M, s, S, x.data(), 1, &ok, 0, 0, out.data(), nullptr) == E && msg(c, "multiples of 2^levels"));
            EXPECT(f(c, N, v, s, S, x.data(), 1, &ok, 0, 0, out.data(), nullptr) == E && msg(c, "multiples of 2^levels"));
        }
        p = ok; p.levels = 4;                        // 16 / 2^3 = 2 < 4 taps: the last level's input is too short for DB2, not for Haar
        EXPECT(f(c, 16, 32, s, S, x.data(), 1, &p, 0, 0, out.data(), nullptr) == E && msg(c, "levels = 4, 4 taps"));
        p = ok; p.levels = 0;                        // 0 is 3
        EXPECT(f(c, 12, 32, s, S, x.data(), 1, &p, 0, 0, out.data(), nullptr) == E && msg(c, "levels = 3"));
        const int bad_o[] = {-1, 8, 100};
        for (int v : bad_o) {
            EXPECT(f(c, N, M, s, S, x.data(), 1, &ok, v, 0, out.data(), nullptr) == E && msg(c, "offsets"));
            EXPECT(f(c, N, M, s, S, x.data(), 1, &ok, 0, v, out.data(), nullptr) == E && msg(c, "offsets"));
        }
        p = ok; p.levels = 1;
        EXPECT(f(c, N, M, s, S, x.data(), 1, &p, 2, 0, out.data(), nullptr) == E && msg(c, "offsets"));
        if (!pass) {                                 // everything fine: refused for the missing context only
            EXPECT(f(c, N, M, s, S, x.data(), 1, &ok, 7, 7, out.data(), cm) == E && msg(c, "ctx"));
            EXPECT(f(c, N, M, s, S, x.data(), 0, &ok, 0, 0, out.data(), nullptr) == E && msg(c, "ctx"));
            p = ok; p.levels = 4; p.filter = QMRI_WAVELET_HAAR; p.joint = 0; p.shift = 9; p.tau = 0.0;      // (shift is ignored: the offsets are arguments)
            EXPECT(f(c, 16, 16, 16, 1, x.data(), 1, &p, 15, 15, out.data(), nullptr) == E && msg(c, "ctx"));
        }
    }
}

static void drive_set() {
    const int E = QMRI_ERR_INVALID_ARG;
    qmri_wavelet_params ok = {};
    ok.tau = 0.25; ok.levels = 2; ok.filter = QMRI_WAVELET_HAAR; ok.joint = 1; ok.shift = 1;
    qmri_llr_params llr = {};
    llr.tau = 0.5; llr.block = 4;
    for (int pass = 0; pass < 2; ++pass) {
        qmri_ctx ctx;
        qmri_ctx* c = pass ? &ctx : nullptr;
        qmri_wavelet_params p = ok;
        p.tau = -1.0; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "tau"));
        p = ok; p.tau = NAN; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "tau"));
        p = ok; p.levels = 5; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "levels must be"));
        p = ok; p.filter = 2; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "filter must be"));
        p = ok; p.joint = 2; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "joint"));
        p = ok; p.shift = 2; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "shift"));
        p = ok; p.shift = -1; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "shift"));
        p = ok; p.reserved[3] = 1; EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "reserved"));
        if (!pass) {
            EXPECT(qmri_set_wavelet(c, &ok) == E && msg(c, "ctx"));
            EXPECT(qmri_set_wavelet(c, nullptr) == E && msg(c, "ctx"));
        } else {                                     // the state a context keeps; a refused call changes nothing
            EXPECT(!ctx.wav.on);
            EXPECT(qmri_set_wavelet(c, &ok) == QMRI_OK && ctx.wav.on && ctx.wav.tau == 0.25 && ctx.wav.levels == 2 && ctx.wav.filter == QMRI_WAVELET_HAAR &&
                   ctx.wav.joint == 1 && ctx.wav.shift == 1);
            p = ok; p.levels = 7;
            EXPECT(qmri_set_wavelet(c, &p) == E && ctx.wav.on && ctx.wav.levels == 2);
            // one regulariser at a time: LLR is refused while the wavelet is set, names the call that clears it and changes nothing
            EXPECT(qmri_set_llr(c, &llr) == QMRI_ERR_STATE && msg(c, "qmri_set_wavelet(ctx, NULL)") && !ctx.llr.on && ctx.wav.on && ctx.wav.levels == 2);
            EXPECT(qmri_set_llr(c, nullptr) == QMRI_OK && ctx.wav.on);                       // clearing what is not set is fine
            p = ok; p.levels = 0; p.filter = QMRI_WAVELET_DB2; p.joint = 0; p.shift = 0;
            EXPECT(qmri_set_wavelet(c, &p) == QMRI_OK && ctx.wav.levels == 3 && ctx.wav.filter == QMRI_WAVELET_DB2 && ctx.wav.joint == 0 && ctx.wav.shift == 0);
            EXPECT(qmri_set_wavelet(c, nullptr) == QMRI_OK && !ctx.wav.on);
            // ... and the other way round
            EXPECT(qmri_set_llr(c, &llr) == QMRI_OK && ctx.llr.on);
            EXPECT(qmri_set_wavelet(c, &ok) == QMRI_ERR_STATE && msg(c, "qmri_set_llr(ctx, NULL)") && !ctx.wav.on && ctx.llr.on && ctx.llr.block == 4);
            p = ok; p.tau = -1.0;                                                            // an invalid argument is reported before the state
            EXPECT(qmri_set_wavelet(c, &p) == E && msg(c, "tau") && !ctx.wav.on);
            EXPECT(qmri_set_wavelet(c, nullptr) == QMRI_OK && ctx.llr.on);
            EXPECT(qmri_set_llr(c, nullptr) == QMRI_OK && !ctx.llr.on);
            EXPECT(qmri_set_wavelet(c, &ok) == QMRI_OK && ctx.wav.on);
            EXPECT(qmri_set_wavelet(c, nullptr) == QMRI_OK && !ctx.wav.on);
        }
    }
}

static void offsets_rule() {
    for (int L = 1; L <= wav::MAX_LEVELS; ++L) {
        const int P = 1 << L;
        std::set<std::pair<int, int>> seen;
        int p1 = -1, p2 = -1;
        for (int it = 0; it < P * P; ++it) {
            int o1 = -1, o2 = -1;
            wav::offsets(it, P, 1, &o1, &o2);
            EXPECT(o1 >= 0 && o1 < P && o2 >= 0 && o2 < P);
            const int q = it % (P * P);
            EXPECT(o1 == q % P && o2 == (q / P + q) % P);
            EXPECT(it == 0 || P < 4 || (o1 != p1 && o2 != p2));   // both coordinates move each iteration (P = 2 has too few offsets for that)
            seen.insert({o1, o2});
            p1 = o1; p2 = o2;
            int r1 = -1, r2 = -1;
            wav::offsets(it + 3 * P * P, P, 1, &r1, &r2);          // periodic
            EXPECT(r1 == o1 && r2 == o2);
            wav::offsets(it, P, 0, &r1, &r2);
            EXPECT(r1 == 0 && r2 == 0);
            int l1 = -1, l2 = -1;
            llr_offsets(it, P, 1, &l1, &l2);                       // section 25's rule with b = P
            EXPECT(l1 == o1 && l2 == o2);
        }
        EXPECT((int)seen.size() == P * P);
    }
}

int main() {
    drive(qmri_wavelet_prox);
    drive(qmri_wavelet_prox_dev);
    drive_set();
    offsets_rule();
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_WAV_OK\n");
    return 0;
}
