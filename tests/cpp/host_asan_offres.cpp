// host_asan_offres.cpp -- the refusals of qmri_set_field_map and of the Toeplitz calls while a field map is attached (api_offres.cpp, api_toep.cpp;
// DESIGN.md section 22) under the host-only AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine
// without a GPU.  Every refusal is decided before the device is touched, so a context in each state is made here by hand: no operator, a gridded
// operator, a trajectory operator, a trajectory operator that claims an attached map.  Run by
// tests/test_offres_host.py::test_refusals_under_address_and_ub_sanitizer.
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
    const int N = 16, m = 6;
    std::vector<double> f((size_t)N * N), t(m);
    for (size_t i = 0; i < f.size(); ++i) f[i] = 10.0 * std::sin(0.1 * (double)i);
    for (int i = 0; i < m; ++i) t[i] = 1e-3 * i;
    const std::vector<double> flat((size_t)N * N, 80.0);
    double x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    qmri_offres_params p{};
    qmri_offres_info info{};
    // no context
    EXPECT(qmri_set_field_map(nullptr, f.data(), t.data(), &p, &info) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_set_field_map(nullptr, nullptr, nullptr, nullptr, nullptr) == QMRI_ERR_INVALID_ARG);
    {   // no operator
        qmri_ctx c;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &p, &info) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "operator not set"));
        EXPECT(qmri_set_field_map(&c, nullptr, nullptr, nullptr, nullptr) == QMRI_ERR_STATE);
    }
    {   // a gridded operator
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_GRIDDED; c.op.N = c.op.M = N; c.op.s = 1; c.op.T = 2; c.op.m = m; c.op.maxB = 2;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &p, &info) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_set_operator_nufft"));
        EXPECT(qmri_set_field_map(&c, nullptr, nullptr, nullptr, nullptr) == QMRI_ERR_UNSUPPORTED);
        c.op.ready = false;                      // (nothing was allocated: nothing for a destructor or qmri_free_operator to release)
    }
    {   // a trajectory operator: the argument checks
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_NUFFT; c.op.N = c.op.M = N; c.op.s = 1; c.op.T = 2; c.op.m = m; c.op.maxB = 2;
        c.op.nu.w = 6; c.op.nu.beta = 13.8;
        EXPECT(qmri_set_field_map(&c, f.data(), nullptr, &p, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "t_s"));
        qmri_offres_params q{};
        q.nseg = -1;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "nseg"));
        q.nseg = 17;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG);
        q.nseg = 4; q.nbins = 15;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "nbins"));
        q.nbins = 1025;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG);
        q.nbins = -3;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG);
        q.nbins = 0; q.tol = -1e-3;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "tol"));
        q.tol = NAN;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG);
        q.tol = INFINITY;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG);
        q.tol = 0.0; q.reserved[3] = 1;
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "reserved"));
        q.reserved[3] = 0; q.nseg = 1;                                  // one segment cannot follow a varying field ...
        EXPECT(qmri_set_field_map(&c, f.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "constant"));
        q.nseg = 4;
        std::vector<double> bad = f;
        bad[37] = NAN;
        EXPECT(qmri_set_field_map(&c, bad.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "f_hz[37]"));
        bad[37] = INFINITY;
        EXPECT(qmri_set_field_map(&c, bad.data(), t.data(), &q, &info) == QMRI_ERR_INVALID_ARG);
        std::vector<double> badt = t;
        badt[m - 1] = NAN;
        EXPECT(qmri_set_field_map(&c, f.data(), badt.data(), &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "t_s[5]"));
        badt[m - 1] = -INFINITY;
        EXPECT(qmri_set_field_map(&c, flat.data(), badt.data(), &q, &info) == QMRI_ERR_INVALID_ARG);
        // without a map the Toeplitz calls are not refused for the map's sake (their own argument checks speak)
        EXPECT(qmri_normal(&c, nullptr, 1, x) == QMRI_ERR_INVALID_ARG);
        EXPECT(offres_refuse_toeplitz(&c, "x") == QMRI_OK && offres_refuse_toeplitz(nullptr, "x") == QMRI_OK);
        // ... and with one attached (claimed here: no table is read before the refusal) they are, naming LSQR
        c.op.nu.fm_set = true; c.op.nu.fm_L = 4;
        EXPECT(qmri_nufft_prepare_normal(&c) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "LSQR"));
        EXPECT(qmri_normal(&c, x, 1, x) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "LSQR"));
        EXPECT(qmri_normal_dev(&c, x, x, 1) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "field map"));
        EXPECT(qmri_xupdate(&c, x, x, 0.1, 1e-6, 5, QMRI_SOLVER_TOEPLITZ, x, nullptr, nullptr) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "LSQR"));
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_TOEPLITZ) == QMRI_ERR_UNSUPPORTED);
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_LSQR) == QMRI_OK);
        c.op.nu.fm_set = false; c.op.nu.fm_L = 0;
        c.op.ready = false;
    }
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_OFFRES_OK\n");
    return 0;
}
