// host_asan_offres_normal.cpp -- the refusals of qmri_nufft_prepare_normal_fm and the host side of its lifetime rules (api_offres.cpp, api_toep.cpp;
// DESIGN.md section 23) under the host-only AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine
// without a GPU.  Every refusal is decided before the device is touched, so a context in each state is made here by hand: no operator, a gridded
// operator, a trajectory operator without a map, one that claims a map, one that claims a map and its prepared normal operator.  Run by
// tests/test_offres_normal_host.py::test_refusals_under_address_and_ub_sanitizer.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

int main() {
    const int N = 16, m = 6;
    double x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    qmri_offres_normal_params p{};
    qmri_offres_normal_info info{};
    // no context
    EXPECT(qmri_nufft_prepare_normal_fm(nullptr, &p, &info) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_nufft_prepare_normal_fm(nullptr, nullptr, nullptr) == QMRI_ERR_INVALID_ARG);
    {   // no operator
        qmri_ctx c;
        EXPECT(qmri_nufft_prepare_normal_fm(&c, &p, &info) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "operator not set"));
        EXPECT(qmri_nufft_prepare_normal_fm(&c, nullptr, nullptr) == QMRI_ERR_STATE);
    }
    {   // a gridded operator
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_GRIDDED; c.op.N = c.op.M = N; c.op.s = 1; c.op.T = 2; c.op.m = m; c.op.maxB = 2;
        EXPECT(qmri_nufft_prepare_normal_fm(&c, &p, &info) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_set_operator_nufft"));
        c.op.ready = false;                      // (nothing was allocated: nothing for a destructor or qmri_free_operator to release)
    }
    {   // a trajectory operator
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_NUFFT; c.op.N = c.op.M = N; c.op.s = 1; c.op.T = 2; c.op.m = m; c.op.maxB = 2;
        c.op.nu.w = 6; c.op.nu.beta = 13.8;
        // without a map: QMRI_ERR_STATE, naming the call that attaches one and the plain call
        EXPECT(qmri_nufft_prepare_normal_fm(&c, &p, &info) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "qmri_set_field_map") &&
               std::strstr(qmri_last_error(&c), "by qmri_nufft_prepare_normal"));
        EXPECT(qmri_nufft_prepare_normal_fm(&c, nullptr, nullptr) == QMRI_ERR_STATE);
        // the argument checks come first, with or without a map
        for (int with_map = 0; with_map < 2; ++with_map) {
            c.op.nu.fm_set = with_map != 0; c.op.nu.fm_L = with_map ? 4 : 0;
            qmri_offres_normal_params q{};
            q.nseg = -1;
            EXPECT(qmri_nufft_prepare_normal_fm(&c, &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "nseg"));
            q.nseg = 1;
            EXPECT(qmri_nufft_prepare_normal_fm(&c, &q, &info) == QMRI_ERR_INVALID_ARG);
            q.nseg = 33;
            EXPECT(qmri_nufft_prepare_normal_fm(&c, &q, &info) == QMRI_ERR_INVALID_ARG);
            q.nseg = 8; q.tol = -1e-3;
            EXPECT(qmri_nufft_prepare_normal_fm(&c, &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "tol"));
            q.tol = NAN;
            EXPECT(qmri_nufft_prepare_normal_fm(&c, &q, &info) == QMRI_ERR_INVALID_ARG);
            q.tol = INFINITY;
            EXPECT(qmri_nufft_prepare_normal_fm(&c, &q, &info) == QMRI_ERR_INVALID_ARG);
            q.tol = 0.0; q.reserved[2] = 1;
            EXPECT(qmri_nufft_prepare_normal_fm(&c, &q, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "reserved"));
        }
        // a map attached (claimed: no table is read before the refusal) and no prepared normal operator: the Toeplitz calls refuse as before,
        // naming LSQR, the field map and now the new call
        EXPECT(qmri_nufft_prepare_normal(&c) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "LSQR"));
        EXPECT(qmri_normal(&c, x, 1, x) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_nufft_prepare_normal_fm"));
        EXPECT(qmri_normal_dev(&c, x, x, 1) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "field map"));
        EXPECT(qmri_xupdate(&c, x, x, 0.1, 1e-6, 5, QMRI_SOLVER_TOEPLITZ, x, nullptr, nullptr) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "LSQR"));
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_TOEPLITZ) == QMRI_ERR_UNSUPPORTED);
        // ... with it prepared (claimed) they are not refused for the map's sake
        c.op.nu.fmn_ready = true; c.op.nu.fmn_L = 8;
        EXPECT(offres_refuse_toeplitz(&c, "x") == QMRI_OK);
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_TOEPLITZ) == QMRI_OK);
        EXPECT(qmri_normal(&c, nullptr, 1, x) == QMRI_ERR_INVALID_ARG);             // (their own argument checks speak)
        EXPECT(qmri_normal_dev(&c, x, x, 3) == QMRI_ERR_INVALID_ARG);
        // dropping it (what qmri_set_field_map and replacing the operator do) brings the refusal back; the plain transform's state is not touched
        c.op.nu.khat_ready = true;
        offres_drop_normal(c.op.nu);
        EXPECT(!c.op.nu.fmn_ready && !c.op.nu.fmn_plain && c.op.nu.fmn_L == 0 && c.op.nu.khat_ready);
        EXPECT(offres_refuse_toeplitz(&c, "x") == QMRI_ERR_UNSUPPORTED);
        // a transform that outlived its map (cleared) is not consulted: without a map nothing is refused
        c.op.nu.fm_set = false; c.op.nu.fm_L = 0;
        EXPECT(offres_refuse_toeplitz(&c, "x") == QMRI_OK);
        c.op.nu.khat_ready = false;
        c.op.ready = false;
    }
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_OFFRES_NORMAL_OK\n");
    return 0;
}
