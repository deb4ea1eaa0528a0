// host_asan_toeplitz.cpp -- the refusals of the Toeplitz normal operator's entry points (api_toep.cpp) under the host-only
// AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided
// before the device is touched, so a context in each state is made here by hand: no operator, a gridded operator, a trajectory operator.
// Run by tests/test_toeplitz_host.py::test_refusals_under_address_and_ub_sanitizer.
#include <cstdio>
#include <cstring>

#include "qmri_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "driver check failed, line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

int main() {
    double x[4] = {0, 0, 0, 0};
    // no context
    EXPECT(qmri_nufft_prepare_normal(nullptr) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_normal(nullptr, x, 1, x) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_normal_dev(nullptr, x, x, 1) == QMRI_ERR_INVALID_ARG);
    {   // no operator
        qmri_ctx c;
        EXPECT(qmri_nufft_prepare_normal(&c) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "operator not set"));
        EXPECT(qmri_normal(&c, x, 1, x) == QMRI_ERR_STATE);
        EXPECT(qmri_normal_dev(&c, x, x, 1) == QMRI_ERR_STATE);
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_TOEPLITZ) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "operator not set"));
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_LSQR) == QMRI_OK && toep_check_solver(&c, QMRI_SOLVER_DIRECT) == QMRI_OK && toep_check_solver(&c, 7) == QMRI_OK);
    }
    {   // a gridded operator
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_GRIDDED; c.op.N = c.op.M = 32; c.op.s = 1; c.op.maxB = 2;
        EXPECT(qmri_nufft_prepare_normal(&c) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_set_operator_nufft"));
        EXPECT(qmri_normal(&c, x, 1, x) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_adjoint(qmri_forward(x))"));
        EXPECT(qmri_normal_dev(&c, x, x, 1) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_adjoint_dev(qmri_forward_dev(x))"));
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_TOEPLITZ) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "QMRI_SOLVER_LSQR"));
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_LSQR) == QMRI_OK);
        c.op.ready = false;                      // (nothing was allocated: nothing for a destructor or qmri_free_operator to release)
    }
    {   // a trajectory operator: the argument checks
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_NUFFT; c.op.N = c.op.M = 32; c.op.s = 1; c.op.maxB = 2;
        EXPECT(qmri_normal(&c, nullptr, 1, x) == QMRI_ERR_INVALID_ARG && qmri_normal(&c, x, 1, nullptr) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_normal_dev(&c, nullptr, x, 1) == QMRI_ERR_INVALID_ARG && qmri_normal_dev(&c, x, nullptr, 1) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_normal_dev(&c, x, x, 0) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_normal_dev(&c, x, x, 3) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "max_batch"));
        EXPECT(toep_check_solver(&c, QMRI_SOLVER_TOEPLITZ) == QMRI_OK);
        c.op.ready = false;
    }
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_TOEPLITZ_OK\n");
    return 0;
}
