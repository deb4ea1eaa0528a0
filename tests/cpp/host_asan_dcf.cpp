// host_asan_dcf.cpp -- the refusals of the density-compensation entry points (api_dcf.cpp) under the host-only
// AddressSanitizer + UBSan build of libqmri (`make -C qmri_pnp_recon_poc_amd/csrc asan-host`), on a machine without a GPU.  Every refusal is decided
// before the device is touched, so a context in each state is made here by hand: no operator, a gridded operator, a trajectory operator without
// weights.  Run by tests/test_dcf_host.py::test_refusals_under_address_and_ub_sanitizer.
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
    double x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    qmri_dcf_params p{};
    qmri_dcf_info info{};
    // no context
    EXPECT(qmri_nufft_dcf(nullptr, &p, x, &info) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_set_sample_weights(nullptr, x) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_adjoint_w(nullptr, x, x) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_adjoint_w_dev(nullptr, x, x, 1) == QMRI_ERR_INVALID_ARG);
    EXPECT(qmri_adjoint_w_mc(nullptr, x, x) == QMRI_ERR_INVALID_ARG);
    {   // no operator
        qmri_ctx c;
        EXPECT(qmri_nufft_dcf(&c, &p, x, &info) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "operator not set"));
        EXPECT(qmri_set_sample_weights(&c, x) == QMRI_ERR_STATE);
        EXPECT(qmri_adjoint_w(&c, x, x) == QMRI_ERR_STATE);
        EXPECT(qmri_adjoint_w_dev(&c, x, x, 1) == QMRI_ERR_STATE);
        EXPECT(qmri_adjoint_w_mc(&c, x, x) == QMRI_ERR_STATE);
    }
    {   // a gridded operator
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_GRIDDED; c.op.N = c.op.M = 32; c.op.s = 1; c.op.T = 2; c.op.m = 4; c.op.maxB = 2;
        EXPECT(qmri_nufft_dcf(&c, &p, x, &info) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_set_operator_nufft"));
        EXPECT(qmri_set_sample_weights(&c, x) == QMRI_ERR_UNSUPPORTED);
        EXPECT(qmri_set_sample_weights(&c, nullptr) == QMRI_ERR_UNSUPPORTED);
        EXPECT(qmri_adjoint_w(&c, x, x) == QMRI_ERR_UNSUPPORTED && std::strstr(qmri_last_error(&c), "qmri_adjoint"));
        EXPECT(qmri_adjoint_w_dev(&c, x, x, 1) == QMRI_ERR_UNSUPPORTED);
        EXPECT(qmri_adjoint_w_mc(&c, x, x) == QMRI_ERR_UNSUPPORTED);
        c.op.ready = false;                      // (nothing was allocated: nothing for a destructor or qmri_free_operator to release)
    }
    {   // a trajectory operator without weights: the argument checks, then the missing weights
        qmri_ctx c;
        c.op.ready = true; c.op.kind = OP_NUFFT; c.op.N = c.op.M = 32; c.op.s = 1; c.op.T = 2; c.op.m = 4; c.op.maxB = 2;
        c.op.nu.w = 6; c.op.nu.beta = 13.8;
        qmri_dcf_params q{};
        q.niter = -1;
        EXPECT(qmri_nufft_dcf(&c, &q, x, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "niter"));
        q.niter = 201;
        EXPECT(qmri_nufft_dcf(&c, &q, x, &info) == QMRI_ERR_INVALID_ARG);
        q.niter = 5; q.tol = -1e-3;
        EXPECT(qmri_nufft_dcf(&c, &q, x, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "tol"));
        q.tol = NAN;
        EXPECT(qmri_nufft_dcf(&c, &q, x, &info) == QMRI_ERR_INVALID_ARG);
        q.tol = 0.0; q.reserved[5] = 1;
        EXPECT(qmri_nufft_dcf(&c, &q, x, &info) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "reserved"));
        double bad[4] = {1.0, 2.0, -0.5, 1.0};
        EXPECT(qmri_set_sample_weights(&c, bad) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "w[2]"));
        bad[2] = INFINITY;
        EXPECT(qmri_set_sample_weights(&c, bad) == QMRI_ERR_INVALID_ARG);
        bad[2] = NAN;
        EXPECT(qmri_set_sample_weights(&c, bad) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_adjoint_w(&c, nullptr, x) == QMRI_ERR_INVALID_ARG && qmri_adjoint_w(&c, x, nullptr) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_adjoint_w_dev(&c, nullptr, x, 1) == QMRI_ERR_INVALID_ARG && qmri_adjoint_w_dev(&c, x, nullptr, 1) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_adjoint_w_dev(&c, x, x, 0) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_adjoint_w_dev(&c, x, x, 3) == QMRI_ERR_INVALID_ARG && std::strstr(qmri_last_error(&c), "max_batch"));
        EXPECT(qmri_adjoint_w_mc(&c, nullptr, x) == QMRI_ERR_INVALID_ARG);
        EXPECT(qmri_adjoint_w(&c, x, x) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "no sample weights attached"));
        EXPECT(qmri_adjoint_w_dev(&c, x, x, 1) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "qmri_nufft_dcf"));
        EXPECT(qmri_adjoint_w_mc(&c, x, x) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "qmri_set_coils"));
        c.op.ncoil = 2;
        EXPECT(qmri_adjoint_w_mc(&c, x, x) == QMRI_ERR_STATE && std::strstr(qmri_last_error(&c), "no sample weights attached"));
        c.op.ncoil = 0;
        c.op.ready = false;
    }
    if (fails) { std::fprintf(stderr, "%d driver checks failed\n", fails); return 1; }
    std::printf("HOST_ASAN_DCF_OK\n");
    return 0;
}
