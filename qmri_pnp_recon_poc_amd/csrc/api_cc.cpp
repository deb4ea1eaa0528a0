// api_cc.cpp -- C ABI of the coil compression (include/qmri.h; kernels: cc_kernels.hip).  A multi-coil EXTENSION with no reference counterpart.
//
// The one step on the host is the eigen-decomposition of the ncoil x ncoil matrix K (ncoil <= 128): a cyclic Jacobi method for Hermitian
// matrices, no LAPACK.  Sweep order: pairs (p, q), p < q, row by row (p ascending, then q ascending).  Each rotation J = D G zeroes a_pq exactly:
// D = diag(1, .., e^{-i phi} at q, ..) makes a_pq = |a_pq| e^{i phi} real, G is the real Jacobi rotation of that 2 x 2 (Golub & Van Loan, sym.schur2).
// Stop rule: after a sweep, off(A) = sqrt(sum_{p != q} |a_pq|^2) <= DBL_EPSILON * ||A||_F (or off = 0); more than 100 sweeps is an error (not
// seen: convergence is quadratic, 6-12 sweeps at n = 128).  Then lambda is sorted descending (a stable sort: equal values keep their order) and
// every column gets the phase rule of qmri.h.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <complex>
#include <numeric>
#include <string>
#include <vector>
#include "qmri_internal.h"

namespace {
using cd = std::complex<double>;
constexpr int CC_MAX_COILS = 128;

bool jacobi(int n, const double2* A, double* lam, double2* U) {
    std::vector<cd> a((size_t)n * n), v((size_t)n * n, cd(0.0, 0.0));
    auto at = [&](std::vector<cd>& x, int i, int j) -> cd& { return x[i + (size_t)j * n]; };
    for (int j = 0; j < n; ++j) {
        for (int i = 0; i < j; ++i) {
            at(a, i, j) = cd(A[i + (size_t)j * n].x, A[i + (size_t)j * n].y);
            at(a, j, i) = std::conj(at(a, i, j));
        }
        at(a, j, j) = cd(A[j + (size_t)j * n].x, 0.0);
        at(v, j, j) = 1.0;
    }
    double fro = 0.0;
    for (const cd& z : a) fro += std::norm(z);
    fro = std::sqrt(fro);
    bool done = false;
    for (int sweep = 0; sweep <= 100 && !done; ++sweep) {
        double off = 0.0;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) if (i != j) off += std::norm(at(a, i, j));
        off = std::sqrt(off);
        if (off == 0.0 || off <= DBL_EPSILON * fro) { done = true; break; }
        if (sweep == 100) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const cd apq = at(a, p, q);
                const double r = std::abs(apq);
                if (r == 0.0) continue;
                const cd e = apq / r;                                          // e^{i phi}
                const double app = at(a, p, p).real(), aqq = at(a, q, q).real();
                const double tau = (aqq - app) / (2.0 * r);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::abs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                // J: J_pp = c, J_pq = s, J_qp = -s conj(e), J_qq = c conj(e);  A <- J^H A J,  V <- V J
                const cd jqp = -s * std::conj(e), jqq = c * std::conj(e);
                for (int k = 0; k < n; ++k) {                                    // columns: A J
                    const cd xp = at(a, k, p), xq = at(a, k, q);
                    at(a, k, p) = c * xp + jqp * xq;
                    at(a, k, q) = s * xp + jqq * xq;
                }
                for (int k = 0; k < n; ++k) {                                    // rows: J^H (A J)
                    const cd xp = at(a, p, k), xq = at(a, q, k);
                    at(a, p, k) = c * xp + std::conj(jqp) * xq;
                    at(a, q, k) = s * xp + std::conj(jqq) * xq;
                }
                at(a, p, q) = at(a, q, p) = 0.0;
                at(a, p, p) = at(a, p, p).real();
                at(a, q, q) = at(a, q, q).real();
                for (int k = 0; k < n; ++k) {
                    const cd xp = at(v, k, p), xq = at(v, k, q);
                    at(v, k, p) = c * xp + jqp * xq;
                    at(v, k, q) = s * xp + jqq * xq;
                }
            }
    }
    if (!done) return false;
    std::vector<int> ord(n);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return at(a, x, x).real() > at(a, y, y).real(); });
    for (int l = 0; l < n; ++l) {
        const int src = ord[l];
        lam[l] = at(a, src, src).real();
        int kmax = 0;
        double best = -1.0;
        for (int k = 0; k < n; ++k) { const double m2 = std::norm(at(v, k, src)); if (m2 > best) { best = m2; kmax = k; } }
        const cd big = at(v, kmax, src);
        const double mag = std::abs(big);
        const cd ph = mag > 0.0 ? std::conj(big) / mag : cd(1.0, 0.0);
        for (int k = 0; k < n; ++k) {
            cd z = at(v, k, src) * ph;
            if (k == kmax) z = cd(mag, 0.0);
            U[k + (size_t)l * n] = make_double2(z.real(), z.imag());
        }
    }
    return true;
}

// the argument rules shared by every entry point; batch: qmri_recon_batch_mc_cc's (fixed nv, one W per slice).  nullptr = fine.
const char* cc_param_error(int ncoil, const qmri_cc_params* p, bool batch, int* code) {
    *code = QMRI_ERR_INVALID_ARG;
    if (!p) return "coil compression params must not be NULL";
    if (ncoil < 1) return "ncoil >= 1";
    if (ncoil > CC_MAX_COILS) { *code = QMRI_ERR_UNSUPPORTED; return "the coil compression takes at most 128 coils (ncoil > 128)"; }
    if (p->nv < 0 || p->nv > ncoil) return "nv must satisfy 0 <= nv <= ncoil";
    if (p->shared != 0 && p->shared != 1) return "shared must be 0 or 1";
    if (batch && (p->nv == 0 || p->shared))
        return "qmri_recon_batch_mc_cc takes a fixed nv > 0 and one W per slice (energy and shared are refused: the stack is split over workers and "
               "launches); choose nv by energy or share W with qmri_coil_compress";
    if (p->nv == 0 && !(p->energy > 0.0 && p->energy <= 1.0)) return "energy must be in (0, 1] when nv == 0";
    return nullptr;
}

int cc_common_checks(qmri_ctx* ctx, int nslices, int ncoil, const void* y, const void* maps, const qmri_cc_params* p, int* nv_out, void* y_out,
                     void* maps_out) {
    if (!ctx->op.ready) { qmri_set_error(ctx, "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; }
    int code;
    if (const char* e = cc_param_error(ncoil, p, false, &code)) { qmri_set_error(ctx, "invalid argument: %s", e); return code; }
    QMRI_CHECK_ARG(ctx, nslices >= 1, "nslices >= 1");
    QMRI_CHECK_ARG(ctx, y && y_out && nv_out, "y_mc / y_out / nv_out must not be NULL");
    QMRI_CHECK_ARG(ctx, (maps == nullptr) == (maps_out == nullptr), "maps_out must be given exactly when maps is");
    QMRI_CHECK_ARG(ctx, y_out != y && (!maps || maps_out != maps), "the outputs must not alias the inputs");
    return QMRI_OK;
}
}  // namespace

int cc_eig_host(qmri_ctx* ctx, int n, const double2* A, double* lam, double2* U) {
    if (!jacobi(n, A, lam, U)) {
        qmri_set_error(ctx, "the Jacobi eigensolver of the coil compression did not converge in 100 sweeps (non-finite data?)");
        return QMRI_ERR_INVALID_ARG;
    }
    return QMRI_OK;
}

int cc_choose_nv(int n, const double* lam, double energy) {
    double tot = 0.0;
    for (int l = 0; l < n; ++l) tot += lam[l];
    const double want = energy * tot;
    double acc = 0.0;
    for (int l = 0; l < n; ++l) {
        acc += lam[l];
        if (acc >= want) return l + 1;
    }
    return n;
}

int cc_batch_param_error(int ncoil, const qmri_cc_params* p, std::string* msg) {
    int code = QMRI_OK;
    if (const char* e = cc_param_error(ncoil, p, true, &code)) { *msg = e; return code; }
    return QMRI_OK;
}

extern "C" int qmri_coil_eig(int n, const void* herm, double* evals, void* evecs) {
    if (n < 1 || n > CC_MAX_COILS || !herm || !evals || !evecs) {
        qmri_set_error(nullptr, "invalid argument: 1 <= n <= 128, herm / evals / evecs must not be NULL");
        return QMRI_ERR_INVALID_ARG;
    }
    return cc_eig_host(nullptr, n, (const double2*)herm, evals, (double2*)evecs);
}

extern "C" int qmri_coil_compress_dev(qmri_ctx* ctx, int nslices, int ncoil, const void* d_y_mc, const void* d_maps, const void* d_noise_cov,
                                      const qmri_cc_params* p, int* nv_out, void* d_y_out, void* d_maps_out, void* d_W_out, double* eig_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(cc_common_checks(ctx, nslices, ncoil, d_y_mc, d_maps, p, nv_out, d_y_out, d_maps_out));
    QMRI_TRY(cc_compress_dev(ctx, nslices, ncoil, (const double2*)d_y_mc, (const double2*)d_maps, (const double2*)d_noise_cov, *p, nv_out,
                             (double2*)d_y_out, (double2*)d_maps_out, (double2*)d_W_out, eig_out));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_coil_compress(qmri_ctx* ctx, int nslices, int ncoil, const void* y_mc, const void* maps, const void* noise_cov, const qmri_cc_params* p,
                                  int* nv_out, void* y_out, void* maps_out, void* W_out, double* eig_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_TRY(cc_common_checks(ctx, nslices, ncoil, y_mc, maps, p, nv_out, y_out, maps_out));
    const OpHost& o = ctx->op;
    CcWork& w = ctx->cc;
    const size_t ny = (size_t)nslices * ncoil * o.m, nm = maps ? (size_t)nslices * ncoil * o.N * o.M : 0;
    QMRI_TRY(cc_ensure_staging(ctx, ny, nm, ny, nm));
    QMRI_HIP(ctx, hipMemcpyAsync(w.sy, y_mc, ny * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    if (maps) QMRI_HIP(ctx, hipMemcpyAsync(w.sm, maps, nm * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    if (noise_cov) {
        const size_t nn = (size_t)ncoil * ncoil;
        QMRI_TRY(w.psi.ensure(ctx, nn));
        QMRI_HIP(ctx, hipMemcpyAsync(w.psi, noise_cov, nn * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    }
    QMRI_TRY(cc_compress_dev(ctx, nslices, ncoil, w.sy, maps ? w.sm : nullptr, noise_cov ? w.psi : nullptr, *p, nv_out, w.oy, maps ? w.om : nullptr,
                             nullptr, eig_out));
    const int nv = *nv_out, nmat = p->shared ? 1 : nslices;
    QMRI_HIP(ctx, hipMemcpyAsync(y_out, w.oy, (size_t)nslices * nv * o.m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    if (maps) QMRI_HIP(ctx, hipMemcpyAsync(maps_out, w.om, (size_t)nslices * nv * o.N * o.M * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    if (W_out) QMRI_HIP(ctx, hipMemcpyAsync(W_out, noise_cov ? w.W : w.U, (size_t)nmat * ncoil * nv * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
