// api_dsvd.cpp -- C ABI of the dictionary compression (include/qmri.h; kernels: dsvd_kernels.hip).  An EXTENSION with no reference counterpart.
// Every refusal is decided here, on the host, before the device is selected; with ctx == NULL the message of the first failing check is left in
// qmri_last_error(NULL), so the argument rules can be exercised on a machine without a GPU.
//
// The eigenpairs: block subspace iteration with Rayleigh-Ritz on G (T x T, on the device), block b = min(T, s_cap + 8).  Per iteration the device
// forms Z = G Q (k_dsvd_gq: the one pass over G) and the host does what is O(T b^2), b <= 24, in fixed loops:
//     A = Q^T Z (symmetrised),  A = W diag(theta) W^T (cyclic Jacobi, theta descending),  X = Q W,  R = Z W - X diag(theta),
//     stop when max_{c < s_cap} |R_c|_2 <= tol theta_1, else Q <- orth(Z W) (modified Gram-Schmidt, two passes per column).
// Nothing on the host grows faster than T b^2 per iteration (2.4 Mflop at T = 1024, b = 24).  A column that vanishes in the Gram-Schmidt (rank of
// G below b) is replaced by the first unit vector that keeps at least half its expected length after orthogonalisation.  The start block is a
// fixed SplitMix64 sequence: equal inputs give equal bits.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>
#include "qmri_internal.h"

namespace {
constexpr int DSVD_MAX_T = 1024, DSVD_MAX_S = 16, DSVD_GUARD = 8;

// QMRI_OK, or the code of the first failing check with its message set on ctx (ctx may be NULL)
int dsvd_checks(qmri_ctx* ctx, int K, int T, const void* F, int f_is_f64, const qmri_dsvd_params* p, const int* s_out, const void* V_out,
                const void* D_out, const void* normD_out) {
    QMRI_CHECK_ARG(ctx, p, "dictionary compression params must not be NULL");
    QMRI_CHECK_ARG(ctx, F && s_out && V_out && D_out && normD_out, "F / s_out / V_out / D_out / normD_out must not be NULL");
    QMRI_CHECK_ARG(ctx, K >= 1 && K <= (1 << 30), "K must satisfy 1 <= K <= 2^30");
    QMRI_CHECK_ARG(ctx, T >= 1 && T <= DSVD_MAX_T, "T must satisfy 1 <= T <= 1024");
    QMRI_CHECK_ARG(ctx, f_is_f64 == 0 || f_is_f64 == 1, "f_is_f64 must be 0 or 1");
    QMRI_CHECK_ARG(ctx, p->s >= 0 && p->s <= DSVD_MAX_S, "s must satisfy 0 <= s <= 16");
    if (p->s == 0) {
        QMRI_CHECK_ARG(ctx, p->s_max >= 1 && p->s_max <= DSVD_MAX_S, "s_max must satisfy 1 <= s_max <= 16 when s == 0");
        QMRI_CHECK_ARG(ctx, p->energy > 0.0 && p->energy <= 1.0, "energy must be in (0, 1] when s == 0");
    } else {
        QMRI_CHECK_ARG(ctx, p->s <= std::min(T, K), "s must not exceed min(T, K)");
    }
    QMRI_CHECK_ARG(ctx, std::isfinite(p->tol) && p->tol >= 0.0 && p->tol < 1.0, "tol must be in [0, 1)");
    QMRI_CHECK_ARG(ctx, p->maxit >= 0, "maxit must be >= 0");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    return QMRI_OK;
}

// cyclic Jacobi on the real symmetric n x n matrix a (column-major, destroyed): eigenvalues descending in lam, vectors in the columns of W
bool jacobi_sym(int n, std::vector<double>& a, std::vector<double>& lam, std::vector<double>& W) {
    std::vector<double> v((size_t)n * n, 0.0);
    auto A = [&](int i, int j) -> double& { return a[i + (size_t)j * n]; };
    auto Vv = [&](int i, int j) -> double& { return v[i + (size_t)j * n]; };
    for (int j = 0; j < n; ++j) Vv(j, j) = 1.0;
    double fro = 0.0;
    for (double z : a) fro += z * z;
    fro = std::sqrt(fro);
    if (!std::isfinite(fro)) return false;
    bool done = false;
    for (int sweep = 0; sweep <= 100 && !done; ++sweep) {
        double off = 0.0;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) if (i != j) off += A(i, j) * A(i, j);
        off = std::sqrt(off);
        if (off == 0.0 || off <= DBL_EPSILON * fro) { done = true; break; }
        if (sweep == 100) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A(p, q);
                if (apq == 0.0) continue;
                const double tau = (A(q, q) - A(p, p)) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::abs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < n; ++k) { const double xp = A(k, p), xq = A(k, q); A(k, p) = c * xp - s * xq; A(k, q) = s * xp + c * xq; }
                for (int k = 0; k < n; ++k) { const double xp = A(p, k), xq = A(q, k); A(p, k) = c * xp - s * xq; A(q, k) = s * xp + c * xq; }
                A(p, q) = A(q, p) = 0.0;
                for (int k = 0; k < n; ++k) { const double xp = Vv(k, p), xq = Vv(k, q); Vv(k, p) = c * xp - s * xq; Vv(k, q) = s * xp + c * xq; }
            }
    }
    if (!done) return false;
    std::vector<int> ord(n);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return A(x, x) > A(y, y); });
    lam.resize(n);
    W.assign((size_t)n * n, 0.0);
    for (int l = 0; l < n; ++l) {
        lam[l] = A(ord[l], ord[l]);
        for (int k = 0; k < n; ++k) W[k + (size_t)l * n] = Vv(k, ord[l]);
    }
    return true;
}

// modified Gram-Schmidt on the b columns of Q (T x b, column-major), two passes per column; a vanishing column is replaced by a unit vector
void orthonormalise(int T, int b, std::vector<double>& Q) {
    auto col = [&](int c) { return Q.data() + (size_t)c * T; };
    auto project_out = [&](int c) {
        for (int pass = 0; pass < 2; ++pass)
            for (int p = 0; p < c; ++p) {
                double r = 0.0;
                for (int i = 0; i < T; ++i) r += col(p)[i] * col(c)[i];
                for (int i = 0; i < T; ++i) col(c)[i] -= r * col(p)[i];
            }
        double n2 = 0.0;
        for (int i = 0; i < T; ++i) n2 += col(c)[i] * col(c)[i];
        return std::sqrt(n2);
    };
    for (int c = 0; c < b; ++c) {
        double n0 = 0.0;
        for (int i = 0; i < T; ++i) n0 += col(c)[i] * col(c)[i];
        n0 = std::sqrt(n0);
        double nrm = project_out(c);
        if (!(nrm > 1e-12 * n0) || !std::isfinite(nrm)) {
            // mean over u of |(I - P) e_u|^2 is (T - c) / T, so some unit vector keeps at least that much: take the first that keeps half of it
            const double need = std::sqrt(0.5 * (T - c) / T);
            for (int u = 0; u < T; ++u) {
                std::fill(col(c), col(c) + T, 0.0);
                col(c)[u] = 1.0;
                nrm = project_out(c);
                if (nrm >= need) break;
            }
        }
        for (int i = 0; i < T; ++i) col(c)[i] /= nrm;
    }
}

double start_value(uint64_t idx) {                      // SplitMix64 of the counter, mapped to [-1, 1)
    uint64_t z = (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// C (T x n) = A (T x b) B (b x n), column-major, the b terms added in ascending order
void mul_tall(int T, int b, int n, const std::vector<double>& A, const std::vector<double>& B, int ldb, std::vector<double>& Cm) {
    Cm.assign((size_t)T * n, 0.0);
    for (int c = 0; c < n; ++c)
        for (int p = 0; p < b; ++p) {
            const double w = B[p + (size_t)c * ldb];
            const double* a = A.data() + (size_t)p * T;
            double* o = Cm.data() + (size_t)c * T;
            for (int i = 0; i < T; ++i) o[i] += w * a[i];
        }
}

// the dominant eigenpairs of d_G: X (T x b) Ritz vectors, theta (b) Ritz values, descending
int dsvd_eig(qmri_ctx* ctx, int T, int b, int s_cap, const double* d_G, double tol, int maxit, std::vector<double>& X, std::vector<double>& theta,
             qmri_dsvd_info* info) {
    DevBuf<double> dQ, dZ;
    QMRI_TRY(dQ.ensure(ctx, (size_t)T * b));
    QMRI_TRY(dZ.ensure(ctx, (size_t)T * b));
    std::vector<double> Q((size_t)T * b), Z((size_t)T * b), A((size_t)b * b), W, ZW;
    for (size_t e = 0; e < Q.size(); ++e) Q[e] = start_value(e);
    orthonormalise(T, b, Q);
    info->iters = 0; info->converged = 0; info->max_resid = 0.0;
    for (int it = 1; it <= maxit; ++it) {
        QMRI_HIP(ctx, hipMemcpyAsync(dQ.p, Q.data(), Q.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QMRI_TRY(dsvd_gq_dev(ctx, T, b, d_G, dQ, dZ));
        QMRI_HIP(ctx, hipMemcpyAsync(Z.data(), dZ.p, Z.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int c = 0; c < b; ++c)
            for (int r = 0; r <= c; ++r) {
                double u = 0.0, l = 0.0;                 // (Q^T Z)[r, c] and [c, r]: equal up to rounding, averaged
                const double *qr = Q.data() + (size_t)r * T, *qc = Q.data() + (size_t)c * T, *zr = Z.data() + (size_t)r * T, *zc = Z.data() + (size_t)c * T;
                for (int i = 0; i < T; ++i) { u += qr[i] * zc[i]; l += qc[i] * zr[i]; }
                A[r + (size_t)c * b] = A[c + (size_t)r * b] = 0.5 * (u + l);
            }
        if (!jacobi_sym(b, A, theta, W)) {
            qmri_set_error(ctx, "invalid argument: the Rayleigh-Ritz eigensolve of the dictionary compression did not converge (non-finite data?)");
            return QMRI_ERR_INVALID_ARG;
        }
        mul_tall(T, b, b, Q, W, b, X);
        mul_tall(T, b, b, Z, W, b, ZW);
        double worst = 0.0;
        for (int c = 0; c < s_cap; ++c) {
            double n2 = 0.0;
            for (int i = 0; i < T; ++i) { const double r = ZW[i + (size_t)c * T] - theta[c] * X[i + (size_t)c * T]; n2 += r * r; }
            worst = std::max(worst, std::sqrt(n2));
        }
        info->iters = it;
        info->max_resid = theta[0] > 0.0 ? worst / theta[0] : 0.0;
        if (!(theta[0] > 0.0) || worst <= tol * theta[0]) { info->converged = 1; break; }
        if (it == maxit) break;
        Q.swap(ZW);
        orthonormalise(T, b, Q);
    }
    return QMRI_OK;
}

// everything after the argument checks, on device arrays; the stream is idle on return
int dsvd_compress_dev(qmri_ctx* ctx, int K, int T, const void* d_F, bool f64, const qmri_dsvd_params& p, int* s_out, double* d_V, float* d_D,
                      float* d_normD, double* eig_out, qmri_dsvd_info* info_out) {
    qmri_dsvd_info info{};
    const int lim = std::min(T, K), s_cap = p.s > 0 ? p.s : std::min(p.s_max, lim), b = std::min(T, s_cap + DSVD_GUARD);
    const double tol = p.tol > 0.0 ? p.tol : 1e-13;
    const int maxit = p.maxit > 0 ? p.maxit : 200;
    DevBuf<double> part, G, diag;
    QMRI_TRY(part.ensure(ctx, dsvd_gram_scratch(K, T)));
    QMRI_TRY(G.ensure(ctx, (size_t)T * T));
    QMRI_TRY(diag.ensure(ctx, (size_t)T));
    QMRI_TRY(dsvd_gram_dev(ctx, K, T, d_F, f64, part, G, diag));
    std::vector<double> dg(T);
    QMRI_HIP(ctx, hipMemcpyAsync(dg.data(), diag.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double trace = 0.0;
    for (double v : dg) trace += v;
    if (!std::isfinite(trace)) {
        qmri_set_error(ctx, "invalid argument: the trace of F^T F is not finite (F holds a NaN or an Inf, or overflows fp64)");
        return QMRI_ERR_INVALID_ARG;
    }
    std::vector<double> X, theta;
    QMRI_TRY(dsvd_eig(ctx, T, b, s_cap, G, tol, maxit, X, theta, &info));
    int s = s_cap;
    info.energy_reached = 1;
    if (p.s == 0) {
        const double want = p.energy * trace;
        double acc = 0.0;
        s = 0;
        for (int c = 0; c < s_cap && s == 0; ++c) { acc += theta[c]; if (acc >= want) s = c + 1; }
        if (s == 0) { s = s_cap; info.energy_reached = 0; }
    }
    double kept = 0.0;
    for (int c = 0; c < s; ++c) kept += theta[c];
    info.s = s;
    info.energy_kept = trace > 0.0 ? kept / trace : 1.0;
    for (int c = 0; c < s; ++c) {                        // sign rule: the entry of largest magnitude (lowest index on ties) is positive
        double* v = X.data() + (size_t)c * T;
        int jm = 0;
        for (int i = 1; i < T; ++i) if (std::abs(v[i]) > std::abs(v[jm])) jm = i;
        if (v[jm] < 0.0) for (int i = 0; i < T; ++i) v[i] = -v[i];
    }
    QMRI_HIP(ctx, hipMemcpyAsync(d_V, X.data(), (size_t)T * s * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(dsvd_project_dev(ctx, K, T, s, d_F, f64, d_V, d_D, d_normD));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *s_out = s;
    if (eig_out) std::copy(theta.begin(), theta.begin() + s, eig_out);
    if (info_out) *info_out = info;
    return QMRI_OK;
}
}  // namespace

extern "C" int qmri_dict_compress_dev(qmri_ctx* ctx, int K, int T, const void* d_F, int f_is_f64, const qmri_dsvd_params* p, int* s_out, double* d_V_out,
                                      float* d_D_out, float* d_normD_out, double* eig_out, qmri_dsvd_info* info) {
    QMRI_TRY(dsvd_checks(ctx, K, T, d_F, f_is_f64, p, s_out, d_V_out, d_D_out, d_normD_out));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    return dsvd_compress_dev(ctx, K, T, d_F, f_is_f64 != 0, *p, s_out, d_V_out, d_D_out, d_normD_out, eig_out, info);
}

extern "C" int qmri_dict_compress(qmri_ctx* ctx, int K, int T, const void* F, int f_is_f64, const qmri_dsvd_params* p, int* s_out, double* V_out,
                                  float* D_out, float* normD_out, double* eig_out, qmri_dsvd_info* info) {
    QMRI_TRY(dsvd_checks(ctx, K, T, F, f_is_f64, p, s_out, V_out, D_out, normD_out));
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nF = (size_t)K * T * (f_is_f64 ? sizeof(double) : sizeof(float));
    DevBuf<unsigned char> dF;
    DevBuf<double> dV;
    DevBuf<float> dD, dn;
    QMRI_TRY(dF.ensure(ctx, nF));
    QMRI_TRY(dV.ensure(ctx, (size_t)T * DSVD_MAX_S));
    QMRI_TRY(dD.ensure(ctx, (size_t)K * DSVD_MAX_S));
    QMRI_TRY(dn.ensure(ctx, (size_t)K));
    QMRI_HIP(ctx, hipMemcpyAsync(dF.p, F, nF, hipMemcpyHostToDevice, ctx->stream));
    QMRI_TRY(dsvd_compress_dev(ctx, K, T, dF.p, f_is_f64 != 0, *p, s_out, dV, dD, dn, eig_out, info));
    const int s = *s_out;
    QMRI_HIP(ctx, hipMemcpyAsync(V_out, dV.p, (size_t)T * s * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(D_out, dD.p, (size_t)K * s * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipMemcpyAsync(normD_out, dn.p, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

extern "C" int qmri_debug_dsvd_gram(qmri_ctx* ctx, int K, int T, const void* F, int f_is_f64, int on_device, double* G_out) {
    QMRI_CHECK_ARG(ctx, F && G_out, "F / G_out must not be NULL");
    QMRI_CHECK_ARG(ctx, K >= 1 && K <= (1 << 30), "K must satisfy 1 <= K <= 2^30");
    QMRI_CHECK_ARG(ctx, T >= 1 && T <= DSVD_MAX_T, "T must satisfy 1 <= T <= 1024");
    QMRI_CHECK_ARG(ctx, (f_is_f64 == 0 || f_is_f64 == 1) && (on_device == 0 || on_device == 1), "f_is_f64 and on_device must be 0 or 1");
    if (!ctx) { qmri_set_error(nullptr, "invalid argument: ctx must not be NULL"); return QMRI_ERR_INVALID_ARG; }
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nF = (size_t)K * T * (f_is_f64 ? sizeof(double) : sizeof(float));
    DevBuf<unsigned char> dF;
    DevBuf<double> part, G, diag;
    QMRI_TRY(part.ensure(ctx, dsvd_gram_scratch(K, T)));
    QMRI_TRY(diag.ensure(ctx, (size_t)T));
    if (!on_device) {
        QMRI_TRY(dF.ensure(ctx, nF));
        QMRI_TRY(G.ensure(ctx, (size_t)T * T));
        QMRI_HIP(ctx, hipMemcpyAsync(dF.p, F, nF, hipMemcpyHostToDevice, ctx->stream));
    }
    QMRI_TRY(dsvd_gram_dev(ctx, K, T, on_device ? F : dF.p, f_is_f64 != 0, part, on_device ? G_out : G.p, diag));
    if (!on_device) QMRI_HIP(ctx, hipMemcpyAsync(G_out, G.p, (size_t)T * T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}
