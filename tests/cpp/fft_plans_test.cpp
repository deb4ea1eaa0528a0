// Host check of the codelets and plans behind the operator's grid sizes (csrc/fft_codelets.h): the radix-3/5/6/10/12 codelets and
// the two-step (R1 x R2) index map of every side in QFFT_PLANS, forward and inverse (conj-FFT-conj), against a naive DFT.
// Built and run by tests/test_fft_plans.py with g++ (no GPU needed).
#include "fft_codelets.h"
#include <cmath>
#include <cstdio>
#include <vector>

using namespace qfft;

// max |X - DFT(x)| / max |DFT(x)|, sign -1 (forward) or +1 (inverse, unnormalised)
static double naive_err(const std::vector<cd>& x, const std::vector<cd>& X, int sign) {
    const int n = (int)x.size();
    double err = 0, ref = 0;
    for (int k = 0; k < n; ++k) {
        double re = 0, im = 0;
        for (int j = 0; j < n; ++j) {
            const double a = sign * 2.0 * M_PI * (double)((long)j * k % n) / n;
            re += x[j].x * cos(a) - x[j].y * sin(a);
            im += x[j].x * sin(a) + x[j].y * cos(a);
        }
        err = fmax(err, hypot(re - X[k].x, im - X[k].y));
        ref = fmax(ref, hypot(re, im));
    }
    return err / ref;
}

template <int R> static double test_codelet() {
    std::vector<cd> x(R), X(R);
    for (int i = 0; i < R; ++i) x[i] = mk(sin(1.0 + 3.7 * i), cos(0.3 + 2.1 * i * i));
    X = x;
    Dft<R>::run(X.data());
    return naive_err(x, X, -1);
}

// the kernels' two steps (dc_device.h fft_lds), with the intermediate at pitch SP inside one LINE; inverse by conjugation
template <int R1, int R2> static double test_plan(bool inverse) {
    typedef Plan<R1, R2> P;
    const int N = P::N;
    std::vector<cd> x(N), X(N), S(P::LINE), tw(N);
    for (int i = 0; i < N; ++i) {
        x[i] = mk(sin(0.5 + 1.3 * i) + 0.01 * i, cos(0.1 + 0.7 * i));
        tw[i] = mk(cos(2.0 * M_PI * i / N), -sin(2.0 * M_PI * i / N));
    }
    for (int n2 = 0; n2 < R2; ++n2) {            // step 1
        cd a[R1];
        for (int n1 = 0; n1 < R1; ++n1) a[n1] = inverse ? conj(x[R2 * n1 + n2]) : x[R2 * n1 + n2];
        Dft<R1>::run(a);
        for (int q = 0; q < R1; ++q) S[P::SP * n2 + q] = q ? mul(a[q], tw[n2 * q]) : a[q];
    }
    for (int k1 = 0; k1 < R1; ++k1) {            // step 2
        cd b[R2];
        for (int n2 = 0; n2 < R2; ++n2) b[n2] = S[P::SP * n2 + k1];
        Dft<R2>::run(b);
        for (int k2 = 0; k2 < R2; ++k2) X[k1 + R1 * k2] = inverse ? conj(b[k2]) : b[k2];
    }
    return naive_err(x, X, inverse ? 1 : -1);
}

int main() {
    double e;
    int bad = 0;
#define CHECK(name, expr) e = (expr); printf("%-16s %.3e\n", name, e); if (!(e < 1e-13)) bad++;
    CHECK("dft3", test_codelet<3>());
    CHECK("dft5", test_codelet<5>());
    CHECK("dft6", test_codelet<6>());
    CHECK("dft10", test_codelet<10>());
    CHECK("dft12", test_codelet<12>());
    int nsides = 0;
    char name[32];
#define PLAN_CHECK(n_, a_, b_)                                                                          \
    static_assert(a_ * b_ == n_ && n_ % 16 == 0, "plan table");                                         \
    snprintf(name, sizeof name, "plan%dx%d", a_, b_); CHECK(name, (test_plan<a_, b_>(false)));          \
    snprintf(name, sizeof name, "plan%dx%d inv", a_, b_); CHECK(name, (test_plan<a_, b_>(true)));       \
    if (!side_supported(n_)) { printf("side %d not supported\n", n_); bad++; }                          \
    ++nsides;
    QFFT_PLANS(PLAN_CHECK)
    if (nsides != 9 || side_supported(230) || side_supported(200) || side_supported(512)) { printf("side table\n"); bad++; }
    return bad;
}
