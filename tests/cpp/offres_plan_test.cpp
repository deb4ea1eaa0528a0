// offres_plan_test.cpp -- the host tables of the off-resonance correction (csrc/offres_plan.h): the functions qmri_set_field_map and
// qmri_nufft_prepare_normal_fm call, on a machine without a GPU and under the address and undefined-behaviour sanitizers.  Built and run by
// tests/test_nufft_plan_host.py, which compares the histogram lines printed here with the counts the code gave before it was moved into the header.
//   stdout: per map  "<name> pixels=<N M> nbins=<bins> digest=<FNV-1a of the counts>", then "dump p<nbins>|dh<nbins> <values, %.17g>" of map16, and the
//           largest figure of every bounded check ("worst <check> <value> <bound>")
// Exit status 1: a check failed (named on stderr).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include "offres_plan.h"

using namespace offres;

static int g_failed = 0;
static std::string g_case = "-";
#define EXPECT(cond) do { if (!(cond)) { if (++g_failed <= 20) fprintf(stderr, "offres_plan_test: %s: line %d: %s is false\n", g_case.c_str(), __LINE__, #cond); } } while (0)
static const double EPS = 2.220446049250313e-16;

// f = scale (sin 2 pi a cos pi b + 0.6 b + 0.2) on a, b in [-1/2, 1/2): tests/offres_ref.py field()
static std::vector<double> field(int N, int M, double scale) {
    std::vector<double> f((size_t)N * M);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < M; ++j) {
            const double a = (i - N / 2.0) / N, b = (j - M / 2.0) / M;
            f[(size_t)i * M + j] = scale * (std::sin(2.0 * PI * a) * std::cos(PI * b) + 0.6 * b + 0.2);
        }
    return f;
}
static void range_of(const std::vector<double>& f, double* lo, double* hi) {
    *lo = *hi = f[0];
    for (double v : f) { *lo = std::min(*lo, v); *hi = std::max(*hi, v); }
}
struct Worst { double v = 0.0, bound = 0.0; void see(double x, double b) { if (x / b >= (bound > 0.0 ? v / bound : -1.0)) { v = x; bound = b; } } };
static void report(const char* what, const Worst& w) { printf("worst %s %.3g %.3g\n", what, w.v, w.bound); }

// ---- the histogram ---------------------------------------------------------------------------------------------------------------------------------
static void check_histogram(const std::vector<double>& f, const MapHist& h, int nbins_asked) {
    double f_min, f_max;
    range_of(f, &f_min, &f_max);
    EXPECT(h.constant == (f_max == f_min) && h.nbins == (h.constant ? 1 : nbins_asked) && h.f0 == 0.5 * (f_min + f_max));
    EXPECT(h.cnt.size() == (size_t)h.nbins && h.pf.size() == 2 * (size_t)h.nbins);
    if (g_failed) return;
    size_t total = 0;
    for (size_t c : h.cnt) total += c;
    EXPECT(total == f.size());
    if (h.constant) { EXPECT(h.p(0) == 1.0 && h.f(0) == 0.0); return; }
    const double lo = f_min - h.f0, width = (f_max - f_min) / h.nbins;
    // every pixel lies between the edges of the bin that the counts hold it in: recount by the edges (the last bin is closed at f_max)
    std::vector<size_t> mine((size_t)h.nbins, 0);
    for (double v : f) {
        const double d = (v - h.f0) - lo;
        int b = 0;
        while (b < h.nbins - 1 && d >= (b + 1) * width) ++b;
        EXPECT(d >= b * width && (d < (b + 1) * width || b == h.nbins - 1));
        mine[b] += 1;
    }
    size_t moved = 0;
    for (int b = 0; b < h.nbins; ++b) {
        moved += mine[b] > h.cnt[b] ? mine[b] - h.cnt[b] : h.cnt[b] - mine[b];
        EXPECT(h.p(b) == (double)h.cnt[b] / (double)f.size() && h.f(b) == lo + (b + 0.5) * width);
    }
    EXPECT(moved == 0);
}

// ---- Cholesky: max |C C^H - A| <= 4 L eps max |A| (the standard backward bound), lower triangular, real positive diagonal ----------------------------
static Worst g_chol;
static void check_fit_system(const MapHist& h, double t_min, double t_max, int L) {
    const FitSystem s = fit_system(h, t_min, t_max, L);
    EXPECT(s.ok && s.tauhat.size() == (size_t)L && s.G.size() == (size_t)h.nbins * L && s.C.size() == (size_t)L * L);
    if (g_failed) return;
    EXPECT(s.tauhat == segment_times(t_min, t_max, L));
    std::vector<cplx> A((size_t)L * L, cplx(0.0, 0.0));
    for (int b = 0; b < h.nbins; ++b)
        for (int l = 0; l < L; ++l) EXPECT(std::fabs(std::abs(s.G[(size_t)b * L + l]) - 1.0) <= 4 * EPS);
    for (int r = 0; r < L; ++r)
        for (int k = 0; k < L; ++k)
            for (int b = 0; b < h.nbins; ++b) A[(size_t)r * L + k] += h.p(b) * std::conj(s.G[(size_t)b * L + r]) * s.G[(size_t)b * L + k];
    double tr = 0.0, amax = 0.0, worst = 0.0;
    for (int r = 0; r < L; ++r) tr += A[(size_t)r * L + r].real();
    for (int r = 0; r < L; ++r) A[(size_t)r * L + r] += 1e-12 * tr / L;
    for (const cplx& a : A) amax = std::max(amax, std::abs(a));
    for (int r = 0; r < L; ++r)
        for (int k = 0; k < L; ++k) {
            const cplx c = s.C[(size_t)r * L + k];
            if (k > r) EXPECT(c == cplx(0.0, 0.0));
            if (k == r) EXPECT(c.real() > 0.0 && c.imag() == 0.0);
            cplx v(0.0, 0.0);
            for (int q = 0; q < L; ++q) v += s.C[(size_t)r * L + q] * std::conj(s.C[(size_t)k * L + q]);
            worst = std::max(worst, std::abs(v - A[(size_t)r * L + k]));
        }
    g_chol.see(worst, 4.0 * L * EPS * amax);
    EXPECT(worst <= 4.0 * L * EPS * amax);
}

// ---- QR: max |Q^T Q - I| <= 4 rows eps, max |Q U - B| <= 4 L rows eps max |B|, U upper triangular with a positive diagonal ----------------------------
static Worst g_orth, g_qu;
static void check_normal_tables(const std::vector<double>& dh, double t_min, double t_max, int L) {
    const int nb = (int)(dh.size() / 2);
    const NormalTables s = normal_tables(dh, t_min, t_max, L);
    EXPECT(s.ok && s.tauhat == segment_times(t_min, t_max, L) && s.G.size() == 2 * (size_t)nb * L && s.Qw.size() == s.G.size() && s.U.size() == (size_t)L * L);
    if (g_failed) return;
    // the stacked table, built here from G; its factors by the same function
    const size_t rows = 2 * (size_t)nb + L;
    double psum = 0.0, bmax = 0.0;
    for (int j = 0; j < nb; ++j) psum += dh[2 * (size_t)j];
    std::vector<double> B(rows * L, 0.0), U;
    for (int l = 0; l < L; ++l) {
        for (int j = 0; j < nb; ++j) {
            const double a = 2.0 * PI * dh[2 * (size_t)j + 1] * s.tauhat[l];
            EXPECT(s.G[2 * ((size_t)j * L + l)] == std::cos(a) && s.G[2 * ((size_t)j * L + l) + 1] == std::sin(a));
            B[(size_t)l * rows + 2 * j] = std::sqrt(dh[2 * (size_t)j]) * std::cos(a);
            B[(size_t)l * rows + 2 * j + 1] = std::sqrt(dh[2 * (size_t)j]) * std::sin(a);
        }
        B[(size_t)l * rows + 2 * nb + l] = std::sqrt(1e-12 * psum);
    }
    for (double v : B) bmax = std::max(bmax, std::fabs(v));
    std::vector<double> Q(B);
    EXPECT(qr_mgs2(Q, rows, L, U) && U == s.U);
    if (g_failed) return;
    for (int j = 0; j < nb; ++j)
        for (int l = 0; l < L; ++l)
            EXPECT(s.Qw[2 * ((size_t)j * L + l)] == std::sqrt(dh[2 * (size_t)j]) * Q[(size_t)l * rows + 2 * j] &&
                   s.Qw[2 * ((size_t)j * L + l) + 1] == std::sqrt(dh[2 * (size_t)j]) * Q[(size_t)l * rows + 2 * j + 1]);
    double orth = 0.0, qu = 0.0;
    for (int a = 0; a < L; ++a)
        for (int b = 0; b < L; ++b) {
            double d = 0.0;
            for (size_t t = 0; t < rows; ++t) d += Q[(size_t)a * rows + t] * Q[(size_t)b * rows + t];
            orth = std::max(orth, std::fabs(d - (a == b ? 1.0 : 0.0)));
            if (a > b) EXPECT(U[(size_t)a * L + b] == 0.0);
            if (a == b) EXPECT(U[(size_t)a * L + a] > 0.0);
        }
    for (int l = 0; l < L; ++l)
        for (size_t t = 0; t < rows; ++t) {
            double v = 0.0;
            for (int i = 0; i <= l; ++i) v += Q[(size_t)i * rows + t] * U[(size_t)i * L + l];
            qu = std::max(qu, std::fabs(v - B[(size_t)l * rows + t]));
        }
    g_orth.see(orth, 4.0 * rows * EPS); g_qu.see(qu, 4.0 * L * rows * EPS * bmax);
    EXPECT(orth <= 4.0 * rows * EPS && qu <= 4.0 * L * rows * EPS * bmax);
}

// ---- the difference histogram: symmetric in j, sums to (sum p)^2 within 4 nbins eps, at g_j = j width -------------------------------------------------
static void check_diff_histogram(const std::vector<double>& p, double width, const std::vector<double>& dh) {
    const int nbins = (int)p.size(), nb = 2 * nbins - 1;
    EXPECT(dh.size() == 2 * (size_t)nb);
    if (g_failed) return;
    double sp = 0.0, sd = 0.0;
    for (double v : p) sp += v;
    for (int j = 0; j < nb; ++j) {
        sd += dh[2 * (size_t)j];
        EXPECT(dh[2 * (size_t)j] == dh[2 * (size_t)(nb - 1 - j)] && dh[2 * (size_t)j + 1] == (j - (nbins - 1)) * width && dh[2 * (size_t)j] >= 0.0);
    }
    EXPECT(std::fabs(sd - sp * sp) <= 4.0 * nbins * EPS);
}

// the first time is t_min and the last one t_max, exactly; the times ascend; L = 1 gives t_min
static void check_segment_times() {
    g_case = "segment_times";
    const double ends[3][2] = {{0.0, 5e-3}, {0.0, 59 * (5e-3 / 60)}, {1.25e-3, 7.5e-3}};
    for (const auto& e : ends) {
        EXPECT(segment_times(e[0], e[1], 1) == std::vector<double>(1, e[0]));
        for (int L = 2; L <= OFFRES_NLMAX; ++L) {
            const std::vector<double> t = segment_times(e[0], e[1], L);
            EXPECT(t.size() == (size_t)L && t[0] == e[0] && t[L - 1] == e[1]);
            for (int l = 1; l < L; ++l) EXPECT(t[l] > t[l - 1]);
        }
    }
}

static void dump(const char* name, const double* v, size_t n, size_t stride) {
    printf("dump %s", name);
    for (size_t i = 0; i < n; ++i) printf(" %.17g", v[i * stride]);
    printf("\n");
}

int main() {
    const double t_min = 0.0, t_max = 59 * (5e-3 / 60);          // the readout of tests/offres_ref.py: 60 samples over 5 ms
    {
        g_case = "cholesky_refusals";
        std::vector<cplx> indefinite = {cplx(1.0, 0.0), cplx(2.0, 0.0), cplx(2.0, 0.0), cplx(1.0, 0.0)}, zero(4, cplx(0.0, 0.0)), fine = {cplx(4.0, 0.0), cplx(0.0, 2.0), cplx(0.0, -2.0), cplx(5.0, 0.0)};
        EXPECT(!cholesky(indefinite, 2) && !cholesky(zero, 2) && cholesky(fine, 2));
        EXPECT(fine[0] == cplx(2.0, 0.0) && fine[1] == cplx(0.0, 0.0) && fine[2] == cplx(0.0, -1.0) && fine[3] == cplx(2.0, 0.0));
        g_case = "qr_refusals";
        std::vector<double> B = {1.0, 2.0, 2.0, 0.0, 0.0, 0.0}, U;      // [rows = 3][L = 2] by columns: the second column is zero
        EXPECT(!qr_mgs2(B, 3, 2, U));
    }
    check_segment_times();
    for (int N : {16, 32})
        for (int nbins : {16, 256}) {
            g_case = "map" + std::to_string(N) + "/nbins" + std::to_string(nbins);
            const std::vector<double> f = field(N, N, 100.0);
            double f_min, f_max;
            range_of(f, &f_min, &f_max);
            const MapHist h = map_histogram(f.data(), f.size(), f_min, f_max, nbins);
            check_histogram(f, h, nbins);
            uint64_t d = 1469598103934665603ull;
            for (size_t c : h.cnt) { const uint64_t c64 = c; for (int i = 0; i < 8; ++i) { d ^= (c64 >> (8 * i)) & 0xff; d *= 1099511628211ull; } }
            printf("%s pixels=%zu nbins=%d digest=%016" PRIx64 "\n", g_case.c_str(), f.size(), h.nbins, d);
            if (g_failed) continue;
            for (int L : {2, 8, 16}) check_fit_system(h, t_min, t_max, L);
            std::vector<double> p((size_t)h.nbins);
            for (int b = 0; b < h.nbins; ++b) p[b] = h.p(b);
            const double width = (f_max - f_min) / h.nbins;
            const std::vector<double> dh = diff_histogram(p, width);
            check_diff_histogram(p, width, dh);
            if (N == 16) {          // both bin counts, for the restatement's difference histogram: "dump p16 | dh16 | p256 | dh256 ..."
                dump(("p" + std::to_string(nbins)).c_str(), p.data(), p.size(), 1); dump(("dh" + std::to_string(nbins)).c_str(), dh.data(), dh.size() / 2, 2);
            }
            for (int L : {2, 8, 32}) check_normal_tables(dh, t_min, t_max, L);
        }
    {   // a constant map: one bin at 0 holding every pixel, one segment at t_min, the 1 x 1 system
        g_case = "constant16";
        const std::vector<double> f(256, 37.5);
        const MapHist h = map_histogram(f.data(), f.size(), 37.5, 37.5, 256);
        check_histogram(f, h, 256);
        printf("%s pixels=%zu nbins=%d digest=%016" PRIx64 "\n", g_case.c_str(), f.size(), h.nbins, (uint64_t)h.cnt[0]);
        check_fit_system(h, t_min, t_max, 1);
        const FitSystem s = fit_system(h, t_min, t_max, 1);
        EXPECT(s.tauhat[0] == t_min && s.G[0] == cplx(1.0, 0.0));
    }
    report("cholesky", g_chol); report("qr_orthogonality", g_orth); report("qr_product", g_qu);
    if (g_failed) fprintf(stderr, "offres_plan_test: %d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
