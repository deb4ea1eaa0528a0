// wav_plan_test.cpp -- the geometry of the joint wavelet soft-thresholding step (csrc/wav_plan.h) swept on the host, as a
// stand-alone program built with the address and undefined-behaviour sanitizers by tests/test_wavelet_host.py.  For N, M in {16, 32, 48, 80, 112,
// 256}, L = 1 .. 4, both filter lengths, s in {1, 16} and B in {1, 3} it walks the launch list of one prox on tagged buffers and checks that
//   - every coefficient position of every level is written by exactly one tile, of the analysis and of the synthesis;
//   - every halo index is in range after wrapping, and a tile with its halo fits the LDS arrays;
//   - no launch reads the buffer it writes, and every launch reads what an earlier launch left there (the ping-pong);
//   - the scratch and partials sizes cover every index of the last plane of the last slice.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wav_plan.h"

using namespace wav;

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { if (++fails < 20) std::fprintf(stderr, "check failed, line %d: %s (N %d M %d L %d T %d s %d B %d)\n", __LINE__, #cond, gN, gM, gL, gT, gs, gB); } \
    } while (0)
static int gN, gM, gL, gT, gs, gB;

// what a position of a buffer holds: nothing, the input, approximation of level l (0: the image itself), detail of level l
enum { NONE = 0, APPROX = 100, DETAIL = 200, SHRUNK = 300 };

struct Plane {
    int N, M;
    std::vector<int> tag, writes;
    Plane(int n, int m) : N(n), M(m), tag((size_t)n * m, NONE), writes((size_t)n * m, 0) {}
    int& at(int r, int c) { return tag[(size_t)r + (size_t)N * c]; }
    void clear_writes() { std::fill(writes.begin(), writes.end(), 0); }
};

static void sweep_one(int N, int M, int L, int T, int s, int B) {
    gN = N; gM = M; gL = L; gT = T; gs = s; gB = B;
    Launch ls[MAX_LAUNCHES];
    const int nl = launch_list(N, M, s, B, L, ls);
    EXPECT(nl == 2 * L + 1);
    Plane x(N, M), s0(N, M), s1(N, M), out(N, M);
    std::fill(x.tag.begin(), x.tag.end(), APPROX + 0);
    Plane* bufs[4] = {&x, &s0, &s1, &out};                     // Buf + 1
    const size_t cap = scratch_elems(N, M, s, B), last_base = ((size_t)B * s - 1) * N * M;
    for (int i = 0; i < nl; ++i) {
        const Launch& l = ls[i];
        if (l.kind == SHRINK) {
            EXPECT(i == L && l.groups == shrink_groups_per_slice(N, M) * B && (size_t)l.groups <= partial_elems(N, M, B));
            EXPECT(shrink_groups_per_slice(N, M) * SHRINK_POS >= (long long)N * M);
            for (int c = 0; c < M; ++c)
                for (int r = 0; r < N; ++r) {
                    const int lev = level_of(r, c, N, M, L);
                    EXPECT(lev >= 0 && lev <= L);
                    EXPECT((lev == 0) == (r < (N >> L) && c < (M >> L)));
                    if (lev == 0) continue;
                    Plane& b = *bufs[buf_of_level(lev) + 1];
                    EXPECT(b.at(r, c) == DETAIL + lev);                       // the detail of its level lives in that buffer at that place
                    EXPECT(last_base + (size_t)r + (size_t)N * c < cap);
                    b.at(r, c) = SHRUNK + lev;
                }
            continue;
        }
        EXPECT(l.src != l.dst && l.src >= BUF_X && l.src <= BUF_S1 && l.dst >= BUF_S0 && l.dst <= BUF_OUT);
        EXPECT((l.src == BUF_X) == (l.kind == FWD && l.level == 1) && (l.dst == BUF_OUT) == (l.kind == INV && l.level == 1));
        Plane& src = *bufs[l.src + 1];
        Plane& dst = *bufs[l.dst + 1];
        const int n = l.n, m = l.m, hn = n / 2, hm = m / 2;
        EXPECT(n == corner(N, l.level) && m == corner(M, l.level) && n % 2 == 0 && m % 2 == 0 && n >= T && m >= T);
        EXPECT(l.tn == tiles(n) && l.tm == tiles(m) && l.groups == (long long)l.tn * l.tm * s * B && l.groups > 0);
        if (l.dst != BUF_OUT) EXPECT(last_base + (size_t)(n - 1) + (size_t)N * (m - 1) < cap);
        dst.clear_writes();
        for (int t2 = 0; t2 < l.tm; ++t2)
            for (int t1 = 0; t1 < l.tn; ++t1) {
                const int len1 = tile_len(n, t1), len2 = tile_len(m, t2);
                EXPECT(len1 > 0 && len1 <= TILE && len1 % 2 == 0 && len2 > 0 && len2 <= TILE && len2 % 2 == 0);
                if (l.kind == FWD) {
                    const int w1 = len1 + fwd_halo(T), w2 = len2 + fwd_halo(T);
                    EXPECT(w1 <= FWD_IN_SIDE && w2 <= FWD_IN_SIDE && FWD_IN_SIDE / 2 + (w1 - 1) / 2 < FWD_IN_STRIDE && len1 <= FWD_MID_STRIDE);
                    for (int j = 0; j < w2; ++j)
                        for (int ii = 0; ii < w1; ++ii) {
                            const int r = wrap(t1 * TILE + ii, n), c = wrap(t2 * TILE + j, m);
                            EXPECT(r >= 0 && r < n && c >= 0 && c < m);
                            EXPECT(src.at(r, c) == APPROX + l.level - 1);     // the approximation of the level before (level 1: the image)
                        }
                    for (int k2 = 0; k2 < len2 / 2; ++k2)
                        for (int k1 = 0; k1 < len1 / 2; ++k1) {
                            // the last tap of the last output stays inside the tile and its halo
                            EXPECT(2 * k1 + T - 1 < w1 && 2 * k2 + T - 1 < w2);
                            for (int p2 = 0; p2 < 2; ++p2)
                                for (int p1 = 0; p1 < 2; ++p1) {
                                    const int r = p1 * hn + t1 * HALF + k1, c = p2 * hm + t2 * HALF + k2;
                                    EXPECT(r < n && c < m);
                                    dst.at(r, c) = (p1 | p2) ? DETAIL + l.level : APPROX + l.level;
                                    ++dst.writes[(size_t)r + (size_t)N * c];
                                }
                        }
                } else {
                    const int hh = inv_halo(T), c1 = len1 / 2 + hh, c2 = len2 / 2 + hh;
                    EXPECT(2 * c1 <= INV_IN_SIDE && 2 * c2 <= INV_IN_SIDE && 2 * c1 <= INV_IN_STRIDE && 2 * c1 <= INV_MID_STRIDE && len2 <= TILE);
                    for (int p2 = 0; p2 < 2; ++p2)
                        for (int p1 = 0; p1 < 2; ++p1)
                            for (int jj = 0; jj < c2; ++jj)
                                for (int ii = 0; ii < c1; ++ii) {
                                    const int k1 = wrap(t1 * HALF - hh + ii, hn), k2 = wrap(t2 * HALF - hh + jj, hm);
                                    EXPECT(k1 >= 0 && k1 < hn && k2 >= 0 && k2 < hm);
                                    const int want = (p1 | p2) ? SHRUNK + l.level : APPROX + l.level;
                                    EXPECT(src.at(p1 * hn + k1, p2 * hm + k2) == want);
                                }
                    for (int j = 0; j < len2; ++j)
                        for (int ii = 0; ii < len1; ++ii) {
                            // output 2 q + p takes the coefficients q - u, u < T / 2: local index q - u + hh in [0, c)
                            EXPECT(ii / 2 - (T / 2 - 1) + hh >= 0 && ii / 2 + hh < c1 && j / 2 + hh < c2);
                            const int r = t1 * TILE + ii, c = t2 * TILE + j;
                            EXPECT(r < n && c < m);
                            dst.at(r, c) = APPROX + l.level - 1;
                            ++dst.writes[(size_t)r + (size_t)N * c];
                        }
                }
            }
        for (int c = 0; c < M; ++c)
            for (int r = 0; r < N; ++r) EXPECT(dst.writes[(size_t)r + (size_t)N * c] == ((r < n && c < m) ? 1 : 0));
    }
    for (int v : out.tag) EXPECT(v == APPROX + 0);                                // the last launch left the whole image in out
}

static void offsets_rule() {
    for (int L = 1; L <= MAX_LEVELS; ++L) {
        const int P = 1 << L;
        std::vector<int> seen((size_t)P * P, 0);
        for (int it = 0; it < 3 * P * P; ++it) {
            int o1 = -1, o2 = -1;
            offsets(it, P, 1, &o1, &o2);
            const int q = it % (P * P);
            if (!(o1 == q % P && o2 == (q / P + q) % P && o1 >= 0 && o1 < P && o2 >= 0 && o2 < P)) { ++fails; continue; }
            ++seen[(size_t)o1 * P + o2];
            offsets(it, P, 0, &o1, &o2);
            if (o1 || o2) ++fails;
        }
        for (int v : seen) if (v != 3) ++fails;                                   // every offset once per P^2 iterations
    }
}

int main() {
    const int sides[] = {16, 32, 48, 80, 112, 256}, ss[] = {1, 16}, Bs[] = {1, 3}, Ts[] = {2, 4};
    int swept = 0, refused = 0;
    for (int N : sides)
        for (int M : sides)
            for (int L = 1; L <= MAX_LEVELS; ++L)
                for (int T : Ts) {
                    if (!sizes_ok(N, M, L, T)) { ++refused; continue; }
                    for (int s : ss)
                        for (int B : Bs) { sweep_one(N, M, L, T, s, B); ++swept; }
                }
    // the size rule itself: 16 takes Haar to L = 4 and DB2 to L = 3; every operator side passes for both filters at every L
    if (!(sizes_ok(16, 16, 4, 2) && !sizes_ok(16, 16, 4, 4) && sizes_ok(16, 16, 3, 4) && !sizes_ok(24, 32, 4, 2) && !sizes_ok(32, 32, 5, 2) &&
          !sizes_ok(32, 32, 0, 2) && !sizes_ok(0, 32, 1, 2) && !sizes_ok(2, 2, 1, 4) && sizes_ok(2, 2, 1, 2)))
        ++fails;
    for (int side = 32; side <= 256; side += 16)
        for (int L = 1; L <= MAX_LEVELS; ++L)
            if (!sizes_ok(side, side, L, 2) || !sizes_ok(side, 256, L, 4)) ++fails;
    offsets_rule();
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("WAV_PLAN_OK swept %d refused %d\n", swept, refused);
    return 0;
}
