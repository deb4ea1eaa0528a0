// wav_plan.h -- what the host decides about one joint wavelet soft-thresholding step (include/qmri.h qmri_wavelet_prox), in
// plain C++17 that compiles alone: the level geometry of the Mallat layout, the offsets rule, the tile grid of each launch and the halo a tile
// loads, the scratch sizes and the launch list of one prox.  wav_kernels.hip and api_wav.cpp call these functions and restate none of the
// arithmetic; tests/cpp/wav_plan_test.cpp sweeps them on the host.
//
// Data: a plane is N x M, index n1 + N n2; a slice holds s planes, a stack B slices.  Level l = 1 .. L reads the (N >> (l-1)) x (M >> (l-1)) corner
// ("the input corner of level l") and writes four half-size sub-bands into the same corner: sub-band (p1, p2), p = 0 approximation, 1 detail, at
// row offset p1 * (n / 2) and column offset p2 * (m / 2).
//
// Buffers.  Two scratch stacks S0 and S1 of B s N M elements.  Analysis level l writes all four sub-bands to S[(l-1) & 1] and reads the
// approximation corner of S[(l-2) & 1] (level 1: the caller's x); the shrink works in place on the detail positions, each in the buffer of its
// level; synthesis level l reads the corner of S[(l-1) & 1] and writes its output into the approximation corner of S[(l-2) & 1] (level 1: the
// caller's out).  No launch reads the buffer it writes.
#ifndef QMRI_WAV_PLAN_H
#define QMRI_WAV_PLAN_H

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WAV_HD __host__ __device__ __forceinline__
#else
#define WAV_HD inline
#endif

namespace wav {

constexpr int MAX_LEVELS = 4, MAX_S = 16, MAX_TAPS = 4, MAX_SIDE = 16384;
constexpr int TILE = 32;                 // side of a tile in the level's input corner (analysis: inputs, synthesis: outputs); its sub-band tiles are TILE / 2
constexpr int HALF = TILE / 2;
constexpr int NT = 256;                  // threads of every workgroup
constexpr int SHRINK_POS = NT;           // positions of a plane per workgroup of the shrink launch

enum Kind { FWD = 0, SHRINK = 1, INV = 2 };
enum Buf { BUF_X = -1, BUF_S0 = 0, BUF_S1 = 1, BUF_OUT = 2 };

WAV_HD int taps(int filter) { return filter == 0 ? 2 : 4; }                       // QMRI_WAVELET_HAAR 0, QMRI_WAVELET_DB2 1
inline bool filter_known(int filter) { return filter == 0 || filter == 1; }
inline int levels_or_default(int levels) { return levels ? levels : 3; }

// 2^L | N, 2^L | M and the input of the last level at least T long on both axes
inline bool sizes_ok(int N, int M, int L, int T) {
    if (L < 1 || L > MAX_LEVELS || N < 1 || M < 1 || N > MAX_SIDE || M > MAX_SIDE) return false;
    const int P = 1 << L;
    return N % P == 0 && M % P == 0 && (N >> (L - 1)) >= T && (M >> (L - 1)) >= T;
}

// side of the input corner of level l (1-based) on an axis of length n
WAV_HD int corner(int n, int l) { return n >> (l - 1); }
// the scratch buffer that holds the sub-bands of level l
WAV_HD int buf_of_level(int l) { return (l - 1) & 1; }
// level whose detail sub-bands hold position (n1, n2); 0: the final approximation corner
WAV_HD int level_of(int n1, int n2, int N, int M, int L) {
    for (int l = 1; l <= L; ++l)
        if (n1 >= (N >> l) || n2 >= (M >> l)) return l;
    return 0;
}

// offsets of ADMM iteration `it` (0-based) with P = 2^L: section 25's rule
inline void offsets(int it, int P, int shift, int* o1, int* o2) {
    *o1 = *o2 = 0;
    if (!shift) return;
    const int q = it % (P * P);
    *o1 = q % P;
    *o2 = (q / P + q) % P;
}

WAV_HD int wrap(int i, int n) { const int r = i % n; return r < 0 ? r + n : r; }

// ---- tiles of one axis of a level: tile t covers [t * TILE, t * TILE + tile_len) of the input corner (an even count) ----
WAV_HD int tiles(int n) { return (n + TILE - 1) / TILE; }
WAV_HD int tile_len(int n, int t) { const int r = n - t * TILE; return r < TILE ? r : TILE; }
// analysis: the tile's outputs are k in [t * HALF, t * HALF + tile_len / 2) of each sub-band; it loads the inputs
// wrap(t * TILE + i, n), 0 <= i < tile_len + fwd_halo(T)
WAV_HD int fwd_halo(int T) { return T - 2; }
// synthesis: the tile's outputs are [t * TILE, t * TILE + tile_len); it loads the coefficients wrap(t * HALF - inv_halo(T) + i, n / 2),
// 0 <= i < tile_len / 2 + inv_halo(T), of both sub-bands of the axis
WAV_HD int inv_halo(int T) { return T / 2 - 1; }

// ---- launches ----
struct Launch {
    int kind, level;          // level 0: the shrink
    int src, dst;             // Buf
    int n, m;                 // FWD / INV: the input corner of the level; SHRINK: N, M
    int tn, tm;               // tiles along each axis (SHRINK: workgroups per plane position run, 1)
    long long groups;         // workgroups of the launch
};

WAV_HD long long shrink_groups_per_slice(int N, int M) { return ((long long)N * M + SHRINK_POS - 1) / SHRINK_POS; }

// the 2 L + 1 launches of one prox on B slices of s channels; returns their count
inline int launch_list(int N, int M, int s, int B, int L, Launch* out) {
    int c = 0;
    for (int l = 1; l <= L; ++l) {
        const int n = corner(N, l), m = corner(M, l);
        out[c++] = {FWD, l, l == 1 ? BUF_X : buf_of_level(l - 1), buf_of_level(l), n, m, tiles(n), tiles(m), (long long)tiles(n) * tiles(m) * s * B};
    }
    out[c++] = {SHRINK, 0, BUF_S0, BUF_S0, N, M, 1, 1, shrink_groups_per_slice(N, M) * B};      // (in place, both buffers: one lane per position)
    for (int l = L; l >= 1; --l) {
        const int n = corner(N, l), m = corner(M, l);
        out[c++] = {INV, l, buf_of_level(l), l == 1 ? BUF_OUT : buf_of_level(l - 1), n, m, tiles(n), tiles(m), (long long)tiles(n) * tiles(m) * s * B};
    }
    return c;
}
constexpr int MAX_LAUNCHES = 2 * MAX_LEVELS + 1;

// ---- scratch ----
inline size_t scratch_elems(int N, int M, int s, int B) { return (size_t)B * s * N * M; }          // each of S0 and S1, complex fp64
inline size_t partial_elems(int N, int M, int B) { return (size_t)shrink_groups_per_slice(N, M) * B; }   // per-workgroup maxima of m

// ---- LDS of a tile, in complex elements ----
constexpr int FWD_IN_SIDE = TILE + MAX_TAPS - 2;          // 34: inputs and halo
constexpr int FWD_IN_STRIDE = FWD_IN_SIDE + 1;            // 35: rows of the N axis, one column of the tile after another
constexpr int FWD_MID_STRIDE = TILE + 1;                  // 33: after the N-axis pass a column holds TILE / 2 a and TILE / 2 d
constexpr int INV_IN_SIDE = 2 * (HALF + MAX_TAPS / 2 - 1);   // 34: both sub-bands of an axis with their halo
constexpr int INV_IN_STRIDE = INV_IN_SIDE + 1;            // 35
constexpr int INV_MID_STRIDE = INV_IN_SIDE + 1;           // 35: after the M-axis pass: TILE columns of INV_IN_SIDE rows
constexpr size_t FWD_LDS_ELEMS = (size_t)FWD_IN_SIDE * FWD_IN_STRIDE + (size_t)FWD_IN_SIDE * FWD_MID_STRIDE;
constexpr size_t INV_LDS_ELEMS = (size_t)INV_IN_SIDE * INV_IN_STRIDE + (size_t)TILE * INV_MID_STRIDE;

}  // namespace wav

#endif  // QMRI_WAV_PLAN_H
