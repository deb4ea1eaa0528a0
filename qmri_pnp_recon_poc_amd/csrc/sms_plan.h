// sms_plan.h -- what the host decides about a simultaneous multi-slice (SMS) solve, in plain C++ (no HIP): the chunk schedule of both image orders,
// the sample -> frame table and the layout of the fixed partial sums.  DESIGN.md section 31; kernels: sms_kernels.hip; tests/cpp/sms_plan_test.cpp.
//
// A call holds G groups of Z slices and ncoil coils.  Its coil images go through the batched transforms max_batch at a time, in one of two orders:
//   forward   q = (g ncoil + j) Z + b    the Z images that add up to the measurements u_{g,j} are adjacent      (unit = Z,     units = G ncoil)
//   adjoint   q = (g Z + b) ncoil + j    the ncoil images that add up to the slice image t_{g,b} are adjacent  (unit = ncoil, units = G Z)
// Either way a chunk is a run of consecutive q, and the sum of a unit may begin in one chunk and go on in the next ones: slice b after slice b - 1
// and coil j after coil j - 1, whichever chunk holds them.  chunk_schedule states that once for both orders.
#ifndef QMRI_SMS_PLAN_H
#define QMRI_SMS_PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sms {
constexpr int MAX_Z = 8;          // slices excited together
constexpr int MAX_E = 8192;       // T x Z phase values at most
constexpr int PS = 256;           // partial sums per slice vector (n complex): mc_kernels.hip's
constexpr int PC = 64;            // partial sums per coil image (m complex): mc_kernels.hip's

// One transform chunk: images q0 .. q0 + cnt - 1, which touch the units u0 .. u0 + nu - 1.  Unit u0 is entered at its member lo0 (> 0: the chunk
// continues a sum an earlier chunk began) and unit u0 + nu - 1 is left after its member hi1 - 1 (< unit: a later chunk goes on); every unit between
// is whole.
struct Chunk {
    int q0, cnt, u0, nu, lo0, hi1;
};
inline bool begins(const Chunk& c, int k) { return k > 0 || c.lo0 == 0; }                    // unit u0 + k starts its sum in this chunk
inline bool finishes(const Chunk& c, int k, int unit) { return k < c.nu - 1 || c.hi1 == unit; }   // ... and ends it here
// members of unit u0 + k inside the chunk: [lo, hi)
inline void members(const Chunk& c, int k, int unit, int* lo, int* hi) {
    *lo = k == 0 ? c.lo0 : 0;
    *hi = k == c.nu - 1 ? c.hi1 : unit;
}

inline std::vector<Chunk> chunk_schedule(int units, int unit, int max_batch) {
    std::vector<Chunk> out;
    const long total = (long)units * unit;
    for (long q0 = 0; q0 < total; q0 += max_batch) {
        const int cnt = (int)std::min<long>(max_batch, total - q0);
        const int u0 = (int)(q0 / unit), u1 = (int)((q0 + cnt - 1) / unit);
        out.push_back({(int)q0, cnt, u0, u1 - u0 + 1, (int)(q0 - (long)u0 * unit), (int)(q0 + cnt - (long)u1 * unit)});
    }
    return out;
}

// frame of every sample in the ABI's frame-major order: frame_ptr [T + 1], frame_ptr[T] = m
inline std::vector<int32_t> frame_table(int T, const int32_t* frame_ptr) {
    std::vector<int32_t> f((size_t)frame_ptr[T]);
    for (int t = 0; t < T; ++t)
        for (int32_t i = frame_ptr[t]; i < frame_ptr[t + 1]; ++i) f[(size_t)i] = t;
    return f;
}

// Partial-sum slots of one solve, in doubles from the start of the buffer: per (g, j) PC each of |u|^2 and |y|^2, then per slice vector (g, b) PS
// each of |u2|^2, |z|^2, |d|^2, |x|^2, |v|^2 -- the layout of mc_kernels.hip with B = G Z slice vectors, so its image-side kernels write them.
struct Parts {
    size_t pu, py, pb, pz, pd, px, pv, total;
};
inline Parts parts(int G, int Z, int ncoil) {
    const size_t img = (size_t)G * ncoil * PC, sl = (size_t)G * Z * PS;
    Parts p;
    p.pu = 0; p.py = img; p.pb = 2 * img; p.pz = p.pb + sl; p.pd = p.pz + sl; p.px = p.pd + sl; p.pv = p.px + sl; p.total = p.pv + sl;
    return p;
}
}  // namespace sms
#endif  // QMRI_SMS_PLAN_H
