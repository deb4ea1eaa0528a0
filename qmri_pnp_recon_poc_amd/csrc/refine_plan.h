// refine_plan.h -- the lines of a gridded dictionary: for every atom and every chosen lut column, the atom's lower and upper neighbour along that
// column, all other columns held equal (qmri_dict_lines; the sub-grid refinement of DESIGN.md section 30 fits a quadratic through an atom and these
// neighbours), and the refinement's table of unnormalised atoms.  No HIP, no context: plain C++17 of floats and integers, so that
// tests/cpp/refine_plan_test.cpp runs the functions the library calls under the host sanitizers on a machine without a GPU.
#ifndef QMRI_REFINE_PLAN_H         // (a guard, not #pragma once: the header is also compiled on its own)
#define QMRI_REFINE_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rplan {

constexpr int MAX_P = 3;            // refined columns of a fit
constexpr int ROW = 16;             // doubles of an atom's row in the refinement's table: s <= 16 channels, zero padded (one 128-byte line)

// lut: K x Q floats, column-major (lut[k + K c], as qmri_set_dictionary takes it).  An atom takes part in lines when all its lut entries are finite
// and its normD is finite and not zero.
inline bool atom_valid(int K, int Q, const float* lut, const float* normD, int k) {
    if (!std::isfinite(normD[k]) || normD[k] == 0.f) return false;
    for (int c = 0; c < Q; ++c)
        if (!std::isfinite(lut[k + (size_t)K * c])) return false;
    return true;
}

// The argument rules of qmri_dict_lines that need no array: P in 1..MAX_P, cols distinct and inside 0..Q-1.  Empty string: fine.
inline std::string check_cols(int Q, int P, const int32_t* cols) {
    if (P < 1 || P > MAX_P) return "1 <= P <= 3 refined columns";
    for (int q = 0; q < P; ++q) {
        if (cols[q] < 0 || cols[q] >= Q) return "lut column " + std::to_string(cols[q]) + " is outside 0.." + std::to_string(Q - 1);
        for (int e = 0; e < q; ++e)
            if (cols[e] == cols[q]) return "lut column " + std::to_string(cols[q]) + " is named twice";
    }
    return std::string();
}

// nbr [K][P][2] (0-based atom, -1 = none; [..][0] the lower, [..][1] the upper neighbour), count [P][3] = atoms with 0, 1 and 2 neighbours per column.
// Atoms a, b are on one line of column c when every other lut column compares equal.  The upper neighbour of k is the atom of k's line with the
// smallest lut[., c] greater than lut[k, c], the lowest index among equal values; the lower neighbour mirrors it.  One lexicographic sort of the
// valid atoms per column (other columns ascending, then column c, then the index): O(Q K log K).  Returns "" or the refusal's message.
inline std::string dict_lines(int K, int Q, const float* lut, const float* normD, int P, const int32_t* cols, int32_t* nbr, int32_t* count) {
    const std::string bad = check_cols(Q, P, cols);
    if (!bad.empty()) return bad;
    std::vector<int32_t> idx;
    idx.reserve((size_t)K);
    for (int k = 0; k < K; ++k)
        if (atom_valid(K, Q, lut, normD, k)) idx.push_back(k);
    std::fill(nbr, nbr + (size_t)K * P * 2, (int32_t)-1);
    auto at = [&](int k, int c) { return lut[k + (size_t)K * c]; };
    for (int q = 0; q < P; ++q) {
        const int c = cols[q];
        auto same_line = [&](int a, int b) {
            for (int o = 0; o < Q; ++o)
                if (o != c && !(at(a, o) == at(b, o))) return false;
            return true;
        };
        std::vector<int32_t> ord(idx);
        std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
            for (int o = 0; o < Q; ++o)
                if (o != c && at(a, o) != at(b, o)) return at(a, o) < at(b, o);
            if (at(a, c) != at(b, c)) return at(a, c) < at(b, c);
            return a < b;
        });
        // a line is a run of ord; inside it, a run of equal values is represented by its first entry (the lowest index)
        const size_t n = ord.size();
        for (size_t l0 = 0; l0 < n;) {
            size_t l1 = l0 + 1;
            while (l1 < n && same_line(ord[l0], ord[l1])) ++l1;
            int32_t prev_rep = -1;
            for (size_t v0 = l0; v0 < l1;) {
                size_t v1 = v0 + 1;
                while (v1 < l1 && at(ord[v1], c) == at(ord[v0], c)) ++v1;
                const int32_t next_rep = v1 < l1 ? ord[v1] : -1;
                for (size_t i = v0; i < v1; ++i) {
                    nbr[((size_t)ord[i] * P + q) * 2 + 0] = prev_rep;
                    nbr[((size_t)ord[i] * P + q) * 2 + 1] = next_rep;
                }
                prev_rep = ord[v0];
                v0 = v1;
            }
            l0 = l1;
        }
        int32_t* cnt = count + 3 * q;
        cnt[0] = cnt[1] = cnt[2] = 0;
        for (int k = 0; k < K; ++k) ++cnt[(nbr[((size_t)k * P + q) * 2] >= 0) + (nbr[((size_t)k * P + q) * 2 + 1] >= 0)];
        if (cnt[1] + cnt[2] == 0) return "lut column " + std::to_string(c) + " has no lines";
    }
    return std::string();
}

// The refinement's table: row k = the unnormalised atom a_k = double(normD[k]) * double(D[k, :]) (D: K x s floats, column-major), zero padded to ROW.
inline void atom_rows(int K, int s, const float* D, const float* normD, double* arow) {
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < ROW; ++j) arow[(size_t)k * ROW + j] = j < s ? (double)normD[k] * (double)D[k + (size_t)K * j] : 0.0;
}

}  // namespace rplan

#endif  // QMRI_REFINE_PLAN_H
