// op_plan.h -- everything qmri_set_operator and qmri_prepare_direct decide or compute on the host for a gridded operator: the two mask builders,
// the k-sorted sample list, the work units of the k-space LSQR (ks_plan_units) and the DIRECT solver's tables.  No HIP, no context: plain C++17,
// so that tests/cpp/op_plan_test.cpp runs the functions the library calls under the host sanitizers on a machine without a GPU.
// api_operator.cpp and api_xupdate.cpp validate, call these, and move the results to the device; nothing else decides.
#ifndef QMRI_OP_PLAN_H             // (a guard, not #pragma once: the header is also compiled on its own)
#define QMRI_OP_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// ---------------------------------------------------------------------------------------------------
// mask builders (integer index math).  Both fill frame_ptr[0..T] and the first `cap` entries of kidx, and return the number of samples m the
// mask has; m > cap: the caller's array was too small (kidx holds the first cap samples).
// ---------------------------------------------------------------------------------------------------
// the exponential spiral of setup_subsampling_spiralgrided.m:7-27 before rounding (shared by qmri_build_spiral and qmri_build_spiral_traj): S angles
// theta_j and radii r_j normalised to [0, 1]; frame f is rotated by f * SPIRAL_DELTA
constexpr double SPIRAL_DELTA = 3.14159265358979323846 / 180.0 * 7.5;
inline void spiral_points(int S, std::vector<double>& theta, std::vector<double>& rad) {
    const double pi = 3.14159265358979323846;
    theta.assign(S, 0.0); rad.assign(S, 0.0);
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int j = 0; j < S; ++j) {
        const double t = (j == S - 1) ? 2.0 * pi : (double)j * (2.0 * pi) / (double)(S - 1);   // linspace(0,2*pi,S)
        theta[j] = 8.0 * t;
        rad[j] = std::pow(1.05, theta[j]);
        lo = std::min(lo, rad[j]);
        hi = std::max(hi, rad[j]);
    }
    for (double& r : rad) r = (r - lo) / (hi - lo);
}

// setup_subsampling_spiralgrided.m:7-34.  8-turn exponential spiral sampled at S points, rotated 7.5 deg per
// frame, rounded onto the N x N grid (MATLAB round = half away from zero), clamped, fftshift-ed; the sample
// order inside a frame is find()'s ascending column-major order.
inline long mask_build_spiral(int N, int S, int T, int32_t* frame_ptr, int32_t* kidx, int cap) {
    const double delta = SPIRAL_DELTA;
    std::vector<double> theta, rad;
    spiral_points(S, theta, rad);
    std::vector<uint8_t> grid((size_t)N * N);
    const int half = N / 2;
    long m = 0;
    for (int f = 0; f < T; ++f) {
        frame_ptr[f] = (int32_t)m;
        std::fill(grid.begin(), grid.end(), 0);
        const double rot = (double)f * delta;
        for (int j = 0; j < S; ++j) {
            double gx = std::round(rad[j] * std::cos(theta[j] + rot) * N / 2.0) + N / 2.0 + 1.0;
            double gy = std::round(rad[j] * std::sin(theta[j] + rot) * N / 2.0) + N / 2.0 + 1.0;
            gx = std::min(gx, (double)N);
            gy = std::min(gy, (double)N);
            const int r = ((int)gx - 1 + half) % N, c = ((int)gy - 1 + half) % N;     // fftshift
            grid[(size_t)c * N + r] = 1;
        }
        for (int k = 0; k < N * N; ++k)
            if (grid[k]) {
                if (m < cap) kidx[m] = k;
                ++m;
            }
    }
    frame_ptr[T] = (int32_t)m;
    return m;
}

// setup_subsampling_epi.m:20-33.  Comb of floor(N/step) k-rows, step = round(1/percentage), shifted down by one
// row (cyclically) before every frame including the first; whole rows are sampled; no fftshift.
inline long mask_build_epi(int N, int M, double percentage, int T, int32_t* frame_ptr, int32_t* kidx, int cap) {
    const int step = (int)std::round(1.0 / percentage);
    const int nlines = N / step;
    std::vector<int> rows;
    for (int r = 0; r < step * nlines; r += step) rows.push_back(r);
    long m = 0;
    for (int f = 0; f < T; ++f) {
        frame_ptr[f] = (int32_t)m;
        for (int& r : rows) r = (r + 1) % N;
        std::vector<int> sorted(rows);
        std::sort(sorted.begin(), sorted.end());
        for (int c = 0; c < M; ++c)
            for (int r : sorted) {
                if (m < cap) kidx[m] = r + N * c;
                ++m;
            }
    }
    frame_ptr[T] = (int32_t)m;
    return m;
}

// ---------------------------------------------------------------------------------------------------
// k-sorted sample list: primary kh = k % N (k-space row), secondary kw = k / N, tertiary frame
// ---------------------------------------------------------------------------------------------------
struct KEntry {          // one sample of the k-sorted measurement list
    uint16_t kw;         // k-space column (second FFT dimension)
    uint16_t t;          // frame
};
struct KSorted {
    std::vector<int32_t> kptr_h;     // [N*M+1] CSR over k' = kh*M + kw into ent_h
    std::vector<KEntry> ent_h;       // [m]     k-sorted: (kh, kw, t) ascending
    std::vector<int32_t> perm_h;     // [m]     k-sorted position -> frame-major measurement index (ABI order)
    std::vector<int32_t> kslot;      // [N*M]   slot of k' among the sampled locations or -1
    int nsampled = 0;
};
inline KSorted op_sort_samples(int N, int M, int T, const int32_t* frame_ptr, const int32_t* kidx) {
    KSorted o;
    const int NM = N * M, m = frame_ptr[T];
    o.kptr_h.assign(NM + 1, 0);
    std::vector<int32_t> frame_of(m);
    for (int t = 0; t < T; ++t)
        for (int i = frame_ptr[t]; i < frame_ptr[t + 1]; ++i) frame_of[i] = t;
    auto kprime = [&](int k) { return (k % N) * M + (k / N); };
    for (int i = 0; i < m; ++i) o.kptr_h[kprime(kidx[i]) + 1]++;
    for (int k = 0; k < NM; ++k) o.kptr_h[k + 1] += o.kptr_h[k];
    std::vector<int32_t> fill(o.kptr_h.begin(), o.kptr_h.end() - 1);
    o.ent_h.resize(m);
    o.perm_h.resize(m);
    for (int i = 0; i < m; ++i) {                    // ascending i == ascending frame inside each k
        const int kp = kprime(kidx[i]);
        const int e = fill[kp]++;
        o.ent_h[e].kw = (uint16_t)(kidx[i] / N);
        o.ent_h[e].t = (uint16_t)frame_of[i];
        o.perm_h[e] = i;
    }
    o.kslot.assign(NM, -1);
    o.nsampled = 0;
    for (int kp = 0; kp < NM; ++kp)
        if (o.kptr_h[kp + 1] > o.kptr_h[kp]) o.kslot[kp] = o.nsampled++;
    return o;
}
// [nsampled+1] first sample of every sampled k location ("slot", k' order), then m
inline std::vector<int32_t> ks_slot_ptr(const KSorted& k) {
    std::vector<int32_t> sptr(k.nsampled + 1);
    int j = 0;
    for (size_t kp = 0; kp < k.kslot.size(); ++kp) if (k.kslot[kp] >= 0) sptr[j++] = k.kptr_h[kp];
    sptr[k.nsampled] = k.kptr_h.back();
    return sptr;
}

// ---------------------------------------------------------------------------------------------------
// k-space LSQR (kslsqr_kernels.hip): work partition over the sampled k locations ("slots", k' order)
// ---------------------------------------------------------------------------------------------------
struct KSample { uint16_t ls, t; };              // slot of a sample relative to its block's first slot; frame
struct KsGroup { uint16_t ls, b, e, pad; };      // <= gcap samples of one slot; b, e relative to the block's first sample
// The shape of a work unit: slots, samples, samples per scatter group, lanes that share a group, scatter groups per block (= ecap / gcap + scap).
// Picked by ks_plan_units below; kslsqr_kernels.hip instantiates its kernels for each (KsCaps):
//   0  dense masks (a sampled k location carries >= 8 samples on average: the spiral), slice batches and single slices whose units fit the chip
//   1  sparse masks (EPI: every k location, 2.7 samples each), ONE slice: 256 slots per unit so that <= 250 units result (one-launch iteration)
//   2  dense, very many samples per k (cut0: 56), ONE slice: 2560 samples per unit, <= 256 units (one-launch iteration)
//   3  sparse masks, slice batches (and whatever 1 does not fit): small units
// Sparse shapes give every scatter group (<= 4 samples of one slot) to ONE lane; the dense ones share a group of <= 32 samples among 8 lanes.
struct KsCapsHost { int scap, ecap, gcap, sl, gcapb; };
constexpr KsCapsHost KS_CAPS[4] = {{64, 1024, 32, 8, 96}, {256, 768, 4, 1, 448}, {64, 2560, 32, 8, 144}, {64, 256, 4, 1, 128}};
constexpr int KS_NCAPS = 4;
struct KsUnit { int32_t s0, s1, e0, e1, g0, g1, pad0, pad1; };   // a work unit: its slots, samples and groups (one 32-byte scalar load)

struct KsPlanIn {
    int m, ns, s, T, max_batch;                  // samples, sampled k locations, channels, frames, slices per launch at most
    const int32_t* sptr;                         // [ns+1] ks_slot_ptr
    const KEntry* ent;                           // [m]    the k-sorted samples (their frames)
    bool one_launch;                             // the one-launch iteration (k_ks_persist) is switched on
    int ncu;                                     // CUs of the device
    bool lds_fits[KS_NCAPS];                     // V (vcap doubles) fits the LDS of the kernels of each unit shape (ks_lds_fits)
};
enum KsPlanStatus {
    KS_PLAN_OK = 0,
    KS_PLAN_BUSY_K = 1,                          // a k location is sampled `n` times, more than the `tried` samples the largest shape tried holds
    KS_PLAN_V_TOO_LARGE = 2                      // V does not fit the on-chip budget of the chosen shape's kernels
};
struct KsPlan {
    KsPlanStatus status = KS_PLAN_OK;
    int n = 0, tried = 0;                        // KS_PLAN_BUSY_K
    int caps = 0, vcap = 0, G = 0;               // unit shape (index into KS_CAPS), doubles of LDS for V, units
    std::vector<int32_t> sgrp;                   // [ns+1] first group of each slot
    std::vector<KSample> es;                     // [m]
    std::vector<KsGroup> grp;                    // scatter groups, unit after unit
    std::vector<KsUnit> units;                   // [G]
};

// The sampled k locations are cut into work units of similar sample count, each unit's samples into scatter groups of <= gcap samples of one
// slot (KS_CAPS: 32 for dense masks, 4 for sparse ones).
inline KsPlan ks_plan_units(const KsPlanIn& in) {
    const int m = in.m, ns = in.ns, s = in.s, T = in.T, max_batch = in.max_batch;
    const int32_t* const sptr = in.sptr;
    KsPlan ks;
    std::vector<int32_t> bslot, gptr;
    std::vector<int32_t>& sgrp = ks.sgrp;
    std::vector<KSample>& es = ks.es;
    std::vector<KsGroup>& grp = ks.grp;
    sgrp.assign(ns + 1, 0);
    es.assign(m, KSample{0, 0});
    // Units of similar sample count, about one per CU.  The one-launch iteration (k_ks_persist) is paced by its slowest workgroup, and two
    // workgroups that share a CU are the slow ones: where the caps allow, the cut is repeated with fewer, larger units until at most
    // 250 result (263 at the headline operator with the first cut: 7 CUs held two).
    // Round 5: four unit shapes (KS_CAPS).  A mask that samples every k a few times (EPI: 784 units of the first shape) or few k very often
    // (cut0: 604) gets the shape under which <= 256 units result, so that a slice runs the one-launch iteration too -- a slice batch as
    // well, a slice or two per launch (ks_launch_persist).  With the one-launch iteration switched off, plans for slice batches keep the
    // small shapes: their grids (units x slices) never fit the chip at once, and small units fill it more evenly.
    auto cut = [&](const KsCapsHost& cp) -> int {
        int want = 256;
        for (int attempt = 0; attempt < 8; ++attempt, want -= 8) {
            bslot.clear(); gptr.clear(); grp.clear();
            const int target = std::max(1, (m + want - 1) / want);
            int j = 0;
            while (j < ns) {
                const int first = j, e0 = sptr[j];
                int ngr = 0;
                bslot.push_back(first);
                gptr.push_back((int32_t)grp.size());
                while (j < ns) {
                    const int cnt = sptr[j + 1] - sptr[j], gj = (cnt + cp.gcap - 1) / cp.gcap;
                    if (cnt > cp.ecap || cnt > 65535) return -cnt;
                    const int have = sptr[j] - e0;
                    if (j > first && (j - first >= cp.scap || have + cnt > cp.ecap || ngr + gj > cp.gcapb || have + cnt / 2 > target)) break;
                    sgrp[j] = (int32_t)grp.size();
                    for (int e = sptr[j]; e < sptr[j + 1]; e += cp.gcap) {
                        KsGroup g;
                        g.ls = (uint16_t)(j - first); g.b = (uint16_t)(e - e0); g.e = (uint16_t)(std::min(e + cp.gcap, sptr[j + 1]) - e0); g.pad = 0;
                        grp.push_back(g);
                    }
                    for (int e = sptr[j]; e < sptr[j + 1]; ++e) { es[e].ls = (uint16_t)(j - first); es[e].t = in.ent[e].t; }
                    ngr += gj;
                    ++j;
                }
            }
            if ((int)bslot.size() <= 250 || (int)bslot.size() > 320) break;     // (> 320: an operator with many more units than CUs; nothing to gain)
        }
        return (int)bslot.size();
    };
    ks.vcap = ((T * s + 10 + 15) / 16) * 16;       // (+10: the channel loops of the kernels are unrolled to 10)
    // sparse masks (fewer than 8 samples per sampled k on average: EPI) give every scatter group of <= 4 samples to one lane; dense ones
    // (the spiral: 11 at cut3, 56 at cut0) share groups of <= 32 samples among 8 lanes (KS_CAPS)
    const bool sparse = ns > 0 && (double)m / ns < 8.0;
    int base = sparse ? 3 : 0;
    ks.caps = base;
    int nunits = cut(KS_CAPS[base]);
    if (sparse && nunits < 0) { base = 0; ks.caps = 0; nunits = cut(KS_CAPS[0]); }      // (sparse on average with one very busy location: the dense shape)
    const bool larger = (max_batch == 1 || in.one_launch) && s == 10;      // the larger shapes: only with one slice per launch or the one-launch iteration
    if (larger && (nunits > 320 || nunits < 0)) {
        const int order[2] = {sparse ? 1 : 2, sparse ? 2 : 1};
        for (int c : order) {
            if (!in.lds_fits[c]) continue;
            const int nu = cut(KS_CAPS[c]);
            // (the larger shapes run one workgroup per CU: every unit needs a CU of its own)
            if (nu > 0 && nu <= in.ncu) { ks.caps = c; nunits = nu; break; }      // (cut0: 256 units of <= 2560 samples -- k = 0 alone is sampled in all 1000 frames)
        }
        if (ks.caps == base) nunits = cut(KS_CAPS[base]);
    }
    if (nunits < 0) {
        // the limit of the shapes that were actually TRIED
        ks.tried = std::max(KS_CAPS[base].ecap, KS_CAPS[0].ecap);
        if (larger) ks.tried = std::max(ks.tried, std::max(KS_CAPS[1].ecap, KS_CAPS[2].ecap));
        ks.n = -nunits;
        ks.status = KS_PLAN_BUSY_K;
        return ks;
    }
    bslot.push_back(ns);
    gptr.push_back((int32_t)grp.size());
    sgrp[ns] = (int32_t)grp.size();
    ks.G = (int)bslot.size() - 1;
    if (!in.lds_fits[ks.caps]) {     // T = 1000, s = 10 (cut0, main_recon_tsmis_FFT.m:41-44) needs 80 KB of the CU's 160 KB; T*s <~ 14 900 fits
        ks.status = KS_PLAN_V_TOO_LARGE;
        return ks;
    }
    ks.units.resize(ks.G);
    for (int g = 0; g < ks.G; ++g) ks.units[g] = KsUnit{bslot[g], bslot[g + 1], sptr[bslot[g]], sptr[bslot[g + 1]], gptr[g], gptr[g + 1], 0, 0};
    return ks;
}

// ---------------------------------------------------------------------------------------------------
// DIRECT solver: (G_k + r I)^-1 for every sampled k, G_k = sum_{t: k in Omega_t} V(t,:)' V(t,:)   (SURVEY.md section 8 a7).
// V is T x s column-major; the result is [nsampled][s*s], symmetric, row-major, in slot order.
// ---------------------------------------------------------------------------------------------------
inline std::vector<double> direct_inverse_tables(const std::vector<double>& V, const std::vector<int32_t>& kptr_h, const std::vector<KEntry>& ent_h,
                                                 int s, int T, double r) {
    const int NM = (int)kptr_h.size() - 1;
    int nsampled = 0;
    for (int kp = 0; kp < NM; ++kp) nsampled += kptr_h[kp + 1] > kptr_h[kp];
    std::vector<double> ginv((size_t)nsampled * s * s);
    std::vector<double> G(s * s), Li(s * s);
    int slot = 0;
    for (int kp = 0; kp < NM; ++kp) {
        const int e0 = kptr_h[kp], e1 = kptr_h[kp + 1];
        if (e1 == e0) continue;
        std::fill(G.begin(), G.end(), 0.0);
        for (int e = e0; e < e1; ++e) {
            const int t = ent_h[e].t;
            for (int a = 0; a < s; ++a)
                for (int b = 0; b < s; ++b) G[a * s + b] += V[t + (size_t)T * a] * V[t + (size_t)T * b];
        }
        for (int a = 0; a < s; ++a) G[a * s + a] += r;
        // Cholesky G = L L^T, then inverse = L^-T L^-1
        for (int j = 0; j < s; ++j) {
            double d = G[j * s + j];
            for (int k = 0; k < j; ++k) d -= G[j * s + k] * G[j * s + k];
            const double ljj = std::sqrt(d);
            G[j * s + j] = ljj;
            for (int i = j + 1; i < s; ++i) {
                double v = G[i * s + j];
                for (int k = 0; k < j; ++k) v -= G[i * s + k] * G[j * s + k];
                G[i * s + j] = v / ljj;
            }
        }
        std::fill(Li.begin(), Li.end(), 0.0);
        for (int c = 0; c < s; ++c) {                 // Li = L^-1 (lower), column by column
            for (int i = c; i < s; ++i) {
                double v = (i == c) ? 1.0 : 0.0;
                for (int k = c; k < i; ++k) v -= G[i * s + k] * Li[k * s + c];
                Li[i * s + c] = v / G[i * s + i];
            }
        }
        double* out = ginv.data() + (size_t)slot * s * s;
        for (int a = 0; a < s; ++a)
            for (int b = 0; b < s; ++b) {
                double v = 0.0;
                for (int k = std::max(a, b); k < s; ++k) v += Li[k * s + a] * Li[k * s + b];
                out[a * s + b] = v;
            }
        ++slot;
    }
    return ginv;
}
#endif
