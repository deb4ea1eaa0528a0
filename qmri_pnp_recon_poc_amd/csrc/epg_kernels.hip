// epg_kernels.hip -- extended-phase-graph simulation of a FISP-MRF dictionary in fp64: an EXTENSION with no reference counterpart (the reference
// loads dictionaries that are already simulated and compressed).  Definition: include/qmri.h, DESIGN.md section 19.
//
// States across lanes: a group of G lanes owns one atom, lane j of the group keeps the R consecutive configuration states n = j R .. j R + R - 1
// of F+, F-, Z in registers (3 R doubles; S <= G R, the states >= S are held at zero).  RF and relaxation are local to a state; the spoiler is a
// register rename inside a lane plus one double from the lane below (F+) and one from the lane above (F-): DPP row shifts when the group is one
// 16-lane row (G = 16), __shfl_up / __shfl_down of width G beyond.  A group never spans two waves (G <= 64).
//   k_epg<G, R>         a workgroup of NT lanes simulates APW = NT / G atoms, FB frames at a time.  Per block of frames lane j < FB of a group
//                       computes that frame's cos / sin of alpha_t b1 (and, when TR / TE vary from frame to frame, its four exponentials) once and
//                       leaves them in LDS, so a transcendental costs 1 / FB per lane and frame; lane 0 of each group stages the signal F+_0 in LDS,
//                       and after the block the workgroup writes FB x APW values, APW atoms contiguous per frame (8 at S = 32: 64 B).
//   k_epg_sp<G, R>      the same per (atom, sub-slice of a slice profile), the weighted sum over the sub-slices taken in LDS (see its comment).
//   k_epg_grad<G, R, P> k_epg with P tangents beside the state and the Cramer-Rao bound of the 1 + P signals in the same launch (see its comment).
//   k_epg_seq<G, R>     k_epg walked over a schedule of blocks (wait, preparation, frames) played several times (see its comment).
//   k_epg_shift<G, R>   the spoiler alone, n times on one atom's given state (qmri_debug_epg_shift: exact-integer test of the lane moves).
// No atomics, no reduction across atoms: equal inputs give equal bits.
#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>
#include "epg_seq_plan.h"
#include "qmri_internal.h"

namespace {
constexpr int NT = 256;          // threads per workgroup
constexpr int FB = 16;           // frames per block (<= the smallest G)
constexpr int NQ = 6;            // doubles per atom and frame in LDS: cos, sin, E1(TE), E2(TE), E1(TR - TE), E2(TR - TE)
constexpr int ROW = FB * NQ + 2; // LDS row stride per atom in doubles (784 B: 16-byte aligned, the groups of a wave fall in distinct banks)
constexpr int EPG_SP_MAX_T = 1024; // frames k_epg_sp's pass accumulator holds (the T limit of the entry points)

// v of the lane `d` below (d = +1) or above (d = -1) within a 16-lane row, zero past the row's ends
template <int D> __device__ __forceinline__ double row_move(double v) {
    constexpr int ctrl = D > 0 ? 0x111 : 0x101;              // row_shr:1 / row_shl:1
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// one dephasing unit.  j: the lane's index in its group; S: the number of states kept
template <int G, int R> __device__ __forceinline__ void epg_shift(double (&fp)[R], double (&fm)[R], int j, int S) {
    double up, dn;                                           // F+ of the state below this lane's first, F- of the state above its last
    if constexpr (G == 16) {
        up = row_move<+1>(fp[R - 1]);
        dn = row_move<-1>(fm[0]);
    } else {
        up = __shfl_up(fp[R - 1], 1, G);
        dn = __shfl_down(fm[0], 1, G);
        if (j == G - 1) dn = 0.0;
    }
#pragma unroll
    for (int r = R - 1; r >= 1; --r) fp[r] = fp[r - 1];
#pragma unroll
    for (int r = 0; r + 1 < R; ++r) fm[r] = fm[r + 1];
    fm[R - 1] = dn;
    fp[0] = j == 0 ? fm[0] : up;                             // F+_0 <- old F-_1 (= the new F-_0)
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (j * R + r >= S) fp[r] = 0.0;                     // the old F+_{S-1} is dropped; F- and Z of the padding are never fed
}

// step 1 on one state: the rotated (F+, F-, Z), all three from the old values (k_epg_grad's tangents; epg_frame states the same for the state)
__device__ __forceinline__ void epg_rf(double p, double m, double zz, double c, double s, double c2, double s2, double& up, double& um, double& uz) {
    up = c2 * p - s2 * m + s * zz;
    um = -s2 * p + c2 * m + s * zz;
    uz = -0.5 * s * (p + m) + c * zz;
}

// The primal recursion of one frame on the R states of a lane, steps 1 to 5: the one statement of it, shared by k_epg and k_epg_grad, so that the
// two give the same bits.  stage(): called on lane 0 of the group when F+_0 is the signal (step 3); mid(): called on every lane between steps 3
// and 4 (k_epg_grad's tangents read the state there; k_epg has nothing to do)
template <int G, int R, typename Stage, typename Mid>
__device__ __forceinline__ void epg_frame(double (&fp)[R], double (&fm)[R], double (&z)[R], double c, double s, double c2, double s2, double ea1,
                                          double ea2, double eb1, double eb2, int j, int S, Stage&& stage, Mid&& mid) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double p = fp[r], m = fm[r], zz = z[r];
        fp[r] = (c2 * p - s2 * m + s * zz) * ea2;
        fm[r] = (-s2 * p + c2 * m + s * zz) * ea2;
        z[r] = (-0.5 * s * (p + m) + c * zz) * ea1;
    }
    if (j == 0) {
        z[0] += 1.0 - ea1;
        stage();
    }
    mid();
#pragma unroll
    for (int r = 0; r < R; ++r) { fp[r] *= eb2; fm[r] *= eb2; z[r] *= eb1; }
    if (j == 0) z[0] += 1.0 - eb1;
    epg_shift<G, R>(fp, fm, j, S);
}

template <int G, int R>
__global__ void __launch_bounds__(NT) k_epg(const double* __restrict__ sched, int T, int K, int S, const double* __restrict__ t1, const double* __restrict__ t2,
                                            const double* __restrict__ b1, int inversion, double ti, double inv_eff, int const_timing,
                                            void* __restrict__ Fout, int out_f64) {
    constexpr int APW = NT / G;
    __shared__ __attribute__((aligned(16))) double sc[APW * ROW];
    __shared__ double sig[FB * APW];
    const double *alpha = sched, *tr = sched + T, *te = sched + 2 * T;
    const int tid = threadIdx.x, g = tid / G, j = tid % G;
    const long long k0 = (long long)blockIdx.x * APW;
    const long long k = k0 + g < K ? k0 + g : (long long)K - 1;                  // the lanes past K repeat the last atom and store nothing
    double T1 = t1[k], T2 = t2[k], B1 = b1 ? b1[k] : 1.0;
    const double inf = std::numeric_limits<double>::infinity();
    const bool bad = !(T1 > 0.0 && T1 < inf && T2 > 0.0 && T2 < inf && B1 >= 0.0 && B1 < inf);
    if (bad) { T1 = 1.0; T2 = 1.0; B1 = 1.0; }                                   // its row becomes NaN at the store
    double fp[R], fm[R], z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) fp[r] = fm[r] = z[r] = 0.0;
    if (j == 0) {
        z[0] = 1.0;
        if (inversion) {
            const double e = exp(-ti / T1);
            z[0] = (-inv_eff * z[0]) * e + (1.0 - e);
        }
    }
    double ea1 = 0.0, ea2 = 0.0, eb1 = 0.0, eb2 = 0.0;
    if (const_timing) {
        const double a = te[0], b = tr[0] - te[0];
        ea1 = exp(-a / T1); ea2 = exp(-a / T2); eb1 = exp(-b / T1); eb2 = exp(-b / T2);
    }
    double* my = sc + g * ROW;
    for (int t0 = 0; t0 < T; t0 += FB) {
        const int nf = min(FB, T - t0);
        __syncthreads();                                     // the previous block's sc and sig have been read
        if (j < nf) {
            double s, c;
            sincos(alpha[t0 + j] * B1, &s, &c);
            my[j * NQ + 0] = c;
            my[j * NQ + 1] = s;
            if (!const_timing) {
                const double a = te[t0 + j], b = tr[t0 + j] - a;
                my[j * NQ + 2] = exp(-a / T1);
                my[j * NQ + 3] = exp(-a / T2);
                my[j * NQ + 4] = exp(-b / T1);
                my[j * NQ + 5] = exp(-b / T2);
            }
        }
        __syncthreads();
        for (int tt = 0; tt < nf; ++tt) {
            const double2 cs = *reinterpret_cast<const double2*>(my + tt * NQ);
            const double c = cs.x, s = cs.y, c2 = (1.0 + c) * 0.5, s2 = (1.0 - c) * 0.5;
            if (!const_timing) {
                const double2 ea = *reinterpret_cast<const double2*>(my + tt * NQ + 2), eb = *reinterpret_cast<const double2*>(my + tt * NQ + 4);
                ea1 = ea.x; ea2 = ea.y; eb1 = eb.x; eb2 = eb.y;
            }
            epg_frame<G, R>(fp, fm, z, c, s, c2, s2, ea1, ea2, eb1, eb2, j, S,
                            [&] { sig[tt * APW + g] = bad ? std::numeric_limits<double>::quiet_NaN() : fp[0]; }, [] {});
        }
        __syncthreads();
        if (tid < nf * APW) {                                // FB * APW <= NT: one value per lane, the atoms of a frame contiguous
            const int tt = tid / APW, a = tid % APW;
            if (k0 + a < K) {
                const size_t o = (size_t)(t0 + tt) * (size_t)K + (size_t)(k0 + a);
                if (out_f64) static_cast<double*>(Fout)[o] = sig[tid];
                else static_cast<float*>(Fout)[o] = (float)sig[tid];
            }
        }
    }
}

// The slice-profile-aware simulation: the work item is the pair (atom, sub-slice q), one group of G lanes per pair with
// k_epg's scheme unchanged; the RF argument is (alpha_t b1) prof[t, q].  sched: T frame records (alpha_t, tr_t, te_t, prof[t, 0 .. Q-1]), then
// weight [Q].
// A workgroup holds GPW = NT / G groups.  Q <= GPW: it simulates A = GPW / Q atoms in one pass, group g = a Q + q (the GPW - A Q groups left
// over repeat a valid pair and their staged signals are never read).  Q > GPW: it simulates one atom in ceil(Q / GPW) passes of GPW sub-slices,
// each pass over the whole train, and carries the partial sums of the T frames in the LDS array acc, which it alone reads and writes.  Per frame
// block one lane per (frame, atom) adds w_q x the staged signals in ascending q (from 0 in the first pass, from acc afterwards) and the last pass
// stores: every output is written once, without atomics, and an atom's bits depend on Q and S only.
// Scalar registers are the scarce resource of this loop nest (sincos and exp keep their constants in them): the kernel is compiled once per
// timing kind (CT), keeps the bad-atom flag and the reducing lanes' addresses in vector registers, and re-reads S from LDS in every frame so that
// epg_shift's R padding masks are not kept in scalar registers across the loops.  With that no instantiation spills.
template <int G, int R, bool CT>                           // CT: TR and TE are the same in every frame
__global__ void __launch_bounds__(NT) k_epg_sp(const double* __restrict__ sched, int T, int K, int S, int Q, const double* __restrict__ t1,
                                               const double* __restrict__ t2, const double* __restrict__ b1, int inversion, double ti, double inv_eff,
                                               void* __restrict__ Fout, int out_f64) {
    constexpr int GPW = NT / G;
    __shared__ __attribute__((aligned(16))) double sc[GPW * ROW];
    __shared__ double sig[FB * GPW];
    __shared__ double acc[EPG_SP_MAX_T];
    __shared__ double wl[64];
    __shared__ int nkeep;                                    // S (see above)
    const int FR = 3 + Q;                                    // doubles per frame record
    const int QP = min(Q, GPW), A = GPW / QP;                // sub-slices per pass, atoms per workgroup (1 when Q > GPW)
    const int tid = threadIdx.x, g = tid / G, j = tid % G, ql = g % QP;
    const int k0 = blockIdx.x * A;                                               // < K <= 2^30
    const int k = min(k0 + min(g / QP, A - 1), K - 1);                           // the groups past A, K or Q repeat a valid pair and are never read
    double T1 = t1[k], T2 = t2[k], B1 = b1 ? b1[k] : 1.0;
    const double inf = std::numeric_limits<double>::infinity();
    const bool bad = !(T1 > 0.0 && T1 < inf && T2 > 0.0 && T2 < inf && B1 >= 0.0 && B1 < inf);
    if (bad) { T1 = 1.0; T2 = 1.0; B1 = 1.0; }                                   // its row becomes NaN at the store: w_q NaN is NaN for every w_q
    const int nanbits = bad ? -1 : 0;                                            // or-ed into the staged signal: all ones is a NaN
    double ea1 = 0.0, ea2 = 0.0, eb1 = 0.0, eb2 = 0.0;
    if constexpr (CT) {
        const double a = sched[2], b = sched[1] - a;
        ea1 = exp(-a / T1); ea2 = exp(-a / T2); eb1 = exp(-b / T1); eb2 = exp(-b / T2);
    }
    double z0 = 0.0;                                         // Z_0 before the first frame (lane 0 of a group), the same in every pass
    if (j == 0) {
        z0 = 1.0;
        if (inversion) {
            const double e = exp(-ti / T1);
            z0 = (-inv_eff * z0) * e + (1.0 - e);
        }
    }
    if (tid == 0) nkeep = S;
    if (tid < Q) wl[tid] = sched[(size_t)T * FR + tid];                         // read after the first __syncthreads()
    // the reducing lanes: lane tid < FB A sums frame tid / A of atom tid % A of every block (FB A <= NT); the lanes past K never pass rt < nf
    const int ra = tid % A, rt = k0 + ra < K ? tid / A : FB;
    const double* sg = sig + min(rt, FB - 1) * GPW + ra * QP;
    const size_t esz = out_f64 ? sizeof(double) : sizeof(float), ostep = (size_t)FB * (size_t)K * esz;
    char* const out0 = static_cast<char*>(Fout) + ((size_t)min(rt, FB - 1) * (size_t)K + (size_t)(k0 + ra)) * esz;      // this lane's frame of block 0
    double* my = sc + g * ROW;
    for (int q0 = 0; q0 < Q; q0 += QP) {                     // one pass
        const int nq = min(QP, Q - q0), q = min(q0 + ql, Q - 1);
        double fp[R], fm[R], z[R];
#pragma unroll
        for (int r = 0; r < R; ++r) fp[r] = fm[r] = z[r] = 0.0;
        z[0] = z0;
        char* out = out0;
        for (int t0 = 0; t0 < T; t0 += FB) {
            const int nf = min(FB, T - t0);
            __syncthreads();                                 // the previous block's sc and sig have been read
            if (j < nf) {
                const double* fr = sched + (t0 + j) * FR;
                double s, c;
                sincos((fr[0] * B1) * fr[3 + q], &s, &c);
                my[j * NQ + 0] = c;
                my[j * NQ + 1] = s;
                if constexpr (!CT) {
                    const double a = fr[2], b = fr[1] - a;
                    my[j * NQ + 2] = exp(-a / T1);
                    my[j * NQ + 3] = exp(-a / T2);
                    my[j * NQ + 4] = exp(-b / T1);
                    my[j * NQ + 5] = exp(-b / T2);
                }
            }
            __syncthreads();
            for (int tt = 0; tt < nf; ++tt) {
                const double2 cs = *reinterpret_cast<const double2*>(my + tt * NQ);
                const double c = cs.x, s = cs.y, c2 = (1.0 + c) * 0.5, s2 = (1.0 - c) * 0.5;
                if constexpr (!CT) {
                    const double2 ea = *reinterpret_cast<const double2*>(my + tt * NQ + 2), eb = *reinterpret_cast<const double2*>(my + tt * NQ + 4);
                    ea1 = ea.x; ea2 = ea.y; eb1 = eb.x; eb2 = eb.y;
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double p = fp[r], m = fm[r], zz = z[r];
                    fp[r] = (c2 * p - s2 * m + s * zz) * ea2;
                    fm[r] = (-s2 * p + c2 * m + s * zz) * ea2;
                    z[r] = (-0.5 * s * (p + m) + c * zz) * ea1;
                }
                if (j == 0) {
                    z[0] += 1.0 - ea1;
                    sig[tt * GPW + g] = __hiloint2double(__double2hiint(fp[0]) | nanbits, __double2loint(fp[0]) | nanbits);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) { fp[r] *= eb2; fm[r] *= eb2; z[r] *= eb1; }
                if (j == 0) z[0] += 1.0 - eb1;
                epg_shift<G, R>(fp, fm, j, nkeep);
            }
            __syncthreads();
            if (rt < nf) {                                   // the atoms of a frame contiguous
                double v = q0 ? acc[t0 + rt] : 0.0;          // written by this lane in the pass before (A = 1: rt = tid)
                for (int i = 0; i < nq; ++i) v += wl[q0 + i] * sg[i];
                if (q0 + QP < Q) acc[t0 + rt] = v;
                else if (out_f64) *reinterpret_cast<double*>(out) = v;
                else *reinterpret_cast<float*>(out) = (float)v;
            }
            out += ostep;
        }
    }
}

// The fingerprint with its derivatives and their Cramer-Rao bound: k_epg's scheme with P tangents (T1, T2 and, P = 3, b1)
// beside the state, 3 R (1 + P) doubles per lane.  A tangent takes the rotation, the scaling and the lane moves of the state; the extra terms are
// local to a configuration state.  Per frame lane j < FB leaves eleven numbers in LDS: cos, sin, the four exponentials, their four derivatives
// E dt / T^2 and alpha_t.  Lane 0 of a group stages 1 + P signals; after a block of frames the workgroup stores those whose pointer is given, and
// the bound's sums advance in ascending t: with V (sv > 0) lane j < sv of the group keeps the 1 + P projections sum_t V[t, j] sig_q[t], without
// lane e < (1 + P)(2 + P) / 2 keeps one entry of the Gram matrix.  After the last frame lane 0 of the group forms G (j ascending), normalises it
// to a unit diagonal, factorises and writes crb [1 + P] and the flag (0; 1 SINGULAR: every bound +inf; 2 an atom the device route could not
// refuse: NaN).  No atomics; an atom's bits depend neither on K nor on its position.  sched: alpha [T], tr [T], te [T], then V [T x sv].
constexpr int NQG = 12;             // doubles per atom and frame in LDS (the eleven above and one of padding: rows of double2)
constexpr int ROWG = FB * NQG + 2;  // LDS row stride per atom (1552 B: 16-byte aligned, the groups of a wave fall in distinct banks)
constexpr double CRB_PIVOT_MIN = 1e-10;

template <int G, int R, int P>
__global__ void __launch_bounds__(NT) k_epg_grad(const double* __restrict__ sched, int T, int K, int S, int sv, const double* __restrict__ t1,
                                                 const double* __restrict__ t2, const double* __restrict__ b1, int inversion, double ti, double inv_eff,
                                                 int const_timing, void* __restrict__ Fout, void* __restrict__ dFout, int out_f64,
                                                 double* __restrict__ crb, int32_t* __restrict__ flags) {
    constexpr int APW = NT / G, NS = 1 + P, NE = NS * (NS + 1) / 2;
    static_assert(ROWG >= 16 * NS && NE <= 16, "the bound's hand-over fits an atom's LDS row");
    __shared__ __attribute__((aligned(16))) double sc[APW * ROWG];
    __shared__ double sig[NS * FB * APW];
    const double *alpha = sched, *tr = sched + T, *te = sched + 2 * T, *V = sched + 3 * T;
    const int tid = threadIdx.x, g = tid / G, j = tid % G;
    const long long k0 = (long long)blockIdx.x * APW;
    const long long k = k0 + g < K ? k0 + g : (long long)K - 1;                  // the lanes past K repeat the last atom and store nothing
    double T1 = t1[k], T2 = t2[k], B1 = b1 ? b1[k] : 1.0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const bool bad = !(T1 > 0.0 && T1 < inf && T2 > 0.0 && T2 < inf && B1 >= 0.0 && B1 < inf);
    if (bad) { T1 = 1.0; T2 = 1.0; B1 = 1.0; }                                   // its rows and its bound become NaN at the stores
    const double r1 = 1.0 / (T1 * T1), r2 = 1.0 / (T2 * T2);                     // E' = E (dt r): one division per atom, an ulp from E dt / T^2
    double fp[R], fm[R], z[R], dfp[P][R], dfm[P][R], dz[P][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        fp[r] = fm[r] = z[r] = 0.0;
#pragma unroll
        for (int q = 0; q < P; ++q) dfp[q][r] = dfm[q][r] = dz[q][r] = 0.0;
    }
    if (j == 0) {
        z[0] = 1.0;
        if (inversion) {
            const double e = exp(-ti / T1), de = e * (ti * r1);
            z[0] = (-inv_eff * z[0]) * e + (1.0 - e);
            dz[0][0] = (-inv_eff) * de - de;
        }
    }
    double ea1 = 0.0, ea2 = 0.0, eb1 = 0.0, eb2 = 0.0, da1 = 0.0, da2 = 0.0, db1 = 0.0, db2 = 0.0;
    if (const_timing) {
        const double a = te[0], b = tr[0] - te[0];
        ea1 = exp(-a / T1); ea2 = exp(-a / T2); eb1 = exp(-b / T1); eb2 = exp(-b / T2);
        da1 = ea1 * (a * r1); da2 = ea2 * (a * r2); db1 = eb1 * (b * r1); db2 = eb2 * (b * r2);
    }
    // the bound's running sums: the projections of the 1 + P signals on column j of V, or (acc[0]) the Gram entry (ga, gb) of lane j < NE
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
    int ga = 0, gb = 0;
    for (int a = 0, e = 0; a < NS; ++a)
        for (int b = a; b < NS; ++b, ++e)
            if (e == j) { ga = a; gb = b; }
    double* my = sc + g * ROWG;
    for (int t0 = 0; t0 < T; t0 += FB) {
        const int nf = min(FB, T - t0);
        __syncthreads();                                     // the previous block's sc and sig have been read
        if (j < nf) {
            double s, c;
            sincos(alpha[t0 + j] * B1, &s, &c);
            my[j * NQG + 0] = c;
            my[j * NQG + 1] = s;
            my[j * NQG + 10] = alpha[t0 + j];
            if (!const_timing) {
                const double a = te[t0 + j], b = tr[t0 + j] - a;
                const double xa1 = exp(-a / T1), xa2 = exp(-a / T2), xb1 = exp(-b / T1), xb2 = exp(-b / T2);
                my[j * NQG + 2] = xa1;
                my[j * NQG + 3] = xa2;
                my[j * NQG + 4] = xb1;
                my[j * NQG + 5] = xb2;
                my[j * NQG + 6] = xa1 * (a * r1);
                my[j * NQG + 7] = xa2 * (a * r2);
                my[j * NQG + 8] = xb1 * (b * r1);
                my[j * NQG + 9] = xb2 * (b * r2);
            }
        }
        __syncthreads();
        for (int tt = 0; tt < nf; ++tt) {
            const double2 cs = *reinterpret_cast<const double2*>(my + tt * NQG);
            const double c = cs.x, s = cs.y, c2 = (1.0 + c) * 0.5, s2 = (1.0 - c) * 0.5;
            if (!const_timing) {
                const double2 ea = *reinterpret_cast<const double2*>(my + tt * NQG + 2), eb = *reinterpret_cast<const double2*>(my + tt * NQG + 4);
                const double2 da = *reinterpret_cast<const double2*>(my + tt * NQG + 6), db = *reinterpret_cast<const double2*>(my + tt * NQG + 8);
                ea1 = ea.x; ea2 = ea.y; eb1 = eb.x; eb2 = eb.y;
                da1 = da.x; da2 = da.y; db1 = db.x; db2 = db.y;
            }
            // steps 1 and 2 of the tangents, from the state before the pulse (p, m, zz) and after it (up, um, uz)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double p = fp[r], m = fm[r], zz = z[r];
                double up, um, uz;
                epg_rf(p, m, zz, c, s, c2, s2, up, um, uz);
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    double vp, vm, vz;
                    epg_rf(dfp[q][r], dfm[q][r], dz[q][r], c, s, c2, s2, vp, vm, vz);
                    if (q == 2) {
                        const double al = my[tt * NQG + 10], xy = al * (-(0.5 * s) * (p + m) + c * zz);
                        vp += xy;
                        vm += xy;
                        vz += al * (-(0.5 * c) * (p + m) - s * zz);
                    }
                    vp *= ea2; vm *= ea2; vz *= ea1;
                    if (q == 1) { vp += da2 * up; vm += da2 * um; }
                    if (q == 0) vz += da1 * uz;
                    dfp[q][r] = vp; dfm[q][r] = vm; dz[q][r] = vz;
                }
            }
            if (j == 0) dz[0][0] -= da1;
            epg_frame<G, R>(
                fp, fm, z, c, s, c2, s2, ea1, ea2, eb1, eb2, j, S,
                [&] {
                    sig[tt * APW + g] = bad ? nan : fp[0];
#pragma unroll
                    for (int q = 0; q < P; ++q) sig[((1 + q) * FB + tt) * APW + g] = bad ? nan : dfp[q][0];
                },
                [&] {                                        // step 4 of the tangents, from the state before its scaling
#pragma unroll
                    for (int r = 0; r < R; ++r) {
#pragma unroll
                        for (int q = 0; q < P; ++q) {
                            double vp = dfp[q][r] * eb2, vm = dfm[q][r] * eb2, vz = dz[q][r] * eb1;
                            if (q == 1) { vp += db2 * fp[r]; vm += db2 * fm[r]; }
                            if (q == 0) vz += db1 * z[r];
                            dfp[q][r] = vp; dfm[q][r] = vm; dz[q][r] = vz;
                        }
                    }
                    if (j == 0) dz[0][0] -= db1;
                });
#pragma unroll
            for (int q = 0; q < P; ++q) epg_shift<G, R>(dfp[q], dfm[q], j, S);
        }
        __syncthreads();
        if (tid < nf * APW) {                                // FB * APW <= NT: one value per lane and signal, the atoms of a frame contiguous
            const int tt = tid / APW, a = tid % APW;
            if (k0 + a < K) {
                const size_t o = (size_t)(t0 + tt) * (size_t)K + (size_t)(k0 + a), KT = (size_t)K * (size_t)T;
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    void* out = q == 0 ? Fout : dFout;
                    if (!out) continue;
                    const size_t oq = q == 0 ? o : o + (size_t)(q - 1) * KT;
                    const double v = sig[q * FB * APW + tid];
                    if (out_f64) static_cast<double*>(out)[oq] = v;
                    else static_cast<float*>(out)[oq] = (float)v;
                }
            }
        }
        if (crb) {
            if (sv > 0) {
                if (j < sv)
                    for (int tt = 0; tt < nf; ++tt) {
                        const double v = V[(size_t)j * T + (t0 + tt)];
#pragma unroll
                        for (int q = 0; q < NS; ++q) acc[q] += v * sig[(q * FB + tt) * APW + g];
                    }
            } else if (j < NE) {
                for (int tt = 0; tt < nf; ++tt) acc[0] += sig[(ga * FB + tt) * APW + g] * sig[(gb * FB + tt) * APW + g];
            }
        }
    }
    if (!crb) return;
    // hand the sums to lane 0 of the group through the atom's LDS row (its last reader passed the barrier that follows the frame loop)
    if (sv > 0) {
        if (j < sv) {
#pragma unroll
            for (int q = 0; q < NS; ++q) my[j * NS + q] = acc[q];
        }
    } else if (j < NE) {
        my[j] = acc[0];
    }
    __syncthreads();
    if (j != 0 || k0 + g >= K) return;
    double Gm[NS][NS];
    if (sv > 0) {
#pragma unroll
        for (int a = 0; a < NS; ++a)
#pragma unroll
            for (int b = a; b < NS; ++b) {
                double v = 0.0;
                for (int i = 0; i < sv; ++i) v += my[i * NS + a] * my[i * NS + b];
                Gm[a][b] = Gm[b][a] = v;
            }
    } else {
        int e = 0;
#pragma unroll
        for (int a = 0; a < NS; ++a)
#pragma unroll
            for (int b = a; b < NS; ++b, ++e) Gm[a][b] = Gm[b][a] = my[e];
    }
    // d = sqrt(diag G), Gn = G / (d d^T), Gn = L L^T; a diagonal entry or a pivot that fails is SINGULAR
    bool sing = false;
    double d[NS], L[NS][NS], Li[NS][NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
        sing = sing || !(Gm[a][a] > 0.0 && Gm[a][a] < inf);
        d[a] = sqrt(Gm[a][a]);
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        double pv = Gm[c][c] / (d[c] * d[c]);
#pragma unroll
        for (int i = 0; i < c; ++i) pv -= L[c][i] * L[c][i];
        sing = sing || !(pv > CRB_PIVOT_MIN && pv < inf);
        L[c][c] = sqrt(pv);
#pragma unroll
        for (int a = c + 1; a < NS; ++a) {
            double v = Gm[a][c] / (d[a] * d[c]);
#pragma unroll
            for (int i = 0; i < c; ++i) v -= L[a][i] * L[c][i];
            L[a][c] = v / L[c][c];
        }
    }
    // [Gn^-1]_qq = sum_{i >= q} (L^-1)_iq^2, L^-1 by forward substitution
    double* out = crb + (size_t)(k0 + g) * NS;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        Li[q][q] = 1.0 / L[q][q];
        double v = Li[q][q] * Li[q][q];
#pragma unroll
        for (int a = q + 1; a < NS; ++a) {
            double w = 0.0;
#pragma unroll
            for (int i = q; i < a; ++i) w -= L[a][i] * Li[i][q];
            Li[a][q] = w / L[a][a];
            v += Li[a][q] * Li[a][q];
        }
        out[q] = bad ? nan : sing ? inf : v / (d[q] * d[q]);
    }
    flags[k0 + g] = bad ? 2 : sing ? 1 : 0;
}

// Prepared, repeated trains: k_epg's scheme, walked over a schedule.  segs: the nseg segments of epg_seq_plan.h, each at
// most FB frames of one block with the block's event in front of its first segment; the list is played ncycles times from one equilibrium start
// and only the last cycle stages and stores.  An event is applied by every lane on its own states from two or three exponentials it computes
// itself (an event is once per block, a frame's transcendentals are shared through LDS as in k_epg):
//   wait            F+- <- F+- exp(-wait / T2), Z <- Z exp(-wait / T1), Z_0 += 1 - exp(-wait / T1)
//   inversion       Z <- (-eff Z) e, Z_0 <- (-eff Z_0) e + (1 - e) with e = exp(-TI / T1) -- the expression of k_epg's inversion --, F+- <- 0
//   T2 preparation  Z <- (eff Z) exp(-prep_time / T2), F+- <- 0
// The segment record is read with scalar loads (it is the same for every lane), so the branches on it are uniform.  One block {T, inversion} or
// {T, none} in one cycle runs the instructions of k_epg on the same numbers: the same bits.
template <int G, int R>
__global__ void __launch_bounds__(NT) k_epg_seq(const double* __restrict__ sched, const epgseq::Segment* __restrict__ segs, int nseg, int ncycles, int T,
                                                int K, int S, const double* __restrict__ t1, const double* __restrict__ t2,
                                                const double* __restrict__ b1, int const_timing, void* __restrict__ Fout, int out_f64) {
    constexpr int APW = NT / G;
    __shared__ __attribute__((aligned(16))) double sc[APW * ROW];
    __shared__ double sig[FB * APW];
    const double *alpha = sched, *tr = sched + T, *te = sched + 2 * T;
    const int tid = threadIdx.x, g = tid / G, j = tid % G;
    const long long k0 = (long long)blockIdx.x * APW;
    const long long k = k0 + g < K ? k0 + g : (long long)K - 1;                  // the lanes past K repeat the last atom and store nothing
    double T1 = t1[k], T2 = t2[k], B1 = b1 ? b1[k] : 1.0;
    const double inf = std::numeric_limits<double>::infinity();
    const bool bad = !(T1 > 0.0 && T1 < inf && T2 > 0.0 && T2 < inf && B1 >= 0.0 && B1 < inf);
    if (bad) { T1 = 1.0; T2 = 1.0; B1 = 1.0; }                                   // its row becomes NaN at the store
    double fp[R], fm[R], z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) fp[r] = fm[r] = z[r] = 0.0;
    if (j == 0) z[0] = 1.0;
    double ea1 = 0.0, ea2 = 0.0, eb1 = 0.0, eb2 = 0.0;
    if (const_timing) {
        const double a = te[0], b = tr[0] - te[0];
        ea1 = exp(-a / T1); ea2 = exp(-a / T2); eb1 = exp(-b / T1); eb2 = exp(-b / T2);
    }
    double* my = sc + g * ROW;
    for (int cyc = 0; cyc < ncycles; ++cyc) {
        const bool rec = cyc == ncycles - 1;
        for (int si = 0; si < nseg; ++si) {
            const int t0 = segs[si].t0, nf = segs[si].nf, prep = segs[si].prep;
            const double wait = segs[si].wait;
            if (wait > 0.0) {
                const double w1 = exp(-wait / T1), w2 = exp(-wait / T2);
#pragma unroll
                for (int r = 0; r < R; ++r) { fp[r] *= w2; fm[r] *= w2; z[r] *= w1; }
                if (j == 0) z[0] += 1.0 - w1;
            }
            if (prep == epgseq::PREP_INVERSION) {
                const double eff = segs[si].prep_eff, e = exp(-segs[si].prep_time / T1);
#pragma unroll
                for (int r = 1; r < R; ++r) z[r] = (-eff * z[r]) * e;
                if (j == 0) z[0] = (-eff * z[0]) * e + (1.0 - e);
                else z[0] = (-eff * z[0]) * e;
#pragma unroll
                for (int r = 0; r < R; ++r) fp[r] = fm[r] = 0.0;
            } else if (prep == epgseq::PREP_T2) {
                const double eff = segs[si].prep_eff, e2 = exp(-segs[si].prep_time / T2);
#pragma unroll
                for (int r = 0; r < R; ++r) { z[r] = (eff * z[r]) * e2; fp[r] = fm[r] = 0.0; }
            }
            __syncthreads();                                 // the previous segment's sc and sig have been read
            if (j < nf) {
                double s, c;
                sincos(alpha[t0 + j] * B1, &s, &c);
                my[j * NQ + 0] = c;
                my[j * NQ + 1] = s;
                if (!const_timing) {
                    const double a = te[t0 + j], b = tr[t0 + j] - a;
                    my[j * NQ + 2] = exp(-a / T1);
                    my[j * NQ + 3] = exp(-a / T2);
                    my[j * NQ + 4] = exp(-b / T1);
                    my[j * NQ + 5] = exp(-b / T2);
                }
            }
            __syncthreads();
            for (int tt = 0; tt < nf; ++tt) {
                const double2 cs = *reinterpret_cast<const double2*>(my + tt * NQ);
                const double c = cs.x, s = cs.y, c2 = (1.0 + c) * 0.5, s2 = (1.0 - c) * 0.5;
                if (!const_timing) {
                    const double2 ea = *reinterpret_cast<const double2*>(my + tt * NQ + 2), eb = *reinterpret_cast<const double2*>(my + tt * NQ + 4);
                    ea1 = ea.x; ea2 = ea.y; eb1 = eb.x; eb2 = eb.y;
                }
                epg_frame<G, R>(fp, fm, z, c, s, c2, s2, ea1, ea2, eb1, eb2, j, S,
                                [&] { sig[tt * APW + g] = bad ? std::numeric_limits<double>::quiet_NaN() : fp[0]; }, [] {});
            }
            if (!rec) continue;                              // uniform: the cycles before the last one store nothing
            __syncthreads();
            if (tid < nf * APW) {                            // FB * APW <= NT: one value per lane, the atoms of a frame contiguous
                const int tt = tid / APW, a = tid % APW;
                if (k0 + a < K) {
                    const size_t o = (size_t)(t0 + tt) * (size_t)K + (size_t)(k0 + a);
                    if (out_f64) static_cast<double*>(Fout)[o] = sig[tid];
                    else static_cast<float*>(Fout)[o] = (float)sig[tid];
                }
            }
        }
    }
}

// st: F+ [S], F- [S], Z [S] of one atom; one group of one wave does the work
template <int G, int R> __global__ void __launch_bounds__(64) k_epg_shift(int S, int nshift, const double* __restrict__ in, double* __restrict__ out) {
    const int lane = threadIdx.x, j = lane % G;
    double fp[R], fm[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = j * R + r;
        fp[r] = n < S ? in[n] : 0.0;
        fm[r] = n < S ? in[S + n] : 0.0;
    }
    for (int i = 0; i < nshift; ++i) epg_shift<G, R>(fp, fm, j, S);
    if (lane >= G) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = j * R + r;
        if (n < S) { out[n] = fp[r]; out[S + n] = fm[r]; out[2 * S + n] = in[2 * S + n]; }
    }
}

// (G, R) for S states: (16,1), (32,1), (64,1), (64,2), (64,4)
template <typename Fn> void epg_dispatch(int S, Fn&& fn) {
    if (S <= 16) fn(std::integral_constant<int, 16>(), std::integral_constant<int, 1>());
    else if (S <= 32) fn(std::integral_constant<int, 32>(), std::integral_constant<int, 1>());
    else if (S <= 64) fn(std::integral_constant<int, 64>(), std::integral_constant<int, 1>());
    else if (S <= 128) fn(std::integral_constant<int, 64>(), std::integral_constant<int, 2>());
    else fn(std::integral_constant<int, 64>(), std::integral_constant<int, 4>());
}
}  // namespace

int epg_atoms_per_workgroup(int S) {
    int apw = 0;
    epg_dispatch(S, [&](auto g, auto) { apw = NT / decltype(g)::value; });
    return apw;
}

int epg_simulate_dev(qmri_ctx* ctx, int K, int T, const double* d_sched, const double* d_t1, const double* d_t2, const double* d_b1,
                     const qmri_epg_params& p, bool const_timing, void* d_F) {
    static_assert(FB * (NT / 16) <= NT && FB <= 16, "one staged value per lane; a frame block fits the smallest group");
    epg_dispatch(p.nstates, [&](auto g, auto r) {
        constexpr int G = decltype(g)::value, R = decltype(r)::value, APW = NT / G;
        const unsigned grid = (unsigned)(((long long)K + APW - 1) / APW);
        k_epg<G, R><<<grid, NT, 0, ctx->stream>>>(d_sched, T, K, p.nstates, d_t1, d_t2, d_b1, p.inversion, p.ti, p.inv_eff, const_timing ? 1 : 0, d_F,
                                                  p.out_is_f64);
    });
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int epg_simulate_grad_dev(qmri_ctx* ctx, int K, int T, int nparams, int sv, const double* d_sched, const double* d_t1, const double* d_t2,
                          const double* d_b1, const qmri_epg_params& p, bool const_timing, void* d_F, void* d_dF, double* d_crb, int32_t* d_flags) {
    if ((nparams != 2 && nparams != 3) || sv < 0 || sv > 16 || !d_crb != !d_flags) {
        qmri_set_error(ctx, "internal: k_epg_grad takes nparams 2 or 3, 0 <= s <= 16, and crb and flags together");
        return QMRI_ERR_INVALID_ARG;
    }
    epg_dispatch(p.nstates, [&](auto g, auto r) {
        constexpr int G = decltype(g)::value, R = decltype(r)::value, APW = NT / G;
        const unsigned grid = (unsigned)(((long long)K + APW - 1) / APW);
        auto* kern = nparams == 2 ? k_epg_grad<G, R, 2> : k_epg_grad<G, R, 3>;
        kern<<<grid, NT, 0, ctx->stream>>>(d_sched, T, K, p.nstates, sv, d_t1, d_t2, d_b1, p.inversion, p.ti, p.inv_eff, const_timing ? 1 : 0, d_F, d_dF,
                                           p.out_is_f64, d_crb, d_flags);
    });
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int epg_simulate_seq_dev(qmri_ctx* ctx, int K, int T, int nseg, int ncycles, const double* d_sched, const void* d_segs, const double* d_t1,
                         const double* d_t2, const double* d_b1, const qmri_epg_params& p, bool const_timing, void* d_F) {
    static_assert(epgseq::FB == FB, "the plan cuts the blocks into the kernel's frame blocks");
    if (nseg < 1 || ncycles < 1 || ncycles > epgseq::MAX_CYCLES) {
        qmri_set_error(ctx, "internal: k_epg_seq takes nseg >= 1 and 1 <= ncycles <= 16");
        return QMRI_ERR_INVALID_ARG;
    }
    epg_dispatch(p.nstates, [&](auto g, auto r) {
        constexpr int G = decltype(g)::value, R = decltype(r)::value, APW = NT / G;
        const unsigned grid = (unsigned)(((long long)K + APW - 1) / APW);
        k_epg_seq<G, R><<<grid, NT, 0, ctx->stream>>>(d_sched, static_cast<const epgseq::Segment*>(d_segs), nseg, ncycles, T, K, p.nstates, d_t1, d_t2, d_b1,
                                                      const_timing ? 1 : 0, d_F, p.out_is_f64);
    });
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int epg_sp_atoms_per_workgroup(int S, int Q) {
    int gpw = epg_atoms_per_workgroup(S);
    return Q >= gpw ? 1 : gpw / Q;
}

int epg_simulate_sp_dev(qmri_ctx* ctx, int K, int T, int Q, const double* d_sched, const double* d_t1, const double* d_t2, const double* d_b1,
                        const qmri_epg_params& p, bool const_timing, void* d_F) {
    if (T < 1 || T > EPG_SP_MAX_T || Q < 1 || Q > 64) { qmri_set_error(ctx, "internal: k_epg_sp takes 1 <= T <= 1024 and 1 <= Q <= 64"); return QMRI_ERR_INVALID_ARG; }
    epg_dispatch(p.nstates, [&](auto g, auto r) {
        constexpr int G = decltype(g)::value, R = decltype(r)::value;
        const int A = epg_sp_atoms_per_workgroup(p.nstates, Q);
        const unsigned grid = (unsigned)(((long long)K + A - 1) / A);
        auto* kern = const_timing ? k_epg_sp<G, R, true> : k_epg_sp<G, R, false>;
        kern<<<grid, NT, 0, ctx->stream>>>(d_sched, T, K, p.nstates, Q, d_t1, d_t2, d_b1, p.inversion, p.ti, p.inv_eff, d_F, p.out_is_f64);
    });
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}

int epg_shift_dev(qmri_ctx* ctx, int S, int nshift, const double* d_in, double* d_out) {
    epg_dispatch(S, [&](auto g, auto r) { k_epg_shift<decltype(g)::value, decltype(r)::value><<<1, 64, 0, ctx->stream>>>(S, nshift, d_in, d_out); });
    QMRI_HIP(ctx, hipGetLastError());
    return QMRI_OK;
}
