// qmri_internal.h -- shared declarations of libqmri.so (host side + kernel launch prototypes).
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/qmri.h"

// ---------------------------------------------------------------------------------------------------
// error handling: nothing throws across the C ABI
// ---------------------------------------------------------------------------------------------------
struct qmri_ctx;
void qmri_set_error(qmri_ctx* ctx, const char* fmt, ...);

#define QMRI_HIP(ctx, expr)                                                                       \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            qmri_set_error((ctx), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return QMRI_ERR_HIP;                                                                  \
        }                                                                                         \
    } while (0)

#define QMRI_CHECK_ARG(ctx, cond, msg)                                                            \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            qmri_set_error((ctx), "invalid argument: %s", (msg));                                 \
            return QMRI_ERR_INVALID_ARG;                                                          \
        }                                                                                         \
    } while (0)

#define QMRI_TRY(expr)                                                                            \
    do {                                                                                          \
        int _s = (expr);                                                                          \
        if (_s != QMRI_OK) return _s;                                                             \
    } while (0)

// ---------------------------------------------------------------------------------------------------
// Owners of device and pinned memory, events and streams (dev_mem.h).  Internal linkage: none of it reaches the library's dynamic symbols.
// ---------------------------------------------------------------------------------------------------
#include "dev_mem.h"
// What the host decides about a gridded operator, in plain C++ (op_plan.h): the mask builders, the k-sorted sample list (KEntry), the work units of
// the k-space LSQR (KSample, KsGroup, KsUnit, KS_CAPS, ks_plan_units) and the DIRECT solver's tables.
#include "op_plan.h"
// The denoiser's layer program, in plain C++ (net_plan.h): ConvKind, conv_cin_pad, the tensor ids (NetTensor), the steps and the resident-run candidates.
#include "net_plan.h"
// The joint wavelet soft-thresholding step's geometry, tiles, buffers and launch list, in plain C++ (wav_plan.h).
#include "wav_plan.h"
// The lines of a gridded dictionary and the refinement's atom table, in plain C++ (refine_plan.h).
#include "refine_plan.h"
// The chunk schedule, frame table and partial-sum layout of a simultaneous multi-slice solve, in plain C++ (sms_plan.h).
#include "sms_plan.h"
// The plan of a trajectory (NUFFT) operator, its kernel constants, the exact spiral and the density compensation's kernel sums, in plain C++ (nufft_plan.h; DESIGN.md sections 14, 21).
#include "nufft_plan.h"
// The field-map histogram, segment times, coefficient system and QR tables of the off-resonance correction, in plain C++ (offres_plan.h; DESIGN.md sections 22, 23).
#include "offres_plan.h"

// ---------------------------------------------------------------------------------------------------
// A/B and diagnostic switches ("knobs").  ONE environment variable, QMRI_DEBUG="name=value,name=value" (read once per process), and
// one entry point, qmri_debug_knob(name, value) (include/qmri.h), set them; every default is the product's behaviour.  The table of
// names and defaults is in api_core.cpp (g_knob_defs; a static_assert there keeps it to this enum's entries and order).
// ---------------------------------------------------------------------------------------------------
enum QmriKnob {
    K_CONV_SCHEME,        // 2: f16 x 3 products (default), 3: bf16 x 6 products from the start
    K_CONV_F32,           // 1: every layer on the f32-MFMA kernels (conv_kernels.hip)
    K_CONV_WT,            // write-through (sc1) output stores of the conv kernels
    K_CONV_XCD,           // XCD-aware tile order
    K_CONV_PERSIST,       // k_conv6p for slice batches
    K_CONV_SPLITK,        // split-K at the deep levels
    K_CONV_MIDCFG, K_CONV_DEEPCFG, K_CONV_DEEPKS,   // tile configuration of the 56 x 56 / 28 x 28 level, largest K split of the latter
    K_CONV_RESIDENT,      // k_conv6r: the full-resolution level's layers as one launch with resident tiles
    K_RES_HEAD, K_RES_TAIL, K_RES_DOWN,             // ... with the head / tail / down-sampling convolution inside
    K_RES_DELAY,          // ... pause before the ring fetch, in units of 64 clocks (res_pipe = 0)
    K_RES_PIPE,           // ... ring exchange pipelined by 16-channel chunk (1, default) or all of it between two layers (0; same bits)
    K_RES_PIPE_DELAY,     // ... res_pipe = 1: pause between the early publish and the first attempt at the neighbours' chunk 0, in units of 64 clocks
    K_RES_REARM,          // ... clean one-launch-per-layer passes after a hand-off time-out before the resident form is tried again
    K_RES_STAMPS, K_CONV_STAMPS, K_CONV_STAMP_LAUNCH, K_LSQR_STAMPS,   // diagnostic builds' in-kernel stamps
    K_CONV_MT2, K_CONV_OCC,                         // f32-MFMA fallback kernels: tile / occupancy choices
    K_FUSE_EW,            // the fused launches between the network and the solve
    K_LSQR_PERSIST,       // k_ks_persist: all LSQR iterations of a solve in one launch
    K_LSQR_FOLD,          // ... and the first Golub-Kahan step (k_ks_b<INIT>) inside that launch
    K_DICTW_LSP,
    K_VERBOSE,            // calibration / guard decisions on stderr
    K_PACK_GPU,           // qmri_set_denoiser: weights split and ordered on the device (1, default) or on the host (0: the round-1 packers, same bits)
    K_NUFFT_SEG,          // qmri_set_operator_nufft: samples per spreading segment (default NU_SEG = 512, at least 32); results change only in rounding
    K_FMAP_FUSE,          // qmri_field_map_estimate: 0 (default) one launch per iteration, 1 h iterations per launch on halo tiles in LDS (same bits; slower as measured)
    K_FMAP_START,         // qmri_field_map_estimate: 1 returns the start f0 (no iteration is run; info.iters = 0): what the tests feed back as f_init
    K_B1_SCRATCH_MB,      // qmri_b1_estimate / qmri_b1_pool: MB of score + box-sum scratch a run of slices may take (default 256; one slice at least; same bits)
    K_COUNT
};
int qmri_knob(QmriKnob k);

// ---------------------------------------------------------------------------------------------------
// forward operator (struct F): device-side description
// ---------------------------------------------------------------------------------------------------
struct OpDev {
    int N, M, s, T, m;
    const double* Vt;        // [T][s]  V(t,c), frame-major
    const KEntry* ent;       // [m]     k-sorted: (kh, kw, t) ascending
    const int32_t* perm;     // [m]     k-sorted position -> frame-major measurement index (ABI order)
    const int32_t* kptr;     // [N*M+1] CSR over k' = kh*M + kw into ent
    const double2* tw_h;     // [N]     exp(-2*pi*i*j/N): twiddles of the h plan
    const double2* tw_w;     // [M]     exp(-2*pi*i*j/M): twiddles of the w plan
    const int32_t* kslot;    // [N*M]   DIRECT solver: slot of k' among sampled locations or -1
    const double* ginv;      // [nsampled][s*s] (G_k + r I)^-1, symmetric, row-major
};

// ---------------------------------------------------------------------------------------------------
// k-space LSQR (kslsqr_kernels.hip): the plan (op_plan.h ks_plan_units: KSample, KsGroup, KsUnit, KS_CAPS) and the state of a solve on the device
// ---------------------------------------------------------------------------------------------------
struct LsqrState;
struct KsDev {
    int ns, G;                                   // sampled k locations; blocks of the iteration kernels
    int caps;                                    // shape of the work units: index into KS_CAPS
    const KsUnit* unit;                          // [G]    slot / sample / group ranges of each block
    const KSample* es;                           // [m]
    const KsGroup* grp;                          // scatter groups, block after block
    const int32_t* sgrp;                         // [ns+1] first group of each slot
    LsqrState* st;                               // [B]
    LsqrState* hst;                              // [B] pinned host copy: the kernel that changes iter / done / flag writes them here too (no copy launch per x-update)
    double* pu[2];                               // [B][2G] partial |u|^2 (image part, then samples), by iteration parity
    double* pv[2];                               // [B][G]  partial |v|^2
    double* pinit;                               // [B][2N] partial |u|^2 of the initial residual, per k-row
    double* pR;                                  // [B][N]  partial R
    const double* pz; int nblk_z;                // [B][nblk_z] partial |z|^2
    double2* cx; double2* cv; double2* cd; double2* cub;   // [B][ns*s] x, v (not normalised), d, u(m+1:end) on the sampled k
    double2* ut; const double2* yk;              // [B][m]
    double2* xhat; double2* zhat;                // [B][n] unitary spectra, layout [c][kh][kw]
    double2* xhat_out;                           // [B][n] assembled solution spectrum (becomes xhat of the next solve)
    double* pdiag;                               // [B][N] partial ||y - A x||^2 or null
    double sr, tol;
    int maxit, ii, vcap;
    int b0;                                      // k_ks_persist: first slice of this launch (a batch goes through it a few slices at a time)
    unsigned long long* stamps;
};

// LSQR (PnP_ADMM.m:102) device state, one per slice
struct LsqrScalars {
    double c, s, phibar, normr, norma, factor;   // recurrences; normar = alpha * factor
    double thet, rho, phi, beta, alpha;          // values A2 needs for the current iteration
    double ua, ub, uc, ue;                       // k-space solver: v, u(m+1:end), d, x - x0 on the never-sampled k, as multiples of (zhat - xhat0)
};
struct LsqrState {
    LsqrScalars sc[2];       // ping-pong by iteration parity
    double n2b, tolb;
    double ny2;              // ||y||^2
    double R;                // k-space solver: sum over never-sampled k of |zhat - xhat0|^2
    double ue_final;         // k-space solver: ue after the last x update
    int32_t iter, done, flag, pad;
};

enum { DC_PLAIN = 0, DC_FWD_H_ONLY = 1, DC_DIAG = 3, DC_DIRECT = 4, DC_SPECTRUM = 5 };
constexpr int DC_SORT_BLOCKS = 64;   // workgroups of k_sort_y per slice (partial sums of |y|^2 added in block order)

struct LsqrDev {
    LsqrState* st;           // [B]
    double* pz;              // [B][nblk_z] partial sums of |z|^2
    double2* yk;             // [B][m]  y in k-sorted order
    double* py;              // [B][DC_SORT_BLOCKS] partial sums of |y|^2 (k_sort_y)
    int nblk_z;
};

// ---------------------------------------------------------------------------------------------------
// denoiser: one packed layer of the conv engine
// ---------------------------------------------------------------------------------------------------
struct ConvLayer {
    ConvKind kind;
    int Cin, Cout;           // logical channels (UP: Cout = real output channels)
    int cin_pad, n_ct;       // padded input channels, number of 32-row output tiles in the packed weights
    int MT;                  // 32-row MFMA tiles per wave
    DevArr<float> wp;        // packed weights (device)
    size_t wp_floats;
    DevArr<void> d_tab;      // tile table {cout tile, ow0, oh0, batch} for (tab_B, tab_MT)
    int tab_B, tab_MT;
    DevArr<void> wp6;        // weights split into f16 pairs (sp6 == 2) or bf16 triples (sp6 == 3), MFMA A-fragment order (conv6_kernels.hip)
    int sp6 = 2;             // pieces per fp32 operand of the matrix-core path
    float w6_descale = 1.f;  // f16 scheme: 2^-k of the power-of-two the packed weights carry (conv6_kernels.hip)
    int nchunk6 = 0, n_ct6 = 0;   // 16-channel chunks (2x2 layers: K steps), 64-row output tiles of wp6
    int nsteps6s = 0;             // 2x2 layers: K steps that carry weights (nchunk6 is padded to a multiple of 3)
    int index = -1;               // position in NetPlan::layers (row of the |output| report, conv6_kernels.hip ACT_LOW)
    size_t w_off = 0;             // first weight of this layer in the caller's flat blob (floats)
};

// activation tensor in HBM: [B][Cal][W+2][hp] fp32, h fastest, permanent zero halo, channels >= C are zero.
// A row holds h0 - 1 unused floats, the top halo, the H interior values (starting at float h0), the bottom halo and padding
// up to the pitch hp; h0 and hp are multiples of 32, so every interior row starts on a 128-byte line.  Kernels address the
// tensor through base1(), relative to which the interior starts at +1 as in a plain [W+2][H+2] layout with pitch hp.
struct PTensor {
    float* p = nullptr;
    int C = 0, Cal = 0, H = 0, W = 0;
    int hp = 0, h0 = 1;
    // BLOCKED: element (c, w, h) of the padded image lives at ((c/8 * plane + w * hp + h) * 8 + c%8 instead of c * plane + w * hp + h -- the
    // interior format of the matrix-core conv kernels (conv6_kernels.hip: 8 channels of a pixel = 32 contiguous bytes = two 16-byte
    // requests).  Same allocation either way (Cal % 8 == 0); a property of the current forward pass, set by net_forward_padded.
    bool blk = false;
    float* base1() const { return p + (h0 - 1); }
    float* fbase() const { return p + (size_t)(h0 - 1) * (blk ? 8 : 1); }      // halo origin of row 0 in the tensor's current format
    size_t plane() const { return (size_t)hp * (W + 2); }
    size_t batch_stride() const { return (size_t)Cal * plane(); }
};

// per-layer reduction of the |output| reports of a forward pass (conv6_act.h); nlayers = 0: nothing to do
struct ActCheckArgs { const float* slots; int* count; float* ref; int record; unsigned* range_flag; unsigned* host_words; int nlayers; };

struct NetPlan {
    qmri_net_desc desc{};
    int H = 0, W = 0, maxB = 0;
    NetProgram prog;         // the layer program (net_plan.h): one step per layer, and the runs the resident-tile launch is offered
    std::vector<ConvLayer> layers;   // ... one per step
    // activation buffers (device, padded planes), by tensor id (NetTensor): per UNet level the skip tensor x and two work tensors a, t;
    // NT_IN32 the normalised network input (in_nc channels, allocated up to the first layer's padded Cin), NT_OUT32 the network output (out_nc channels)
    PTensor ten[NT_COUNT];
    DevPool pool;            // the tensors above and the plan-lifetime arrays below
    unsigned* d_counter = nullptr;   // tile-queue counter of the persistent conv kernels
    unsigned counter_base = 0;       // host mirror of its value after the launches issued so far
    bool counter_by_memset = false;  // a launch under a stream capture: the queue is reset before every launch instead
    bool force_f32 = false;             // calibration (qmri_set_denoiser): run the f32-MFMA kernels whatever the scheme
    unsigned* d_range_flag = nullptr;   // f16 scheme: raised by a conv kernel whose output leaves the f16-splittable range
    PinnedArr<unsigned> h_range_flag;   // pinned host words written by k_act_check at the end of every forward pass: [0] overflow bit, [1 + layer] low-magnitude bit
    int h_range_words = 0;              // ... how many (1 + layers must fit, else the ADMM loop copies the device flag instead)
    int fallbacks = 0;                  // times a run-time guard moved the network from the f16 to the bf16 scheme since qmri_set_denoiser
    float* d_act_slots = nullptr;       // f16 scheme: largest |output| per (reporting launch, wave) of the current forward pass (conv6_kernels.hip, ACT_LOW)
    int* d_act_count = nullptr;         // ... valid slots per reporting launch
    float* d_act_ref = nullptr;         // ... the magnitude of every layer under the set-up probe (calibrated reference)
    int act_rows = 0;                    // rows of the three arrays (= layers)
    bool act_on = false, act_record = false;   // a reporting forward pass is under way; it is the calibration probe
    // the PnP-ADMM loop lets the kernel after the forward pass finish the per-layer |output| report (conv6_act.h) instead of launching k_act_check
    bool act_defer = false, act_pending_valid = false;
    ActCheckArgs act_pending{};
    int sp6 = 2;                     // scheme the layers are packed for
    bool blk_ok = false;             // the network's interior tensors may be BLOCKED (PTensor::blk): every layer runs on the conv6 kernels, channels % 8 == 0
    int interior_fmt = -1;           // format the interior tensors were last written in (-1: untouched zeros, 0 planar, 1 blocked): a change re-zeroes them (halo)
    std::vector<float> w_host;       // the caller's weights (kept to re-pack the layers for the other scheme; knob pack_gpu = 0 only)
    float* d_wflat = nullptr;        // ... on the device, in the caller's order (knob pack_gpu = 1, default: the packers run there)
    std::vector<float> w_max;        // ... and every layer's largest |w| (from the device): the f16 scheme's per-layer scale
    DevArr<float> d_c6part;          // split-K partial outputs of k_conv6 (conv6_kernels.hip), grown on demand
    void* d_stamps = nullptr;        // diagnostic: per-workgroup timing stamps of the last conv launch (knob conv_stamps = 1)
    // resident-tile ResBlock runs (conv6_kernels.hip k_conv6r): the exchange buffer of the tiles' edge pixels (two layer parities x tiles x 23.5 KB), the
    // running tag of its granules (never reset), and the switch a timed-out hand-off turns off for the life of the plan
    unsigned char* d_res_xbuf = nullptr;
    int res_tiles = 0;
    unsigned res_epoch = 0;
    bool res_off = false;
    bool res_forced_off = false;     // ... by qmri_debug_conv_resident(ctx, 0, ..): never re-armed
    double setup_ms[3] = {0, 0, 0};  // qmri_set_denoiser: weight packing + upload / tensors and buffers / calibration probe (qmri_get_health)
    int res_timeouts = 0;            // hand-off time-outs since qmri_set_denoiser (three: the form stays off)
    int res_clean = 0;               // clean one-launch-per-layer passes since the last one (K_RES_REARM of them re-arm the form)
    int res_drop = 0;                // test hook: bit 0 = tile 0 withholds its hand-off
    DevArr<double> d_io;             // qmri_denoise: device staging of the caller's doubles (elements), kept between calls
    void* d_res_stamps = nullptr;    // diagnostic: phase stamps of the last k_conv6r launch (knob res_stamps), 4 x 2 x R_MAXL (10) x 16 of 2048 values
    bool ready = false;
};

// multi-coil LSQR of B slices (mc_kernels.hip): work buffers owned by the context, grown only when B or B x ncoil grows
struct McWork {
    DevArr<double2> ut;                 // [B][ncoil][m]  u(1:m) of every coil image, unscaled
    DevArr<double2> ub, v, d, t;        // [B][n]  u(m+1:end) unscaled, v, d, A_mc' u
    DevArr<double2> scr;                // [max_batch][n] coil images of one transform chunk
    DevArr<double> part;                // fixed partial sums (mc_kernels.hip McParts)
    DevArr<LsqrState> st;               // [B] device state; sc[0] only
    PinnedArr<LsqrState> hst;           // [B] pinned: iter / done / flag written by the kernel that changes them
    int pred = 8;                       // iterations enqueued before the first event wait after the initial step (the last solve's count + 1)
    int pred_cg = 8;                    // ... of the Toeplitz CG (toep_kernels.hip)
    // staging of the host-array entry points: maps [B][ncoil][N*M], y [B][ncoil][m], x and z (or x0) [B][n]
    DevArr<double2> sm, sy, sx, sz;
};
int mc_ensure_staging(qmri_ctx* ctx, int B, int ncoil);
int mc_adjoint_batch_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_maps, const double2* d_y, double2* d_x);
int mc_ensure_work(qmri_ctx* ctx, int B, int ncoil);
// the coil products of a transform chunk (coil images g0 .. g0 + cnt - 1 of [B][ncoil]); st (nullable): slices whose solve has stopped are skipped
int mc_launch_coil_mul(qmri_ctx* ctx, int ncoil, int g0, int cnt, const double2* x, const double2* maps, const LsqrState* st, double2* out);
int mc_launch_coil_sum(qmri_ctx* ctx, int ncoil, int g0, int cnt, const double2* xj, const double2* maps, const LsqrState* st, double2* t);
// the image-side vector kernels of the LSQR on B slice vectors with one state each (mode 0: initial step, 1: iteration); partials: MC_PS per vector
constexpr int MC_PS = 256, MC_PC = 64;   // fixed partial sums per slice vector (n complex) / per coil image (m complex)
int mc_launch_ub(qmri_ctx* ctx, int mode, int B, double sr, const double2* z, const double2* x, const LsqrState* st, double2* ub, double2* v, double2* d,
                 double* pb, double* pz);
int mc_launch_dupd(qmri_ctx* ctx, int B, const double2* v, const double2* x, const LsqrState* st, double2* d, double* pd, double* px);
int mc_launch_vupd(qmri_ctx* ctx, int mode, int B, double sr, const double2* t, const double2* ub, const double2* d, const LsqrState* st, double2* x,
                   double2* v, double* pv);
int qmri_lsqr_mc_batch_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                           double2* d_x, int32_t* iters_out, int32_t* flags_out);

// coil compression of multi-coil stacks (cc_kernels.hip, api_cc.cpp): work buffers owned by the context, grown only when a call needs more
struct CcWork {
    DevArr<double2> part, R, X, L, U, W;        // partials, R / K, scratch, chol(Psi), U_nv, W
    PinnedArr<double2> hK;                      // pinned: K to the host eigensolve, then U_nv back
    PinnedArr<int> hbad;                        // pinned: Cholesky of Psi failed
    bool lds_attr = false;                      // > 64 KB dynamic LDS allowed for the 128-coil covariance kernel
    // staging of the host-array entry point and of Psi: y / maps in, y / maps out
    DevArr<double2> psi, sy, sm, oy, om;
};
int cc_ensure_staging(qmri_ctx* ctx, size_t ny, size_t nm, size_t nyo, size_t nmo);
int cc_compress_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_y, const double2* d_maps, const double2* d_psi, const qmri_cc_params& prm,
                    int* nv_out, double2* d_yout, double2* d_mout, double2* d_Wout, double* eig_out);
// host (api_cc.cpp): eigen-decomposition of the Hermitian n x n matrix whose upper triangle is A (column-major), lambda descending, the phase rule
// applied (cyclic Jacobi); and the smallest nv whose leading eigenvalues hold `energy` of the sum
int cc_eig_host(qmri_ctx* ctx, int n, const double2* A, double* lam, double2* U);
int cc_choose_nv(int n, const double* lam, double energy);
int cc_batch_param_error(int ncoil, const qmri_cc_params* p, std::string* msg);   // qmri_recon_batch_mc_cc's rules: QMRI_OK or the code + *msg

// coil sensitivity maps from calibration data (csm_kernels.hip, api_csm.cpp).  Scratch lives for the call (DevBuf).
int csm_chunk_coils(int ncoil, int p);   // coils per LDS chunk of k_csm_eig (= ncoil: all resident); a function of its arguments alone
int csm_maps_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_calib, const qmri_csm_params& prm, double2* d_maps, double2* d_img, double* d_lam,
                 qmri_csm_info* info);

// dictionary compression to its SVD subspace (dsvd_kernels.hip, api_dsvd.cpp).  All pointers are device pointers; the launches
// go to ctx->stream and are not waited for.
int dsvd_gram_chunk();                   // atoms per split-K partial of the Gram kernel: a constant, so G's bits depend on (K, T) alone
size_t dsvd_gram_scratch(int K, int T);  // doubles of partial tiles dsvd_gram_dev needs
int dsvd_gram_dev(qmri_ctx* ctx, int K, int T, const void* d_F, bool f64, double* d_part, double* d_G, double* d_diag);      // G = F^T F, diag = its diagonal
int dsvd_gq_dev(qmri_ctx* ctx, int T, int b, const double* d_G, const double* d_Q, double* d_Z);                               // Z = G Q (T x b)
int dsvd_project_dev(qmri_ctx* ctx, int K, int T, int s, const void* d_F, bool f64, const double* d_V, float* d_D, float* d_normD);

// FISP dictionary simulation by extended phase graphs (epg_kernels.hip, api_epg.cpp).  All d_ pointers are device pointers;
// d_sched holds alpha, tr, te (3 T doubles); the launches go to ctx->stream and are not waited for.
int epg_atoms_per_workgroup(int S);      // atoms a workgroup simulates (= the contiguous run of its stores) with S states
int epg_simulate_dev(qmri_ctx* ctx, int K, int T, const double* d_sched, const double* d_t1, const double* d_t2, const double* d_b1 /* or NULL */,
                     const qmri_epg_params& p, bool const_timing, void* d_F);
// the fingerprints with their derivatives and the Cramer-Rao bound in one launch.  d_sched: alpha, tr, te, then V [T x sv]
// column-major (sv = 0: none).  d_F, d_dF (nparams arrays of K x T) and the pair d_crb [K x (1 + nparams)] / d_flags [K] are each optional
int epg_simulate_grad_dev(qmri_ctx* ctx, int K, int T, int nparams, int sv, const double* d_sched, const double* d_t1, const double* d_t2,
                          const double* d_b1 /* or NULL */, const qmri_epg_params& p, bool const_timing, void* d_F, void* d_dF, double* d_crb,
                          int32_t* d_flags);
// the slice-profile-aware simulation.  d_sched: T frame records (alpha_t, tr_t, te_t, prof[t, 0 .. Q-1]), then weight [Q]
int epg_sp_atoms_per_workgroup(int S, int Q);      // atoms a workgroup simulates with S states and Q sub-slices (1 when Q fills its groups)
int epg_simulate_sp_dev(qmri_ctx* ctx, int K, int T, int Q, const double* d_sched, const double* d_t1, const double* d_t2,
                        const double* d_b1 /* or NULL */, const qmri_epg_params& p, bool const_timing, void* d_F);
// prepared, repeated trains.  d_segs: nseg records of epg_seq_plan.h (epgseq::Segment), played ncycles times
int epg_simulate_seq_dev(qmri_ctx* ctx, int K, int T, int nseg, int ncycles, const double* d_sched, const void* d_segs, const double* d_t1,
                         const double* d_t2, const double* d_b1 /* or NULL */, const qmri_epg_params& p, bool const_timing, void* d_F);
int epg_shift_dev(qmri_ctx* ctx, int S, int nshift, const double* d_in, double* d_out);      // the spoiler alone on one atom's state (3 S doubles)

// field map from multi-echo images (fmap_kernels.hip, api_fmap.cpp).  All d_ pointers are device pointers; the stream is
// idle on return (the per-slice results are read back for info).
constexpr int FMAP_MAX_PAIRS = 28;       // L <= 8 echoes
struct FmapPlan {
    int nslices, L, C, N, M, P, iters, sign;
    double beta;                         // B = beta (2 pi (t_{L-1} - t_0))^2
    double unwrap_limit_hz;
    double d[FMAP_MAX_PAIRS];            // 2 pi (t_b - t_a) per pair
    int pa[FMAP_MAX_PAIRS], pb[FMAP_MAX_PAIRS];
};
int fmap_halo();                         // h: iterations per fused launch
int fmap_estimate_dev(qmri_ctx* ctx, const FmapPlan& pl, const double2* d_Y, const double* d_f_init /* or NULL */, double* d_f_out,
                      double* d_trust_out /* or NULL */, qmri_fieldmap_info* info /* host, or NULL */);

// locally low-rank proximal step (llr_kernels.hip, api_llr.cpp).  All d_ pointers are device pointers; the launches go to
// ctx->stream and are not waited for.
struct LlrPlan { int N, M, s, block, o1, o2, real; double tau; };
struct LlrState { bool on = false; double tau = 0.0; int block = 8, shift = 0; };    // qmri_set_llr
void llr_offsets(int it, int block, int shift, int* o1, int* o2);                     // the offsets of ADMM iteration `it` (0-based)
// d_out [B][s][M][N] = LLR_tau(d_x + d_u) (d_u NULL: of d_x; real: of the real part, imaginary part 0); d_out may be d_x.  d_bsmax (nullable):
// [B][blocks per slice] sigma_max per block, and with it d_smax (nullable): [B] the slice's maximum (a second small launch)
int llr_prox_dev(qmri_ctx* ctx, const LlrPlan& pl, int B, const double2* d_x, const double2* d_u, double2* d_out, double* d_bsmax, double* d_smax);
// uold += x - v; z = v - uold; pz [B][nblk_z] partial sums of ||z||^2 (n elements per slice)
int llr_dual_dev(qmri_ctx* ctx, int B, size_t n, const double2* d_x, const double2* d_v, double2* d_u, double2* d_z, double* d_pz, int nblk_z);

// joint wavelet soft-thresholding (wav_kernels.hip, api_wav.cpp, wav_plan.h).  All d_ pointers are device pointers; the
// launches go to ctx->stream and are not waited for.  levels is 1 .. 4 here (the ABI's 0 is resolved by the caller).
struct WavPlan { int N, M, s, levels, filter, joint, o1, o2, real; double tau; };
struct WavState { bool on = false; double tau = 0.0; int levels = 3, filter = QMRI_WAVELET_DB2, joint = 1, shift = 0; };    // qmri_set_wavelet
// d_out [B][s][M][N] = Wav_tau(d_x + d_u) (d_u NULL: of d_x; real: of the real part, imaginary part 0); d_out may be d_x.  d_cmax (nullable): [B]
// the largest m of each slice before thresholding (one more small launch).  The scratch (wav_plan.h) is the context's and grows on first use.
int wav_prox_dev(qmri_ctx* ctx, const WavPlan& pl, int B, const double2* d_x, const double2* d_u, double2* d_out, double* d_cmax);

// ---------------------------------------------------------------------------------------------------
// trajectory (NUFFT) operator (nufft_kernels.hip, api_nufft.cpp).  Planned once on the host per qmri_set_operator_nufft by
// nufft_plan.h (nu_plan: NU_TB, NuSeg, NuRed; knob nufft_seg): the device's view of the plan and the arrays the operator owns.
// ---------------------------------------------------------------------------------------------------
struct NufftDev {
    int N, M, s, T, m, w;
    double beta, hw;                             // kernel exp(beta (sqrt(1 - (d / hw)^2) - 1)), hw = w / 2
    int ntile2, nseg, nred, nslot;
    const double* Vt;                            // [T][s]
    const double2* u;                            // [m] sorted: oversampled grid coordinates (omega1 N / pi, omega2 M / pi)
    const double2* ph;                           // [m] sorted: exp(-i (omega1 N / 2 + omega2 M / 2))
    const int32_t* t;                            // [m] sorted: frame
    const int32_t* perm;                         // [m] sorted position -> ABI index
    const int32_t* list;                         // spreading lists of the segments (sorted positions)
    const NuSeg* seg;                            // [nseg]
    const NuRed* red;                            // [nred]
    const double* dp1; const double* dp2;        // [N], [M] deapodisation 1 / Phi at n - N/2
    const double2* r1; const double2* r2;        // [N], [M] exp(-i pi (n - N/2) / N): the half-bin ramps
    const double* wgt;                           // [m] ABI order: the attached sample weights or null; read by k_nu_spread<true> only
    // the segment of a field map that a launch works on; read by the OFFRES instantiations only, null / 0 without a map
    const double2* pm;                           // [N*M] plane order (n1 + N n2): exp(-i 2 pi (f - f0) tau^_l)
    const double2* bl;                           // [m] sorted: b_l(tau_i) exp(-i 2 pi f0 tau_i)
    int acc;                                     // 1: add to the output (segments l > 0), 0: overwrite it
};
struct NufftHost {
    double* d_u = nullptr; double* d_ph = nullptr; int32_t* d_t = nullptr; int32_t* d_perm = nullptr; int32_t* d_list = nullptr;
    NuSeg* d_seg = nullptr; NuRed* d_red = nullptr; double* d_dp = nullptr; double2* d_r = nullptr;
    double2* d_g = nullptr; double2* d_grid = nullptr; double2* d_part = nullptr;   // [4 maxB][n] x2, [maxB][nslot][s][256]
    double2* d_ones = nullptr;                   // [N*M] the unit coil of qmri_xupdate / qmri_pnp_admm on a trajectory
    int w = 0, nseg = 0, nred = 0, nslot = 0;
    double beta = 0.0;
    // Toeplitz normal operator (toep_kernels.hip): the 2N x 2M DFT of the s x s point-spread function of A^H A, times 1/4,
    // Hermitian-packed: [pair (c <= c') = c' (c' + 1) / 2 + c][a][j1][j2], bin (2 j1 + a1, 2 j2 + a2).  Built by toep_prepare, in the operator's pool.
    double2* d_khat = nullptr;
    bool khat_ready = false;
    // sample weights of the weighted adjoint (density compensation): [m] in ABI order, attached by qmri_nufft_dcf or
    // qmri_set_sample_weights, read by the qmri_adjoint_w* calls alone (replacing the operator drops them)
    DevArr<double> d_w;
    bool w_set = false;
    // field map of the off-resonance correction (time segmentation): attached by qmri_set_field_map, read by nufft_launch_fwd /
    // _adj (every caller of the operator); replacing the operator drops it.  Sized at attach time.
    DevArr<double2> d_pm;                        // [fm_L][N*M] phase maps of the segments
    DevArr<double2> d_bl;                        // [fm_L][m] coefficients in the plan's sorted order, the centre-frequency phase folded in
    int fm_L = 0;                                // segments
    bool fm_set = false;
    // what the attached map's field-aware normal operator is defined by, kept on the host at attach time
    std::vector<double> fm_f, fm_ts, fm_p;       // the map [N*M], the readout times [m] (ABI order), the histogram p_h [fm_nbins]
    double fm_f0 = 0.0, fm_fmin = 0.0, fm_fmax = 0.0, fm_tmin = 0.0, fm_tmax = 0.0;
    int fm_nbins = 0;
    // field-aware Toeplitz normal operator (qmri_nufft_prepare_normal_fm): A_f^H A_f ~ sum_l P_l^H T_l P_l over fmn_L segments of
    // the DIFFERENCE phase.  Belongs to the attached map: qmri_set_field_map and replacing the operator drop it.  d_khat above is never touched by it.
    DevArr<double2> d_khat_fm;                   // [fmn_L][pair][a][j1][j2], T_l built with the sample weights c_l(tau_i)
    DevArr<double2> d_pm_n;                      // [fmn_L][N*M] phase maps at the fmn_L segment times (d_pm is at the operator's own times)
    DevArr<double2> d_xs;                        // [maxB][n] x kept while the segments add into out (out may be x)
    int fmn_L = 0;                               // segments; 1 with fmn_plain: a constant map, the plain d_khat serves
    bool fmn_plain = false;
    bool fmn_ready = false;
};
int nufft_launch_fwd(qmri_ctx* ctx, int B, const double2* x, double2* y);    // x [B][n] -> y [B][m] (ABI order)
int nufft_launch_adj(qmri_ctx* ctx, int B, const double2* y, double2* x);    // y [B][m] -> x [B][n]
int nufft_launch_adj_plain(qmri_ctx* ctx, int B, const double2* y, double2* x);  // ... uncorrected even while a field map is attached (the Toeplitz set-ups)
int nufft_launch_adj_w(qmri_ctx* ctx, int B, const double2* y, double2* x);  // ... of w .* y, w the attached sample weights (multiplied where k_nu_spread stages y)
// Pipe-Menon density compensation on the plan's own kernel and spreading lists (dcf_kernels.hip, api_dcf.cpp): niter
// iterations (1..200) from w = 1, stopped early once max |d - 1| <= tol (tol <= 0: never), then d_w_out [m] (ABI order) = kappa * w.  Uses the plan's
// d_grid / d_part as scratch; waits for its kernels.
int dcf_weights_dev(qmri_ctx* ctx, int niter, double tol, double kappa, double* d_w_out, qmri_dcf_info* info);
// time-segmented off-resonance correction (offres_kernels.hip, api_offres.cpp)
struct OffresFit { double fit_max, fit_rms; };
// d_pm [L][N*M] = exp(-i 2 pi (f - f0) tauhat_l) from d_f [N*M]
int offres_phase_maps_dev(qmri_ctx* ctx, int L, size_t plane, const double* d_f, double f0, const double* d_tauhat, double2* d_pm);
// d_bl [L][m] (sorted order) from the Cholesky factor d_chol [L][L] (lower, row-major) of G^H P G + eps I, the histogram d_hist [nbins] (x: p_h,
// y: f_h) and its table d_G [nbins][L]; exact = a constant map (b = 1).  Fills *fit (device reductions in a fixed order) and waits for its kernels.
int offres_coefficients_dev(qmri_ctx* ctx, int L, int nbins, bool exact, const double2* d_hist, const double2* d_G, const double2* d_chol,
                            const double* d_ts, double f0, double2* d_bl, OffresFit* fit);
// QMRI_ERR_UNSUPPORTED with a message naming LSQR while a field map is attached and qmri_nufft_prepare_normal_fm has not built the field-aware
// transform for it, else QMRI_OK (host check only)
int offres_refuse_toeplitz(qmri_ctx* ctx, const char* what);
// the real coefficients c [L][m] (sorted order) of the difference-phase segmentation (k_offres_ncoef) from the thin QR B = Q U of
// the stacked table [sqrt(p~) cos; sqrt(p~) sin; sqrt(eps) I]: d_Qw [nb][L] (x / y: sqrt(p~_j) times Q's cos / sin row of bin j), d_U [L][L] (upper,
// row-major), the difference histogram d_dh [nb] (x: p~_j, y: g_j) and its table d_G [nb][L] = exp(i 2 pi g_j tauhat_l).  Fills *fit (device
// reductions in a fixed order) and waits for its kernels.
int offres_ncoefficients_dev(qmri_ctx* ctx, int L, int nb, const double2* d_dh, const double2* d_G, const double2* d_Qw, const double* d_U,
                             const double* d_ts, double* d_c, OffresFit* fit);
void offres_drop_normal(NufftHost& h);             // forgets the field-aware transform and frees its device buffers (K^, phase maps, staging)
int nufft_check_gridded(qmri_ctx* ctx, const char* what, const char* instead);   // QMRI_ERR_UNSUPPORTED on a trajectory operator, else QMRI_OK
NufftDev nufft_dev_view(const qmri_ctx* ctx);
int nufft_launch_ramps(qmri_ctx* ctx, int B, const double2* x, double2* g);      // k_nu_pre without 1 / Phi:  x [B][n] -> g [B][4][n]
int nufft_launch_unramps(qmri_ctx* ctx, int B, const double2* g, double2* x);    // k_nu_post without 1 / Phi
int nufft_launch_ramps_pm(qmri_ctx* ctx, int B, const double2* x, double2* g, const double2* pm);                // ... of x .* pm, pm [N*M]
int nufft_launch_unramps_pm(qmri_ctx* ctx, int B, const double2* g, double2* x, const double2* pm, bool acc);    // ... times conj(pm); acc: x += 
// Toeplitz normal operator of a trajectory (toep_kernels.hip, api_toep.cpp)
int toep_prepare(qmri_ctx* ctx);                                                  // builds K^ once per trajectory (idempotent)
// K^ of segment l of the field-aware normal into khat [pair][a][j1][j2]: the pipeline of toep_prepare with the per-sample real weights d_c [m] (sorted)
int toep_build_weighted(qmri_ctx* ctx, const double* d_c, double2* khat);
// out [B][n] = A^H A x [B][n], B <= max_batch; out may be x.  With a field map attached (and its transform prepared): the segment loop of section 23
int toep_apply(qmri_ctx* ctx, int B, const double2* x, double2* out);
int qmri_cg_toep_batch_dev(qmri_ctx* ctx, int B, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                           double2* d_x, int32_t* iters_out, int32_t* flags_out);  // the call shape of qmri_lsqr_mc_batch_dev
// the x-update of the multi-coil loops by the solver of qmri_admm_params (LSQR or TOEPLITZ)
int mc_xupdate_dev(qmri_ctx* ctx, int solver, int B, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                   double2* d_x, int32_t* iters_out, int32_t* flags_out);
// The multi-coil PnP-ADMM loop around a start image and an x-update (api_admm.cpp): what differs between the SENSE loop and the simultaneous
// multi-slice loop (api_sms.cpp).  nsolve LSQR counts per x-update; B slice images go through Step 2.
struct AdmmSolve {
    int nsolve = 0;
    std::function<int(double2* d_x)> start;
    std::function<int(const double2* d_z, double2* d_x, int32_t* iters)> solve;
};
int mc_admm_check(qmri_ctx* ctx, const qmri_admm_params* prm);     // a Step 2 is configured and fits the operator; the parameters' ranges; the solver
int mc_admm_loop(qmri_ctx* ctx, int B, const qmri_admm_params* prm, const AdmmSolve& sv, double2* d_x, int32_t* li_out, int li_stride);
int toep_check_solver(qmri_ctx* ctx, int solver);   // QMRI_SOLVER_TOEPLITZ without an operator: QMRI_ERR_STATE, on a gridded one: QMRI_ERR_UNSUPPORTED; else QMRI_OK

// ---------------------------------------------------------------------------------------------------
// simultaneous multi-slice (SMS) groups (sms_kernels.hip, api_sms.cpp, sms_plan.h): the state of qmri_set_sms and the work
// buffers of its solves.  It lives in the operator (OpHost), so replacing the operator drops it, as the sample weights.  Z = 0: not set.
// ---------------------------------------------------------------------------------------------------
struct SmsWork {
    int Z = 0;
    std::vector<double2> E;             // [Z][T] the caller's phases, E[t + T b]
    bool on_device = false;             // d_E / d_frame hold E and the frame table (uploaded at the first call that needs them)
    DevArr<double2> d_E;                // [Z][T]
    DevArr<int32_t> d_frame;            // [m] frame of every sample, ABI order
    DevArr<LsqrState> st;               // [G] the LSQR state of every group (McWork::st holds its copies, one per slice vector)
    PinnedArr<LsqrState> hst;           // [G] pinned: iter / done / flag
    DevArr<double2> acc;                // [G][ncoil][m] the sum over slices while chunks add to it
    DevArr<double2> ex;                 // [max_batch][m] conj(E) u of one adjoint chunk
    int pred = 8;                       // iterations enqueued before the first wait after the initial step
};
int sms_forward_dev(qmri_ctx* ctx, int G, int ncoil, const double2* d_maps, const double2* d_x, double2* d_y);      // y [G][ncoil][m] = A_sms x
int sms_adjoint_dev(qmri_ctx* ctx, int G, int ncoil, const double2* d_maps, const double2* d_y, double2* d_x);      // x [G][Z][n] = A_sms^H y
// LSQR on [A_sms; sqrt(r) I] x = [y; sqrt(r) z] for G groups from x0 = d_x (overwritten); the call shape of qmri_lsqr_mc_batch_dev, one count per group
int sms_lsqr_dev(qmri_ctx* ctx, int G, int ncoil, const double2* d_maps, const double2* d_y, const double2* d_z, double r, double tol, int maxit,
                 double2* d_x, int32_t* iters_out, int32_t* flags_out);

// ---------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------
enum { OP_GRIDDED = 0, OP_NUFFT = 1 };
struct OpHost {
    int kind = OP_GRIDDED;              // OP_NUFFT: qmri_set_operator_nufft (nu below; the k-space tables are not allocated)
    NufftHost nu;
    DevPool pool;                       // every plan-lifetime device array of the operator: the raw pointers below, in ks / ls and in nu
    bool ready = false;
    int N = 0, M = 0, s = 0, T = 0, m = 0, maxB = 0, nsampled = 0;
    double* d_Vt = nullptr; KEntry* d_ent = nullptr; int32_t* d_perm = nullptr; int32_t* d_kptr = nullptr;
    double2* d_tw = nullptr; int32_t* d_kslot = nullptr; double* d_ginv = nullptr;
    DevArr<double2> d_coils; int ncoil = 0;   // multi-coil extension: [ncoil][N*M] sensitivity maps (qmri_set_coils)
    McWork mc;                          // ... and the work buffers of its LSQR
    SmsWork sms;                        // simultaneous multi-slice state (qmri_set_sms) and the buffers of its solves
    KsDev ks{};                         // k-space LSQR plan + state
    bool xhat_valid = false;            // ks.xhat holds the spectrum of d_x
    double ginv_r = -1.0;
    std::vector<double> V;              // T x s column-major (host copy)
    std::vector<int32_t> frame_ptr, kidx, kptr_h, perm_h;
    std::vector<KEntry> ent_h;
    // workspaces
    double2* d_tmp = nullptr;           // [B][s][N][M]
    double2* d_xa = nullptr; double2* d_xb = nullptr;   // [B][n] staging for host-pointer entry points
    double2* d_ya = nullptr;            // [B][m]
    LsqrDev ls{};
    // ADMM state
    double2* d_x = nullptr; double2* d_u = nullptr; double2* d_vv = nullptr; double2* d_z = nullptr;
    double2* d_chat = nullptr;          // DIRECT: unitary FFT2 of A'y
    double* d_mm = nullptr;             // [B][nblk_z][2] min/max partials
    double* d_norm = nullptr;           // [B][2] lo, range
    DevArr<double> d_diag;              // [B][iters][2], sized by the diagnostic call
    double* d_pd = nullptr;             // diag partials
    PinnedArr<LsqrState> h_state;       // pinned
    PinnedArr<LsqrState> h_ring;        // pinned [ADMM iteration][slice]: LSQR state of a reconstruction whose host never waits (api_admm.cpp)
};

// components of the tissue-fraction unmixing (qmri_set_components; pv_kernels.hip, api_pv.cpp).  The table the kernel reads, PV_TAB
// doubles: A [16][8] (channel j, component c; zero padded), G [8][8], asum [16] = sum_c a_c, na [8] = sqrt(G_cc)
constexpr int PV_MAX_C = 8, PV_MAX_S = 16, PV_TAB_A = 0, PV_TAB_G = 128, PV_TAB_ASUM = 192, PV_TAB_NA = 208, PV_TAB = 216;
struct PvHost { int C = 0, s = 0; double min_pivot = 0.0; DevArr<double> d_tab; };
// Pure host code: the table of C components (1-based atoms) of the dictionary D [K][s column-major] / normD, and the smallest Cholesky pivot of the
// unit-diagonal-scaled G.  QMRI_OK, or QMRI_ERR_INVALID_ARG with *msg set (index outside 1..K, repeated, zero or non-finite atom, C > s, collinear).
int pv_form_components(const float* D, const float* normD, int K, int s, int C, const int32_t* atoms, double* tab, double* min_pivot, std::string* msg);
int pv_launch(qmri_ctx* ctx, const double2* d_X, int Npix, int mode, double* d_w, double* d_frac, double2* d_pd, double* d_res, int32_t* d_flags);

// sub-grid refinement of a match (qmri_set_refine; refine_kernels.hip, api_refine.cpp): P = 0 none.  d_nbr [K][P][2] the lines
// (refine_plan.h), d_arow [K][16] the unnormalised atoms in fp64, one 128-byte row each.
struct RefineHost { int P = 0; int cols[3] = {0, 0, 0}; int32_t count[3][3] = {}; DevArr<int32_t> d_nbr; DevArr<double> d_arow; };
int refine_launch(qmri_ctx* ctx, const double2* d_X, int Npix, const int32_t* d_dm, double* d_qmap, double2* d_pd, double* d_res, double* d_t,
                  int32_t* d_centre, int32_t* d_flags);

struct DictHost {
    bool ready = false;
    int K = 0, s = 0, Q = 0, ntiles = 0;
    // s <= 16 (dict_kernels.hip): d_pack = [ntiles][lane][4 | 8] MFMA A-fragments.
    // s  > 16 (wide = 1, dictw_kernels.hip): d_pack = [ntiles (padded to 128-atom tiles)][G8][lane][4], G8 = groups of 8 channels (s padded to 16)
    int wide = 0, G8 = 0;
    DevPool pool;                                         // the dictionary's own arrays: d_pack, d_normD, d_lut, d_pack16
    float* d_pack = nullptr;
    DevArr<float4> d_xp;                                  // wide: the pixels as single-precision B-fragments, [tile32][G8][re | -im][lane][4]
    DevArr<float4> d_win;                                 // per pixel (re ip, im ip, atom, |ip|) of the winner, kept when Xfit is asked for
    int slots_w = 0;                                      // workgroups of k_dictw_match the device holds at once
    float* d_normD = nullptr; float* d_lut = nullptr;
    DevArr<float4> d_part;                                // (|ip|, atom index, re, im) per (atom part, pixel) when the atoms are split over workgroups
    int slots = 0, slots_f = 0;                           // workgroups of k_dict_match / k_dict_match_f the device holds at once (occupancy query, first launch)
    // f16 filter in front of the exact products (dict_kernels.hip): hi / lo pieces of g D as A-fragments, [ntiles][hi | lo][64 lanes] of 16 bytes;
    // nullptr when D holds a non-finite entry (no filter then).  marg_coef = 2^-14 (g R)^2, R = largest row 2-norm of D.
    uint4* d_pack16 = nullptr;
    DevArr<int> d_gmax;                                   // per pixel: largest filtered |ip|^2 seen by any wave (float bits), -1 at launch
    float marg_coef = 0.f;
    int filter_on = 1; float margin_scale = 1.f;          // qmri_debug_dict_filter
    // groups of a narrow dictionary (qmri_set_dictionary_groups; dictg_kernels.hip): G = 0 none.  d_gpack / d_gpack16 are
    // d_pack / d_pack16 again with every group starting on a 32-atom tile (gtile_h[g], gtile_h[G] tiles in all); d_gwork is the per-call scratch of
    // the pixel bucketing
    int G = 0, gtiles_max = 0;
    std::vector<int> gtile_h;
    DevArr<float> d_gpack; DevArr<uint4> d_gpack16;
    DevArr<int> d_gptr, d_gtile; DevArr<double> d_gval;
    DevArr<int> d_gwork;
    int slots_g = 0, slots_gf = 0;                        // as slots / slots_f, for the grouped instantiations
    // the B1 estimate (dictb_kernels.hip, api_b1.cpp): scores and box sums of a run of slices, the atom parts' maxima, group_val of a pool call
    DevArr<float> d_bscore, d_bpart; DevArr<double> d_bT, d_bval;
    int slots_b = 0;                                      // workgroups of k_dictb_scores the device holds at once
    std::vector<float> D_h, normD_h, lut_h;               // narrow dictionaries: the caller's D [K x s column-major], normD and lut [K x Q column-major], kept for qmri_set_components and qmri_set_refine
    PvHost pv;                                            // ... and the components in force (C = 0: none); dropped with the dictionary
    RefineHost rf;                                        // ... and the refinement in force (P = 0: none); dropped with the dictionary
};

struct qmri_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    OpHost op;
    NetPlan net;
    DictHost dict;
    CcWork cc;                          // coil compression (cc_kernels.hip)
    int prof_level = 0;
    qmri_profile prof{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_state = nullptr;      // LSQR state copied to the host
    // profile level 2: the 3x3 conv kernels are launched with hipExtLaunchKernelGGL and a (start, stop) event pair each,
    // which takes the timestamps of the kernel's own dispatch packet -- the duration rocprofv3 --kernel-trace reports --
    // without putting extra packets between dependent kernels (event records in the stream add 3-5 us per kernel)
    std::vector<hipEvent_t> chain;      // pairs: [2i] start, [2i+1] stop
    size_t chain_n = 0;                 // events handed out in the current forward
    std::vector<int> chain_kind;        // which accumulator of qmri_profile a pair's duration goes to (PROF_*)
    std::vector<double> chain_flop;     // fp32-equivalent algorithmic flop of the launch(es) a pair brackets (convolutions)
    bool conv6_attr[4][2] = {};         // dynamic LDS size of k_conv6<CFG, SP> allowed
    bool conv6p_attr[2][3] = {{false, false, false}, {false, false, false}};   // ... of k_conv6p<CFG, NRES>
    bool conv6r_attr = false;           // ... of k_conv6r
    bool ks_lds_attr[2] = {false, false};   // large dynamic LDS allowed for the k-space LSQR kernels
    int lsqr_pred = 20;                 // predicted LSQR iteration count for launch chunking
    int ks_persist = -1;                // k_ks_persist (all LSQR iterations in one launch): -1 = knob lsqr_persist (default on), 0 / 1 set by qmri_debug_lsqr_persist
    int ks_persist_cap = -1;            // ... workgroups of it the device holds at once (occupancy query, first use)
    DevArr<void> d_ks_gran;             // ... its tagged partial sums (granules)
    unsigned ks_tag = 16;               // ... tag of the next solve's first granule (tags are unique across solves)
    // round 6 (qmri_get_health): what a slow or repeated reconstruction was doing.  Counters since qmri_create.
    int ks_timeouts = 0;                // one-launch LSQR kernels that gave up waiting for a partial sum (the solve / reconstruction was repeated)
    int admm_repeats = 0;               // qmri_pnp_admm_dev calls that ran their reconstruction a second time (LSQR time-out, f16 range guard, hand-off time-out)
    // profile level 3: stage MARKS -- event records at the stage boundaries of the PnP-ADMM loop, never waited for inside the loop; resolved after
    // the call's own final synchronisation into prof.ms_* and last_call_ms (level 1 synchronises at every boundary and is for stage splits only)
    std::vector<hipEvent_t> marks;      // [2i] start, [2i+1] stop of a stage interval
    std::vector<int> mark_kind;         // 0 x-update, 1 denoiser, 2 elementwise, 3 diagnostics
    size_t marks_n = 0;
    double last_call_ms[4] = {0, 0, 0, 0};   // stage times of the most recent qmri_pnp_admm_dev call (levels 1 and 3)
    double last_call_wall_ms = 0;            // ... its host wall clock, entry to return (always)
    LlrState llr;                       // the regulariser of the PnP-ADMM loops' Step 2 while set (qmri_set_llr), else the network
    bool llr_lds_attr[3] = {false, false, false};   // large dynamic LDS allowed for k_llr_prox<4 | 8 | 16>
    WavState wav;                       // ... or the joint wavelet soft-thresholding (qmri_set_wavelet); at most one of the two is on
    DevArr<double2> wav_s[2];           // its two coefficient stacks (wav_plan.h scratch_elems), grown on first use
    DevArr<double> wav_part, wav_cmax;  // the shrink launch's per-workgroup maxima; the slices' maxima when asked for
    int ncu = 0;                        // CU count of the device (qmri_create)
    int conv_occ[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};   // f32-MFMA conv kernels (conv_kernels.hip): resident workgroups per CU by (kind, MT)
};

OpDev qmri_opdev(const qmri_ctx* ctx);
#define REQUIRE_OP(ctx)                                                                   \
    do {                                                                                  \
        if (!(ctx)) return QMRI_ERR_INVALID_ARG;                                          \
        QMRI_HIP((ctx), hipSetDevice((ctx)->device));                                     \
        if (!(ctx)->op.ready) { qmri_set_error((ctx), "operator not set: call qmri_set_operator first"); return QMRI_ERR_STATE; } \
    } while (0)

// ---------------------------------------------------------------------------------------------------
// kernel launchers (dc_kernels.hip)
// ---------------------------------------------------------------------------------------------------
bool dc_size_supported(int N);
// forward:  src [B][n] -> (mode-dependent) ; tmp workspace [B][n]
int dc_launch_fwd(qmri_ctx* ctx, const OpDev& op, const LsqrDev& ls, int mode, int B, const double2* src, double2* tmp,
                  double2* y_out, double* pdiag);
int dc_launch_adj(qmri_ctx* ctx, const OpDev& op, int B, const double2* y_in, double2* tmp, double2* dst);
int dc_launch_adj_h(qmri_ctx* ctx, const OpDev& op, int B, const double2* tmp, double2* dst, const double2* u = nullptr,
                    double* mm = nullptr, bool mm_cpx = false);   // inverse h-pass only (+ partial min / max of real(dst + u) per workgroup;
                                                                  //  mm_cpx: of its real and imaginary parts)
// the step between the denoiser and the next x-update in one launch (dc_kernels.hip, k_dual_fwd_h)
struct DualArgs {
    const float* out32; const float* in32; int php, pplane; size_t out_bs, in_bs; int residual_noise;
    const double* norm; const double2* x; double2* u; double* pz;
    int complex_tsmi;        // v = complex(plane c, plane c + s) (QMRI_DENOISER_COMPLEX); 0: v = plane c, the reference's real TSMIs
};
int dc_hpass_blocks(const OpDev& op);
// what the ADMM loop fuses into the launches around a solve (qmri_lsqr_run)
struct LsqrFuse { int z_hpass_nblk = 0; const double2* mm_u = nullptr; double* mm = nullptr; bool mm_cpx = false; };
int dc_launch_dual_fwd_h(qmri_ctx* ctx, const OpDev& op, int B, const DualArgs& d, const ActCheckArgs& ac, double2* tmp);
// host functions that cross files: api_operator.cpp (operator), api_xupdate.cpp (DIRECT tables, LSQR), api_net.cpp (denoiser; hidden: file-local until the ADMM drivers left that file), api_dict.cpp
void qmri_free_operator(qmri_ctx* ctx);
void qmri_free_net(qmri_ctx* ctx);
void qmri_free_dict(qmri_ctx* ctx);
int qmri_prepare_direct(qmri_ctx* ctx, double r);
int qmri_lsqr_run(qmri_ctx* ctx, int B, const double2* d_z, double r, double tol, int maxit, double2* d_x,
                  int32_t* iters_out, int32_t* flag_out, double* pdiag, LsqrState* hslot, bool* deferred, const LsqrFuse* fuse);
__attribute__((visibility("hidden"))) int net_forward(qmri_ctx* ctx, int B);                       // in32 -> out32 on the context's padded tensors
__attribute__((visibility("hidden"))) int net_range_tripped(qmri_ctx* ctx, bool& tripped);         // after a synchronisation: a guard of the f16 scheme / the resident launch asks for a repeat
__attribute__((visibility("hidden"))) bool host_range_tripped(const NetPlan& p);                   // ... the same question from the pinned host words, without a copy
// k-space LSQR (kslsqr_kernels.hip)
int ks_launch_init(qmri_ctx* ctx, const OpDev& op, const KsDev& ks, int B, const double2* hpass_tmp = nullptr, bool first_step = true);
int ks_launch_iter(qmri_ctx* ctx, const OpDev& op, const KsDev& ks, int B);
int ks_launch_final(qmri_ctx* ctx, const OpDev& op, const KsDev& ks, int B, double2* tmp);
int ks_persist_plan(qmri_ctx* ctx, const OpDev& op, const KsDev& ks, int B, int* per_launch);                             // slices per k_ks_persist launch (0: not applicable)
int ks_launch_persist(qmri_ctx* ctx, const OpDev& op, const KsDev& ks, int B, void* gran, unsigned tag0, bool init_here, bool* ran);   // all iterations in one launch
size_t ks_gran_bytes(int G, int B);   // tmp <- conj-domain inverse w-pass of xhat
int ks_lds_fits(qmri_ctx* ctx, int N, int s, int M, int vcap, int caps, bool* ok);   // V (vcap doubles) fits the LDS of every k-space LSQR kernel with unit shape `caps`
int dc_launch_direct(qmri_ctx* ctx, const OpDev& op, int B, const double2* z, const double2* chat, double r,
                     double2* tmp, double2* x_out);
// y (ABI order) -> k-sorted order, plus ||y||^2 into state
int dc_launch_sort_y(qmri_ctx* ctx, const OpDev& op, const LsqrDev& ls, int B, const double2* y);
// z = v - u, partial ||z||^2
int dc_launch_prepare_z(qmri_ctx* ctx, const OpDev& op, const LsqrDev& ls, int B, const double2* v, const double2* u,
                        double2* z);
// elementwise ADMM stages (PnP_ADMM.m:115-121,138,144)
int ew_launch_minmax_normalise(qmri_ctx* ctx, int B, size_t n, int plane, int H, int s, int multi_level, double noise_std,
                               const double2* x, const double2* u, double* mm, double* norm, int nblk, const PTensor& in32, bool mm_ready = false,
                               bool complex_tsmi = false);   // complex_tsmi: 2s planes real / imaginary, noise plane 2s
int ew_launch_unnormalise_dual(qmri_ctx* ctx, int B, size_t n, int plane, int H, const PTensor& out32, const PTensor& in32,
                               int residual_noise, const double* norm, const double2* x, double2* u, double2* v, double2* z,
                               double* pz, int nblk_z, int s = 0, bool complex_tsmi = false);   // also z = v - u and the partials of ||z||^2 for the next x-update
int ew_launch_diag(qmri_ctx* ctx, const OpDev& op, const LsqrDev& ls, int B, const double2* x, const double2* gt,
                   double* pd, double* diag_slot, int iters_total, int it);
int ew_launch_pack(qmri_ctx* ctx, int B, int C, int H, int W, const void* src, int src_is_double, const PTensor& dst, float scale = 1.f);
int ew_launch_absmax(qmri_ctx* ctx, const float* x, const float* y, size_t n, unsigned* d_out);   // calibration: max |x - y| (y may be NULL) as a bit pattern
int ew_launch_unpack(qmri_ctx* ctx, int B, int C, int H, int W, const PTensor& out32, const PTensor& in32, int residual_noise,
                     void* dst, int dst_is_double, float scale = 1.f);
int ew_launch_real_to_complex(qmri_ctx* ctx, size_t count, const double* in, double2* out);
// multi-coil extension (ew_kernels.hip): coil maps times image / conjugate coil combination, `cnt` coils of a chunk at a time
int ew_launch_coil_mul(qmri_ctx* ctx, size_t n, size_t plane, int cnt, const double2* x, const double2* maps, double2* out);
int ew_launch_coil_sum(qmri_ctx* ctx, size_t n, size_t plane, int cnt, const double2* xj, const double2* maps, double2* x, int accumulate);

// conv engine (conv_kernels.hip)
int conv_launch(qmri_ctx* ctx, ConvLayer& L, int B, const PTensor& in, const PTensor& out, const PTensor* add1,
                const PTensor* add2, int relu_out);
// profile level 2: what an event pair times
enum { PROF_CONV3 = 0, PROF_CONV2 = 1, PROF_LSQR = 2, PROF_TV = 3 };
int qmri_prof_pair(qmri_ctx* ctx, hipEvent_t* start, hipEvent_t* stop, int kind = PROF_CONV3, double flop = 0.0);   // profile level 2: next event pair (else nullptrs)
int qmri_prof_chain_finish(qmri_ctx* ctx, long count = -1);   // synchronises, adds the pairs' durations to the profile; count >= 0: only the first `count` pairs
// 16-bit matrix-core path of the convolutions, f16 x 3 or bf16 x 6 products (conv6_kernels.hip; 2x2 / stride-2 layers: conv6s_kernels.hip)
bool conv6_enabled();
int conv6_act_begin(qmri_ctx* ctx, int nlayers);           // f16 scheme: start / finish the per-layer |output| report of a forward pass
int conv6_act_end(qmri_ctx* ctx);
int conv6_default_sp();                                    // 2 = f16 x 3 products, 3 = bf16 x 6 products (knob conv_scheme = 3)
bool conv6_weights_fit_f16(const float* w, size_t n);
void conv6_plan_pack(ConvLayer& L, const float* w, std::vector<uint16_t>& packed);
int conv6_pack_dev(qmri_ctx* ctx, ConvLayer& L, const float* d_w, float wmax);       // the same on the device from the flat blob there (allocates L.wp6)
int conv6s_pack_dev(qmri_ctx* ctx, ConvLayer& L, const float* d_w, float wmax);
int conv_pack_weights_dev(qmri_ctx* ctx, ConvLayer& L, const float* d_w);           // ... the f32 A-fragments of the fallback kernels (allocates L.wp)
int conv6_launch(qmri_ctx* ctx, const ConvLayer& L, int B, const PTensor& in, const PTensor& out, const PTensor* add1,
                 const PTensor* add2, int relu_out);           // every 3x3 layer; its launch form: conv6_form.h conv6_choose_form
// a run of 3x3 layers of the full-resolution level as ONE launch with LDS-resident tiles (conv6r_kernels.hip k_conv6r): nres = 2 nb ResBlock layers
// 64 -> 64 on src -> cur (+ skip at the last one), optionally with the network's head in front (head_in -> src)
struct Conv6rRun {
    const ConvLayer* head = nullptr; const PTensor* head_in = nullptr;
    const ConvLayer* res = nullptr; int nres = 0;
    const PTensor* src = nullptr; const PTensor* cur = nullptr; const PTensor* skip = nullptr;
    const ConvLayer* tail = nullptr; const PTensor* tail_out = nullptr;   // optional last layer 64 -> out_nc writing the planar network output
    const ConvLayer* down = nullptr; const PTensor* down_out = nullptr;   // optional last layer: the level's 2x2 / stride-2 convolution 64 -> 128 into the next level's tensor (cur is then not written)
};
int conv6r_try(qmri_ctx* ctx, const Conv6rRun& run, int B, bool* done);   // *done = false: not eligible, nothing launched
size_t conv6r_xbuf_bytes(int tiles);
void conv6s_plan_pack(ConvLayer& L, const float* w, std::vector<uint16_t>& packed);   // 2x2 / stride-2 layers
bool conv6s_usable(const ConvLayer& L, const PTensor& in, const PTensor& out);
int conv6s_launch(qmri_ctx* ctx, const ConvLayer& L, int B, const PTensor& in, const PTensor& out);
size_t conv_pack_weights(const ConvLayer& L, const float* w_src, std::vector<float>& packed);
void conv_plan_layer(ConvLayer& L, ConvKind kind, int Cin, int Cout);

// dictionary match (dict_kernels.hip)
// `cache` (a slots_* of DictHost) = workgroups of `kernel` the device holds at once; queried on first use
template <class Kernel>
int dict_resident_slots(qmri_ctx* ctx, Kernel kernel, int threads, int& cache) {
    if (cache) return QMRI_OK;
    int per_cu = 0;
    hipDeviceProp_t prop;
    QMRI_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
    QMRI_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0));
    cache = std::max(1, per_cu) * prop.multiProcessorCount;
    return QMRI_OK;
}
// f(std::integral_constant<int, NPAIR>) for the channel pairs of a narrow dictionary, 1 .. 8: the kernels are instantiated per pair count
template <class F>
void dict_dispatch_npair(int npair, F&& f) {
    switch (npair) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}
int dict_launch(qmri_ctx* ctx, const double2* d_X, int Npix, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm, float2* d_xfit);
int dict_launch_xfit(qmri_ctx* ctx, const float4* win, int Npix, float2* d_xfit);
// grouped match (dictg_kernels.hip: groups, pixel bucketing; dict_kernels.hip: the match on slot tiles)
struct DictGroupView;
int dict_group_pixel_width(const qmri_ctx* ctx);
int dict_launch_grouped(qmri_ctx* ctx, const double2* d_X, int Npix, const DictGroupView& gv, int nslot_tiles, float* d_qmap, float* d_pd, float* d_mt,
                        int32_t* d_dm, float4* win);
int dictg_set_groups(qmri_ctx* ctx, int G, const int32_t* group_ptr, const double* group_val);
void dictg_free(qmri_ctx* ctx);
int dictg_launch(qmri_ctx* ctx, const double2* d_X, int Npix, const double* d_sel, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm, int32_t* d_grp,
                 float2* d_xfit);
int dict_launch_merge(qmri_ctx* ctx, const float4* part, int P, int Npix, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm, float4* win);
// B1 estimate (dictb_kernels.hip): group scores of the pixels p0 .. p0 + n - 1 of X (Npix x s), d_score[g * n + i]; the pooled argmax of the slices
// sl0 .. sl0 + nsl - 1, d_score[g * sstride + (pixel - soff)], mask and outputs by pixel of the whole stack
int dictb_launch_scores(qmri_ctx* ctx, const double2* d_X, size_t Npix, size_t p0, int n, float* d_score);
int b1_launch_pool(qmri_ctx* ctx, int G, const double* d_gval, int N, int M, int sl0, int nsl, const float* d_score, size_t sstride, size_t soff,
                   const uint8_t* d_mask, int hw, double* d_b1, int32_t* d_grp, double* d_conf);
// wide dictionaries (16 < s <= 1024; dictw_kernels.hip)
int dictw_pack_dictionary(qmri_ctx* ctx, const float* D_host, int K, int s);    // fills ctx->dict.d_pack / G8 / ntiles
int dictw_launch(qmri_ctx* ctx, const double2* d_X, int Npix, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm, float4* win);
