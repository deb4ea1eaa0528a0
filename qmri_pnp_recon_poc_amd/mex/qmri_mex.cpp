// qmri_mex.cpp -- MATLAB gateway for libqmri.so (compile-gated: needs mex.h, which is absent from the build image).
//
//   mex -R2018a qmri_mex.cpp -I../../include -L.. -lqmri        (interleaved-complex API: mxComplexDouble == (re,im) doubles)
//
// One mexFunction with a leading command string; a persistent context is created on first use and released by
// mexAtExit.  Every libqmri status != 0 becomes mexErrMsgIdAndTxt('qmri:<code>', qmri_last_error(ctx)), which is how
// the reference's plugins report errors (MATLAB exceptions, denoiseImage_PnP_ADMM.m:123-135).
// The MATLAB wrappers in ../matlab give these commands the reference's own signatures.
//
// Batches and devices (round 5).  The reference's denoiser handle takes H x W x C x N batches (denoiseImage_PnP_ADMM.m:13-17) and north_star
// shards a slice batch over the GPUs of a node.  The gateway therefore
//   * keeps persistent copies of what defines the plans (V / frame_ptr / kidx, the denoiser's weights and shape, the dictionary), so that
//   * a call that brings more slices than the current plan holds re-plans by itself: 'denoise' with a 4-D array of N > max_batch slices,
//     'pnp_admm' with a measurement MATRIX (m x S) -- the plan then grows to min(S, 15) slices per launch;
//   * 'device' selects the GPU of the single-context commands;
//   * 'recon_batch' hands a whole slice stack to qmri_recon_batch: one worker (host thread + context) per entry of `devs`, slices_per_launch
//     slices advanced together on each (k_conv6p, batched LSQR), x and the T1 / T2 / PD maps of every slice back.
//   * 'set_trajectory' plans a non-Cartesian operator (qmri_set_operator_nufft; 'build_spiral_traj' gives the reference's spiral before rounding):
//     'forward', 'adjoint' and 'pnp_admm' then run on it (a measurement matrix slice by slice; no diagnostics), 'recon_batch*' refuse it.
//     'normal' applies A^H A as a Toeplitz convolution (qmri_normal) and param.solver = 2 ('toeplitz' in PnP_ADMM_hip.m) solves the x-update with it.
//     'dcf' computes and attaches density weights (qmri_nufft_dcf; extension), 'set_sample_weights' attaches the caller's,
//     'adjoint_w' is the weighted adjoint A^H (w .* y).  Re-planning the operator drops the weights: 'set_trajectory', 'device', and any
//     call that brings more slices than the plan's max_batch (it re-plans the operator for them); call 'dcf' / 'set_sample_weights' again after it.
//     'set_field_map' attaches a field map for the off-resonance correction (qmri_set_field_map; extension).  The same
//     re-plans drop the map with the weights: call 'set_field_map' again after them.
//     'prepare_normal_fm' builds the Toeplitz normal operator of the attached map (qmri_nufft_prepare_normal_fm; extension):
//     'normal' and param.solver = 2 then run with the map.  param.field_normal = 1 (with field_normal_nseg / field_normal_tol; param.field_normal
//     in PnP_ADMM_hip.m) has 'pnp_admm' build it before the loop.  A new map, or any re-plan above, drops it.
//   * 'recon_batch_mc' is the same for multi-coil stacks, every slice with its own coil maps (qmri_recon_batch_mc; an extension, no reference
//     counterpart); with a coil-compression argument every launch compresses its slices on the device first (qmri_recon_batch_mc_cc).
//   * 'coil_compress' compresses a multi-coil stack to virtual coils (qmri_coil_compress; extension).
//   * 'coil_maps' estimates coil sensitivity maps from calibration data (qmri_coil_maps; extension).
//   * 'dict_compress' compresses a simulated dictionary to its SVD subspace (qmri_dict_compress; extension); it needs no plan.
//   * 'dict_simulate' simulates the fingerprints of a FISP-MRF sequence by extended phase graphs (qmri_dict_simulate; extension); it needs no plan.
//   * 'dict_simulate_sp' is 'dict_simulate' integrated over a slice profile (qmri_dict_simulate_sp; extension); it needs no plan.
//   * 'dict_simulate_seq' simulates a prepared, repeated FISP train, block by block (qmri_dict_simulate_seq; extension); it needs no plan.
//   * 'dict_simulate_grad' is 'dict_simulate' with the derivatives of the fingerprints and their Cramer-Rao bound (qmri_dict_simulate_grad;
//     extension); it needs no plan.
//   * 'set_llr' / 'clear_llr' select the locally low-rank proximal step as Step 2 of 'pnp_admm' (qmri_set_llr; extension), which
//     then needs no denoiser; 'llr_prox' is the step alone (qmri_llr_prox).
//   * 'set_wavelet' / 'clear_wavelet' select joint wavelet soft-thresholding as Step 2 of 'pnp_admm' the same way (qmri_set_wavelet; extension,
//     DESIGN.md section 29); 'wavelet_prox' is the step alone (qmri_wavelet_prox).  One of the two regularisers at a time.
//   * 'field_map_estimate' estimates the field map that 'set_field_map' takes from multi-echo images (qmri_field_map_estimate; extension, DESIGN.md
//     section 24); it needs no plan.
// tests/cpp/mex_mock.cpp is a small stand-in for the MATLAB runtime's C API under which this file is compiled, LINKED against libqmri.so and
// driven command by command on the GPU box (tests/test_gpu_mex.py); with MATLAB's own mex.h nothing here changes.
#include "mex.h"
#include "qmri.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static qmri_ctx* g_ctx = nullptr;
static int g_device = 0;

// what the current plans were made from (persistent mxArrays: they survive the call that brought them)
struct OperatorSpec { mxArray* V = nullptr; mxArray* fp = nullptr; mxArray* kidx = nullptr; int N = 0, M = 0, max_batch = 0;
                     mxArray* omega = nullptr; int width = 0; };      // omega (m x 2) set: a trajectory operator ('set_trajectory'), kidx unset
struct DenoiserSpec { mxArray* w = nullptr; qmri_net_desc d{}; int H = 0, W = 0, max_batch = 0; };
struct DictSpec { mxArray* D = nullptr; mxArray* normD = nullptr; mxArray* lut = nullptr; };
static OperatorSpec g_op;
static DenoiserSpec g_net;
static DictSpec g_dict;
static std::vector<int32_t> g_comp;                    // 'set_components' in force (1-based atoms); 'set_dictionary' drops them
static std::vector<int32_t> g_refine;                  // 'set_refine' in force (0-based lut columns); 'set_dictionary' drops them
static int g_ngroups = 0;                              // 'set_dictionary_groups' in force (G); 'set_dictionary' and a device switch drop them
static bool g_llr = false;                             // 'set_llr' is in force: 'pnp_admm' needs no denoiser
static bool g_wav = false;                             // 'set_wavelet' is in force: the same
static mxArray* g_sms = nullptr;                       // 'set_sms' in force (E, T x Z complex double): re-attached whenever the operator is re-planned; a new operator drops it
static const int DEFAULT_SLICES_PER_LAUNCH = 15;       // what a measurement matrix grows the plans to (the batched kernels' design point)

static void drop(mxArray*& a) { if (a) { mxDestroyArray(a); a = nullptr; } }
static mxArray* keep(const mxArray* a) { mxArray* c = mxDuplicateArray(a); mexMakeArrayPersistent(c); return c; }

static void cleanup() {
    if (g_ctx) { qmri_destroy(g_ctx); g_ctx = nullptr; }
    drop(g_op.V); drop(g_op.fp); drop(g_op.kidx); drop(g_op.omega); g_op = OperatorSpec();
    drop(g_net.w); g_net = DenoiserSpec();
    drop(g_dict.D); drop(g_dict.normD); drop(g_dict.lut);
    drop(g_sms);
    g_comp.clear();
    g_refine.clear();
    g_ngroups = 0;
    g_llr = false;
    g_wav = false;
}

static void check(int st) {
    if (st == QMRI_OK) return;
    char id[32];
    snprintf(id, sizeof id, "qmri:err%d", -st);
    mexErrMsgIdAndTxt(id, "%s", qmri_last_error(g_ctx));
}

static qmri_ctx* ctx() {
    if (!g_ctx) {
        int st = qmri_create(g_device, &g_ctx);
        if (st != QMRI_OK) mexErrMsgIdAndTxt("qmri:create", "%s", qmri_last_error(nullptr));
    }
    static bool registered = false;
    if (!registered) { mexAtExit(cleanup); mexLock(); registered = true; }
    return g_ctx;
}

static double scalar_field(const mxArray* s, const char* name, double dflt) {
    const mxArray* f = mxGetField(s, 0, name);
    return f ? mxGetScalar(f) : dflt;
}

static void need(int nrhs, int n, const char* usage) {
    if (nrhs < n) mexErrMsgIdAndTxt("qmri:usage", "%s", usage);
}
// The C ABI takes plain pointers: what a MATLAB array must be and hold is checked HERE, before the library reads it (a wrong class or a short
// array would otherwise be read past its end).  Errors are MATLAB exceptions with an identifier, like the reference's validateInputImage.
static void want(bool ok, const char* id, const char* msg) {
    if (!ok) mexErrMsgIdAndTxt(id, "%s", msg);
}
static bool is_cdouble(const mxArray* a) { return mxIsDouble(a) && mxIsComplex(a); }
// a MATLAB scalar that is about to become an int / size_t: real, finite, integer-valued and inside [lo, hi] BEFORE the cast (a NaN or a negative
// double cast to an integer type is undefined behaviour)
static int int_arg(const mxArray* a, double lo, double hi, const char* id, const char* msg) {
    want(a && mxIsDouble(a) && !mxIsComplex(a) && mxGetNumberOfElements(a) == 1, id, msg);
    const double v = mxGetScalar(a);
    want(std::isfinite(v) && v == std::floor(v) && v >= lo && v <= hi, id, msg);
    return (int)v;
}
static size_t image_numel() {                                       // N * M * s of the planned operator
    want(g_op.V != nullptr, "qmri:state", "no operator: call qmri_mex('set_operator', ...) (qmri_make_F) first");
    return (size_t)g_op.N * (size_t)g_op.M * mxGetN(g_op.V);
}
static size_t dims_numel(const mxArray* d) {                        // the [N M s] argument
    want(mxIsDouble(d) && !mxIsComplex(d) && mxGetNumberOfElements(d) == 3, "qmri:size", "the size argument must be [N M s]");
    const double* v = mxGetDoubles(d);
    for (int i = 0; i < 3; ++i) want(std::isfinite(v[i]) && v[i] == std::floor(v[i]) && v[i] >= 1 && v[i] <= 1e6, "qmri:size", "[N M s] must hold positive integers");
    const size_t n = (size_t)v[0] * (size_t)v[1] * (size_t)v[2];
    want(n == image_numel(), "qmri:size", "[N M s] does not match the operator (N x M grid, s = columns of V)");
    return n;
}
static size_t operator_m() {
    int m = 0;
    check(qmri_operator_m(ctx(), &m));
    return (size_t)m;
}

// nseg and tol of the field-aware normal operator ('prepare_normal_fm', param.field_normal): nseg 0 or 2..32, tol finite and >= 0
static qmri_offres_normal_params normal_fm_params(const mxArray* nseg, const mxArray* tol, const char* id_nseg, const char* id_tol) {
    qmri_offres_normal_params p{};
    if (nseg) {
        p.nseg = int_arg(nseg, 0, 32, id_nseg, "nseg must be an integer in 2..32 (0: automatic)");
        want(p.nseg != 1, id_nseg, "nseg must be an integer in 2..32 (0: automatic)");
    }
    if (tol) {
        want(mxIsDouble(tol) && !mxIsComplex(tol) && mxGetNumberOfElements(tol) == 1, id_tol, "tol must be a real double scalar");
        p.tol = mxGetScalar(tol);
        want(std::isfinite(p.tol) && p.tol >= 0.0, id_tol, "tol must be finite and >= 0 (0: the default 1e-4)");
    }
    return p;
}

// (re-)make the plans from the kept specifications
static void plan_operator(int max_batch) {
    const int T = (int)mxGetM(g_op.V), s = (int)mxGetN(g_op.V);
    if (g_op.omega) {                                               // MATLAB's m x 2 (column-major) -> the ABI's interleaved (omega1, omega2) pairs
        const size_t m = mxGetM(g_op.omega);
        const double* om = mxGetDoubles(g_op.omega);
        std::vector<double> pairs(2 * m);
        for (size_t i = 0; i < m; ++i) { pairs[2 * i] = om[i]; pairs[2 * i + 1] = om[m + i]; }
        qmri_nufft_params np{};
        np.width = g_op.width;
        check(qmri_set_operator_nufft(ctx(), g_op.N, g_op.M, s, T, mxGetDoubles(g_op.V), (const int32_t*)mxGetData(g_op.fp), pairs.data(), max_batch, &np));
    } else {
        check(qmri_set_operator(ctx(), g_op.N, g_op.M, s, T, mxGetDoubles(g_op.V), (const int32_t*)mxGetData(g_op.fp), (const int32_t*)mxGetData(g_op.kidx), max_batch));
    }
    g_op.max_batch = max_batch;
    if (g_sms) check(qmri_set_sms(ctx(), (int)mxGetN(g_sms), mxGetComplexDoubles(g_sms)));   // (the library drops the phases with the operator)
}
static void plan_denoiser(int max_batch) {
    check(qmri_set_denoiser(ctx(), &g_net.d, (const float*)mxGetData(g_net.w), mxGetNumberOfElements(g_net.w) * 4, g_net.H, g_net.W, max_batch));
    g_net.max_batch = max_batch;
}
static void plan_dictionary() {
    check(qmri_set_dictionary(ctx(), (int)mxGetM(g_dict.D), (int)mxGetN(g_dict.D), (int)mxGetN(g_dict.lut), (const float*)mxGetData(g_dict.D),
                              (const float*)mxGetData(g_dict.normD), (const float*)mxGetData(g_dict.lut)));
}
// a call brings B slices: grow the plans that hold fewer
static void reserve(int B, bool op, bool net) {
    if (op && g_op.V && B > g_op.max_batch) plan_operator(B);
    if (net && g_net.w && B > g_net.max_batch) plan_denoiser(B);
}

static qmri_admm_params admm_params(const mxArray* P, bool want_diag) {
    qmri_admm_params p;
    p.gamma = scalar_field(P, "gamma", 0.05);
    p.iters = (int)scalar_field(P, "iter", 100);
    p.cg_tol = scalar_field(P, "cg_tol", 1e-4);
    p.cg_maxit = 100;                                               // literal in PnP_ADMM.m:102
    p.solver = (int)scalar_field(P, "solver", QMRI_SOLVER_LSQR);
    p.denoiser_type = (int)scalar_field(P, "multi_level", 0);
    if (scalar_field(P, "complex_tsmi", 0) != 0) p.denoiser_type |= QMRI_DENOISER_COMPLEX;   // param.tsmi_domain = 'complex' 
    p.noise_std = scalar_field(P, "noise_std", 0.01);
    p.want_diag = want_diag ? 1 : 0;
    return p;
}

// coil compression options: a scalar nv, or a struct with the fields nv (default 0: choose by energy), energy (default 0.99), shared (default 0)
static qmri_cc_params cc_params(const mxArray* a, const char* id) {
    qmri_cc_params p;
    p.nv = 0; p.energy = 0.99; p.shared = 0;
    if (mxIsStruct(a)) {
        const mxArray* f = mxGetField(a, 0, "nv");
        if (f) p.nv = int_arg(f, 0, 1024, id, "cc.nv must be an integer in [0, ncoil]");
        p.energy = scalar_field(a, "energy", 0.99);
        f = mxGetField(a, 0, "shared");
        if (f) p.shared = int_arg(f, 0, 1, id, "cc.shared must be 0 or 1");
    } else {
        p.nv = int_arg(a, 0, 1024, id, "cc must be a scalar nv or a struct with fields nv, energy, shared");
    }
    return p;
}
// a noise covariance argument: [] or a complex double ncoil x ncoil matrix
static const void* noise_cov_arg(const mxArray* a, size_t ncoil, const char* id) {
    if (mxIsEmpty(a)) return nullptr;
    want(is_cdouble(a) && mxGetM(a) == ncoil && mxGetN(a) == ncoil, id, "noise_cov must be [] or complex double, ncoil x ncoil");
    return mxGetComplexDoubles(a);
}

// Simultaneous multi-slice groups (extension).  MATLAB shapes: maps N x M x ncoil x Z x G, y m x ncoil x G, images
// N x M x s x Z x G (trailing singleton dimensions may be missing); Z is the column count of the E of 'set_sms'.
static size_t dim_or_1(const mxArray* a, size_t k) { return k < mxGetNumberOfDimensions(a) ? mxGetDimensions(a)[k] : 1; }
struct SmsShape { size_t ncoil, Z, G; };
static SmsShape sms_shape(const mxArray* maps, const char* id) {
    want(is_cdouble(maps) && mxGetNumberOfDimensions(maps) <= 5, id, "maps must be complex double, N x M x ncoil x Z x G");   // (what needs no plan comes first)
    (void)image_numel();
    want(g_sms != nullptr, "qmri:state", "no simultaneous multi-slice phases: call qmri_mex('set_sms', E) (qmri_set_sms) first");
    SmsShape sh;
    sh.Z = mxGetN(g_sms);
    want(dim_or_1(maps, 0) == (size_t)g_op.N && dim_or_1(maps, 1) == (size_t)g_op.M, id, "maps must be complex double, N x M x ncoil x Z x G");
    sh.ncoil = dim_or_1(maps, 2);
    sh.G = dim_or_1(maps, 4);
    want(sh.ncoil >= 1 && sh.ncoil <= 1024 && dim_or_1(maps, 3) == sh.Z && sh.G >= 1, id, "maps must be N x M x ncoil x Z x G with 1 <= ncoil <= 1024 and the Z of 'set_sms'");
    return sh;
}
static void sms_want_y(const mxArray* y, const SmsShape& sh, const char* id) {
    want(is_cdouble(y) && mxGetNumberOfElements(y) == operator_m() * sh.ncoil * sh.G && dim_or_1(y, 0) == operator_m(), id, "y must be complex double, m x ncoil x G");
}
static void sms_want_images(const mxArray* x, const SmsShape& sh, bool real_ok, const char* id) {
    want(mxIsDouble(x) && (real_ok || mxIsComplex(x)) && mxGetNumberOfElements(x) == image_numel() * sh.Z * sh.G && dim_or_1(x, 0) == (size_t)g_op.N, id,
         "the images must be complex double, N x M x s x Z x G");
}
static mxArray* sms_new_images(const SmsShape& sh) {
    const mwSize dims[5] = {(mwSize)g_op.N, (mwSize)g_op.M, (mwSize)mxGetN(g_op.V), (mwSize)sh.Z, (mwSize)sh.G};
    return mxCreateNumericArray(5, dims, mxDOUBLE_CLASS, mxCOMPLEX);
}

static void set_denoiser_from(const mxArray* w, const qmri_net_desc& d, int H, int W, int max_batch) {
    if (!mxIsSingle(w) || mxIsComplex(w)) mexErrMsgIdAndTxt("qmri:set_denoiser:type", "the weights must be a real single vector");
    drop(g_net.w);
    g_net.w = keep(w); g_net.d = d; g_net.H = H; g_net.W = W;
    plan_denoiser(std::max(1, max_batch));
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 1 || !mxIsChar(prhs[0])) mexErrMsgIdAndTxt("qmri:usage", "first argument must be a command string");
    char cmd[64];
    mxGetString(prhs[0], cmd, sizeof cmd);
    const std::string c(cmd);

    if (c == "device") {                             // qmri_mex('device', d): the GPU of the single-context commands (plans are re-made on it)
        need(nrhs, 2, "qmri_mex('device', d)");
        const int d = int_arg(prhs[1], 0, 1023, "qmri:device", "the device id must be a non-negative integer");
        if (d != g_device || !g_ctx) {
            // try the new device first: a failed qmri_create must leave the gateway on the device it had (with its context and plans)
            qmri_ctx* fresh = nullptr;
            if (qmri_create(d, &fresh) != QMRI_OK) mexErrMsgIdAndTxt("qmri:create", "%s", qmri_last_error(nullptr));
            if (g_ctx) qmri_destroy(g_ctx);
            g_ctx = fresh; g_device = d;
            g_ngroups = 0;                                          // (the groups lived in the old context)
            (void)ctx();                                            // (registers the exit hook and the lock on first use)
            if (g_op.V) plan_operator(std::max(1, g_op.max_batch));
            if (g_net.w) plan_denoiser(std::max(1, g_net.max_batch));
            if (g_dict.D) plan_dictionary();
            if (g_dict.D && !g_comp.empty()) check(qmri_set_components(ctx(), (int)g_comp.size(), g_comp.data(), nullptr));
            if (g_dict.D && !g_refine.empty()) check(qmri_set_refine(ctx(), (int)g_refine.size(), g_refine.data(), nullptr));
        }
        if (nlhs > 0) plhs[0] = mxCreateDoubleScalar((double)g_device);
    } else if (c == "set_operator") {                // qmri_mex('set_operator', N, M, V, frame_ptr(int32), kidx(int32) [, max_batch])
        need(nrhs, 6, "qmri_mex('set_operator', N, M, V, frame_ptr, kidx [, max_batch])");
        if (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])) mexErrMsgIdAndTxt("qmri:set_operator:type", "V must be a real double T x s matrix");
        want(mxIsInt32(prhs[4]) && mxIsInt32(prhs[5]), "qmri:set_operator:type", "frame_ptr and kidx must be int32 (as 'build_spiral' / 'build_epi' return them)");
        {
            const size_t T = mxGetM(prhs[3]);
            want(mxGetNumberOfElements(prhs[4]) == T + 1, "qmri:set_operator:size", "frame_ptr must have T + 1 entries (T = rows of V)");
            const int32_t total = ((const int32_t*)mxGetData(prhs[4]))[T];
            want(total >= 0 && mxGetNumberOfElements(prhs[5]) == (size_t)total, "qmri:set_operator:size", "kidx must have frame_ptr(end) entries");
        }
        const int Nn = int_arg(prhs[1], 1, 65536, "qmri:set_operator:size", "N must be a positive integer");
        const int Mm = int_arg(prhs[2], 1, 65536, "qmri:set_operator:size", "M must be a positive integer");
        const int mb = nrhs > 6 ? int_arg(prhs[6], 1, 4096, "qmri:set_operator:size", "max_batch must be a positive integer") : 1;
        drop(g_op.V); drop(g_op.fp); drop(g_op.kidx); drop(g_op.omega); g_op = OperatorSpec();
        drop(g_sms);
        g_op.N = Nn; g_op.M = Mm;
        g_op.V = keep(prhs[3]); g_op.fp = keep(prhs[4]); g_op.kidx = keep(prhs[5]);
        plan_operator(mb);
    } else if (c == "set_trajectory") {              // qmri_mex('set_trajectory', N, M, V, frame_ptr(int32), omega(m x 2 double) [, max_batch [, width]])
        need(nrhs, 6, "qmri_mex('set_trajectory', N, M, V, frame_ptr, omega [, max_batch [, width]])");
        want(mxIsDouble(prhs[3]) && !mxIsComplex(prhs[3]), "qmri:set_trajectory:type", "V must be a real double T x s matrix");
        want(mxIsInt32(prhs[4]), "qmri:set_trajectory:type", "frame_ptr must be int32 (as 'build_spiral_traj' returns it)");
        want(mxIsDouble(prhs[5]) && !mxIsComplex(prhs[5]) && mxGetNumberOfDimensions(prhs[5]) == 2 && mxGetN(prhs[5]) == 2, "qmri:set_trajectory:type",
             "omega must be a real double m x 2 matrix (radians per pixel; column 1 along N, column 2 along M)");
        {
            const size_t T = mxGetM(prhs[3]);
            want(mxGetNumberOfElements(prhs[4]) == T + 1, "qmri:set_trajectory:size", "frame_ptr must have T + 1 entries (T = rows of V)");
            const int32_t total = ((const int32_t*)mxGetData(prhs[4]))[T];
            want(total >= 0 && mxGetM(prhs[5]) == (size_t)total, "qmri:set_trajectory:size", "omega must have frame_ptr(end) rows");
        }
        const int Nn = int_arg(prhs[1], 1, 65536, "qmri:set_trajectory:size", "N must be a positive integer");
        const int Mm = int_arg(prhs[2], 1, 65536, "qmri:set_trajectory:size", "M must be a positive integer");
        const int mb = nrhs > 6 ? int_arg(prhs[6], 1, 4096, "qmri:set_trajectory:size", "max_batch must be a positive integer") : 1;
        const int wd = nrhs > 7 ? int_arg(prhs[7], 0, 64, "qmri:set_trajectory:size", "width must be a non-negative integer (0: the default)") : 0;
        drop(g_op.V); drop(g_op.fp); drop(g_op.kidx); drop(g_op.omega); g_op = OperatorSpec();
        drop(g_sms);
        g_op.N = Nn; g_op.M = Mm; g_op.width = wd;
        g_op.V = keep(prhs[3]); g_op.fp = keep(prhs[4]); g_op.omega = keep(prhs[5]);
        plan_operator(mb);
    } else if (c == "build_spiral_traj") {           // [frame_ptr, omega] = qmri_mex('build_spiral_traj', N, S, T)   (host code: no GPU needed)
        need(nrhs, 4, "[frame_ptr, omega] = qmri_mex('build_spiral_traj', N, S, T)");
        const int N = int_arg(prhs[1], 1, 65536, "qmri:build_spiral_traj:size", "N must be a positive integer");
        const int S = int_arg(prhs[2], 2, 1 << 20, "qmri:build_spiral_traj:size", "S must be an integer >= 2");
        const int T = int_arg(prhs[3], 1, 65535, "qmri:build_spiral_traj:size", "T must be a positive integer");
        want((double)S * T <= 2147483647.0, "qmri:build_spiral_traj:size", "S * T exceeds the int32 sample index");
        const size_t m = (size_t)S * T;
        std::vector<double> pairs(2 * m);
        int mo = 0;
        plhs[0] = mxCreateNumericMatrix(T + 1, 1, mxINT32_CLASS, mxREAL);
        if (qmri_build_spiral_traj(nullptr, N, S, T, (int32_t*)mxGetData(plhs[0]), pairs.data(), (int)m, &mo) != QMRI_OK)
            mexErrMsgIdAndTxt("qmri:mask", "%s", qmri_last_error(nullptr));
        mxArray* om = mxCreateDoubleMatrix(m, 2, mxREAL);
        double* o = mxGetDoubles(om);
        for (size_t i = 0; i < m; ++i) { o[i] = pairs[2 * i]; o[m + i] = pairs[2 * i + 1]; }
        if (nlhs > 1) plhs[1] = om; else mxDestroyArray(om);
    } else if (c == "build_spiral" || c == "build_epi") {   // [frame_ptr, kidx] = qmri_mex('build_spiral', N, S, T)   (host integer code: no GPU needed)
        need(nrhs, 4, "[frame_ptr, kidx] = qmri_mex('build_spiral', N, S, T) | qmri_mex('build_epi', N, M, pct, T)");
        const int N = (int)mxGetScalar(prhs[1]);
        int m = 0, st;
        if (c == "build_spiral") {
            const int S = (int)mxGetScalar(prhs[2]), T = (int)mxGetScalar(prhs[3]);
            plhs[0] = mxCreateNumericMatrix(T + 1, 1, mxINT32_CLASS, mxREAL);
            mxArray* k = mxCreateNumericMatrix((size_t)S * T, 1, mxINT32_CLASS, mxREAL);
            st = qmri_build_spiral(nullptr, N, S, T, (int32_t*)mxGetData(plhs[0]), (int32_t*)mxGetData(k), S * T, &m);
            mxSetM(k, m);
            plhs[1] = k;
        } else {
            need(nrhs, 5, "[frame_ptr, kidx] = qmri_mex('build_epi', N, M, pct, T)");
            const int M = (int)mxGetScalar(prhs[2]);
            const double pct = mxGetScalar(prhs[3]);
            const int T = (int)mxGetScalar(prhs[4]);
            const int cap = N * M * T;
            plhs[0] = mxCreateNumericMatrix(T + 1, 1, mxINT32_CLASS, mxREAL);
            mxArray* k = mxCreateNumericMatrix((size_t)cap, 1, mxINT32_CLASS, mxREAL);
            st = qmri_build_epi(nullptr, N, M, pct, T, (int32_t*)mxGetData(plhs[0]), (int32_t*)mxGetData(k), cap, &m);
            mxSetM(k, m);
            plhs[1] = k;
        }
        if (st != QMRI_OK) mexErrMsgIdAndTxt("qmri:mask", "%s", qmri_last_error(nullptr));
    } else if (c == "forward") {                     // y = qmri_mex('forward', x)   (F.forward, main_recon_tsmis_FFT.m:228)
        need(nrhs, 2, "y = qmri_mex('forward', x)");
        want(mxIsDouble(prhs[1]) && mxGetNumberOfElements(prhs[1]) == image_numel(), "qmri:forward:size", "x must be a double N x M x s array");
        plhs[0] = mxCreateDoubleMatrix(operator_m(), 1, mxCOMPLEX);
        const bool cx = mxIsComplex(prhs[1]);
        check(qmri_forward(ctx(), cx ? (const void*)mxGetComplexDoubles(prhs[1]) : (const void*)mxGetDoubles(prhs[1]), cx,
                           mxGetComplexDoubles(plhs[0])));
    } else if (c == "adjoint") {                     // x = qmri_mex('adjoint', y, [N M s])   (F.adjoint, :229)
        need(nrhs, 3, "x = qmri_mex('adjoint', y, [N M s])");
        (void)dims_numel(prhs[2]);
        want(is_cdouble(prhs[1]) && mxGetNumberOfElements(prhs[1]) == operator_m(), "qmri:adjoint:size", "y must be a complex double vector with one entry per sample");
        const double* d = mxGetDoubles(prhs[2]);
        const mwSize dims[3] = {(mwSize)d[0], (mwSize)d[1], (mwSize)d[2]};
        plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxCOMPLEX);
        check(qmri_adjoint(ctx(), mxGetComplexDoubles(prhs[1]), mxGetComplexDoubles(plhs[0])));
    } else if (c == "normal") {                      // z = qmri_mex('normal', x): A^H A x on a trajectory operator (qmri_normal)
        need(nrhs, 2, "z = qmri_mex('normal', x)");
        want(mxIsDouble(prhs[1]) && mxGetNumberOfElements(prhs[1]) == image_numel(), "qmri:normal:size", "x must be a double N x M x s array");
        plhs[0] = mxCreateNumericArray(mxGetNumberOfDimensions(prhs[1]), mxGetDimensions(prhs[1]), mxDOUBLE_CLASS, mxCOMPLEX);
        const bool cx = mxIsComplex(prhs[1]);
        check(qmri_normal(ctx(), cx ? (const void*)mxGetComplexDoubles(prhs[1]) : (const void*)mxGetDoubles(prhs[1]), cx,
                          mxGetComplexDoubles(plhs[0])));
    } else if (c == "dcf") {                         // [w, info] = qmri_mex('dcf' [, niter [, tol]]): density weights of the trajectory, attached (qmri_nufft_dcf)
        qmri_dcf_params dp{};                                       // (the argument checks come first: they need no operator)
        if (nrhs > 1) dp.niter = int_arg(prhs[1], 0, 200, "qmri:dcf:niter", "niter must be an integer in 1..200 (0: the default 20)");
        if (nrhs > 2) {
            want(mxIsDouble(prhs[2]) && !mxIsComplex(prhs[2]) && mxGetNumberOfElements(prhs[2]) == 1, "qmri:dcf:tol", "tol must be a real double scalar");
            dp.tol = mxGetScalar(prhs[2]);
            want(std::isfinite(dp.tol) && dp.tol >= 0.0, "qmri:dcf:tol", "tol must be finite and >= 0 (0: never stop early)");
        }
        want(g_op.V != nullptr, "qmri:state", "no operator: call qmri_mex('set_trajectory', ...) (qmri_make_F_traj) first");
        want(g_op.omega != nullptr, "qmri:dcf:trajectory", "density compensation needs a trajectory operator ('set_trajectory'); a gridded mask has nothing to compensate");
        plhs[0] = mxCreateDoubleMatrix(operator_m(), 1, mxREAL);
        qmri_dcf_info di{};
        check(qmri_nufft_dcf(ctx(), &dp, mxGetDoubles(plhs[0]), &di));
        if (nlhs > 1) {
            const char* names[] = {"iters", "dev", "clamped", "split_tiles"};
            plhs[1] = mxCreateStructMatrix(1, 1, 4, names);
            mxSetFieldByNumber(plhs[1], 0, 0, mxCreateDoubleScalar((double)di.iters));
            mxSetFieldByNumber(plhs[1], 0, 1, mxCreateDoubleScalar(di.dev));
            mxSetFieldByNumber(plhs[1], 0, 2, mxCreateDoubleScalar((double)di.clamped));
            mxSetFieldByNumber(plhs[1], 0, 3, mxCreateDoubleScalar((double)di.split_tiles));
        }
    } else if (c == "set_sample_weights") {          // qmri_mex('set_sample_weights', w): the caller's own weights, m x 1 real double, finite and >= 0; [] clears
        need(nrhs, 2, "qmri_mex('set_sample_weights', w)");
        want(mxIsDouble(prhs[1]) && !mxIsComplex(prhs[1]), "qmri:set_sample_weights:type", "w must be a real double vector (or [])");
        want(g_op.V != nullptr, "qmri:state", "no operator: call qmri_mex('set_trajectory', ...) (qmri_make_F_traj) first");
        want(g_op.omega != nullptr, "qmri:set_sample_weights:trajectory", "sample weights need a trajectory operator ('set_trajectory')");
        if (mxIsEmpty(prhs[1])) { check(qmri_set_sample_weights(ctx(), nullptr)); return; }
        want(mxGetNumberOfElements(prhs[1]) == operator_m(), "qmri:set_sample_weights:size", "w must have one entry per sample");
        check(qmri_set_sample_weights(ctx(), mxGetDoubles(prhs[1])));
    } else if (c == "adjoint_w") {                   // x = qmri_mex('adjoint_w', y): A^H (w .* y) with the attached weights, N x M x s (qmri_adjoint_w)
        need(nrhs, 2, "x = qmri_mex('adjoint_w', y)");
        want(is_cdouble(prhs[1]), "qmri:adjoint_w:type", "y must be a complex double vector");
        (void)image_numel();
        want(g_op.omega != nullptr, "qmri:adjoint_w:trajectory", "the weighted adjoint needs a trajectory operator ('set_trajectory')");
        want(mxGetNumberOfElements(prhs[1]) == operator_m(), "qmri:adjoint_w:size", "y must have one entry per sample");
        const mwSize dims[3] = {(mwSize)g_op.N, (mwSize)g_op.M, (mwSize)mxGetN(g_op.V)};
        plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxCOMPLEX);
        check(qmri_adjoint_w(ctx(), mxGetComplexDoubles(prhs[1]), mxGetComplexDoubles(plhs[0])));
    } else if (c == "set_field_map") {               // info = qmri_mex('set_field_map', f, t [, nseg [, nbins [, tol]]]): N x M real Hz, m x 1 seconds; f = [] clears
        need(nrhs, 2, "info = qmri_mex('set_field_map', f, t [, nseg, nbins, tol])");
        want(mxIsDouble(prhs[1]) && !mxIsComplex(prhs[1]), "qmri:set_field_map:type", "f must be a real double N x M array in Hz (or [])");
        qmri_offres_params fp{};                                    // (the argument checks come first: they need no operator)
        if (nrhs > 3) fp.nseg = int_arg(prhs[3], 0, 16, "qmri:set_field_map:nseg", "nseg must be an integer in 1..16 (0: automatic)");
        if (nrhs > 4) {
            fp.nbins = int_arg(prhs[4], 0, 1024, "qmri:set_field_map:nbins", "nbins must be an integer in 16..1024 (0: the default 256)");
            want(fp.nbins == 0 || fp.nbins >= 16, "qmri:set_field_map:nbins", "nbins must be an integer in 16..1024 (0: the default 256)");
        }
        if (nrhs > 5) {
            want(mxIsDouble(prhs[5]) && !mxIsComplex(prhs[5]) && mxGetNumberOfElements(prhs[5]) == 1, "qmri:set_field_map:tol", "tol must be a real double scalar");
            fp.tol = mxGetScalar(prhs[5]);
            want(std::isfinite(fp.tol) && fp.tol >= 0.0, "qmri:set_field_map:tol", "tol must be finite and >= 0 (0: the default 1e-4)");
        }
        want(g_op.V != nullptr, "qmri:state", "no operator: call qmri_mex('set_trajectory', ...) (qmri_make_F_traj) first");
        want(g_op.omega != nullptr, "qmri:set_field_map:trajectory", "a field map needs a trajectory operator ('set_trajectory'): a gridded mask has no readout times");
        if (mxIsEmpty(prhs[1])) { check(qmri_set_field_map(ctx(), nullptr, nullptr, nullptr, nullptr)); return; }
        need(nrhs, 3, "info = qmri_mex('set_field_map', f, t [, nseg, nbins, tol])");
        want(mxGetNumberOfElements(prhs[1]) == (size_t)g_op.N * (size_t)g_op.M && mxGetM(prhs[1]) == (size_t)g_op.N, "qmri:set_field_map:size",
             "f must be N x M, one entry per pixel");
        want(mxIsDouble(prhs[2]) && !mxIsComplex(prhs[2]), "qmri:set_field_map:type", "t must be a real double vector of readout times in seconds");
        want(mxGetNumberOfElements(prhs[2]) == operator_m(), "qmri:set_field_map:size", "t must have one entry per sample");
        qmri_offres_info fi{};
        check(qmri_set_field_map(ctx(), mxGetDoubles(prhs[1]), mxGetDoubles(prhs[2]), &fp, &fi));
        const char* names[] = {"nseg", "tol_reached", "fit_max", "fit_rms", "f_min", "f_max", "t_min", "t_max"};
        const double vals[] = {(double)fi.nseg, (double)fi.tol_reached, fi.fit_max, fi.fit_rms, fi.f_min, fi.f_max, fi.t_min, fi.t_max};
        plhs[0] = mxCreateStructMatrix(1, 1, 8, names);
        for (int k = 0; k < 8; ++k) mxSetFieldByNumber(plhs[0], 0, k, mxCreateDoubleScalar(vals[k]));
    } else if (c == "field_map_estimate") {          // [f, info, trust] = qmri_mex('field_map_estimate', Y, t [, iters [, beta [, phase_sign]]])
        // extension (no reference counterpart): the field map in Hz of L gradient-echo images per slice (qmri_field_map_estimate).  Y: complex double
        // N x M x L (one coil), N x M x C x L or N x M x C x L x S; t: the L echo times in seconds.  f: N x M (x S); info: struct of 1 x S rows; trust as f.
        const char* usage = "[f, info, trust] = qmri_mex('field_map_estimate', Y, t [, iters, beta, phase_sign])";
        need(nrhs, 3, usage);
        want(nlhs <= 3, "qmri:usage", usage);
        want(is_cdouble(prhs[1]), "qmri:field_map_estimate:type", "Y must be a complex double array (N x M x L, N x M x C x L or N x M x C x L x S)");
        want(mxIsDouble(prhs[2]) && !mxIsComplex(prhs[2]), "qmri:field_map_estimate:t", "t must be a real double vector of echo times in seconds");
        const size_t L = mxGetNumberOfElements(prhs[2]);
        want(L >= 2 && L <= 8, "qmri:field_map_estimate:t", "t must hold 2 <= L <= 8 echo times");
        const double* t = mxGetDoubles(prhs[2]);
        for (size_t l = 0; l < L; ++l)
            want(std::isfinite(t[l]) && (l == 0 || t[l] > t[l - 1]), "qmri:field_map_estimate:t", "t must be finite and strictly increasing");
        const size_t nd = mxGetNumberOfDimensions(prhs[1]);
        const mwSize* yd = mxGetDimensions(prhs[1]);
        want(nd >= 3 && nd <= 5, "qmri:field_map_estimate:size", "Y must be N x M x L, N x M x C x L or N x M x C x L x S");
        const size_t N = yd[0], M = yd[1], Cc = nd == 3 ? 1 : yd[2], Ly = nd == 3 ? yd[2] : yd[3], S = nd == 5 ? yd[4] : 1;
        want(Ly == L, "qmri:field_map_estimate:size", "the echo dimension of Y must have one image per entry of t");
        want(N >= 2 && N <= 4096 && M >= 2 && M <= 4096 && Cc >= 1 && Cc <= 128 && S >= 1 && S <= 4096, "qmri:field_map_estimate:size",
             "Y: 2 <= N, M <= 4096, at most 128 coils and 4096 slices");
        qmri_fieldmap_params fp{};
        if (nrhs > 3) fp.iters = int_arg(prhs[3], 0, 100000, "qmri:field_map_estimate:iters", "iters must be an integer in 1..100000 (0: the default 200)");
        if (nrhs > 4) {
            want(mxIsDouble(prhs[4]) && !mxIsComplex(prhs[4]) && mxGetNumberOfElements(prhs[4]) == 1, "qmri:field_map_estimate:beta", "beta must be a real double scalar");
            fp.beta = mxGetScalar(prhs[4]);
            want(std::isfinite(fp.beta) && fp.beta >= 0.0, "qmri:field_map_estimate:beta", "beta must be finite and >= 0 (0: the default 0.01)");
        }
        if (nrhs > 5) {
            fp.phase_sign = int_arg(prhs[5], -1, 1, "qmri:field_map_estimate:phase_sign", "phase_sign must be -1 or +1");
            want(fp.phase_sign != 0, "qmri:field_map_estimate:phase_sign", "phase_sign must be -1 or +1");
        }
        // MATLAB's N x M x C x L x S is the ABI's [slice][echo][coil][n1 + N n2] as it stands
        const mwSize fd[3] = {(mwSize)N, (mwSize)M, (mwSize)S};
        plhs[0] = mxCreateNumericArray(S > 1 ? 3 : 2, fd, mxDOUBLE_CLASS, mxREAL);
        mxArray* trust = nlhs > 2 ? mxCreateNumericArray(S > 1 ? 3 : 2, fd, mxDOUBLE_CLASS, mxREAL) : nullptr;
        std::vector<qmri_fieldmap_info> fi(S);
        check(qmri_field_map_estimate(ctx(), (int)S, (int)L, (int)Cc, (int)N, (int)M, mxGetComplexDoubles(prhs[1]), t, nullptr, &fp, mxGetDoubles(plhs[0]),
                                      trust ? mxGetDoubles(trust) : nullptr, fi.data()));
        if (nlhs > 1) {
            const char* names[] = {"cost0", "cost", "f_min", "f_max", "iters", "unwrap_limit_hz"};
            plhs[1] = mxCreateStructMatrix(1, 1, 6, names);          // every field a 1 x S row: info.cost(k) is slice k's
            for (int k = 0; k < 6; ++k) {
                mxArray* row = mxCreateDoubleMatrix(1, (mwSize)S, mxREAL);
                double* v = mxGetDoubles(row);
                for (size_t i = 0; i < S; ++i) {
                    const double vals[] = {fi[i].cost0, fi[i].cost, fi[i].f_min, fi[i].f_max, (double)fi[i].iters, fi[i].unwrap_limit_hz};
                    v[i] = vals[k];
                }
                mxSetFieldByNumber(plhs[1], 0, k, row);
            }
        }
        if (trust) plhs[2] = trust;
    } else if (c == "set_llr") {                     // qmri_mex('set_llr', tau [, block [, shift]]): Step 2 of 'pnp_admm' becomes the locally low-rank prox
        // extension (no reference counterpart; qmri_set_llr): tau >= 0 in the units of the TSMI, block 4, 8 (default) or 16,
        // shift 1 (default): the block offsets cycle with the ADMM iteration.  No denoiser is needed while it is set.
        need(nrhs, 2, "qmri_mex('set_llr', tau [, block, shift])");
        want(mxIsDouble(prhs[1]) && !mxIsComplex(prhs[1]) && mxGetNumberOfElements(prhs[1]) == 1, "qmri:set_llr:tau", "tau must be a real double scalar");
        qmri_llr_params lp{};
        lp.tau = mxGetScalar(prhs[1]);
        want(std::isfinite(lp.tau) && lp.tau >= 0.0, "qmri:set_llr:tau", "tau must be finite and >= 0");
        lp.block = nrhs > 2 ? int_arg(prhs[2], 4, 16, "qmri:set_llr:block", "block must be 4, 8 or 16") : 8;
        want(lp.block == 4 || lp.block == 8 || lp.block == 16, "qmri:set_llr:block", "block must be 4, 8 or 16");
        lp.shift = nrhs > 3 ? int_arg(prhs[3], 0, 1, "qmri:set_llr:shift", "shift must be 0 or 1") : 1;
        check(qmri_set_llr(ctx(), &lp));
        g_llr = true;
    } else if (c == "clear_llr") {                   // qmri_mex('clear_llr'): Step 2 of 'pnp_admm' is the network again
        check(qmri_set_llr(ctx(), nullptr));
        g_llr = false;
    } else if (c == "llr_prox") {                    // [out, smax] = qmri_mex('llr_prox', x, tau [, block [, o1, o2]])
        // the locally low-rank proximal step alone (qmri_llr_prox).  x: double N x M x s (x S), complex, or real (real mode: the output's imaginary
        // part is exactly 0); N and M multiples of block, s <= 16.  out: complex like x; smax: 1 x S, the largest singular value of each slice's blocks.
        const char* usage = "[out, smax] = qmri_mex('llr_prox', x, tau [, block, o1, o2])";
        need(nrhs, 3, usage);
        want(nlhs <= 2 && nrhs != 5, "qmri:usage", usage);
        want(mxIsDouble(prhs[1]), "qmri:llr_prox:type", "x must be a double array (complex, or real for real mode)");
        want(mxIsDouble(prhs[2]) && !mxIsComplex(prhs[2]) && mxGetNumberOfElements(prhs[2]) == 1, "qmri:llr_prox:tau", "tau must be a real double scalar");
        qmri_llr_params lp{};
        lp.tau = mxGetScalar(prhs[2]);
        want(std::isfinite(lp.tau) && lp.tau >= 0.0, "qmri:llr_prox:tau", "tau must be finite and >= 0");
        lp.block = nrhs > 3 ? int_arg(prhs[3], 4, 16, "qmri:llr_prox:block", "block must be 4, 8 or 16") : 8;
        want(lp.block == 4 || lp.block == 8 || lp.block == 16, "qmri:llr_prox:block", "block must be 4, 8 or 16");
        const int o1 = nrhs > 5 ? int_arg(prhs[4], 0, lp.block - 1, "qmri:llr_prox:offset", "o1 and o2 must be integers in 0 .. block - 1") : 0;
        const int o2 = nrhs > 5 ? int_arg(prhs[5], 0, lp.block - 1, "qmri:llr_prox:offset", "o1 and o2 must be integers in 0 .. block - 1") : 0;
        const size_t nd = mxGetNumberOfDimensions(prhs[1]);
        const mwSize* xd = mxGetDimensions(prhs[1]);
        want(nd >= 2 && nd <= 4, "qmri:llr_prox:size", "x must be N x M x s or N x M x s x S");
        const size_t N = xd[0], M = xd[1], s = nd > 2 ? xd[2] : 1, S = nd > 3 ? xd[3] : 1;
        want(N >= 1 && M >= 1 && N <= 16384 && M <= 16384 && N % lp.block == 0 && M % lp.block == 0, "qmri:llr_prox:size", "N and M must be positive multiples of block");
        want(s >= 1 && s <= 16 && S >= 1 && S <= 65536, "qmri:llr_prox:size", "x must hold 1 <= s <= 16 channels and at least one slice");
        const mwSize od[4] = {(mwSize)N, (mwSize)M, (mwSize)s, (mwSize)S};
        plhs[0] = mxCreateNumericArray(S > 1 ? 4 : 3, od, mxDOUBLE_CLASS, mxCOMPLEX);
        mxArray* sm = mxCreateDoubleMatrix(1, (mwSize)S, mxREAL);
        const bool cpx = mxIsComplex(prhs[1]);
        check(qmri_llr_prox(ctx(), (int)N, (int)M, (int)s, (int)S, cpx ? (const void*)mxGetComplexDoubles(prhs[1]) : (const void*)mxGetDoubles(prhs[1]), cpx ? 1 : 0,
                            &lp, o1, o2, mxGetComplexDoubles(plhs[0]), mxGetDoubles(sm)));
        if (nlhs > 1) plhs[1] = sm; else mxDestroyArray(sm);
    } else if (c == "set_wavelet") {                 // qmri_mex('set_wavelet', tau [, levels [, filter [, joint [, shift]]]]): Step 2 of 'pnp_admm' becomes the wavelet prox
        // extension (no reference counterpart; qmri_set_wavelet): tau >= 0 in the units of the TSMI, levels 1 .. 4 (default 3),
        // filter 0 Haar or 1 Daubechies-2 (default), joint 1 (default): the s channels are thresholded together, shift 1 (default): the offsets cycle
        // with the ADMM iteration.  No denoiser is needed while it is set; refused (qmri:state) while 'set_llr' is in force.
        need(nrhs, 2, "qmri_mex('set_wavelet', tau [, levels, filter, joint, shift])");
        want(mxIsDouble(prhs[1]) && !mxIsComplex(prhs[1]) && mxGetNumberOfElements(prhs[1]) == 1, "qmri:set_wavelet:tau", "tau must be a real double scalar");
        qmri_wavelet_params wp{};
        wp.tau = mxGetScalar(prhs[1]);
        want(std::isfinite(wp.tau) && wp.tau >= 0.0, "qmri:set_wavelet:tau", "tau must be finite and >= 0");
        wp.levels = nrhs > 2 ? int_arg(prhs[2], 1, 4, "qmri:set_wavelet:levels", "levels must be 1, 2, 3 or 4") : 3;
        wp.filter = nrhs > 3 ? int_arg(prhs[3], 0, 1, "qmri:set_wavelet:filter", "filter must be 0 (Haar) or 1 (Daubechies-2)") : QMRI_WAVELET_DB2;
        wp.joint = nrhs > 4 ? int_arg(prhs[4], 0, 1, "qmri:set_wavelet:joint", "joint must be 0 or 1") : 1;
        wp.shift = nrhs > 5 ? int_arg(prhs[5], 0, 1, "qmri:set_wavelet:shift", "shift must be 0 or 1") : 1;
        check(qmri_set_wavelet(ctx(), &wp));
        g_wav = true;
    } else if (c == "clear_wavelet") {               // qmri_mex('clear_wavelet'): Step 2 of 'pnp_admm' is the network again
        check(qmri_set_wavelet(ctx(), nullptr));
        g_wav = false;
    } else if (c == "wavelet_prox") {                // [out, cmax] = qmri_mex('wavelet_prox', x, tau [, levels [, filter [, joint [, o1, o2]]]])
        // joint wavelet soft-thresholding alone (qmri_wavelet_prox).  x: double N x M x s (x S), complex, or real (real mode: the output's imaginary
        // part is exactly 0); N and M multiples of 2^levels, s <= 16.  out: complex like x; cmax: 1 x S, the largest m of each slice's detail positions.
        const char* usage = "[out, cmax] = qmri_mex('wavelet_prox', x, tau [, levels, filter, joint, o1, o2])";
        need(nrhs, 3, usage);
        want(nlhs <= 2 && nrhs != 7 && nrhs <= 8, "qmri:usage", usage);
        want(mxIsDouble(prhs[1]), "qmri:wavelet_prox:type", "x must be a double array (complex, or real for real mode)");
        want(mxIsDouble(prhs[2]) && !mxIsComplex(prhs[2]) && mxGetNumberOfElements(prhs[2]) == 1, "qmri:wavelet_prox:tau", "tau must be a real double scalar");
        qmri_wavelet_params wp{};
        wp.tau = mxGetScalar(prhs[2]);
        want(std::isfinite(wp.tau) && wp.tau >= 0.0, "qmri:wavelet_prox:tau", "tau must be finite and >= 0");
        wp.levels = nrhs > 3 ? int_arg(prhs[3], 1, 4, "qmri:wavelet_prox:levels", "levels must be 1, 2, 3 or 4") : 3;
        wp.filter = nrhs > 4 ? int_arg(prhs[4], 0, 1, "qmri:wavelet_prox:filter", "filter must be 0 (Haar) or 1 (Daubechies-2)") : QMRI_WAVELET_DB2;
        wp.joint = nrhs > 5 ? int_arg(prhs[5], 0, 1, "qmri:wavelet_prox:joint", "joint must be 0 or 1") : 1;
        const int P = 1 << wp.levels, T = wp.filter == QMRI_WAVELET_HAAR ? 2 : 4;
        const int o1 = nrhs > 7 ? int_arg(prhs[6], 0, P - 1, "qmri:wavelet_prox:offset", "o1 and o2 must be integers in 0 .. 2^levels - 1") : 0;
        const int o2 = nrhs > 7 ? int_arg(prhs[7], 0, P - 1, "qmri:wavelet_prox:offset", "o1 and o2 must be integers in 0 .. 2^levels - 1") : 0;
        const size_t nd = mxGetNumberOfDimensions(prhs[1]);
        const mwSize* xd = mxGetDimensions(prhs[1]);
        want(nd >= 2 && nd <= 4, "qmri:wavelet_prox:size", "x must be N x M x s or N x M x s x S");
        const size_t N = xd[0], M = xd[1], s = nd > 2 ? xd[2] : 1, S = nd > 3 ? xd[3] : 1;
        want(N >= 1 && M >= 1 && N <= 16384 && M <= 16384 && N % P == 0 && M % P == 0 && (N >> (wp.levels - 1)) >= (size_t)T && (M >> (wp.levels - 1)) >= (size_t)T,
             "qmri:wavelet_prox:size", "N and M must be multiples of 2^levels, and N / 2^(levels-1) and M / 2^(levels-1) at least the filter length");
        want(s >= 1 && s <= 16 && S >= 1 && S <= 65536, "qmri:wavelet_prox:size", "x must hold 1 <= s <= 16 channels and at least one slice");
        const mwSize od[4] = {(mwSize)N, (mwSize)M, (mwSize)s, (mwSize)S};
        plhs[0] = mxCreateNumericArray(S > 1 ? 4 : 3, od, mxDOUBLE_CLASS, mxCOMPLEX);
        mxArray* cm = mxCreateDoubleMatrix(1, (mwSize)S, mxREAL);
        const bool cpx = mxIsComplex(prhs[1]);
        check(qmri_wavelet_prox(ctx(), (int)N, (int)M, (int)s, (int)S, cpx ? (const void*)mxGetComplexDoubles(prhs[1]) : (const void*)mxGetDoubles(prhs[1]),
                                cpx ? 1 : 0, &wp, o1, o2, mxGetComplexDoubles(plhs[0]), mxGetDoubles(cm)));
        if (nlhs > 1) plhs[1] = cm; else mxDestroyArray(cm);
    } else if (c == "set_sms") {                     // qmri_mex('set_sms', E): E T x Z complex double, the phase of slice b in frame t; [] clears
        // extension (no reference counterpart; qmri_set_sms): attached to the operator in force, kept across the gateway's own
        // re-plans, dropped by 'set_operator' / 'set_trajectory'
        need(nrhs, 2, "qmri_mex('set_sms', E)");
        if (mxIsEmpty(prhs[1])) {
            (void)image_numel();
            drop(g_sms);
            check(qmri_set_sms(ctx(), 0, nullptr));
        } else {
            want(is_cdouble(prhs[1]) && mxGetNumberOfDimensions(prhs[1]) == 2, "qmri:set_sms:type", "E must be a complex double T x Z matrix (or [] to clear)");
            want(mxGetN(prhs[1]) >= 1 && mxGetN(prhs[1]) <= 8, "qmri:set_sms:size", "E must be T x Z with T the rows of V and 1 <= Z <= 8");
            const double* e = (const double*)mxGetComplexDoubles(prhs[1]);
            for (size_t i = 0; i < 2 * mxGetNumberOfElements(prhs[1]); ++i) want(std::isfinite(e[i]), "qmri:set_sms:value", "every value of E must be finite");
            (void)image_numel();
            want(mxGetM(prhs[1]) == mxGetM(g_op.V), "qmri:set_sms:size", "E must be T x Z with T the rows of V and 1 <= Z <= 8");
            check(qmri_set_sms(ctx(), (int)mxGetN(prhs[1]), mxGetComplexDoubles(prhs[1])));
            drop(g_sms);
            g_sms = keep(prhs[1]);
        }
    } else if (c == "forward_sms") {                 // y = qmri_mex('forward_sms', maps, x): m x ncoil x G
        need(nrhs, 3, "y = qmri_mex('forward_sms', maps, x)");
        const SmsShape sh = sms_shape(prhs[1], "qmri:forward_sms:size");
        sms_want_images(prhs[2], sh, true, "qmri:forward_sms:size");
        const mwSize dims[3] = {(mwSize)operator_m(), (mwSize)sh.ncoil, (mwSize)sh.G};
        plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxCOMPLEX);
        const bool cpx = mxIsComplex(prhs[2]);
        check(qmri_forward_sms(ctx(), (int)sh.G, (int)sh.ncoil, mxGetComplexDoubles(prhs[1]), cpx ? (const void*)mxGetComplexDoubles(prhs[2]) : (const void*)mxGetDoubles(prhs[2]),
                               cpx ? 1 : 0, mxGetComplexDoubles(plhs[0])));
    } else if (c == "adjoint_sms") {                 // x = qmri_mex('adjoint_sms', maps, y): N x M x s x Z x G
        need(nrhs, 3, "x = qmri_mex('adjoint_sms', maps, y)");
        const SmsShape sh = sms_shape(prhs[1], "qmri:adjoint_sms:size");
        sms_want_y(prhs[2], sh, "qmri:adjoint_sms:size");
        plhs[0] = sms_new_images(sh);
        check(qmri_adjoint_sms(ctx(), (int)sh.G, (int)sh.ncoil, mxGetComplexDoubles(prhs[1]), mxGetComplexDoubles(prhs[2]), mxGetComplexDoubles(plhs[0])));
    } else if (c == "xupdate_sms") {                 // [x, iters, flags] = qmri_mex('xupdate_sms', maps, y, z, r [, tol [, maxit [, x0]]])
        need(nrhs, 5, "[x, iters, flags] = qmri_mex('xupdate_sms', maps, y, z, r [, tol [, maxit [, x0]]])");
        want(mxIsDouble(prhs[4]) && !mxIsComplex(prhs[4]) && mxGetNumberOfElements(prhs[4]) == 1 && std::isfinite(mxGetScalar(prhs[4])) && mxGetScalar(prhs[4]) > 0,
             "qmri:xupdate_sms:r", "r must be a positive real double scalar");
        double tol = 1e-4;
        if (nrhs > 5) {
            want(mxIsDouble(prhs[5]) && !mxIsComplex(prhs[5]) && mxGetNumberOfElements(prhs[5]) == 1 && mxGetScalar(prhs[5]) >= 0, "qmri:xupdate_sms:tol", "tol must be a real double scalar >= 0");
            tol = mxGetScalar(prhs[5]);
        }
        const int maxit = nrhs > 6 ? int_arg(prhs[6], 0, 1e6, "qmri:xupdate_sms:maxit", "maxit must be a non-negative integer") : 100;
        const SmsShape sh = sms_shape(prhs[1], "qmri:xupdate_sms:size");
        sms_want_y(prhs[2], sh, "qmri:xupdate_sms:size");
        sms_want_images(prhs[3], sh, false, "qmri:xupdate_sms:size");
        const bool has_x0 = nrhs > 7 && !mxIsEmpty(prhs[7]);
        if (has_x0) sms_want_images(prhs[7], sh, false, "qmri:xupdate_sms:size");
        plhs[0] = sms_new_images(sh);
        mxArray* it = mxCreateNumericMatrix(sh.G, 1, mxINT32_CLASS, mxREAL);
        mxArray* fl = mxCreateNumericMatrix(sh.G, 1, mxINT32_CLASS, mxREAL);
        check(qmri_xupdate_sms(ctx(), (int)sh.G, (int)sh.ncoil, mxGetComplexDoubles(prhs[1]), mxGetComplexDoubles(prhs[2]), mxGetComplexDoubles(prhs[3]), mxGetScalar(prhs[4]),
                               tol, maxit, has_x0 ? mxGetComplexDoubles(prhs[7]) : nullptr, mxGetComplexDoubles(plhs[0]), (int32_t*)mxGetData(it), (int32_t*)mxGetData(fl)));
        if (nlhs > 1) plhs[1] = it; else mxDestroyArray(it);
        if (nlhs > 2) plhs[2] = fl; else mxDestroyArray(fl);
    } else if (c == "pnp_admm_sms") {                // [x, lsqr_iters] = qmri_mex('pnp_admm_sms', maps, y, param_struct [, X0 [, groups_per_launch]])
        need(nrhs, 4, "[x, lsqr_iters] = qmri_mex('pnp_admm_sms', maps, y, param [, X0 [, groups_per_launch]])");
        want(mxIsStruct(prhs[3]), "qmri:pnp_admm_sms:type", "param must be a struct");
        const qmri_admm_params p = admm_params(prhs[3], false);
        const int gpl = nrhs > 5 ? int_arg(prhs[5], 1, 4096, "qmri:pnp_admm_sms:groups", "groups_per_launch must be a positive integer") : 1;
        const SmsShape sh = sms_shape(prhs[1], "qmri:pnp_admm_sms:size");
        sms_want_y(prhs[2], sh, "qmri:pnp_admm_sms:size");
        const bool has_x0 = nrhs > 4 && !mxIsEmpty(prhs[4]);
        if (has_x0) sms_want_images(prhs[4], sh, false, "qmri:pnp_admm_sms:size");
        want(g_net.w != nullptr || g_llr || g_wav, "qmri:state", "no denoiser: call qmri_mex('set_denoiser' | 'load_onnx', ...) (qmri_make_net), qmri_mex('set_llr', ...) (qmri_make_llr) or qmri_mex('set_wavelet', ...) (qmri_make_wavelet) first");
        const int it = p.iters > 0 ? p.iters : 1;
        plhs[0] = sms_new_images(sh);
        mxArray* li = mxCreateNumericMatrix(it, sh.G, mxINT32_CLASS, mxREAL);
        reserve((int)(std::min<size_t>(gpl, sh.G) * sh.Z), true, true);      // a launch holds groups_per_launch x Z slice images: the plans grow to it
        check(qmri_pnp_admm_sms(ctx(), (int)sh.G, gpl, (int)sh.ncoil, mxGetComplexDoubles(prhs[1]), mxGetComplexDoubles(prhs[2]), &p,
                                has_x0 ? mxGetComplexDoubles(prhs[4]) : nullptr, mxGetComplexDoubles(plhs[0]), (int32_t*)mxGetData(li)));
        if (nlhs > 1) plhs[1] = li; else mxDestroyArray(li);
    } else if (c == "prepare_normal_fm") {           // info = qmri_mex('prepare_normal_fm' [, nseg [, tol]]): the Toeplitz normal operator of the attached map
        const qmri_offres_normal_params np = normal_fm_params(nrhs > 1 ? prhs[1] : nullptr, nrhs > 2 ? prhs[2] : nullptr, "qmri:prepare_normal_fm:nseg",
                                                              "qmri:prepare_normal_fm:tol");     // (the argument checks come first: they need no operator)
        want(g_op.V != nullptr, "qmri:state", "no operator: call qmri_mex('set_trajectory', ...) (qmri_make_F_traj) first");
        want(g_op.omega != nullptr, "qmri:prepare_normal_fm:trajectory", "the field-aware normal operator needs a trajectory operator ('set_trajectory') with a field map");
        qmri_offres_normal_info ni{};
        check(qmri_nufft_prepare_normal_fm(ctx(), &np, &ni));
        const char* names[] = {"nseg", "tol_reached", "fit_max", "fit_rms", "khat_bytes"};
        const double vals[] = {(double)ni.nseg, (double)ni.tol_reached, ni.fit_max, ni.fit_rms, (double)ni.khat_bytes};
        plhs[0] = mxCreateStructMatrix(1, 1, 5, names);
        for (int k = 0; k < 5; ++k) mxSetFieldByNumber(plhs[0], 0, k, mxCreateDoubleScalar(vals[k]));
    } else if (c == "set_denoiser") {                // qmri_mex('set_denoiser', weights(single), in_nc, out_nc, nc(1x4), nb, residual_noise, H, W [, max_batch])
        need(nrhs, 9, "qmri_mex('set_denoiser', weights, in_nc, out_nc, nc, nb, residual_noise, H, W [, max_batch])");
        qmri_net_desc d;
        d.arch = QMRI_ARCH_UNETRES;
        d.in_nc = (int)mxGetScalar(prhs[2]); d.out_nc = (int)mxGetScalar(prhs[3]);
        want(mxIsDouble(prhs[4]) && mxGetNumberOfElements(prhs[4]) == 4, "qmri:set_denoiser:size", "nc must hold the four channel counts");
        const double* nc = mxGetDoubles(prhs[4]);
        for (int i = 0; i < 4; ++i) d.nc[i] = (int)nc[i];
        d.nb = (int)mxGetScalar(prhs[5]); d.residual_noise = (int)mxGetScalar(prhs[6]);
        set_denoiser_from(prhs[1], d, (int)mxGetScalar(prhs[7]), (int)mxGetScalar(prhs[8]), nrhs > 9 ? (int)mxGetScalar(prhs[9]) : 1);
    } else if (c == "load_onnx") {                   // [in_nc, out_nc] = qmri_mex('load_onnx', denoiser_path, residual_noise, H, W [, max_batch])
        // the weight-loading half of `Net = importONNXNetwork(denoiser_path, ...)` (main_recon_tsmis_FFT.m:138) + set_denoiser
        need(nrhs, 5, "[in_nc, out_nc] = qmri_mex('load_onnx', denoiser_path, residual_noise, H, W [, max_batch])");
        char path[4096];
        if (mxGetString(prhs[1], path, sizeof path)) mexErrMsgIdAndTxt("qmri:usage", "denoiser_path must be a char vector");
        qmri_net_desc d;
        size_t n = 0;
        if (qmri_onnx_read_unetres(path, &d, nullptr, 0, &n) != QMRI_OK) mexErrMsgIdAndTxt("qmri:onnx", "%s", qmri_last_error(nullptr));
        mxArray* w = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL);
        if (qmri_onnx_read_unetres(path, &d, (float*)mxGetData(w), n, &n) != QMRI_OK) mexErrMsgIdAndTxt("qmri:onnx", "%s", qmri_last_error(nullptr));
        d.residual_noise = (int)mxGetScalar(prhs[2]);
        set_denoiser_from(w, d, (int)mxGetScalar(prhs[3]), (int)mxGetScalar(prhs[4]), nrhs > 5 ? (int)mxGetScalar(prhs[5]) : 1);
        mxDestroyArray(w);
        plhs[0] = mxCreateDoubleScalar((double)d.in_nc);
        if (nlhs > 1) plhs[1] = mxCreateDoubleScalar((double)d.out_nc);
    } else if (c == "denoise") {                     // I = qmri_mex('denoise', A, out_nc)   (param.net, :164): A is H x W x C or H x W x C x N (denoiseImage_PnP_ADMM.m:13-17)
        need(nrhs, 3, "I = qmri_mex('denoise', A, out_nc)");
        const mwSize* dm = mxGetDimensions(prhs[1]);
        const int nd = (int)mxGetNumberOfDimensions(prhs[1]);
        if (mxIsComplex(prhs[1]) || !mxIsDouble(prhs[1]) || nd > 4)
            mexErrMsgIdAndTxt("images:denoiseImage:invalidImageFormat", "A must be a real double H x W x C (x N) array");
        const int H = (int)dm[0], W = (int)dm[1], C = nd > 2 ? (int)dm[2] : 1, B = nd > 3 ? (int)dm[3] : 1;
        // the library writes H * W * (the PLAN's out_nc) * B doubles: the output array is sized from the plan, and what the caller says is checked
        // against it here (an out_nc below the plan's would otherwise be a write past the end of a MATLAB array)
        want(g_net.w != nullptr, "qmri:state", "no denoiser: call qmri_mex('set_denoiser' | 'load_onnx', ...) (qmri_make_net) first");
        want(H == g_net.H && W == g_net.W && C == g_net.d.in_nc, "qmri:denoise:size", "A must be H x W x in_nc (x N) as given to set_denoiser");
        want(int_arg(prhs[2], 1, 1 << 20, "qmri:denoise:size", "out_nc must be a positive integer") == g_net.d.out_nc, "qmri:denoise:size",
             "out_nc does not match the denoiser's output channels");
        want(B >= 1, "qmri:denoise:size", "A holds no slice");
        reserve(B, false, true);                                    // a batch larger than the plan: re-planned, as the reference's handle takes any N
        const mwSize od[4] = {(mwSize)H, (mwSize)W, (mwSize)g_net.d.out_nc, (mwSize)B};
        plhs[0] = mxCreateNumericArray(B > 1 ? 4 : 3, od, mxDOUBLE_CLASS, mxREAL);
        check(qmri_denoise(ctx(), mxGetDoubles(prhs[1]), H, W, C, B, mxGetDoubles(plhs[0])));
    } else if (c == "pnp_admm") {                    // [x, diag, lsqr_iters] = qmri_mex('pnp_admm', y, param_struct, X0, gt, [N M s])
        // y: m x 1 -> x is N x M x s;  y: m x S (a slice stack) -> x is N x M x s x S, diag 2 x iter x S, lsqr_iters iter x S: the slices advance together
        // through the batched kernels, slices_per_launch = min(S, 15) at a time, on the current device (X0 / gt: N x M x s x S or empty)
        need(nrhs, 6, "[x, diag, lsqr_iters] = qmri_mex('pnp_admm', y, param, X0, gt, [N M s])");
        want(mxIsStruct(prhs[2]), "qmri:pnp_admm:type", "param must be a struct");
        const qmri_admm_params p = admm_params(prhs[2], nlhs > 1 && !g_op.omega);   // (a trajectory computes no diagnostics: diag stays NaN)
        // param.field_normal = 1: build the field-aware Toeplitz normal operator before the loop (field_normal_nseg / field_normal_tol: its parameters)
        const bool field_normal = scalar_field(prhs[2], "field_normal", 0) != 0;
        qmri_offres_normal_params fnp{};
        if (field_normal) {
            fnp = normal_fm_params(mxGetField(prhs[2], 0, "field_normal_nseg"), mxGetField(prhs[2], 0, "field_normal_tol"), "qmri:pnp_admm:field_normal",
                                   "qmri:pnp_admm:field_normal");
            want(g_op.omega != nullptr, "qmri:pnp_admm:field_normal", "param.field_normal needs a trajectory operator ('set_trajectory') with a field map");
        }
        const double* d = mxGetDoubles(prhs[5]);
        const size_t S = mxGetN(prhs[1]), m = mxGetM(prhs[1]), n = dims_numel(prhs[5]);
        want(is_cdouble(prhs[1]) && S >= 1 && m == operator_m(), "qmri:pnp_admm:size", "y must be complex double, one column of m samples per slice");
        want(g_net.w != nullptr || g_llr || g_wav, "qmri:state", "no denoiser: call qmri_mex('set_denoiser' | 'load_onnx', ...) (qmri_make_net), qmri_mex('set_llr', ...) (qmri_make_llr) or qmri_mex('set_wavelet', ...) (qmri_make_wavelet) first");
        want((mxIsEmpty(prhs[3]) || is_cdouble(prhs[3])) && (mxIsEmpty(prhs[4]) || is_cdouble(prhs[4])), "qmri:pnp_admm:type", "X0 and gt_tsmi must be complex double or empty");
        const int it = p.iters > 0 ? p.iters : 1;
        const mwSize dims[4] = {(mwSize)d[0], (mwSize)d[1], (mwSize)d[2], (mwSize)S};
        plhs[0] = mxCreateNumericArray(S > 1 ? 4 : 3, dims, mxDOUBLE_CLASS, mxCOMPLEX);
        const mwSize ddims[3] = {2, (mwSize)it, (mwSize)S};
        mxArray* diag = mxCreateNumericArray(S > 1 ? 3 : 2, ddims, mxDOUBLE_CLASS, mxREAL);
        if (g_op.omega) std::fill(mxGetDoubles(diag), mxGetDoubles(diag) + mxGetNumberOfElements(diag), NAN);
        mxArray* li = mxCreateNumericMatrix(it, S, mxINT32_CLASS, mxREAL);
        const mxComplexDouble* y = mxGetComplexDoubles(prhs[1]);
        const mxComplexDouble* x0 = mxIsEmpty(prhs[3]) ? nullptr : mxGetComplexDoubles(prhs[3]);
        const mxComplexDouble* gt = mxIsEmpty(prhs[4]) ? nullptr : mxGetComplexDoubles(prhs[4]);
        if (x0 && mxGetNumberOfElements(prhs[3]) != n * S) mexErrMsgIdAndTxt("qmri:pnp_admm:size", "X0 must hold N x M x s values per slice");
        if (gt && mxGetNumberOfElements(prhs[4]) != n * S) mexErrMsgIdAndTxt("qmri:pnp_admm:size", "gt_tsmi must hold N x M x s values per slice");
        if (field_normal) check(qmri_nufft_prepare_normal_fm(ctx(), &fnp, nullptr));    // (a trajectory's launch size is 1: no re-plan follows)
        if (S == 1) {
            check(qmri_pnp_admm(ctx(), y, &p, x0, gt, mxGetComplexDoubles(plhs[0]), p.want_diag ? mxGetDoubles(diag) : nullptr, (int32_t*)mxGetData(li)));
        } else {
            // several slices on this device: the plans grow to the launch size, then qmri_pnp_admm_batch walks the stack
            const int spl = g_op.omega ? 1 : (int)std::min<size_t>(S, DEFAULT_SLICES_PER_LAUNCH);   // (a trajectory: one slice per launch)
            reserve(spl, true, true);
            check(qmri_pnp_admm_batch(ctx(), (int)S, spl, y, &p, x0, gt, mxGetComplexDoubles(plhs[0]), p.want_diag ? mxGetDoubles(diag) : nullptr,
                                      (int32_t*)mxGetData(li)));
        }
        if (nlhs > 1) plhs[1] = diag; else mxDestroyArray(diag);
        if (nlhs > 2) plhs[2] = li; else mxDestroyArray(li);
    } else if (c == "recon_batch" || c == "recon_batch_mc") {   // [X, qmap, pd] = qmri_mex('recon_batch', Y(m x S), param_struct, devs, slices_per_launch, [N M s])
        // north_star's batch path: S independent slices sharded over the GPUs in `devs` (one worker = host thread + context per entry; an id may
        // repeat), slices_per_launch advanced together on each; 100 PnP-ADMM iterations + dictionary match per slice (the match only when a dictionary
        // is set and maps are asked for).  Uses the operator / denoiser / dictionary given to 'set_operator' / 'set_denoiser' / 'set_dictionary'.
        // 'recon_batch_mc' (multi-coil extension, no reference counterpart): qmri_mex('recon_batch_mc', Y(m x ncoil x S), maps(N x M x ncoil x S),
        // param_struct, devs, slices_per_launch, [N M s]) -- every slice with its own coil maps (qmri_recon_batch_mc).
        const bool mc = c == "recon_batch_mc";
        const int o = mc ? 1 : 0;                                  // (arguments after Y move one place right)
        // Optional 8th / 9th arguments of 'recon_batch_mc': cc (scalar nv or struct, 'coil_compress') and noise_cov ([] or ncoil x ncoil): every launch
        // compresses its slices on the device before the reconstruction (qmri_recon_batch_mc_cc).
        if (mc) need(nrhs, 7, "[X, qmap, pd] = qmri_mex('recon_batch_mc', Y, maps, param, devs, slices_per_launch, [N M s] [, cc, noise_cov])");
        else need(nrhs, 6, "[X, qmap, pd] = qmri_mex('recon_batch', Y, param, devs, slices_per_launch, [N M s])");
        if (!g_op.V || !g_net.w) mexErrMsgIdAndTxt("qmri:recon_batch:state", "set_operator and set_denoiser (or load_onnx) must come first");
        want(!g_op.omega, "qmri:recon_batch:trajectory", "the batch workers need a gridded mask (set_operator); reconstruct a trajectory with 'pnp_admm'");
        size_t S = mxGetN(prhs[1]), ncoil = 0;
        if (mc) {
            const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
            const mwSize* yd = mxGetDimensions(prhs[1]);
            ncoil = nd >= 2 ? yd[1] : 1;
            S = nd >= 3 ? yd[2] : 1;
            want(nd <= 3 && is_cdouble(prhs[1]) && ncoil >= 1 && S >= 1 && yd[0] == operator_m(), "qmri:recon_batch_mc:size",
                 "Y must be complex double, m x ncoil x S");
            const mwSize md = mxGetNumberOfDimensions(prhs[2]);
            const mwSize* cd = mxGetDimensions(prhs[2]);
            want(is_cdouble(prhs[2]) && md >= 2 && md <= 4 && (mwSize)cd[0] == (mwSize)g_op.N && (mwSize)cd[1] == (mwSize)g_op.M &&
                 mxGetNumberOfElements(prhs[2]) == (size_t)g_op.N * g_op.M * ncoil * S, "qmri:recon_batch_mc:maps",
                 "maps must be complex double, N x M x ncoil x S");
        }
        (void)dims_numel(prhs[5 + o]);
        want(mxIsStruct(prhs[2 + o]), "qmri:recon_batch:type", "param must be a struct");
        if (!mc) want(is_cdouble(prhs[1]) && S >= 1 && mxGetM(prhs[1]) == operator_m(), "qmri:recon_batch:size", "Y must be complex double, one column of m samples per slice");
        want(mxIsDouble(prhs[3 + o]) && !mxIsComplex(prhs[3 + o]), "qmri:recon_batch:devs", "devs must be a double vector of device ids");
        const double* d = mxGetDoubles(prhs[5 + o]);
        std::vector<int> devs(mxGetNumberOfElements(prhs[3 + o]));
        for (size_t i = 0; i < devs.size(); ++i) devs[i] = (int)mxGetDoubles(prhs[3 + o])[i];
        if (devs.empty()) mexErrMsgIdAndTxt("qmri:recon_batch:devs", "devs must name at least one device");
        const bool maps = nlhs > 1 && g_dict.D;
        qmri_problem pb;
        std::memset(&pb, 0, sizeof pb);
        pb.N = g_op.N; pb.M = g_op.M; pb.T = (int)mxGetM(g_op.V); pb.s = (int)mxGetN(g_op.V);
        pb.V = mxGetDoubles(g_op.V); pb.frame_ptr = (const int32_t*)mxGetData(g_op.fp); pb.kidx = (const int32_t*)mxGetData(g_op.kidx);
        pb.net = &g_net.d; pb.weights = (const float*)mxGetData(g_net.w); pb.weights_nbytes = mxGetNumberOfElements(g_net.w) * 4;
        if (maps) {
            pb.K = (int)mxGetM(g_dict.D); pb.Q = (int)mxGetN(g_dict.lut);
            pb.D = (const float*)mxGetData(g_dict.D); pb.normD = (const float*)mxGetData(g_dict.normD); pb.lut = (const float*)mxGetData(g_dict.lut);
        }
        pb.admm = admm_params(prhs[2 + o], false);
        pb.slices_per_launch = std::max(1, (int)mxGetScalar(prhs[4 + o]));
        const mwSize xd[4] = {(mwSize)d[0], (mwSize)d[1], (mwSize)d[2], (mwSize)S};
        plhs[0] = mxCreateNumericArray(4, xd, mxDOUBLE_CLASS, mxCOMPLEX);
        mxArray *qm = nullptr, *pd = nullptr;
        if (maps) {
            const mwSize qd[4] = {(mwSize)d[0], (mwSize)d[1], (mwSize)pb.Q, (mwSize)S};
            const mwSize pdd[3] = {(mwSize)d[0], (mwSize)d[1], (mwSize)S};
            qm = mxCreateNumericArray(4, qd, mxSINGLE_CLASS, mxREAL);
            pd = mxCreateNumericArray(3, pdd, mxSINGLE_CLASS, mxCOMPLEX);
        }
        const bool use_cc = mc && nrhs > 7 && !mxIsEmpty(prhs[7]);
        qmri_cc_params ccp{};
        const void* psi = nullptr;
        if (use_cc) {
            ccp = cc_params(prhs[7], "qmri:recon_batch_mc:cc");
            if (nrhs > 8) psi = noise_cov_arg(prhs[8], ncoil, "qmri:recon_batch_mc:noise_cov");
        }
        char err[1024] = "";
        const int st = use_cc ? qmri_recon_batch_mc_cc((int)devs.size(), devs.data(), (int)S, &pb, (int)ncoil, mxGetComplexDoubles(prhs[2]), mxGetComplexDoubles(prhs[1]),
                                                       mxGetComplexDoubles(plhs[0]), qm ? (float*)mxGetData(qm) : nullptr, pd ? (float*)mxGetData(pd) : nullptr,
                                                       err, sizeof err, psi, &ccp)
                     : mc ? qmri_recon_batch_mc((int)devs.size(), devs.data(), (int)S, &pb, (int)ncoil, mxGetComplexDoubles(prhs[2]), mxGetComplexDoubles(prhs[1]),
                                                mxGetComplexDoubles(plhs[0]), qm ? (float*)mxGetData(qm) : nullptr, pd ? (float*)mxGetData(pd) : nullptr, err, sizeof err)
                          : qmri_recon_batch((int)devs.size(), devs.data(), (int)S, &pb, mxGetComplexDoubles(prhs[1]), mxGetComplexDoubles(plhs[0]),
                                             qm ? (float*)mxGetData(qm) : nullptr, pd ? (float*)mxGetData(pd) : nullptr, err, sizeof err);
        if (st != QMRI_OK) {
            char id[32];
            snprintf(id, sizeof id, "qmri:err%d", -st);
            mexErrMsgIdAndTxt(id, "%s", err);
        }
        if (nlhs > 1) plhs[1] = qm ? qm : mxCreateNumericMatrix(0, 0, mxSINGLE_CLASS, mxREAL);
        if (nlhs > 2) plhs[2] = pd ? pd : mxCreateNumericMatrix(0, 0, mxSINGLE_CLASS, mxCOMPLEX); else if (pd) mxDestroyArray(pd);
    } else if (c == "coil_compress") {               // [yc, mapsc, W, eig] = qmri_mex('coil_compress', Y(m x ncoil x S), maps, noise_cov, cc)
        // multi-coil extension (no reference counterpart): maps [] or N x M x ncoil x S, noise_cov [] or ncoil x ncoil, cc a scalar nv or a struct
        // (nv, energy, shared).  yc m x nv x S, mapsc N x M x nv x S (or []), W ncoil x nv x S (1 when shared), eig ncoil x S (1 when shared).
        need(nrhs, 5, "[yc, mapsc, W, eig] = qmri_mex('coil_compress', Y, maps, noise_cov, cc)");
        want(g_op.V != nullptr, "qmri:state", "no operator: call qmri_mex('set_operator', ...) (qmri_make_F) first");
        const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
        const mwSize* yd = mxGetDimensions(prhs[1]);
        const size_t m = operator_m(), ncoil = nd >= 2 ? yd[1] : 1, S = nd >= 3 ? yd[2] : 1, plane = (size_t)g_op.N * g_op.M;
        want(nd <= 3 && is_cdouble(prhs[1]) && yd[0] == m && ncoil >= 1 && S >= 1, "qmri:coil_compress:size", "Y must be complex double, m x ncoil x S");
        const bool has_maps = !mxIsEmpty(prhs[2]);
        if (has_maps) {
            const mwSize* cd = mxGetDimensions(prhs[2]);
            want(is_cdouble(prhs[2]) && mxGetNumberOfDimensions(prhs[2]) >= 2 && cd[0] == (mwSize)g_op.N && cd[1] == (mwSize)g_op.M &&
                 mxGetNumberOfElements(prhs[2]) == plane * ncoil * S, "qmri:coil_compress:maps", "maps must be [] or complex double, N x M x ncoil x S");
        }
        const void* psi = noise_cov_arg(prhs[3], ncoil, "qmri:coil_compress:noise_cov");
        const qmri_cc_params p = cc_params(prhs[4], "qmri:coil_compress:cc");
        const size_t nmat = p.shared ? 1 : S;
        std::vector<double> yo(2 * S * ncoil * m), mo(has_maps ? 2 * S * ncoil * plane : 0), Wo(2 * nmat * ncoil * ncoil), eo(nmat * ncoil);
        int nv = 0;
        check(qmri_coil_compress(ctx(), (int)S, (int)ncoil, mxGetComplexDoubles(prhs[1]), has_maps ? mxGetComplexDoubles(prhs[2]) : nullptr, psi, &p, &nv,
                                 yo.data(), has_maps ? mo.data() : nullptr, Wo.data(), eo.data()));
        const mwSize yc[3] = {(mwSize)m, (mwSize)nv, (mwSize)S};
        plhs[0] = mxCreateNumericArray(3, yc, mxDOUBLE_CLASS, mxCOMPLEX);
        std::memcpy(mxGetComplexDoubles(plhs[0]), yo.data(), S * nv * m * 2 * sizeof(double));
        if (nlhs > 1) {
            const mwSize mc4[4] = {(mwSize)g_op.N, (mwSize)g_op.M, (mwSize)nv, (mwSize)S};
            plhs[1] = has_maps ? mxCreateNumericArray(4, mc4, mxDOUBLE_CLASS, mxCOMPLEX) : mxCreateDoubleMatrix(0, 0, mxCOMPLEX);
            if (has_maps) std::memcpy(mxGetComplexDoubles(plhs[1]), mo.data(), S * nv * plane * 2 * sizeof(double));
        }
        if (nlhs > 2) {
            const mwSize wd[3] = {(mwSize)ncoil, (mwSize)nv, (mwSize)nmat};
            plhs[2] = mxCreateNumericArray(3, wd, mxDOUBLE_CLASS, mxCOMPLEX);
            std::memcpy(mxGetComplexDoubles(plhs[2]), Wo.data(), nmat * ncoil * nv * 2 * sizeof(double));
        }
        if (nlhs > 3) {
            plhs[3] = mxCreateDoubleMatrix(ncoil, nmat, mxREAL);
            std::memcpy(mxGetDoubles(plhs[3]), eo.data(), nmat * ncoil * sizeof(double));
        }
    } else if (c == "coil_maps") {                   // [maps, img, lam, info] = qmri_mex('coil_maps', calib, opts)
        // multi-coil extension (no reference counterpart): coil sensitivity maps from calibration data (qmri_coil_maps).  calib: complex double,
        // cN x cM x ncoil x S (a centred k-space block, opts.images = 0) or N x M x ncoil x S (calibration images, opts.images = 1); opts: a struct with
        // the optional fields images (0), patch (3), window (1), phase_coil (0: object phase, 1: strongest coil), thresh (0).
        // maps N x M x ncoil x S, img N x M x S, lam N x M x S, info a struct (max_iters, not_converged).
        need(nrhs, 3, "[maps, img, lam, info] = qmri_mex('coil_maps', calib, opts)");
        want(mxIsStruct(prhs[2]), "qmri:coil_maps:opts", "opts must be a struct (fields images, patch, window, phase_coil, thresh)");
        want(g_op.V != nullptr, "qmri:state", "no operator: call qmri_mex('set_operator', ...) (qmri_make_F) first");
        const mxArray* O = prhs[2];
        const mxArray* f;
        qmri_csm_params p = QMRI_CSM_PARAMS_DEFAULT(0, 0);
        if ((f = mxGetField(O, 0, "images"))) p.kind = int_arg(f, 0, 1, "qmri:coil_maps:opts", "opts.images must be 0 or 1") ? QMRI_CSM_IMAGES : QMRI_CSM_KSPACE;
        if ((f = mxGetField(O, 0, "patch"))) p.patch = int_arg(f, 0, 4, "qmri:coil_maps:opts", "opts.patch must be an integer in [0, 4]");
        if ((f = mxGetField(O, 0, "window"))) p.window = int_arg(f, 0, 1, "qmri:coil_maps:opts", "opts.window must be 0 or 1");
        if ((f = mxGetField(O, 0, "phase_coil"))) p.phase_ref = int_arg(f, 0, 1, "qmri:coil_maps:opts", "opts.phase_coil must be 0 or 1") ? QMRI_CSM_PHASE_COIL : QMRI_CSM_PHASE_OBJECT;
        p.thresh = scalar_field(O, "thresh", 0.0);
        want(std::isfinite(p.thresh) && p.thresh >= 0.0, "qmri:coil_maps:opts", "opts.thresh must be finite and >= 0");
        const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
        const mwSize* cd = mxGetDimensions(prhs[1]);
        want(is_cdouble(prhs[1]) && nd >= 2 && nd <= 4, "qmri:coil_maps:size", "calib must be complex double, c1 x c2 x ncoil x S");
        const size_t c1 = cd[0], c2 = cd[1], ncoil = nd >= 3 ? cd[2] : 1, S = nd >= 4 ? cd[3] : 1, plane = (size_t)g_op.N * g_op.M;
        want(ncoil >= 1 && ncoil <= 128 && S >= 1, "qmri:coil_maps:size", "calib needs 1..128 coils and at least one slice");
        if (p.kind == QMRI_CSM_IMAGES) want(c1 == (size_t)g_op.N && c2 == (size_t)g_op.M, "qmri:coil_maps:size", "calibration images must be N x M x ncoil x S");
        else want(c1 % 2 == 0 && c2 % 2 == 0 && c1 >= 8 && c2 >= 8 && c1 <= (size_t)g_op.N && c2 <= (size_t)g_op.M, "qmri:coil_maps:size",
                  "the calibration block must have even sides with 8 <= cN <= N and 8 <= cM <= M");
        p.cN = (int)c1; p.cM = (int)c2;
        const mwSize md[4] = {(mwSize)g_op.N, (mwSize)g_op.M, (mwSize)ncoil, (mwSize)S}, id3[3] = {(mwSize)g_op.N, (mwSize)g_op.M, (mwSize)S};
        plhs[0] = mxCreateNumericArray(4, md, mxDOUBLE_CLASS, mxCOMPLEX);
        mxArray* img = mxCreateNumericArray(3, id3, mxDOUBLE_CLASS, mxCOMPLEX);
        mxArray* lam = mxCreateNumericArray(3, id3, mxDOUBLE_CLASS, mxREAL);
        (void)plane;
        qmri_csm_info info{0, 0};
        check(qmri_coil_maps(ctx(), (int)S, (int)ncoil, g_op.N, g_op.M, mxGetComplexDoubles(prhs[1]), &p, mxGetComplexDoubles(plhs[0]), mxGetComplexDoubles(img),
                             mxGetDoubles(lam), &info));
        if (nlhs > 1) plhs[1] = img; else mxDestroyArray(img);
        if (nlhs > 2) plhs[2] = lam; else mxDestroyArray(lam);
        if (nlhs > 3) {
            const char* names[] = {"max_iters", "not_converged"};
            plhs[3] = mxCreateStructMatrix(1, 1, 2, names);
            mxSetFieldByNumber(plhs[3], 0, 0, mxCreateDoubleScalar((double)info.max_iters));
            mxSetFieldByNumber(plhs[3], 0, 1, mxCreateDoubleScalar((double)info.not_converged));
        }
    } else if (c == "dict_compress") {               // [V, D, normD, eig, info] = qmri_mex('dict_compress', F, params)
        // extension (no reference counterpart): a simulated dictionary compressed to its SVD subspace (qmri_dict_compress).  F: K x T real double or
        // single, K fingerprints of T <= 1024 frames; params: a struct with s (the rank, 1..16) or energy (and s_max, 16), and the optional tol, maxit.
        // V T x s double, D K x s single, normD K x 1 single, eig s x 1 double, info a struct.  Needs no operator, denoiser or dictionary.
        need(nrhs, 3, "[V, D, normD, eig, info] = qmri_mex('dict_compress', F, params)");
        want(mxIsStruct(prhs[2]), "qmri:dict_compress:params", "params must be a struct (fields s or energy, s_max, tol, maxit)");
        const mxArray* A = prhs[1];
        want((mxIsDouble(A) || mxIsSingle(A)) && !mxIsComplex(A) && mxGetNumberOfDimensions(A) == 2, "qmri:dict_compress:F",
             "F must be a real double or single K x T matrix (complex fingerprints are not supported)");
        const size_t K = mxGetM(A), T = mxGetN(A);
        want(K >= 1 && K <= ((size_t)1 << 30) && T >= 1 && T <= 1024, "qmri:dict_compress:F", "F must be K x T with K >= 1 and 1 <= T <= 1024");
        const mxArray* P = prhs[2];
        const mxArray* f;
        const char* pid = "qmri:dict_compress:params";
        qmri_dsvd_params p = {0, 16, 0.0, 0.0, 0};
        const bool has_s = mxGetField(P, 0, "s") != nullptr, has_e = mxGetField(P, 0, "energy") != nullptr;
        want(has_s != has_e, pid, "params needs exactly one of the fields s and energy");
        const double smax_here = (double)std::min<size_t>(16, std::min(K, T));
        if (has_s) p.s = int_arg(mxGetField(P, 0, "s"), 1, smax_here, pid, "params.s must be an integer with 1 <= s <= min(16, K, T)");
        else {
            p.energy = scalar_field(P, "energy", 0.0);
            want(p.energy > 0.0 && p.energy <= 1.0, pid, "params.energy must be in (0, 1]");
            if ((f = mxGetField(P, 0, "s_max"))) p.s_max = int_arg(f, 1, 16, pid, "params.s_max must be an integer in [1, 16]");
        }
        p.tol = scalar_field(P, "tol", 0.0);
        want(std::isfinite(p.tol) && p.tol >= 0.0 && p.tol < 1.0, pid, "params.tol must be in [0, 1)");
        if ((f = mxGetField(P, 0, "maxit"))) p.maxit = int_arg(f, 0, 1e9, pid, "params.maxit must be an integer >= 0");
        std::vector<double> Vo(T * 16), eo(16);
        std::vector<float> Do(K * 16);
        mxArray* nd = mxCreateNumericMatrix(K, 1, mxSINGLE_CLASS, mxREAL);
        int s = 0;
        qmri_dsvd_info info{};
        const int st = qmri_dict_compress(ctx(), (int)K, (int)T, mxGetData(A), mxIsDouble(A) ? 1 : 0, &p, &s, Vo.data(), Do.data(), (float*)mxGetData(nd), eo.data(), &info);
        if (st != QMRI_OK) mxDestroyArray(nd);
        check(st);
        plhs[0] = mxCreateDoubleMatrix(T, s, mxREAL);
        std::memcpy(mxGetDoubles(plhs[0]), Vo.data(), T * s * sizeof(double));
        if (nlhs > 1) {
            plhs[1] = mxCreateNumericMatrix(K, s, mxSINGLE_CLASS, mxREAL);
            std::memcpy(mxGetData(plhs[1]), Do.data(), K * s * sizeof(float));
        }
        if (nlhs > 2) plhs[2] = nd; else mxDestroyArray(nd);
        if (nlhs > 3) {
            plhs[3] = mxCreateDoubleMatrix(s, 1, mxREAL);
            std::memcpy(mxGetDoubles(plhs[3]), eo.data(), s * sizeof(double));
        }
        if (nlhs > 4) {
            const char* names[] = {"s", "iters", "converged", "energy_reached", "max_resid", "energy_kept"};
            const double vals[] = {(double)info.s, (double)info.iters, (double)info.converged, (double)info.energy_reached, info.max_resid, info.energy_kept};
            plhs[4] = mxCreateStructMatrix(1, 1, 6, names);
            for (int k = 0; k < 6; ++k) mxSetFieldByNumber(plhs[4], 0, k, mxCreateDoubleScalar(vals[k]));
        }
    } else if (c == "dict_simulate") {               // F = qmri_mex('dict_simulate', alpha, tr, te, t1, t2, b1, params)
        // extension (no reference counterpart): the fingerprints of a FISP-MRF sequence by extended phase graphs (qmri_dict_simulate).  alpha: T flip
        // angles in radians, T <= 1024; tr, te: T values or one, seconds; t1, t2: K values each, seconds; b1: K values or [] (1); all real double.
        // params: a struct with the optional nstates (32), inversion (1), ti (0), inv_eff (1), single (0: F double; 1: F single).  F is K x T.
        need(nrhs, 8, "F = qmri_mex('dict_simulate', alpha, tr, te, t1, t2, b1, params)");
        want(mxIsStruct(prhs[7]), "qmri:dict_simulate:params", "params must be a struct (fields nstates, inversion, ti, inv_eff, single)");
        auto real_vec = [](const mxArray* a, const char* id, const char* msg) {
            want(mxIsDouble(a) && !mxIsComplex(a), id, msg);
            return mxGetNumberOfElements(a);
        };
        const size_t T = real_vec(prhs[1], "qmri:dict_simulate:alpha", "alpha must be a real double vector (complex flip angles are not supported)");
        want(T >= 1 && T <= 1024, "qmri:dict_simulate:alpha", "alpha must hold 1 <= T <= 1024 flip angles");
        std::vector<double> sched[2];
        const char* sid[2] = {"qmri:dict_simulate:tr", "qmri:dict_simulate:te"};
        for (int q = 0; q < 2; ++q) {
            const size_t n = real_vec(prhs[2 + q], sid[q], "tr / te must be real double, one value or one per frame");
            want(n == 1 || n == T, sid[q], "tr / te must be real double, one value or one per frame");
            sched[q].resize(T);
            for (size_t t = 0; t < T; ++t) sched[q][t] = mxGetDoubles(prhs[2 + q])[n == 1 ? 0 : t];
        }
        const char* aid = "qmri:dict_simulate:atoms";
        const size_t K = real_vec(prhs[4], aid, "t1, t2 and b1 must be real double (complex values are not supported)");
        want(K >= 1 && K <= ((size_t)1 << 30) && real_vec(prhs[5], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid,
             "t1 and t2 must hold the same number K >= 1 of atoms");
        const bool has_b1 = mxGetNumberOfElements(prhs[6]) > 0;
        if (has_b1) want(real_vec(prhs[6], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid, "b1 must be [] or hold K values");
        const mxArray* P = prhs[7];
        const mxArray* f;
        const char* pid = "qmri:dict_simulate:params";
        qmri_epg_params p = {32, 1, 0.0, 1.0, 1};
        if ((f = mxGetField(P, 0, "nstates"))) p.nstates = int_arg(f, 1, 256, pid, "params.nstates must be an integer in [1, 256]");
        if ((f = mxGetField(P, 0, "inversion"))) p.inversion = int_arg(f, 0, 1, pid, "params.inversion must be 0 or 1");
        if ((f = mxGetField(P, 0, "single"))) p.out_is_f64 = 1 - int_arg(f, 0, 1, pid, "params.single must be 0 or 1");
        p.ti = scalar_field(P, "ti", 0.0);
        p.inv_eff = scalar_field(P, "inv_eff", 1.0);
        want(std::isfinite(p.ti) && p.ti >= 0.0, pid, "params.ti must be finite and >= 0");
        want(p.inv_eff > 0.0 && p.inv_eff <= 1.0, pid, "params.inv_eff must be in (0, 1]");
        mxArray* Fo = mxCreateNumericMatrix(K, T, p.out_is_f64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS, mxREAL);
        const int st = qmri_dict_simulate(ctx(), (int)K, (int)T, mxGetDoubles(prhs[1]), sched[0].data(), sched[1].data(), mxGetDoubles(prhs[4]), mxGetDoubles(prhs[5]),
                                          has_b1 ? mxGetDoubles(prhs[6]) : nullptr, &p, mxGetData(Fo));
        if (st != QMRI_OK) mxDestroyArray(Fo);
        check(st);
        plhs[0] = Fo;
    } else if (c == "dict_simulate_sp") {            // F = qmri_mex('dict_simulate_sp', alpha, tr, te, t1, t2, b1, params, prof, w)
        // extension (no reference counterpart): 'dict_simulate' integrated over a slice profile (qmri_dict_simulate_sp).  The
        // first seven arguments are those of 'dict_simulate'.  w: Q weights, 1 <= Q <= 64; prof: the flip-angle scales, Q x 1 (the same in every
        // frame) or Q x T (column-major: q fastest); both real double.  F is K x T.
        need(nrhs, 10, "F = qmri_mex('dict_simulate_sp', alpha, tr, te, t1, t2, b1, params, prof, w)");
        want(mxIsStruct(prhs[7]), "qmri:dict_simulate_sp:params", "params must be a struct (fields nstates, inversion, ti, inv_eff, single)");
        auto real_vec = [](const mxArray* a, const char* id, const char* msg) {
            want(mxIsDouble(a) && !mxIsComplex(a), id, msg);
            return mxGetNumberOfElements(a);
        };
        const size_t T = real_vec(prhs[1], "qmri:dict_simulate_sp:alpha", "alpha must be a real double vector (complex flip angles are not supported)");
        want(T >= 1 && T <= 1024, "qmri:dict_simulate_sp:alpha", "alpha must hold 1 <= T <= 1024 flip angles");
        std::vector<double> sched[2];
        const char* sid[2] = {"qmri:dict_simulate_sp:tr", "qmri:dict_simulate_sp:te"};
        for (int q = 0; q < 2; ++q) {
            const size_t n = real_vec(prhs[2 + q], sid[q], "tr / te must be real double, one value or one per frame");
            want(n == 1 || n == T, sid[q], "tr / te must be real double, one value or one per frame");
            sched[q].resize(T);
            for (size_t t = 0; t < T; ++t) sched[q][t] = mxGetDoubles(prhs[2 + q])[n == 1 ? 0 : t];
        }
        const char* aid = "qmri:dict_simulate_sp:atoms";
        const size_t K = real_vec(prhs[4], aid, "t1, t2 and b1 must be real double (complex values are not supported)");
        want(K >= 1 && K <= ((size_t)1 << 30) && real_vec(prhs[5], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid,
             "t1 and t2 must hold the same number K >= 1 of atoms");
        const bool has_b1 = mxGetNumberOfElements(prhs[6]) > 0;
        if (has_b1) want(real_vec(prhs[6], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid, "b1 must be [] or hold K values");
        const mxArray* P = prhs[7];
        const mxArray* f;
        const char* pid = "qmri:dict_simulate_sp:params";
        qmri_epg_params p = {32, 1, 0.0, 1.0, 1};
        if ((f = mxGetField(P, 0, "nstates"))) p.nstates = int_arg(f, 1, 256, pid, "params.nstates must be an integer in [1, 256]");
        if ((f = mxGetField(P, 0, "inversion"))) p.inversion = int_arg(f, 0, 1, pid, "params.inversion must be 0 or 1");
        if ((f = mxGetField(P, 0, "single"))) p.out_is_f64 = 1 - int_arg(f, 0, 1, pid, "params.single must be 0 or 1");
        p.ti = scalar_field(P, "ti", 0.0);
        p.inv_eff = scalar_field(P, "inv_eff", 1.0);
        want(std::isfinite(p.ti) && p.ti >= 0.0, pid, "params.ti must be finite and >= 0");
        want(p.inv_eff > 0.0 && p.inv_eff <= 1.0, pid, "params.inv_eff must be in (0, 1]");
        const char* qid = "qmri:dict_simulate_sp:profile";
        const size_t Q = real_vec(prhs[9], qid, "prof and w must be real double (complex profiles are not supported)");
        want(Q >= 1 && Q <= 64, qid, "w must hold 1 <= Q <= 64 weights");
        const size_t np = real_vec(prhs[8], qid, "prof and w must be real double (complex profiles are not supported)");
        want(np == Q || np == Q * T, qid, "prof must be Q x 1 or Q x T");
        want(np == Q || mxGetM(prhs[8]) == Q, qid, "prof must be Q x 1 or Q x T");
        const qmri_epg_profile sp = {(int32_t)Q, np == Q ? 0 : 1, mxGetDoubles(prhs[8]), mxGetDoubles(prhs[9])};
        mxArray* Fo = mxCreateNumericMatrix(K, T, p.out_is_f64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS, mxREAL);
        const int st = qmri_dict_simulate_sp(ctx(), (int)K, (int)T, mxGetDoubles(prhs[1]), sched[0].data(), sched[1].data(), mxGetDoubles(prhs[4]),
                                             mxGetDoubles(prhs[5]), has_b1 ? mxGetDoubles(prhs[6]) : nullptr, &p, &sp, mxGetData(Fo));
        if (st != QMRI_OK) mxDestroyArray(Fo);
        check(st);
        plhs[0] = Fo;
    } else if (c == "dict_simulate_seq") {           // F = qmri_mex('dict_simulate_seq', alpha, tr, te, t1, t2, b1, params, blocks, ncycles)
        // extension (no reference counterpart): the fingerprints of a prepared, repeated FISP train (qmri_dict_simulate_seq).
        // The first six arguments are those of 'dict_simulate'; params takes nstates (32) and single (0).  blocks: a real double 5 x B matrix,
        // 1 <= B <= 64, one column per block: nframes; prep (0 none, 1 inversion, 2 T2 preparation); wait; prep_time; prep_eff -- what
        // matlab/qmri_dict_simulate_seq.m makes of its struct array.  ncycles: an integer in [1, 16].  F is K x T.
        need(nrhs, 10, "F = qmri_mex('dict_simulate_seq', alpha, tr, te, t1, t2, b1, params, blocks, ncycles)");
        want(mxIsStruct(prhs[7]), "qmri:dict_simulate_seq:params", "params must be a struct (fields nstates, single)");
        auto real_vec = [](const mxArray* a, const char* id, const char* msg) {
            want(mxIsDouble(a) && !mxIsComplex(a), id, msg);
            return mxGetNumberOfElements(a);
        };
        const size_t T = real_vec(prhs[1], "qmri:dict_simulate_seq:alpha", "alpha must be a real double vector (complex flip angles are not supported)");
        want(T >= 1 && T <= 1024, "qmri:dict_simulate_seq:alpha", "alpha must hold 1 <= T <= 1024 flip angles");
        std::vector<double> sched[2];
        const char* sid[2] = {"qmri:dict_simulate_seq:tr", "qmri:dict_simulate_seq:te"};
        for (int q = 0; q < 2; ++q) {
            const size_t n = real_vec(prhs[2 + q], sid[q], "tr / te must be real double, one value or one per frame");
            want(n == 1 || n == T, sid[q], "tr / te must be real double, one value or one per frame");
            sched[q].resize(T);
            for (size_t t = 0; t < T; ++t) sched[q][t] = mxGetDoubles(prhs[2 + q])[n == 1 ? 0 : t];
        }
        const char* aid = "qmri:dict_simulate_seq:atoms";
        const size_t K = real_vec(prhs[4], aid, "t1, t2 and b1 must be real double (complex values are not supported)");
        want(K >= 1 && K <= ((size_t)1 << 30) && real_vec(prhs[5], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid,
             "t1 and t2 must hold the same number K >= 1 of atoms");
        const bool has_b1 = mxGetNumberOfElements(prhs[6]) > 0;
        if (has_b1) want(real_vec(prhs[6], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid, "b1 must be [] or hold K values");
        const mxArray* P = prhs[7];
        const mxArray* f;
        const char* pid = "qmri:dict_simulate_seq:params";
        qmri_epg_params p = {32, 0, 0.0, 1.0, 1};
        if ((f = mxGetField(P, 0, "nstates"))) p.nstates = int_arg(f, 1, 256, pid, "params.nstates must be an integer in [1, 256]");
        if ((f = mxGetField(P, 0, "single"))) p.out_is_f64 = 1 - int_arg(f, 0, 1, pid, "params.single must be 0 or 1");
        const char* bid = "qmri:dict_simulate_seq:blocks";
        const size_t nb = real_vec(prhs[8], bid, "blocks must be a real double 5 x B matrix, 1 <= B <= 64");
        want(mxGetM(prhs[8]) == 5 && nb >= 5 && nb <= 5 * 64, bid, "blocks must be a real double 5 x B matrix, 1 <= B <= 64");
        const size_t B = nb / 5;
        std::vector<qmri_epg_block> blocks(B);
        for (size_t b = 0; b < B; ++b) {
            const double* col = mxGetDoubles(prhs[8]) + 5 * b;
            // the two integers are checked before the cast; the three times are the library's to refuse
            want(std::isfinite(col[0]) && col[0] == std::floor(col[0]) && col[0] >= 1.0 && col[0] <= 1024.0, bid, "blocks(1, :) (nframes) must be integers in [1, 1024]");
            want(std::isfinite(col[1]) && col[1] == std::floor(col[1]) && col[1] >= 0.0 && col[1] <= 2.0, bid, "blocks(2, :) (prep) must be 0, 1 or 2");
            blocks[b] = {(int32_t)col[0], (int32_t)col[1], col[2], col[3], col[4]};
        }
        const int ncycles = int_arg(prhs[9], 1, 16, "qmri:dict_simulate_seq:ncycles", "ncycles must be an integer in [1, 16]");
        const qmri_epg_seq seq = {(int32_t)B, ncycles, blocks.data(), {0, 0, 0, 0}};
        mxArray* Fo = mxCreateNumericMatrix(K, T, p.out_is_f64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS, mxREAL);
        const int st = qmri_dict_simulate_seq(ctx(), (int)K, (int)T, mxGetDoubles(prhs[1]), sched[0].data(), sched[1].data(), mxGetDoubles(prhs[4]),
                                              mxGetDoubles(prhs[5]), has_b1 ? mxGetDoubles(prhs[6]) : nullptr, &p, &seq, mxGetData(Fo));
        if (st != QMRI_OK) mxDestroyArray(Fo);
        check(st);
        plhs[0] = Fo;
    } else if (c == "dict_simulate_grad") {          // [F, dF, crb, flags] = qmri_mex('dict_simulate_grad', alpha, tr, te, t1, t2, b1, params, V)
        // extension (no reference counterpart): the fingerprints of 'dict_simulate' with their derivatives and the Cramer-Rao bound they give
        // (qmri_dict_simulate_grad).  The first seven arguments are those of 'dict_simulate'; params also takes nparams (2:
        // T1, T2, the default; 3: T1, T2, b1) and bound_only (0; 1: F and dF are not computed and come back empty).  V: [] or a real double T x s
        // subspace, 1 <= s <= 16.  F is K x T, dF K x T x P, crb (1 + P) x K (atom k in column k), flags int32 K x 1.  dF is computed from two
        // outputs on, the bound from three on.
        need(nrhs, 9, "[F, dF, crb, flags] = qmri_mex('dict_simulate_grad', alpha, tr, te, t1, t2, b1, params, V)");
        want(mxIsStruct(prhs[7]), "qmri:dict_simulate_grad:params", "params must be a struct (fields nstates, inversion, ti, inv_eff, single, nparams, bound_only)");
        auto real_vec = [](const mxArray* a, const char* id, const char* msg) {
            want(mxIsDouble(a) && !mxIsComplex(a), id, msg);
            return mxGetNumberOfElements(a);
        };
        const size_t T = real_vec(prhs[1], "qmri:dict_simulate_grad:alpha", "alpha must be a real double vector (complex flip angles are not supported)");
        want(T >= 1 && T <= 1024, "qmri:dict_simulate_grad:alpha", "alpha must hold 1 <= T <= 1024 flip angles");
        std::vector<double> sched[2];
        const char* sid[2] = {"qmri:dict_simulate_grad:tr", "qmri:dict_simulate_grad:te"};
        for (int q = 0; q < 2; ++q) {
            const size_t n = real_vec(prhs[2 + q], sid[q], "tr / te must be real double, one value or one per frame");
            want(n == 1 || n == T, sid[q], "tr / te must be real double, one value or one per frame");
            sched[q].resize(T);
            for (size_t t = 0; t < T; ++t) sched[q][t] = mxGetDoubles(prhs[2 + q])[n == 1 ? 0 : t];
        }
        const char* aid = "qmri:dict_simulate_grad:atoms";
        const size_t K = real_vec(prhs[4], aid, "t1, t2 and b1 must be real double (complex values are not supported)");
        want(K >= 1 && K <= ((size_t)1 << 30) && real_vec(prhs[5], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid,
             "t1 and t2 must hold the same number K >= 1 of atoms");
        const bool has_b1 = mxGetNumberOfElements(prhs[6]) > 0;
        if (has_b1) want(real_vec(prhs[6], aid, "t1, t2 and b1 must be real double (complex values are not supported)") == K, aid, "b1 must be [] or hold K values");
        const mxArray* P = prhs[7];
        const mxArray* f;
        const char* pid = "qmri:dict_simulate_grad:params";
        qmri_epg_params p = {32, 1, 0.0, 1.0, 1};
        if ((f = mxGetField(P, 0, "nstates"))) p.nstates = int_arg(f, 1, 256, pid, "params.nstates must be an integer in [1, 256]");
        if ((f = mxGetField(P, 0, "inversion"))) p.inversion = int_arg(f, 0, 1, pid, "params.inversion must be 0 or 1");
        if ((f = mxGetField(P, 0, "single"))) p.out_is_f64 = 1 - int_arg(f, 0, 1, pid, "params.single must be 0 or 1");
        p.ti = scalar_field(P, "ti", 0.0);
        p.inv_eff = scalar_field(P, "inv_eff", 1.0);
        want(std::isfinite(p.ti) && p.ti >= 0.0, pid, "params.ti must be finite and >= 0");
        want(p.inv_eff > 0.0 && p.inv_eff <= 1.0, pid, "params.inv_eff must be in (0, 1]");
        qmri_epg_grad_params gp = {2, 0, nullptr, {0, 0, 0, 0}};
        int bound_only = 0;
        if ((f = mxGetField(P, 0, "nparams"))) gp.nparams = int_arg(f, 2, 3, pid, "params.nparams must be 2 or 3");
        if ((f = mxGetField(P, 0, "bound_only"))) bound_only = int_arg(f, 0, 1, pid, "params.bound_only must be 0 or 1");
        const char* vid = "qmri:dict_simulate_grad:V";
        if (mxGetNumberOfElements(prhs[8]) > 0) {
            const size_t nv = real_vec(prhs[8], vid, "V must be [] or a real double T x s matrix, 1 <= s <= 16");
            want(mxGetM(prhs[8]) == T && nv / T >= 1 && nv / T <= 16 && nv % T == 0, vid, "V must be [] or a real double T x s matrix, 1 <= s <= 16");
            gp.s = (int32_t)(nv / T);
            gp.V = mxGetDoubles(prhs[8]);
        }
        const bool want_F = !bound_only, want_dF = !bound_only && nlhs > 1, want_crb = bound_only || nlhs > 2;
        const mxClassID cls = p.out_is_f64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS;
        const mwSize d3[3] = {(mwSize)K, (mwSize)T, (mwSize)gp.nparams};
        mxArray* out[4] = {want_F ? mxCreateNumericMatrix(K, T, cls, mxREAL) : mxCreateNumericMatrix(0, 0, cls, mxREAL),
                           want_dF ? mxCreateNumericArray(3, d3, cls, mxREAL) : mxCreateNumericMatrix(0, 0, cls, mxREAL),
                           want_crb ? mxCreateDoubleMatrix(1 + gp.nparams, K, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL),
                           want_crb ? mxCreateNumericMatrix(K, 1, mxINT32_CLASS, mxREAL) : mxCreateNumericMatrix(0, 0, mxINT32_CLASS, mxREAL)};
        const int st = qmri_dict_simulate_grad(ctx(), (int)K, (int)T, mxGetDoubles(prhs[1]), sched[0].data(), sched[1].data(), mxGetDoubles(prhs[4]),
                                               mxGetDoubles(prhs[5]), has_b1 ? mxGetDoubles(prhs[6]) : nullptr, &p, &gp, want_F ? mxGetData(out[0]) : nullptr,
                                               want_dF ? mxGetData(out[1]) : nullptr, want_crb ? mxGetDoubles(out[2]) : nullptr,
                                               want_crb ? static_cast<int32_t*>(mxGetData(out[3])) : nullptr);
        for (int k = 0; k < 4; ++k)
            if (st != QMRI_OK || k >= std::max(nlhs, 1)) mxDestroyArray(out[k]);
        check(st);
        for (int k = 0; k < std::max(nlhs, 1) && k < 4; ++k) plhs[k] = out[k];
    } else if (c == "lrtv") {                        // [x, info] = qmri_mex('lrtv', y, param_struct, [N M s])   (FISTA_deep, main_recon_tsmis_FFT.m:273-282)
        need(nrhs, 4, "[x, info] = qmri_mex('lrtv', y, param, [N M s])");
        const mxArray* P = prhs[2];
        want(mxIsStruct(P), "qmri:lrtv:type", "param must be a struct");
        (void)dims_numel(prhs[3]);
        want(is_cdouble(prhs[1]) && mxGetNumberOfElements(prhs[1]) == operator_m(), "qmri:lrtv:size", "y must be a complex double vector with one entry per sample");
        qmri_lrtv_params p;
        p.K = scalar_field(P, "K", 4e-5);
        p.iters = (int)scalar_field(P, "iter", 200);
        p.step = scalar_field(P, "step", 0.0);
        p.tol = scalar_field(P, "tol", 1e-4);
        p.backtrack = (int)scalar_field(P, "backtrack", 1);
        p.prox_tol = 0.0; p.prox_maxit = 0;                        // prox_tv defaults (prox_tv.m:99-101)
        const double* d = mxGetDoubles(prhs[3]);
        const mwSize dims[3] = {(mwSize)d[0], (mwSize)d[1], (mwSize)d[2]};
        plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxCOMPLEX);
        qmri_lrtv_info info;
        check(qmri_lrtv(ctx(), mxGetComplexDoubles(prhs[1]), &p, mxGetComplexDoubles(plhs[0]), &info));
        if (nlhs > 1) {
            const char* names[] = {"iters", "halvings", "step", "obj", "prox_calls", "prox_iters_total"};
            plhs[1] = mxCreateStructMatrix(1, 1, 6, names);
            const double v[6] = {(double)info.iters, (double)info.halvings, info.step, info.obj, (double)info.prox_calls, (double)info.prox_iters_total};
            for (int i = 0; i < 6; ++i) mxSetFieldByNumber(plhs[1], 0, i, mxCreateDoubleScalar(v[i]));
        }
    } else if (c == "set_dictionary") {              // qmri_mex('set_dictionary', D(single KxS), normD(single), lut(single KxQ))
        // a complex mxArray holds interleaved (re,im) pairs: reading it as K x s reals would match against garbage atoms.
        // mrf_dtm_hip.m passes real(D) after checking that imag(D) is zero; anything else is refused here.
        for (int a = 1; a <= 3; ++a)
            if (nrhs <= a || mxIsComplex(prhs[a]) || !mxIsSingle(prhs[a]))
                mexErrMsgIdAndTxt("qmri:set_dictionary:type", "D, normD and lut must be real single arrays (argument %d is not)", a);
        if (mxGetNumberOfElements(prhs[2]) != mxGetM(prhs[1]) || mxGetM(prhs[3]) != mxGetM(prhs[1]))
            mexErrMsgIdAndTxt("qmri:set_dictionary:size", "normD must have K elements and lut K rows (K = rows of D)");
        drop(g_dict.D); drop(g_dict.normD); drop(g_dict.lut);
        g_dict.D = keep(prhs[1]); g_dict.normD = keep(prhs[2]); g_dict.lut = keep(prhs[3]);
        g_comp.clear();
        g_refine.clear();
        g_ngroups = 0;
        plan_dictionary();
    } else if (c == "dict_match") {                  // [qmap, pd, mt, dm, xfit] = qmri_mex('dict_match', X(Npix x s complex double), Q)
        need(nrhs, 3, "[qmap, pd, mt, dm, xfit] = qmri_mex('dict_match', X, Q)");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) (mrf_dtm_hip(dict, [], [])) first");
        want(is_cdouble(prhs[1]) && mxGetN(prhs[1]) == mxGetN(g_dict.D), "qmri:dict_match:size", "X must be complex double, Npix x s (s = columns of dict.D)");
        want((size_t)mxGetScalar(prhs[2]) == mxGetN(g_dict.lut), "qmri:dict_match:size", "Q must be the number of columns of dict.lut");
        const int npix = (int)mxGetM(prhs[1]), Q = (int)mxGetScalar(prhs[2]);
        mxArray* xfit = (nlhs > 4) ? mxCreateNumericMatrix(npix, mxGetN(prhs[1]), mxSINGLE_CLASS, mxCOMPLEX) : nullptr;   // out.Xfit, mrf_dtm_cpu.m:129-134
        plhs[0] = mxCreateNumericMatrix(npix, Q, mxSINGLE_CLASS, mxREAL);
        mxArray* pd = mxCreateNumericMatrix(npix, 1, mxSINGLE_CLASS, mxCOMPLEX);
        mxArray* mt = mxCreateNumericMatrix(npix, 1, mxSINGLE_CLASS, mxREAL);
        mxArray* dm = mxCreateNumericMatrix(npix, 1, mxINT32_CLASS, mxREAL);
        check(qmri_dict_match_xfit(ctx(), mxGetComplexDoubles(prhs[1]), npix, (float*)mxGetData(plhs[0]), (float*)mxGetData(pd),
                                   (float*)mxGetData(mt), (int32_t*)mxGetData(dm), xfit ? (float*)mxGetData(xfit) : nullptr));
        if (nlhs > 1) plhs[1] = pd; else mxDestroyArray(pd);
        if (nlhs > 2) plhs[2] = mt; else mxDestroyArray(mt);
        if (nlhs > 3) plhs[3] = dm; else mxDestroyArray(dm);
        if (nlhs > 4) plhs[4] = xfit;
    } else if (c == "set_dictionary_groups") {       // qmri_mex('set_dictionary_groups', group_ptr(G+1 doubles, 0-based), group_val(G doubles)); ([], []) clears
        // groups of the set dictionary for 'dict_match_grouped' (extension; qmri.h qmri_set_dictionary_groups).  'set_dictionary' drops them.
        need(nrhs, 3, "qmri_mex('set_dictionary_groups', group_ptr, group_val)");
        for (int a = 1; a <= 2; ++a)
            want(mxIsDouble(prhs[a]) && !mxIsComplex(prhs[a]), "qmri:set_dictionary_groups:type", "group_ptr and group_val must be real double arrays");
        const size_t G = mxGetNumberOfElements(prhs[2]);
        const bool clear = G == 0 && mxGetNumberOfElements(prhs[1]) == 0;
        want(clear || (G >= 1 && G <= 256 && mxGetNumberOfElements(prhs[1]) == G + 1), "qmri:set_dictionary_groups:size",
             "group_val must have 1 <= G <= 256 elements and group_ptr G + 1");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) first");
        if (clear) { check(qmri_set_dictionary_groups(ctx(), 0, nullptr, nullptr)); g_ngroups = 0; return; }
        std::vector<int32_t> gp(G + 1);
        const double* v = mxGetDoubles(prhs[1]);
        for (size_t g = 0; g <= G; ++g) {
            want(std::isfinite(v[g]) && v[g] == std::floor(v[g]) && v[g] >= 0 && v[g] <= 2147483647.0, "qmri:set_dictionary_groups:size", "group_ptr must hold 0-based atom offsets");
            gp[g] = (int32_t)v[g];
        }
        check(qmri_set_dictionary_groups(ctx(), (int)G, gp.data(), mxGetDoubles(prhs[2])));
        g_ngroups = (int)G;
    } else if (c == "dict_match_grouped") {          // [qmap, pd, mt, dm, grp, xfit] = qmri_mex('dict_match_grouped', X(Npix x s complex double), Q, sel(Npix double))
        need(nrhs, 4, "[qmap, pd, mt, dm, grp, xfit] = qmri_mex('dict_match_grouped', X, Q, sel)");
        want(is_cdouble(prhs[1]) && mxGetM(prhs[1]) >= 1 && mxGetM(prhs[1]) <= 2147483647u, "qmri:dict_match_grouped:type", "X must be complex double, Npix x s");
        want(mxIsDouble(prhs[2]) && !mxIsComplex(prhs[2]) && mxGetNumberOfElements(prhs[2]) == 1, "qmri:dict_match_grouped:type", "Q must be a real double scalar");
        want(mxIsDouble(prhs[3]) && !mxIsComplex(prhs[3]), "qmri:dict_match_grouped:type", "sel must be a real double array");
        want(mxGetNumberOfElements(prhs[3]) == mxGetM(prhs[1]), "qmri:dict_match_grouped:size", "sel must have one value per row of X");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) (mrf_dtm_b1_hip) first");
        want(mxGetN(prhs[1]) == mxGetN(g_dict.D), "qmri:dict_match_grouped:size", "X must have s columns (s = columns of dict.D)");
        want(mxGetScalar(prhs[2]) == (double)mxGetN(g_dict.lut), "qmri:dict_match_grouped:size", "Q must be the number of columns of dict.lut");
        const int npix = (int)mxGetM(prhs[1]), Q = (int)mxGetScalar(prhs[2]);
        mxArray* xfit = (nlhs > 5) ? mxCreateNumericMatrix(npix, mxGetN(prhs[1]), mxSINGLE_CLASS, mxCOMPLEX) : nullptr;
        plhs[0] = mxCreateNumericMatrix(npix, Q, mxSINGLE_CLASS, mxREAL);
        mxArray* pd = mxCreateNumericMatrix(npix, 1, mxSINGLE_CLASS, mxCOMPLEX);
        mxArray* mt = mxCreateNumericMatrix(npix, 1, mxSINGLE_CLASS, mxREAL);
        mxArray* dm = mxCreateNumericMatrix(npix, 1, mxINT32_CLASS, mxREAL);
        mxArray* grp = mxCreateNumericMatrix(npix, 1, mxINT32_CLASS, mxREAL);
        check(qmri_dict_match_grouped(ctx(), mxGetComplexDoubles(prhs[1]), npix, mxGetDoubles(prhs[3]), (float*)mxGetData(plhs[0]), (float*)mxGetData(pd),
                                      (float*)mxGetData(mt), (int32_t*)mxGetData(dm), (int32_t*)mxGetData(grp), xfit ? (float*)mxGetData(xfit) : nullptr));
        if (nlhs > 1) plhs[1] = pd; else mxDestroyArray(pd);
        if (nlhs > 2) plhs[2] = mt; else mxDestroyArray(mt);
        if (nlhs > 3) plhs[3] = dm; else mxDestroyArray(dm);
        if (nlhs > 4) plhs[4] = grp; else mxDestroyArray(grp);
        if (nlhs > 5) plhs[5] = xfit;
    } else if (c == "group_scores") {                // score(Npix x G single) = qmri_mex('group_scores', X(Npix x s complex double))
        // per group the mt of 'dict_match_grouped' with a constant selector (extension; qmri.h qmri_dict_group_scores)
        const char* usage = "score = qmri_mex('group_scores', X)";
        need(nrhs, 2, usage);
        want(nlhs <= 1, "qmri:usage", usage);
        want(is_cdouble(prhs[1]) && mxGetM(prhs[1]) >= 1 && mxGetM(prhs[1]) <= 2147483647u, "qmri:group_scores:type", "X must be complex double, Npix x s");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) first");
        want(mxGetN(prhs[1]) == mxGetN(g_dict.D), "qmri:group_scores:size", "X must have s columns (s = columns of dict.D)");
        want(g_ngroups > 0, "qmri:state", "no groups: call qmri_mex('set_dictionary_groups', group_ptr, group_val) first");
        const size_t npix = mxGetM(prhs[1]);
        plhs[0] = mxCreateNumericMatrix(npix, (size_t)g_ngroups, mxSINGLE_CLASS, mxREAL);
        check(qmri_dict_group_scores(ctx(), mxGetComplexDoubles(prhs[1]), (int)npix, (float*)mxGetData(plhs[0])));
    } else if (c == "b1_estimate") {                 // [b1, grp, conf, info] = qmri_mex('b1_estimate', X(Npix x s complex double), [N M nslices], mask(Npix double | []), half_window)
        // the B1 map from the fingerprints: group scores, then the pooled argmax over (2h+1)^2 windows (extension; qmri.h qmri_b1_estimate)
        const char* usage = "[b1, grp, conf, info] = qmri_mex('b1_estimate', X, [N M nslices], mask, half_window)";
        need(nrhs, 5, usage);
        want(nlhs <= 4, "qmri:usage", usage);
        want(is_cdouble(prhs[1]) && mxGetM(prhs[1]) >= 1 && mxGetM(prhs[1]) <= 2147483647u, "qmri:b1_estimate:type", "X must be complex double, Npix x s");
        want(mxIsDouble(prhs[2]) && !mxIsComplex(prhs[2]) && mxGetNumberOfElements(prhs[2]) == 3, "qmri:b1_estimate:size", "the size argument must be [N M nslices]");
        const double* dv = mxGetDoubles(prhs[2]);
        for (int k = 0; k < 3; ++k)
            want(std::isfinite(dv[k]) && dv[k] == std::floor(dv[k]) && dv[k] >= 1 && dv[k] <= 2147483647.0, "qmri:b1_estimate:size", "[N M nslices] must hold positive integers");
        const size_t npix = mxGetM(prhs[1]);
        want(dv[0] * dv[1] * dv[2] == (double)npix, "qmri:b1_estimate:size", "X must have N * M * nslices rows");
        want(mxIsDouble(prhs[3]) && !mxIsComplex(prhs[3]) && (mxGetNumberOfElements(prhs[3]) == 0 || mxGetNumberOfElements(prhs[3]) == npix),
             "qmri:b1_estimate:type", "mask must be a real double array with one value per row of X, or []");
        qmri_b1est_params prm{};
        prm.half_window = int_arg(prhs[4], 0, 32, "qmri:b1_estimate:window", "half_window must be an integer in 0 .. 32");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) first");
        want(mxGetN(prhs[1]) == mxGetN(g_dict.D), "qmri:b1_estimate:size", "X must have s columns (s = columns of dict.D)");
        want(g_ngroups > 0, "qmri:state", "no groups: call qmri_mex('set_dictionary_groups', group_ptr, group_val) first");
        std::vector<uint8_t> mask;
        if (mxGetNumberOfElements(prhs[3])) {
            mask.resize(npix);
            const double* mv = mxGetDoubles(prhs[3]);
            for (size_t k = 0; k < npix; ++k) mask[k] = mv[k] != 0.0;
        }
        plhs[0] = mxCreateDoubleMatrix(npix, 1, mxREAL);
        mxArray* grp = mxCreateNumericMatrix(npix, 1, mxINT32_CLASS, mxREAL);
        mxArray* conf = mxCreateDoubleMatrix(npix, 1, mxREAL);
        qmri_b1est_info info{};
        check(qmri_b1_estimate(ctx(), mxGetComplexDoubles(prhs[1]), (int)dv[0], (int)dv[1], (int)dv[2], mask.empty() ? nullptr : mask.data(), &prm,
                               mxGetDoubles(plhs[0]), (int32_t*)mxGetData(grp), mxGetDoubles(conf), &info));
        if (nlhs > 1) plhs[1] = grp; else mxDestroyArray(grp);
        if (nlhs > 2) plhs[2] = conf; else mxDestroyArray(conf);
        if (nlhs > 3) {
            const char* names[] = {"n_estimated", "n_unmatched", "mean_conf"};
            plhs[3] = mxCreateStructMatrix(1, 1, 3, names);
            const double f[3] = {(double)info.n_estimated, (double)info.n_unmatched, info.mean_conf};
            for (int k = 0; k < 3; ++k) mxSetFieldByNumber(plhs[3], 0, k, mxCreateDoubleScalar(f[k]));
        }
    } else if (c == "set_components") {              // info = qmri_mex('set_components', atoms(1..8 doubles, 1-based)); [] clears
        // the components of 'dict_unmix' (extension; qmri.h qmri_set_components).  'set_dictionary' drops them.
        need(nrhs, 2, "info = qmri_mex('set_components', atoms)");
        want(nlhs <= 1, "qmri:usage", "info = qmri_mex('set_components', atoms)");
        want(mxIsDouble(prhs[1]) && !mxIsComplex(prhs[1]), "qmri:set_components:type", "atoms must be a real double array");
        const size_t nc = mxGetNumberOfElements(prhs[1]);
        want(nc <= 8, "qmri:set_components:size", "atoms must hold 1 to 8 atom indices ([] clears)");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) first");
        std::vector<int32_t> atoms(nc);
        const double* v = mxGetDoubles(prhs[1]);
        for (size_t k = 0; k < nc; ++k) {
            want(std::isfinite(v[k]) && v[k] == std::floor(v[k]) && v[k] >= 1 && v[k] <= (double)mxGetM(g_dict.D), "qmri:set_components:size",
                 "atoms must be 1-based atom indices (1 .. rows of dict.D)");
            atoms[k] = (int32_t)v[k];
        }
        qmri_pv_info info{};
        check(qmri_set_components(ctx(), (int)nc, nc ? atoms.data() : nullptr, &info));
        g_comp = atoms;
        if (nlhs > 0) {
            const char* names[] = {"min_pivot", "C", "s"};
            plhs[0] = mxCreateStructMatrix(1, 1, 3, names);
            const double f[3] = {info.min_pivot, (double)info.C, (double)info.s};
            for (int k = 0; k < 3; ++k) mxSetFieldByNumber(plhs[0], 0, k, mxCreateDoubleScalar(f[k]));
        }
    } else if (c == "dict_unmix") {                  // [w, frac, pd, res, flags] = qmri_mex('dict_unmix', X(Npix x s complex double), mode(0 real | 1 phase))
        const char* usage = "[w, frac, pd, res, flags] = qmri_mex('dict_unmix', X, mode)";
        need(nrhs, 3, usage);
        want(nlhs <= 5, "qmri:usage", usage);
        want(is_cdouble(prhs[1]) && mxGetM(prhs[1]) >= 1 && mxGetM(prhs[1]) <= 2147483647u, "qmri:dict_unmix:type", "X must be complex double, Npix x s");
        const int mode = int_arg(prhs[2], 0, 1, "qmri:dict_unmix:mode", "mode must be 0 (real) or 1 (phase)");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) first");
        want(mxGetN(prhs[1]) == mxGetN(g_dict.D), "qmri:dict_unmix:size", "X must have s columns (s = columns of dict.D)");
        want(!g_comp.empty(), "qmri:state", "no components: call qmri_mex('set_components', atoms) first");
        const size_t npix = mxGetM(prhs[1]), nc = g_comp.size();
        plhs[0] = mxCreateDoubleMatrix(npix, nc, mxREAL);
        mxArray* frac = (nlhs > 1) ? mxCreateDoubleMatrix(npix, nc, mxREAL) : nullptr;
        mxArray* pd = (nlhs > 2) ? mxCreateDoubleMatrix(npix, 1, mxCOMPLEX) : nullptr;
        mxArray* res = (nlhs > 3) ? mxCreateDoubleMatrix(npix, 1, mxREAL) : nullptr;
        mxArray* flags = (nlhs > 4) ? mxCreateNumericMatrix(npix, 1, mxINT32_CLASS, mxREAL) : nullptr;
        check(qmri_dict_unmix(ctx(), mxGetComplexDoubles(prhs[1]), (int)npix, mode, mxGetDoubles(plhs[0]), frac ? mxGetDoubles(frac) : nullptr,
                              pd ? (double*)mxGetComplexDoubles(pd) : nullptr, res ? mxGetDoubles(res) : nullptr, flags ? (int32_t*)mxGetData(flags) : nullptr));
        if (nlhs > 1) plhs[1] = frac;
        if (nlhs > 2) plhs[2] = pd;
        if (nlhs > 3) plhs[3] = res;
        if (nlhs > 4) plhs[4] = flags;
    } else if (c == "set_refine") {                  // info = qmri_mex('set_refine', cols(1..3 doubles, 0-based lut columns)); [] clears
        // the refined columns of 'dict_refine' (extension; qmri.h qmri_set_refine).  'set_dictionary' drops them.
        need(nrhs, 2, "info = qmri_mex('set_refine', cols)");
        want(nlhs <= 1, "qmri:usage", "info = qmri_mex('set_refine', cols)");
        want(mxIsDouble(prhs[1]) && !mxIsComplex(prhs[1]), "qmri:set_refine:type", "cols must be a real double array");
        const size_t np_ = mxGetNumberOfElements(prhs[1]);
        want(np_ <= 3, "qmri:set_refine:size", "cols must hold 1 to 3 lut columns ([] clears)");
        std::vector<int32_t> cols(np_);
        const double* v = mxGetDoubles(prhs[1]);
        for (size_t k = 0; k < np_; ++k) {
            want(std::isfinite(v[k]) && v[k] == std::floor(v[k]) && v[k] >= 0 && v[k] <= 1023, "qmri:set_refine:value", "cols must be 0-based lut column indices");
            cols[k] = (int32_t)v[k];
        }
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) first");
        qmri_refine_info info{};
        check(qmri_set_refine(ctx(), (int)np_, np_ ? cols.data() : nullptr, &info));
        g_refine = cols;
        if (nlhs > 0) {
            const char* names[] = {"P", "K", "s", "count"};
            plhs[0] = mxCreateStructMatrix(1, 1, 4, names);
            const double f[3] = {(double)info.P, (double)info.K, (double)info.s};
            for (int k = 0; k < 3; ++k) mxSetFieldByNumber(plhs[0], 0, k, mxCreateDoubleScalar(f[k]));
            mxArray* cnt = mxCreateDoubleMatrix(np_, 3, mxREAL);       // row q: atoms with 0, 1, 2 neighbours along cols(q)
            for (size_t q = 0; q < np_; ++q)
                for (int j = 0; j < 3; ++j) mxGetDoubles(cnt)[q + np_ * j] = (double)info.count[q][j];
            mxSetFieldByNumber(plhs[0], 0, 3, cnt);
        }
    } else if (c == "dict_refine") {                 // [qmap, pd, res, t, centre, flags] = qmri_mex('dict_refine', X(Npix x s complex double), dm(Npix int32))
        const char* usage = "[qmap, pd, res, t, centre, flags] = qmri_mex('dict_refine', X, dm)";
        need(nrhs, 3, usage);
        want(nlhs <= 6, "qmri:usage", usage);
        want(is_cdouble(prhs[1]) && mxGetM(prhs[1]) >= 1 && mxGetM(prhs[1]) <= 2147483647u, "qmri:dict_refine:type", "X must be complex double, Npix x s");
        want(mxIsInt32(prhs[2]) && !mxIsComplex(prhs[2]) && mxGetNumberOfElements(prhs[2]) == mxGetM(prhs[1]), "qmri:dict_refine:dm",
             "dm must be int32 with one start atom per row of X (as 'dict_match' returns it)");
        want(g_dict.D != nullptr, "qmri:state", "no dictionary: call qmri_mex('set_dictionary', ...) first");
        want(mxGetN(prhs[1]) == mxGetN(g_dict.D), "qmri:dict_refine:size", "X must have s columns (s = columns of dict.D)");
        want(!g_refine.empty(), "qmri:state", "no refinement: call qmri_mex('set_refine', cols) first");
        const size_t npix = mxGetM(prhs[1]), nq = mxGetN(g_dict.lut), np_ = g_refine.size();
        plhs[0] = mxCreateDoubleMatrix(npix, nq, mxREAL);
        mxArray* pd = (nlhs > 1) ? mxCreateDoubleMatrix(npix, 1, mxCOMPLEX) : nullptr;
        mxArray* res = (nlhs > 2) ? mxCreateDoubleMatrix(npix, 1, mxREAL) : nullptr;
        mxArray* t = (nlhs > 3) ? mxCreateDoubleMatrix(npix, np_, mxREAL) : nullptr;
        mxArray* centre = (nlhs > 4) ? mxCreateNumericMatrix(npix, 1, mxINT32_CLASS, mxREAL) : nullptr;
        mxArray* flags = (nlhs > 5) ? mxCreateNumericMatrix(npix, 1, mxINT32_CLASS, mxREAL) : nullptr;
        check(qmri_dict_refine(ctx(), mxGetComplexDoubles(prhs[1]), (int)npix, (const int32_t*)mxGetData(prhs[2]), mxGetDoubles(plhs[0]),
                               pd ? (double*)mxGetComplexDoubles(pd) : nullptr, res ? mxGetDoubles(res) : nullptr, t ? mxGetDoubles(t) : nullptr,
                               centre ? (int32_t*)mxGetData(centre) : nullptr, flags ? (int32_t*)mxGetData(flags) : nullptr));
        if (nlhs > 1) plhs[1] = pd;
        if (nlhs > 2) plhs[2] = res;
        if (nlhs > 3) plhs[3] = t;
        if (nlhs > 4) plhs[4] = centre;
        if (nlhs > 5) plhs[5] = flags;
    } else if (c == "health") {                      // h = qmri_mex('health'): qmri_get_health of the gateway's context as a struct
        qmri_health h;
        check(qmri_get_health(ctx(), &h));
        const char* names[] = {"denoiser_scheme", "denoiser_fallbacks", "resident_armed", "resident_timeouts", "lsqr_one_launch", "lsqr_timeouts",
                               "repeated_calls", "last_call_wall_ms", "last_call_stage_ms", "set_denoiser_ms"};
        plhs[0] = mxCreateStructMatrix(1, 1, 10, names);
        const double v[8] = {(double)h.denoiser_scheme, (double)h.denoiser_fallbacks, (double)h.resident_armed, (double)h.resident_timeouts,
                             (double)h.lsqr_one_launch, (double)h.lsqr_timeouts, (double)h.repeated_calls, h.last_call_wall_ms};
        for (int i = 0; i < 8; ++i) mxSetFieldByNumber(plhs[0], 0, i, mxCreateDoubleScalar(v[i]));
        mxArray* st = mxCreateDoubleMatrix(1, 4, mxREAL);           // x-update, denoiser, elementwise, diagnostics
        for (int i = 0; i < 4; ++i) mxGetDoubles(st)[i] = h.last_call_stage_ms[i];
        mxSetFieldByNumber(plhs[0], 0, 8, st);
        mxArray* sd = mxCreateDoubleMatrix(1, 3, mxREAL);           // pack + upload, tensors, calibration probe
        for (int i = 0; i < 3; ++i) mxGetDoubles(sd)[i] = h.set_denoiser_ms[i];
        mxSetFieldByNumber(plhs[0], 0, 9, sd);
    } else if (c == "release") {
        cleanup();
        if (mexIsLocked()) mexUnlock();
    } else {
        mexErrMsgIdAndTxt("qmri:usage", "unknown command '%s'", cmd);
    }
}
