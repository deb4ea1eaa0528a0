/*
 * qmri.h -- C ABI of libqmri.so: the MI355X (gfx950) PnP-ADMM MR-Fingerprinting reconstruction engine.
 *
 * This is the drop-in boundary for the hot path of ketanfatania/QMRI-PnP-Recon-POC.  The reference has no
 * FFI of its own (pure MATLAB); its plugin surface for this path is a set of MATLAB values, and every entry
 * point below states which of them it replaces (file:line relative to the reference root):
 *
 *   struct F with F.forward / F.adjoint          main_recon_tsmis_FFT.m:228-229   -> qmri_set_operator, qmri_forward, qmri_adjoint
 *   P = setup_subsampling_spiralgrided(N,M,S,V)   setup_subsampling_spiralgrided.m:1-43 -> qmri_build_spiral
 *   P = setup_subsampling_epi(N,M,pct,V)          setup_subsampling_epi.m:1-36     -> qmri_build_epi
 *   param.net = @(x) denoiseImage_PnP_ADMM(...)   main_recon_tsmis_FFT.m:164, denoiseImage_PnP_ADMM.m:1-117 -> qmri_set_denoiser, qmri_denoise
 *   Net = importONNXNetwork(denoiser_path, ...)   main_recon_tsmis_FFT.m:138 (weights only)      -> qmri_onnx_read_unetres
 *   x = PnP_ADMM(y, param)                        PnP_ADMM.m:1                      -> qmri_pnp_admm
 *     with complex TSMIs (cat(3, real, imag) denoiser, no reference counterpart) -> denoiser_type | QMRI_DENOISER_COMPLEX
 *   out = mrf_dtm_cpu(dict, data, par)            mrf_dtm_cpu.m:1                   -> qmri_set_dictionary, qmri_dict_match
 *   x = FISTA_deep(data, param) (LRTV option)     FISTA_deep.m:1, main_recon_tsmis_FFT.m:273-282 -> qmri_lrtv, qmri_prox_tv, qmri_norm_tv
 *
 * Conventions (frozen):
 *   - every function returns 0 on success or a negative qmri_status; the message is qmri_last_error(ctx).
 *     Nothing throws across the boundary.
 *   - arrays are column-major; complex numbers are interleaved (re,im) doubles -- MATLAB R2018a+
 *     mxComplexDouble layout.  A MATLAB array X(h,w,c) is the C array [c][w][h].
 *   - k-space indices crossing the ABI are 0-based column-major k = row + N*col; the measurement vector is
 *     ordered frame-major, ascending k inside a frame (the row order of P in setup_subsampling_*.m:34-37).
 *   - dm (dictionary index) is 1-based, as mrf_dtm_cpu.m:92 returns it.
 *   - host-pointer entry points copy in/out around the call; *_dev entry points take device pointers that are
 *     already resident in HBM (used by the benchmark and by callers that chain stages on the GPU).
 *   - a context is owned by one host thread at a time (MATLAB calls from one thread); it is not locked.
 *   - the library fails loudly (QMRI_ERR_HIP) when no gfx950 device is usable; there is no CPU fallback.
 */
#ifndef QMRI_H
#define QMRI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMRI_ABI_VERSION 1

typedef enum {
    QMRI_OK = 0,
    QMRI_ERR_INVALID_ARG = -1,   /* bad pointer / size / enum (MATLAB: validateattributes errors) */
    QMRI_ERR_STATE = -2,         /* operator / denoiser / dictionary not set yet */
    QMRI_ERR_HIP = -3,           /* HIP runtime error, or no usable GPU */
    QMRI_ERR_UNSUPPORTED = -4,   /* size or architecture outside what the kernels implement */
    QMRI_ERR_NOMEM = -5
} qmri_status;

typedef struct qmri_ctx qmri_ctx;

/* ---- context -------------------------------------------------------------------------------------- */
int qmri_abi_version(void);
/* One context = one device, one HIP stream, all device buffers and workspaces. */
int qmri_create(int device, qmri_ctx** out);
int qmri_destroy(qmri_ctx* ctx);
/* Message of the last failing call on this context (ctx == NULL: last failing qmri_create on this thread). */
const char* qmri_last_error(const qmri_ctx* ctx);
/* Launch on the caller's hipStream_t instead of the context's own stream (NULL restores it). */
int qmri_set_stream(qmri_ctx* ctx, void* hip_stream);
int qmri_synchronize(qmri_ctx* ctx);

/* ---- forward-operator plugin: struct F, main_recon_tsmis_FFT.m:228-229 ------------------------------ */
/* Mask builders (host, integer): replace setup_subsampling_spiralgrided.m:7-34 / setup_subsampling_epi.m:20-33.
 * frame_ptr has T+1 entries, kidx holds up to cap entries; *m_out receives the total sample count.
 * Returns QMRI_ERR_INVALID_ARG with *m_out set if cap is too small.  ctx may be NULL. */
int qmri_build_spiral(qmri_ctx* ctx, int N, int S, int T, int32_t* frame_ptr, int32_t* kidx, int cap, int* m_out);
int qmri_build_epi(qmri_ctx* ctx, int N, int M, double percentage, int T, int32_t* frame_ptr, int32_t* kidx,
                   int cap, int* m_out);
/* Defines P (setup_subsampling_*.m:36-42): V is T x s column-major real (main_recon_tsmis_FFT.m:129).
 * Grid: N, M in {32, 64, 96, 112, 128, 160, 192, 224, 256}, chosen independently (N: first, contiguous index; M: second); any other
 * side returns QMRI_ERR_UNSUPPORTED.  The spiral builder makes square masks only (setup_subsampling_spiralgrided.m:28-31).
 * max_batch = number of slices the context can hold at once (>= 1). */
int qmri_set_operator(qmri_ctx* ctx, int N, int M, int s, int T, const double* V, const int32_t* frame_ptr,
                      const int32_t* kidx, int max_batch);
int qmri_operator_m(const qmri_ctx* ctx, int* m_out);
/* y = F.forward(x): x is N*M*s (complex if x_is_complex else real doubles), y is m complex. */
int qmri_forward(qmri_ctx* ctx, const void* x, int x_is_complex, void* y);
/* x = F.adjoint(y): y m complex -> x N*M*s complex. */
int qmri_adjoint(qmri_ctx* ctx, const void* y, void* x);
/* The same two maps for MATLAB `single` arrays (interleaved complex floats at the boundary; x real if !x_is_complex).  The arithmetic
 * stays complex double as in the reference's F (fft2 of a single array would be single in MATLAB: these entry points are at least as
 * accurate); results are rounded to single once, on the way out. */
int qmri_forward_f32(qmri_ctx* ctx, const float* x, int x_is_complex, float* y);
int qmri_adjoint_f32(qmri_ctx* ctx, const float* y, float* x);
/* device-resident variants, `batch` slices stored back to back */
int qmri_forward_dev(qmri_ctx* ctx, const void* d_x, void* d_y, int batch);
int qmri_adjoint_dev(qmri_ctx* ctx, const void* d_y, void* d_x, int batch);
/* Multi-coil extension of F (BASELINE.json configs[4]: "complex-valued multi-coil forward op").  The reference simulates ONE coil (README.md:63): no
 * interface there to replace, parity unpinned.  maps: N x M x ncoil complex doubles (coil sensitivities C_j; ncoil = 0 clears them; set after
 * qmri_set_operator).  y = A_mc x: m x ncoil complex, y(:, j) = F.forward(C_j .* x);  x = A_mc^H y = sum_j conj(C_j) .* F.adjoint(y(:, j)). */
int qmri_set_coils(qmri_ctx* ctx, int ncoil, const void* maps);
int qmri_forward_mc(qmri_ctx* ctx, const void* x, int x_is_complex, void* y);
int qmri_adjoint_mc(qmri_ctx* ctx, const void* y, void* x);
/* ... and the reconstruction on top of it (round 6; the same label: an extension, no reference counterpart, parity unpinned).  The x-update of
 * PnP_ADMM.m:102,153-171 with A replaced by A_mc -- x = lsqr(@afun, [y_mc; sqrt(r) z], tol, maxit, [], [], x0), afun: [A_mc; sqrt(r) I] -- as an
 * image-domain LSQR (coil maps act in image space, so the k-space iteration of the single-coil path does not apply), recurrences and stop rules as the
 * single-coil restatement of MATLAB's lsqr; and the PnP-ADMM loop of PnP_ADMM.m:76-146 around it (x0 NULL: x = A_mc^H y as :84; returns x as :148).
 * y_mc: m x ncoil complex doubles; z, x0, x_out: N x M x s complex doubles; lsqr_iters_out (nullable): prm->iters entries.  One slice, LSQR solver only. */
int qmri_xupdate_mc(qmri_ctx* ctx, const void* y_mc, const void* z, double r, double tol, int maxit, const void* x0, void* x_out,
                    int32_t* iters_out, int32_t* flag_out);
/* The x-update alone: x = lsqr(@afun,[y; sqrt(r) z], tol, maxit, [], [], x)  (PnP_ADMM.m:102,153-171), or the
 * closed-form minimiser when solver == QMRI_SOLVER_DIRECT.  Host buffers; x is in/out (warm start). */
int qmri_xupdate(qmri_ctx* ctx, const void* y, const void* z, double r, double tol, int maxit, int solver,
                 void* x, int32_t* iters_out, int32_t* flag_out);

/* ---- non-Cartesian trajectories (NUFFT operator) ------------------------------ */
/* The exact spiral of setup_subsampling_spiralgrided.m:7-27 BEFORE it is rounded onto the grid: all S points of every frame, m = S * T, frame-major.
 * Point j of frame f: omega = (pi r_j cos(theta_j + f delta), pi r_j sin(theta_j + f delta)) in radians per pixel, (omega1, omega2) interleaved.
 * frame_ptr: T+1 entries; omega: cap pairs (2 * cap doubles).  Capacity rules and ctx == NULL as qmri_build_spiral. */
int qmri_build_spiral_traj(qmri_ctx* ctx, int N, int S, int T, int32_t* frame_ptr, double* omega, int cap, int* m_out);
/* A trajectory operator.  Sample i (frame t(i) by frame_ptr, frame-major as the ABI's y) lies at omega_i = (omega1, omega2) radians per pixel,
 * omega1 along N (first index), omega2 along M; every omega finite and in [-pi, pi]:
 *   y_i = (1 / sqrt(N M)) sum_{n1 < N, n2 < M} (sum_c V(t(i), c) x_c[n1, n2]) exp(-i (omega1 n1 + omega2 n2))
 * and the adjoint is its exact Hermitian transpose.  On-grid points (omega = 2 pi k / N wrapped into [-pi, pi)) give qmri_forward of the mask of
 * those k.  Computed by a 2x oversampled NUFFT with an "exponential of semicircle" kernel of width w (relative error about 10^(1-w); DESIGN.md
 * section 14).  Replaces the context's operator (qmri_set_operator makes it gridded again).  N, M, s, T, max_batch as qmri_set_operator.  The
 * arguments are checked before the context is used (ctx == NULL: QMRI_ERR_INVALID_ARG, the message of the first failing check in qmri_last_error(NULL)). */
typedef struct {
    int32_t width;           /* kernel width w in oversampled grid points, 2..16; 0 = default (12: error about 3e-11) */
    int32_t reserved[7];     /* must be zero */
} qmri_nufft_params;
int qmri_set_operator_nufft(qmri_ctx* ctx, int N, int M, int s, int T, const double* V, const int32_t* frame_ptr, const double* omega,
                            int max_batch, const qmri_nufft_params* p);
/* The normal operator A^H A of a trajectory operator as a block-Toeplitz convolution: out = A^H A x without a gather, by a
 * zero-padded 2N x 2M FFT against the transform of the s x s point-spread function.  qmri_nufft_prepare_normal builds that transform (once per
 * trajectory, s (s + 1) / 2 * 4 N M complex doubles on the device, with the kernel width of the operator's qmri_nufft_params); it is idempotent, the
 * first call that needs the transform builds it too, and replacing the operator drops it.  qmri_normal: host buffers, x as qmri_forward takes it,
 * out N*M*s complex.  qmri_normal_dev: device buffers [batch][N*M*s], batch <= max_batch, out may be x; a slice's result is the same bits alone and at
 * any position of any batch.  Agrees with qmri_adjoint(qmri_forward(x)) to about twice the NUFFT's own error.  On a gridded operator all three return
 * QMRI_ERR_UNSUPPORTED (there qmri_adjoint(qmri_forward(x)) is the route). */
int qmri_nufft_prepare_normal(qmri_ctx* ctx);
int qmri_normal(qmri_ctx* ctx, const void* x, int x_is_complex, void* out);
int qmri_normal_dev(qmri_ctx* ctx, const void* d_x, void* d_out, int batch);
/* Density compensation for a trajectory operator (an EXTENSION, no reference counterpart, parity unpinned).  The bare adjoint
 * of a trajectory that oversamples the centre of k-space (every spiral) is a blurred, mis-scaled image; x = A^H (w .* y) with density weights w is the
 * gridding reconstruction.  qmri_nufft_dcf computes w by the iteration of Pipe & Menon (MRM 1999) on the operator's own interpolation kernel psi
 * (width and shape of qmri_nufft_params) and oversampled coordinates u_i, all m samples of all frames as one set on the periodic 2N x 2M grid:
 *   w_i = 1;  repeat:  g[k] = sum_j w_j psi(u_j1 - k1) psi(u_j2 - k2);  d_i = sum_k g[k] psi(u_i1 - k1) psi(u_i2 - k2);  w_i <- w_i / d_i
 * for p->niter iterations (1..200; 0 = 20), stopped after the first iteration whose dev = max_i |d_i - 1| is <= p->tol (tol = 0: never), and then
 * scaled once, w <- kappa w, kappa = (T / 4) I_1^2 I_2^2, I_a = sum_k psi(k) over the window of a sample at zero offset: with orthonormal V and equal
 * weight per frame A^H W A then has unit transfer where the trajectory has support.  All sums run in a fixed order without floating-point atomics:
 * the weights are the same bits on every call.  A sample with d_i <= 0 or non-finite (impossible for finite input) gets w_i = 0 and is counted in
 * info->clamped.  The weights are ATTACHED to the operator and, when w_out != NULL, copied out (m doubles, ABI order).  p == NULL: the defaults;
 * info nullable (iters: iterations run, dev: that of the last one, split_tiles: tiles of the plan whose samples went through partial tiles and
 * the reduction).  qmri_set_sample_weights attaches the caller's own weights (m finite doubles
 * >= 0; NULL clears).  Replacing the operator drops the weights.
 * Only the three qmri_adjoint_w* calls read the weights -- x = A^H (w .* y), the product formed where the spreading kernel stages y, no pass over y;
 * the same bits as qmri_adjoint* of the caller's own w .* y.  qmri_adjoint*, every solver and every other _mc call ignore them, bit for bit.
 * Refusals, all decided on the host before the device is selected: ctx == NULL, a NULL array, niter outside 0..200, tol negative or non-finite,
 * reserved != 0, batch outside 1..max_batch, a weight that is negative or non-finite: QMRI_ERR_INVALID_ARG; no operator, a qmri_adjoint_w* call
 * without attached weights, qmri_adjoint_w_mc without coil maps: QMRI_ERR_STATE; a gridded operator: QMRI_ERR_UNSUPPORTED. */
typedef struct { int32_t niter; double tol; int32_t reserved[6]; } qmri_dcf_params;      /* zeros = defaults */
typedef struct { int32_t iters; double dev; int32_t clamped; int32_t split_tiles; int32_t reserved[4]; } qmri_dcf_info;
int qmri_nufft_dcf(qmri_ctx* ctx, const qmri_dcf_params* p, double* w_out, qmri_dcf_info* info);
int qmri_set_sample_weights(qmri_ctx* ctx, const double* w);
int qmri_adjoint_w(qmri_ctx* ctx, const void* y, void* x);                 /* x = A^H (w .* y) */
int qmri_adjoint_w_dev(qmri_ctx* ctx, const void* d_y, void* d_x, int batch);
int qmri_adjoint_w_mc(qmri_ctx* ctx, const void* y_mc, void* x);           /* sum_j conj(C_j) A^H (w .* y_j) */
/* Off-resonance correction for a trajectory operator by time segmentation (an EXTENSION, no reference counterpart, parity unpinned; DESIGN.md
 * section 22).  A pixel f Hz off resonance accumulates the phase 2 pi f tau over a readout; with a field map attached the operator is
 *   y_i = (1 / sqrt(N M)) sum_n (sum_c V(t(i), c) x_c[n]) exp(-i omega_i . n) exp(-i 2 pi f[n] tau_i)
 * f_hz: N*M doubles in the layout of one channel plane of x (n1 + N n2), t_s: the m readout times tau_i in seconds in the order of y.  It is
 * computed as L NUFFTs (Sutton, Noll & Fessler, IEEE TMI 2003):  exp(-i 2 pi f tau) ~ sum_{l<L} b_l(tau) exp(-i 2 pi f tau^_l)  with
 *   - the centre frequency f0 = (f_min + f_max) / 2 taken out exactly (every sample carries exp(-i 2 pi f0 tau_i), the segmentation sees f - f0);
 *   - segment times tau^_l = t_min + l (t_max - t_min) / (L - 1) (L = 1: t_min);
 *   - per sample the least-squares coefficients over the nbins-bin histogram (p_h, f_h) of f - f0 (equal bins on [f_min - f0, f_max - f0], f_h the
 *     bin centres, p_h the fraction of pixels):  (G^H P G + eps I) b = G^H P e(tau_i),  G_hl = exp(-i 2 pi f_h tau^_l),  eps = 1e-12 tr(G^H P G) / L.
 *     The L x L matrix is factored once on the host; the m right-hand sides and substitutions run on the device in a fixed order (same bits on
 *     every call);
 *   - a constant map (f_max == f_min) is L = 1 and exact whatever nseg asks for (b = 1, fit 0).
 * nseg = 0 (auto) tries L = 2, 3, ... 16 and keeps the first whose fit_max <= tol, else keeps 16 with info->tol_reached = 0.  info (nullable):
 * fit_max / fit_rms are the maximum and the p-weighted rms over occupied bins x samples of |exp(-i 2 pi f_h tau_i) - sum_l b_l G_hl|, computed on
 * the device.  The adjoint is the exact Hermitian transpose of what the forward computes (conj(b_l) on the samples, the conjugate phase maps on the
 * images), so adjointness holds to rounding.  The map BELONGS TO THE OPERATOR: every call that runs the operator -- qmri_forward* / _adjoint*, the
 * _mc calls, the image-domain LSQR of qmri_xupdate* and both PnP-ADMM loops, qmri_adjoint_w* (A_f^H (w .* y)) -- uses it, for every batch entry
 * (every coil, every slice of a stack: ONE map per operator, per-slice maps are not built); replacing the operator drops it; f_hz == NULL clears it
 * (t_s and p are then not read) and restores the bits of the operator without a map.  qmri_nufft_dcf is unaffected (the trajectory alone).
 * Costs: about L times the plain transform per call; tables of L (N M + m) complex doubles on the device.
 * Refusals, decided on the host before the device is selected: ctx == NULL, t_s == NULL with a map, a non-finite f or t, nseg outside 0..16, nbins
 * outside {0, 16..1024}, tol negative or non-finite, reserved != 0, nseg = 1 with a non-constant map: QMRI_ERR_INVALID_ARG; no operator:
 * QMRI_ERR_STATE; a gridded operator: QMRI_ERR_UNSUPPORTED.  While a map is attached qmri_nufft_prepare_normal, qmri_normal(_dev) and
 * QMRI_SOLVER_TOEPLITZ return QMRI_ERR_UNSUPPORTED unless qmri_nufft_prepare_normal_fm (below) has built the field-aware transform for that map:
 * use QMRI_SOLVER_LSQR, or that call. */
typedef struct { int32_t nseg;    /* 1..16; 0 = auto */
                 int32_t nbins;   /* histogram bins, 16..1024; 0 = 256 */
                 double  tol;     /* auto: smallest L whose fit_max <= tol; 0 = 1e-4 */
                 int32_t reserved[4]; } qmri_offres_params;          /* zeros = defaults */
typedef struct { int32_t nseg; int32_t tol_reached;
                 double fit_max, fit_rms, f_min, f_max, t_min, t_max;
                 int32_t reserved[4]; } qmri_offres_info;
int qmri_set_field_map(qmri_ctx* ctx, const double* f_hz, const double* t_s, const qmri_offres_params* p, qmri_offres_info* info);
/* The Toeplitz normal operator of a trajectory operator WITH a field map (an EXTENSION).  Segmenting the DIFFERENCE phase
 * (Fessler, Lee, Olafsson, Shi & Noll, IEEE Trans. Signal Process. 2005) needs L' terms, not L^2:
 *   (A_f^H A_f)_{c,c'}[n, n'] = (1/NM) sum_i V(t_i,c) V(t_i,c') exp(i omega_i . (n - n')) exp(i 2 pi (f[n] - f[n']) tau_i)
 *   exp(i 2 pi g tau) ~ sum_{l<L'} c_l(tau) exp(i 2 pi g tau^_l),  g = f[n] - f[n'] in [-(f_max - f_min), f_max - f_min],   so that
 *   A_f^H A_f ~ sum_{l<L'} P_l^H T_l P_l,   P_l = diag(exp(-i 2 pi (f - f0) tau^_l)),
 * T_l the block-Toeplitz operator of qmri_nufft_prepare_normal built with the sample weights c_l(tau_i).  f0, f_min, f_max, t_min, t_max, nbins and
 * the histogram (p_h, f_h) are those of the attached map (kept on the host at attach time).  The difference histogram is p~_j = sum_h p_h p_{h-j}
 * over 2 nbins - 1 bins at g_j = j (f_max - f_min) / nbins; tau^_l = t_min + l (t_max - t_min) / (L' - 1); c(tau_i) solves the REAL system
 *   (R + eps I) c = rho(tau_i),  R_ll' = sum_j p~_j cos 2 pi g_j (tau^_l - tau^_l'),  rho_l(tau) = sum_j p~_j cos 2 pi g_j (tau - tau^_l),  eps = 1e-12 tr(R) / L'
 * (p~ is symmetric in g, so the coefficients are real and every T_l is Hermitian).  The system is solved as the least-squares
 * problem it is the normal equations of: B = [sqrt(p~_j) cos 2 pi g_j tau^_l; sqrt(p~_j) sin 2 pi g_j tau^_l; sqrt(eps) I] = Q U is factored on the host
 * in fp64 (U is the Cholesky factor of R + eps I, transposed, but formed at B's condition, which is the square root of R's), and c = U^-1 Q^T b(tau_i);
 * Q^T b, the back substitution and the fit run on the device in a fixed order.  fit_max is the maximum of |exp(i 2 pi g_j tau_i) - sum_l c_l exp(i 2 pi g_j
 * tau^_l)| over occupied difference bins x samples, fit_rms its p~-weighted rms.  nseg = 0 (auto) tries L' = 2 .. 32 by the fit alone and builds the
 * transform once, for the first L' whose fit_max <= tol, else for 32 with tol_reached = 0.  Expect L' ~ 2 L - 1 for the accuracy of an L-segment
 * operator: the range of g is twice that of f.  A constant map is the plain normal operator: nseg = 1, fit_max = 0 whatever nseg asks for, the plain
 * transform built or reused.  The transform is [L'][s (s + 1) / 2][4 N M] complex doubles on the device (khat_bytes), plus L' N M phase-map entries
 * and a max_batch image buffer; an allocation failure returns QMRI_ERR_NOMEM and leaves the context as it was before the call.
 * OPT-IN: without this call for the map in force qmri_nufft_prepare_normal, qmri_normal(_dev) and QMRI_SOLVER_TOEPLITZ refuse as described above.
 * After it they run the field-aware normal operator (the one-slice qmri_xupdate, both PnP-ADMM loops, every coil chunk); qmri_nufft_prepare_normal
 * returns QMRI_OK and builds nothing; a slice's bits are the same alone, at any batch position and at any max_batch, and out may be x.
 * qmri_set_field_map (a new map or NULL) and replacing the operator drop the transform; calling again with other parameters rebuilds it.  The plain
 * transform of qmri_nufft_prepare_normal is a separate buffer that is never touched: built before the map, it serves again, with the same bits, once
 * the map is cleared, and it is never used with a (non-constant) map.
 * Refusals, decided on the host before the device is selected: ctx == NULL, nseg outside {0, 2..32}, tol negative or non-finite, reserved != 0:
 * QMRI_ERR_INVALID_ARG; no operator, or a trajectory operator without a map (attach one with qmri_set_field_map; without a map the plain
 * qmri_nufft_prepare_normal is the call): QMRI_ERR_STATE; a gridded operator: QMRI_ERR_UNSUPPORTED.  p == NULL: the defaults; info nullable. */
typedef struct { int32_t nseg;   /* 2..32; 0 = auto */
                 double  tol;    /* auto: smallest L' whose fit_max <= tol; 0 = 1e-4 */
                 int32_t reserved[4]; } qmri_offres_normal_params;     /* zeros / NULL = defaults */
typedef struct { int32_t nseg; int32_t tol_reached;
                 double fit_max, fit_rms;
                 uint64_t khat_bytes;
                 int32_t reserved[4]; } qmri_offres_normal_info;
int qmri_nufft_prepare_normal_fm(qmri_ctx* ctx, const qmri_offres_normal_params* p, qmri_offres_normal_info* info);
/* On a trajectory operator these work unchanged: qmri_forward / _adjoint (and _f32, _dev), qmri_operator_m, qmri_set_coils, qmri_forward_mc /
 * _adjoint_mc, qmri_xupdate_mc(_batch), qmri_pnp_admm_mc(_batch, _dev), qmri_coil_compress*, and qmri_xupdate / qmri_pnp_admm (one slice, LSQR,
 * no diagnostics) as the image-domain LSQR with one unit coil -- bit for bit the qmri_*_mc call with that coil.  Everything else that needs the
 * operator (the DIRECT solver, the per-iteration diagnostics, qmri_pnp_admm_dev with several slices, qmri_pnp_admm_batch with several slices per
 * launch, qmri_lrtv) returns QMRI_ERR_UNSUPPORTED. */

/* ---- denoiser plugin: param.net, main_recon_tsmis_FFT.m:138-171 ----------------------------------- */
enum { QMRI_ARCH_UNETRES = 0, QMRI_ARCH_SEQ_CONV = 1 };
typedef struct {
    int32_t arch;            /* QMRI_ARCH_UNETRES: network_unet.py:68-117;  QMRI_ARCH_SEQ_CONV: conv3x3(+ReLU) stack */
    int32_t in_nc;           /* 10 single_level, 11 multi_level (main_test.py:245-252) */
    int32_t out_nc;          /* 10 */
    int32_t nc[4];           /* {64,128,256,512}; SEQ_CONV uses nc[0] as width */
    int32_t nb;              /* ResBlocks per stage (4); SEQ_CONV: number of conv layers */
    int32_t residual_noise;  /* denoiseImage_PnP_ADMM.m:99-104: 1 = return input - CNN(input) */
} qmri_net_desc;
/* weights: flat fp32 in state_dict() order, Conv2d OIHW / ConvTranspose2d IOHW (what export_to_onnx,
 * PyTorch_Denoiser/utils.py:444-485, serialises).  nbytes must equal 4 * qmri_net_nparams(desc). */
size_t qmri_net_nparams(const qmri_net_desc* desc);
int qmri_set_denoiser(qmri_ctx* ctx, const qmri_net_desc* desc, const float* weights, size_t nbytes,
                      int H, int W, int max_batch);
/* Weight ingestion from the ONNX file the reference loads with `Net = importONNXNetwork(denoiser_path, ...)`
 * (main_recon_tsmis_FFT.m:79-83,138), i.e. what export_to_onnx (PyTorch_Denoiser/utils.py:468-481: opset 9, weights as
 * graph initializers) writes.  Reads the Conv / ConvTranspose weights in graph order, checks that they form a UNetRes,
 * fills desc_out (arch, in_nc, out_nc, nc, nb; residual_noise = 0) and *nfloats_out, and -- when weights != NULL --
 * copies the blob qmri_set_denoiser takes (capacity_floats >= *nfloats_out).  Call once with weights == NULL to size
 * the buffer.  Host-only (no GPU, no ONNX / protobuf library); errors via qmri_last_error(NULL). */
int qmri_onnx_read_unetres(const char* path, qmri_net_desc* desc_out, float* weights, size_t capacity_floats,
                           size_t* nfloats_out);
/* out = denoiseImage_PnP_ADMM(in, net, true, residual_noise): in H x W x C x B doubles -> out H x W x out_nc x B. */
int qmri_denoise(qmri_ctx* ctx, const double* in, int H, int W, int C, int B, double* out);
/* raw network forward on device fp32 tensors [B][C][W][H] (no casts); the dominant kernel chain.  Precondition of the default
 * (f16-split) arithmetic: inputs at ordinary scale, as the [0, 1] images of PnP_ADMM.m:121 are; the call synchronises, reads the
 * range guard and -- like qmri_denoise / qmri_pnp_admm -- repeats itself on the bf16 scheme if an activation left the f16 range.
 * The repeated pass reads d_in again: d_in and d_out must not overlap (QMRI_ERR_INVALID_ARG otherwise). */
int qmri_net_forward_dev(qmri_ctx* ctx, const float* d_in, int B, float* d_out);
/* Which arithmetic the convolutions run on: *scheme_out = 2 (f16 pieces, 3 MFMA products per fp32 product) or 3 (bf16 pieces, 6
 * products: no range limits, twice the matrix time); *fallbacks_out = how often a run-time guard has moved the network from 2
 * to 3 since qmri_set_denoiser (a call that trips the guard is repeated transparently: a 2x slower call is visible here).
 * Either pointer may be NULL. */
int qmri_denoiser_scheme(const qmri_ctx* ctx, int* scheme_out, int* fallbacks_out);

/* ---- PnP-ADMM: x = PnP_ADMM(y, param), PnP_ADMM.m:1 ----------------------------------------------- */
enum { QMRI_SOLVER_LSQR = 0, QMRI_SOLVER_DIRECT = 1, QMRI_SOLVER_TOEPLITZ = 2 };
/* QMRI_SOLVER_TOEPLITZ: an EXTENSION for trajectory operators (qmri_set_operator_nufft), parity unpinned.  The x-update is solved by plain conjugate
 * gradients on the normal equations (A^H A + r I) x = A^H y + r z (with coils: A_mc), A^H A applied as qmri_normal applies it, warm-started from x.
 * Stop rule: the first k with || b - (A^H A + r I) x_k ||_2 <= cg_tol * || b ||_2, b the right-hand side and the residual that of the CG recurrence:
 * flag 0 and k iterations reported; flag 1 when cg_maxit is reached first (cg_maxit = 0 returns x0); flag 3 on a breakdown (p^H (A^H A + r I) p not
 * positive: non-finite data).  The reference's lsqr stops on a different quantity, so the iterates of the two solvers at tol = 1e-4 differ at the 1e-4
 * level; both converge to the same minimiser.  Accepted by qmri_xupdate, qmri_pnp_admm (one slice), qmri_pnp_admm_mc(_batch, _dev) and
 * qmri_recon_batch_mc* on a trajectory operator; on a gridded operator QMRI_ERR_UNSUPPORTED (use QMRI_SOLVER_LSQR there).  LSQR stays the default. */
/* denoiser_type is a set of bits: 0 single_level, 1 multi_level, 2 complex single_level, 3 complex multi_level; any other value is
 * QMRI_ERR_INVALID_ARG.  QMRI_DENOISER_COMPLEX (complex TSMIs; the reference's TSMIs are real, PnP_ADMM.m:115-118) changes Step 2 only:
 *   v = x + uold ; V = cat(3, real(v), imag(v))        N x M x 2s, planes 0..s-1 real, s..2s-1 imaginary
 *   [V, lo, hi, range] = norm_zero_to_one(V)          one min / max over all 2s*N*M values of the slice
 *   multi_level: V = cat(3, V, noise_map)             noise plane at channel 2s
 *   V = net(V) ; V = V*range + lo ; v = complex(V(:,:,1:s), V(:,:,s+1:2s)) ; uold = uold + x - v ; z = v - uold
 * The denoiser then has in_nc == 2s (+1) and out_nc == 2s (the 2s-channel layout of qmri_synthesize_tsmi_complex); any other network, and a
 * 2s-channel network in real mode, is QMRI_ERR_STATE with a message naming the channel counts (other misfits in real mode: QMRI_ERR_INVALID_ARG).
 * Every PnP-ADMM entry point takes the mode through this field (single- and multi-coil, slice batches, qmri_recon_batch(_mc)). */
enum { QMRI_DENOISER_SINGLE_LEVEL = 0, QMRI_DENOISER_MULTI_LEVEL = 1, QMRI_DENOISER_COMPLEX = 2 };
typedef struct {
    double gamma;            /* param.gamma = sigma_squared/eta = 0.05   main_recon_tsmis_FFT.m:285-287 */
    int32_t iters;           /* param.iter = 100                          :288 */
    double cg_tol;           /* param.cg_tol = 1e-4                       :289 */
    int32_t cg_maxit;        /* 100 (literal in PnP_ADMM.m:102) */
    int32_t solver;          /* QMRI_SOLVER_LSQR reproduces the reference; DIRECT is the exact minimiser; TOEPLITZ: trajectories (above) */
    int32_t denoiser_type;   /* param.denoiser_type                       :167  (| QMRI_DENOISER_COMPLEX: complex TSMIs, see above) */
    double noise_std;        /* build_noise_map(0.01,...)                 :76,:170 */
    int32_t want_diag;       /* the two per-iteration diagnostics of PnP_ADMM.m:106-109 */
} qmri_admm_params;
/* y: m complex.  x0: N*M*s complex or NULL (=> F.adjoint(y), main_recon_tsmis_FFT.m:292).  gt: N*M*s complex or
 * NULL (param.gt_tsmi, only for the second diagnostic).  x_out: N*M*s complex (the LAST lsqr solution, as the
 * reference returns).  diag_out: iters*2 doubles or NULL.  lsqr_iters_out: iters int32 or NULL. */
int qmri_pnp_admm(qmri_ctx* ctx, const void* y, const qmri_admm_params* p, const void* x0, const void* gt,
                  void* x_out, double* diag_out, int32_t* lsqr_iters_out);
/* nslices independent slices, device-resident y / x0 / gt / x_out (slice-major); diag/lsqr outputs are host. */
int qmri_pnp_admm_dev(qmri_ctx* ctx, int nslices, const void* d_y, const qmri_admm_params* p, const void* d_x0,
                      const void* d_gt, void* d_x_out, double* diag_out, int32_t* lsqr_iters_out);

/* A slice stack from HOST buffers through one context: y nslices x m, x0 / gt nslices x N*M*s or NULL, x_out nslices x N*M*s (slice-major =
 * the columns of a MATLAB m x S matrix / the 4th dimension of an N x M x s x S array), advanced slices_per_launch at a time
 * (<= max_batch of qmri_set_operator and qmri_set_denoiser).  diag_out: nslices x iters x 2 or NULL; lsqr_iters_out: nslices x iters or NULL.
 * What `PnP_ADMM_hip(Y, param)` calls for a measurement matrix; qmri_recon_batch is the pipelined multi-GPU form. */
int qmri_pnp_admm_batch(qmri_ctx* ctx, int nslices, int slices_per_launch, const void* y, const qmri_admm_params* p, const void* x0,
                        const void* gt, void* x_out, double* diag_out, int32_t* lsqr_iters_out);
/* Multi-coil extension of the loop (see qmri_xupdate_mc above: no reference counterpart, parity unpinned). */
int qmri_pnp_admm_mc(qmri_ctx* ctx, const void* y_mc, const qmri_admm_params* prm, const void* x0, void* x_out, int32_t* lsqr_iters_out);
/* Slice stacks of the multi-coil extension, each slice with its own maps (no reference counterpart, parity unpinned).  Slice-major layouts:
 * maps nslices x ncoil x N*M, y_mc nslices x ncoil x m, z / x0 / x_out nslices x N*M*s (complex doubles).  The LSQR keeps every scalar on the device
 * and its reductions in one fixed order per slice: a slice's result does not depend on the batch it is solved in or on max_batch.  These calls
 * neither read nor change the maps of qmri_set_coils.  iters_out / flags_out: nslices entries (nullable); lsqr_iters_out: nslices x prm->iters. */
int qmri_xupdate_mc_batch(qmri_ctx* ctx, int nslices, int ncoil, const void* maps, const void* y_mc, const void* z, double r, double tol, int maxit,
                          const void* x0, void* x_out, int32_t* iters_out, int32_t* flags_out);
int qmri_pnp_admm_mc_batch(qmri_ctx* ctx, int nslices, int slices_per_launch, int ncoil, const void* maps, const void* y_mc,
                           const qmri_admm_params* prm, const void* x0, void* x_out, int32_t* lsqr_iters_out);
/* the same with device arrays, nslices <= max_batch of the operator and the denoiser; d_x_out must not alias d_x0 */
int qmri_pnp_admm_mc_dev(qmri_ctx* ctx, int nslices, int ncoil, const void* d_maps, const void* d_y, const qmri_admm_params* prm,
                         const void* d_x0, void* d_x_out, int32_t* lsqr_iters_out);

/* ---- LRTV option: x = FISTA_deep(data, param), main_recon_tsmis_FFT.m:273-282 -------------------------- */
/* FISTA with backtracking on 0.5 |y - F.forward(x)|^2 + K |x|_TV (FISTA_deep.m:31-104); the TV prox is unlocbox's
 * prox_tv (prox_tv.m:99-203) on the stacked image [real(x); imag(x)] of 2N rows x M*s columns (FISTA_deep.m:66,75). */
typedef struct {
    double  K;           /* param.K = 4e-5 (:275); 0 skips the prox (FISTA_deep.m:74) */
    int32_t iters;       /* param.iter = 200 (:276) */
    double  step;        /* param.step; <= 0: numel(X0)/numel(Y) (:277) */
    double  tol;         /* param.tol = 1e-4: stop when |obj - obj_prev| / obj < tol (FISTA_deep.m:103) */
    int32_t backtrack;   /* param.backtrack = 1 (:279) */
    double  prox_tol;    /* prox_tv param.tol; <= 0: 10e-4 (prox_tv.m:99) */
    int32_t prox_maxit;  /* prox_tv param.maxit; <= 0: 200 (prox_tv.m:101) */
} qmri_lrtv_params;
typedef struct {
    int32_t iters;             /* FISTA iterations performed */
    int32_t halvings;          /* 'reducing stepsize...' events */
    double  step;              /* final step size */
    double  obj;               /* last objective 0.5 |y - Fx|^2 + K |x|_TV */
    int32_t prox_calls;
    int32_t prox_iters_total;  /* inner iterations over all prox_tv calls */
} qmri_lrtv_info;
/* y: m complex doubles (ABI order); x_out: N x M x s complex doubles; info may be NULL.  Needs qmri_set_operator. */
int qmri_lrtv(qmri_ctx* ctx, const void* y, const qmri_lrtv_params* p, void* x_out, qmri_lrtv_info* info);
/* [sol, info] = prox_tv(b, gamma, param) on a real column-major R x C image (prox_tv.m:1); host buffers.
 * iters_out / obj_out (info.iter, the last objective) may be NULL. */
int qmri_prox_tv(qmri_ctx* ctx, const double* b, int R, int C, double gamma, double tol, int maxit, double* sol,
                 int32_t* iters_out, double* obj_out);
/* y = norm_tv(I) (unlocbox/utils/norm_tv.m:45-55), same layout. */
int qmri_norm_tv(qmri_ctx* ctx, const double* I, int R, int C, double* out);

/* ---- dictionary match: out = mrf_dtm_cpu(dict, data, par), mrf_dtm_cpu.m:1 --------------------------- */
/* D: K x s column-major unit-norm atoms, normD: K, lut: K x Q column-major (dict.D / .normD / .lut, :8-12).  s <= 1024: the compressed
 * atoms of the shipped script (s = 10; s <= 16 keeps a pixel tile in registers) or uncompressed fingerprints (s = T; mrf_dtm_cpu.m:41-50 takes T
 * from size(data.X)), matched by a channel-blocked GEMM. */
int qmri_set_dictionary(qmri_ctx* ctx, int K, int s, int Q, const float* D, const float* normD, const float* lut);
/* X: Npix x s complex double column-major (data.X reshaped, :50).  qmap: Npix x Q (NaN->0, :136-141);
 * pd: Npix complex single interleaved (:144-148); mt: Npix or NULL (:150-154); dm: Npix 1-based or NULL (:156-160).
 * The outputs are those of the single-precision products ip = D x^H (:91) and max(abs(ip)) with the first index winning (:92), bit for bit;
 * which 32-atom tiles need those products is decided by a filter on f16 pieces with a proven margin (qmri_debug_dict_filter switches it
 * off; dictionaries with non-finite entries are matched without it). */
int qmri_dict_match(qmri_ctx* ctx, const void* X, int Npix, float* qmap, float* pd, float* mt, int32_t* dm);
int qmri_dict_match_dev(qmri_ctx* ctx, const void* d_X, int Npix, float* d_qmap, float* d_pd, float* d_mt,
                        int32_t* d_dm);
/* The same with out.Xfit (par.f.Xout, mrf_dtm_cpu.m:95,129-134): xfit (nullable) = Npix x s complex single interleaved, column-major,
 * Xfit(p,:) = ip(dm(p)) .* D(dm(p),:) -- the matched atom scaled by the unnormalised inner product, before the division by normD (:96). */
int qmri_dict_match_xfit(qmri_ctx* ctx, const void* X, int Npix, float* qmap, float* pd, float* mt, int32_t* dm, float* xfit);
int qmri_dict_match_xfit_dev(qmri_ctx* ctx, const void* d_X, int Npix, float* d_qmap, float* d_pd, float* d_mt,
                             int32_t* d_dm, float* d_xfit);

/* ---- groups of a dictionary and the grouped match (extension, no reference counterpart, parity unpinned) ---------- */
/* A dictionary simulated over a transmit-field axis (qmri_dict_simulate: atoms carry T1, T2 and b1) is matched per pixel against the atoms of
 * that pixel's MEASURED B1 only (B1-corrected MRF: Buonincontri & Sawiak 2016; Ma et al. 2017) -- 1/G of the products of a match over all atoms,
 * and no attempt to estimate B1 from the fingerprint.  The reference's mrf_dtm_cpu.m has one flat list of atoms.
 *
 * Groups.  The dictionary of qmri_set_dictionary (narrow form, s <= 16) is given G groups: group g holds atoms group_ptr[g] .. group_ptr[g+1]-1
 * (0-based) and has the selector value group_val[g] (e.g. its b1).  1 <= G <= 256, group_ptr[0] == 0, group_ptr[G] == K, group_ptr strictly
 * increasing (no empty group), group_val finite and strictly ascending; anything else, NULL arrays included: QMRI_ERR_INVALID_ARG.  G = 0 clears
 * the groups (the arrays are not read).  No dictionary set: QMRI_ERR_STATE.  A wide dictionary (s > 16, the channel-blocked match):
 * QMRI_ERR_UNSUPPORTED -- groups for wide dictionaries are not implemented.  qmri_set_dictionary drops the groups.  Setting groups changes nothing
 * about qmri_dict_match*: those still match all K atoms, with the same bits.  A call that fails, for whatever reason, leaves the groups as they
 * were.  (Costs a second device copy of the packed dictionary in which every
 * group starts on a 32-atom tile.) */
int qmri_set_dictionary_groups(qmri_ctx* ctx, int G, const int32_t* group_ptr, const double* group_val);
/* Assignment.  For a selector value b, g(b) is the LOWEST g that minimises fabs(b - group_val[g]), evaluated in fp64: values outside the range of
 * group_val go to the end groups, an exact midpoint goes to the lower group, and a non-finite b (NaN, +-Inf) means UNMATCHED.  This is that rule
 * on the host, without a context: grp_out[i] = g(sel[i]) + 1, or 0 for unmatched, i < n.  The grouped match gives the same integers.
 * 1 <= G <= 256, group_val finite and strictly ascending, n >= 0, no NULL array (sel / grp_out may be NULL when n == 0): else QMRI_ERR_INVALID_ARG. */
int qmri_dict_group_assign(int G, const double* group_val, int n, const double* sel, int32_t* grp_out);
/* Grouped match.  X, qmap, pd, mt, dm and xfit exactly as in qmri_dict_match_xfit (every output nullable); sel: Npix doubles, the selector map;
 * grp (nullable): the 1-based group of each pixel, 0 for unmatched.  Needs qmri_set_dictionary and qmri_set_dictionary_groups (else QMRI_ERR_STATE).
 * For a pixel p with g = g(sel[p]) the outputs are, BIT FOR BIT, what qmri_dict_match_xfit returns for that pixel on a dictionary holding only rows
 * group_ptr[g] .. group_ptr[g+1]-1 of D / normD / lut, with dm shifted by group_ptr[g] (so dm indexes the whole dictionary, 1-based): the
 * single-precision products and magnitudes of mrf_dtm_cpu.m:91-96, ties going to the first index OF THE GROUP, NaN in lut -> 0 (:136-160).
 * An unmatched pixel gets dm = 0, grp = 0, mt = 0, pd = 0, every qmap column 0 and xfit 0, and costs no atom work: a NaN outside the body in the B1
 * map is the foreground mask.  A pixel's result depends neither on the other pixels of the call, nor on their order, nor on the filter switch
 * (qmri_debug_dict_filter). */
int qmri_dict_match_grouped(qmri_ctx* ctx, const void* X, int Npix, const double* sel, float* qmap, float* pd, float* mt, int32_t* dm, int32_t* grp,
                            float* xfit);
/* The same on device arrays, asynchronous on ctx's stream. */
int qmri_dict_match_grouped_dev(qmri_ctx* ctx, const void* d_X, int Npix, const double* d_sel, float* d_qmap, float* d_pd, float* d_mt, int32_t* d_dm,
                                int32_t* d_grp, float* d_xfit);

/* ---- the B1 map estimated from the fingerprints by a windowed group match (extension, no reference counterpart, parity unpinned;
 *      DESIGN.md section 28) --------------------------------------------------------------------------------------------------------------------
 * The grouped match above needs a measured B1 map.  Without one, B1 can be taken from the fingerprints if it is held constant over a window: for
 * unit-norm atoms min_rho ||x - rho d_k||^2 = ||x||^2 - |<d_k, x>|^2, so under white noise the maximum-likelihood group of a window maximises the
 * summed explained energy sum_{p in window} max_{k in g} |<d_k, x_p>|^2, with T1, T2 and PD free per pixel.  Two stages and one composed call.
 *
 * Stage 1, group scores.  score: G x Npix float32, the pixel contiguous (score[g * Npix + p]).  score[g][p] is, BIT FOR BIT, the mt that
 * qmri_dict_match_grouped returns for pixel p when sel[p] = group_val[g]: max over the atoms of group g of sqrtf(fmaf(im, im, re * re)) of the
 * single-precision fmaf chain over c = 0 .. s-1, whatever that gives for zero and non-finite pixels (-1 for a pixel whose magnitudes are all NaN).
 * X as in qmri_dict_match.  Refusals: Npix < 1, NULL X or score: QMRI_ERR_INVALID_ARG (also with ctx == NULL); no dictionary or no groups:
 * QMRI_ERR_STATE; a wide dictionary (s > 16): QMRI_ERR_UNSUPPORTED. */
int qmri_dict_group_scores(qmri_ctx* ctx, const void* X, int Npix, float* score);
/* The same on device arrays, asynchronous on ctx's stream. */
int qmri_dict_group_scores_dev(qmri_ctx* ctx, const void* d_X, int Npix, float* d_score);
/* Stage 2, pooled argmax; needs no dictionary.  Pixel p = i + N j inside a slice (i < N contiguous, j < M), nslices slices stacked;
 * score: G x (nslices N M) float32 as above; mask (nullable): one uint8 per pixel, non-zero = foreground; half_window h, 0 <= h <= 32.
 * Everything in fp64.  E[g][p] = (double)S (double)S where p is foreground and S = score[g][p] is finite and > 0, else 0.
 *   T[g][i, j] = sum over d = -h .. h, ascending, of E[g][i + d, j];   P[g][i, j] = sum over d ascending of T[g][i, j + d];
 * terms outside the slice are skipped (a window never crosses a slice), the additions are plain and left to right (direct sums, no running sum).
 * g^ = the LOWEST g with the largest P.  grp[p] = g^ + 1, b1[p] = group_val[g^], conf[p] = (P_best - P_second) / P_best with P_second the largest P
 * among the other groups (conf = 1 for G = 1).  A background pixel, or one whose P_best is not > 0: grp 0, b1 NaN, conf 0 -- NaN is what the grouped
 * match treats as unmatched.  A slice's bits do not depend on the stack.  b1, grp, conf: nslices N M entries each, every one nullable.
 * group_val: G doubles ON THE HOST in both variants.  QMRI_ERR_INVALID_ARG (also with ctx == NULL): G outside 1 .. 256, group_val NULL, non-finite
 * or not strictly ascending, h outside 0 .. 32, N, M or nslices < 1, score NULL. */
int qmri_b1_pool(qmri_ctx* ctx, int G, const double* group_val, int N, int M, int nslices, const float* score, const uint8_t* mask, int half_window,
                 double* b1, int32_t* grp, double* conf);
/* The same on device arrays (group_val on the host), asynchronous on ctx's stream. */
int qmri_b1_pool_dev(qmri_ctx* ctx, int G, const double* group_val, int N, int M, int nslices, const float* d_score, const uint8_t* d_mask,
                     int half_window, double* d_b1, int32_t* d_grp, double* d_conf);
/* Composed call: stage 1, then stage 2 with the dictionary's own groups, a run of slices at a time so that the scratch (G N M 12 bytes per slice)
 * stays under 256 MB (one slice at least).  X: (nslices N M) x s complex doubles, column-major, as in qmri_dict_match.  The outputs are those of
 * qmri_dict_group_scores followed by qmri_b1_pool, bit for bit.  params NULL: half_window 4.  Refusals: those of the two stages; a non-zero
 * reserved entry, N M nslices beyond 2^31 - 1: QMRI_ERR_INVALID_ARG.  Not built: interpolation between groups, weights other than a 0/1 mask,
 * wide dictionaries, the qmri_recon_batch* workers, estimating B1 inside the ADMM loop. */
typedef struct {
    int32_t half_window;     /* h: the window is (2h + 1) x (2h + 1) pixels, 0 <= h <= 32 */
    int32_t reserved[7];     /* must be zero */
} qmri_b1est_params;
typedef struct {
    int32_t n_estimated;     /* pixels with grp > 0 */
    int32_t n_unmatched;     /* the others: background, or no positive pooled energy */
    double mean_conf;        /* mean conf over the estimated pixels, summed in pixel order (0 when there is none) */
    int32_t reserved[4];
} qmri_b1est_info;
int qmri_b1_estimate(qmri_ctx* ctx, const void* X, int N, int M, int nslices, const uint8_t* mask, const qmri_b1est_params* params, double* b1,
                     int32_t* grp, double* conf, qmri_b1est_info* info);
/* The same on device arrays, asynchronous on ctx's stream; info (nullable) is zeroed: it is filled by the host variant only. */
int qmri_b1_estimate_dev(qmri_ctx* ctx, const void* d_X, int N, int M, int nslices, const uint8_t* d_mask, const qmri_b1est_params* params,
                         double* d_b1, int32_t* d_grp, double* d_conf, qmri_b1est_info* info);

/* ---- tissue-fraction maps: each pixel as a non-negative mix of chosen atoms (an EXTENSION, no reference counterpart, parity unpinned;
 *      DESIGN.md section 27) --------------------------------------------------------------------------------------------------------------------
 * The match above gives every pixel ONE atom.  A pixel that holds two or three tissues (a boundary, a thick slice) gets a (T1, T2) that belongs to
 * none of them; partial-volume MRF (Deshmane et al., 2019) writes the pixel's compressed fingerprint as a non-negative combination of a few chosen
 * atoms -- white matter, grey matter, CSF -- and reports the weights as tissue-fraction maps.
 * Components.  The caller names C atoms, 1 <= C <= 8, of the narrow dictionary (s <= 16) set by qmri_set_dictionary, 1-based like dm.  Component c is
 *   the UNNORMALISED atom a_c = normD[k_c] * D[k_c, :], s real values widened to fp64, so a weight is in the units of PD.  A = [a_1 .. a_C] (s x C),
 *   G = A^T A in fp64 with the channels summed in ascending order.
 * Per pixel, x (complex, s channels) = one row of the Npix x s complex-double column-major array qmri_dict_match takes:
 *   1. the real vector b and the phase phi.  QMRI_PV_REAL: b = Re x, phi = 0 (the project's real-TSMI domain).  QMRI_PV_PHASE: q = sum_j x_j^2 (no
 *      conjugate), phi0 = atan2(Im q, Re q) / 2 (0 when q = 0), b0 = Re(x e^{-i phi0}); if sum_j b0_j (sum_c a_c)_j < 0 then phi = phi0 + pi and
 *      b = -b0 (e^{-i phi} is the negated e^{-i phi0}, so b = -b0 exactly), else phi = phi0, b = b0.
 *   2. w = argmin_{w >= 0} ||b - A w||_2 by Lawson & Hanson's active-set method on the normal equations, h = A^T b (channels ascending):
 *      start with w = 0 and an empty passive set P.
 *      Outer step: g = h - G w; stop when no i outside P has g_i > tau_i; otherwise the lowest index attaining the largest such g_i moves into P.
 *        tau_i = 2^-48 ||a_i|| ||b|| (||a_i|| = sqrt(G_ii)): the size of g_i's own rounding error.  With tau = 0 a pixel that IS a mix of the
 *        components (every dual exactly 0) would move indices in and out on rounding noise until the cap.
 *      Inner step: solve G_PP z_P = h_P by Cholesky in ascending index order (z = 0 outside P).  If every z_i, i in P, is > 0: w = z, back to the
 *        outer step.  Otherwise alpha = min over {i in P, z_i <= 0} of w_i / (w_i - z_i) (0 when w_i = 0), w = w + alpha (z - w); every index that
 *        attains alpha, and any with w_i <= 0, is set to exactly 0 and leaves P; repeat the inner step.
 *      At most 3 C inner solves per pixel: a pixel that would need more keeps its current w and gets flag bit 0 (QMRI_PV_FLAG_CAP).
 *   A pixel with a non-finite x gets all outputs 0 and flag bit 1 (QMRI_PV_FLAG_NONFINITE), like the match's NaN -> 0 rule.
 * Outputs, column-major, all nullable except w:  w Npix x C fp64;  frac Npix x C = w / sum_c w_c (0 where the sum is 0);  pd Npix complex doubles =
 *   (sum_c w_c) e^{i phi};  res Npix = ||x e^{-i phi} - A w||_2 / ||x||_2, imaginary part included, from A and not from G (0 for x = 0);  flags Npix
 *   int32.  A pixel's result depends on no other pixel of the call, nor on Npix or the pixels' order, bit for bit.
 * Not built: components per B1 group, wide dictionaries, more than 8 components, sparse selection of the components from the whole dictionary,
 *   unmixing inside the batch workers. */
enum { QMRI_PV_REAL = 0, QMRI_PV_PHASE = 1 };
enum { QMRI_PV_FLAG_CAP = 1, QMRI_PV_FLAG_NONFINITE = 2 };
typedef struct {
    double min_pivot;        /* smallest pivot of the Cholesky factorisation of G scaled to a unit diagonal, in (0, 1]: 1 = orthogonal components */
    int32_t C, s;            /* components and channels in force */
    int32_t reserved[4];
} qmri_pv_info;
/* Forms A and G on the host from the dictionary's host copy and uploads them.  atoms: C indices, 1-based; info nullable; C = 0 clears (atoms may be
 * NULL).  qmri_set_dictionary drops the components.  A failed call leaves earlier components in place.  Refusals: C outside 0..8, a NULL array, an
 * index outside 1..K, a repeated index, a zero or non-finite atom, C > s, collinear components (a scaled pivot <= 1e-10): QMRI_ERR_INVALID_ARG (the
 * first two also with ctx == NULL); no dictionary: QMRI_ERR_STATE; a wide dictionary (s > 16): QMRI_ERR_UNSUPPORTED. */
int qmri_set_components(qmri_ctx* ctx, int C, const int32_t* atoms, qmri_pv_info* info);
/* The unmixing on host arrays; returns after the kernel has finished.  mode: QMRI_PV_REAL or QMRI_PV_PHASE.  Refusals, decided before the device is
 * touched: Npix < 1, NULL X, NULL w, mode outside {0, 1}: QMRI_ERR_INVALID_ARG (also with ctx == NULL); no components set: QMRI_ERR_STATE. */
int qmri_dict_unmix(qmri_ctx* ctx, const void* X, int Npix, int mode, double* w, double* frac, double* pd, double* res, int32_t* flags);
/* The same on device arrays, asynchronous on ctx's stream.  d_X as for qmri_dict_match_dev. */
int qmri_dict_unmix_dev(qmri_ctx* ctx, const void* d_X, int Npix, int mode, double* d_w, double* d_frac, double* d_pd, double* d_res, int32_t* d_flags);

/* ---- sub-grid refinement: matched T1 / T2 moved off the dictionary's grid by a fit through neighbouring atoms (an EXTENSION,
 *      no reference counterpart, parity unpinned) -------------------------------------------------------------------------
 * Every match above returns lut[dm]: maps quantised to the dictionary's grid.  The dictionary samples the signal manifold; a quadratic through the
 * matched atom and its neighbours along each parameter axis is a local model of it, and fitting the pixel to that model is a least-squares problem
 * in 1 to 3 unknowns per pixel in the compressed space.  It needs no sequence knowledge and works for any gridded narrow dictionary (s <= 16).
 * tests/refine_ref.py states the fit in numpy, operation for operation, and is the definition; this is its summary.
 * Lines.  P in 1..3 lut columns cols[q] (0-based, distinct, < Q) are refined.  Atoms a, b are on one line of column c when every OTHER lut column
 *   compares equal.  nbr [K][P][2] int32, 0-based, -1 = none: nbr[k][q][1] is the atom on k's line with the smallest lut[., c] greater than lut[k, c]
 *   (the lowest index among equal values), nbr[k][q][0] mirrors it (the largest value smaller than lut[k, c]).  An atom with a non-finite lut entry,
 *   or a zero or non-finite normD, has no neighbours and is nobody's neighbour.  With lut = (T1, T2, b1) and cols = {0, 1} a line never leaves a b1
 *   group.  qmri_dict_lines is that rule on the host, without a context or a device: lut K x Q floats column-major and normD as
 *   qmri_set_dictionary takes them; info [P][3] int32 = atoms with 0, 1 and 2 neighbours per column.  QMRI_ERR_INVALID_ARG: a NULL array, K < 1,
 *   Q < 1, P outside 1..3, a column repeated or out of range, a column in which no atom has a neighbour ("lut column c has no lines").
 * Model, all in fp64.  a_k = double(normD[k]) * double(D[k, :]), the unnormalised atom.  Per pixel, centre atom k, per column q with neighbours a+, a-:
 *   both: g_q = (a+ - a-) / 2, h_q = (a+ + a-) / 2 - a0, box [-1, 1];  only a+: g_q = a+ - a0, h_q = 0, box [0, 1];  only a-: g_q = a0 - a-, h_q = 0,
 *   box [-1, 0];  none: t_q fixed at 0.  d(t) = a0 + sum_q (t_q g_q + t_q^2 h_q); the parameter theta_q(t_q) is the same polynomial through the lut
 *   values, so non-uniform (logarithmic) grids need no special case.
 * Fit.  f(t) = ||x - rho d(t)||^2 with rho = (d . x) / (d . d), evaluated as this residual norm.  Variable-projection Gauss-Newton from t = 0:
 *   J_q = g_q + 2 t_q h_q, H = |rho|^2 (J^T J - (J^T d)(d^T J) / (d . d)) + 1e-12 trace(H) I, gvec = Re(conj(rho) (P_perp J)^T r), r = x - rho d;
 *   Cholesky; the step clipped to the box; a coordinate is pinned for a step when it has no neighbour, when J_q is collinear with d
 *   (|P_perp J_q|^2 <= 1e-12 |J_q|^2) or when it sits on a bound and gvec_q points outside.  Converged when the clipped step is <= 1e-10 in every
 *   coordinate.  Otherwise backtracking alpha = 1, 1/2 .. 2^-10, the first alpha with f_new <= f taken; none: the fit ends, with the STALLED flag
 *   when the refused step was larger than 1e-6 (a smaller one is the resolution of f in fp64, not a failure).  More than 30 steps: the CAP flag.
 * Re-centring.  After a fit, the first column q (ascending) with t_q = +-1 whose neighbour in that direction has a further neighbour in that
 *   direction: that neighbour becomes the centre and the fit restarts from t = 0; at most 4 moves; the last centre's result is returned.
 * X: Npix x s complex doubles, column-major, as in qmri_dict_match.  dm: Npix int32, the 1-based start atom from ANY match (plain or grouped); a
 *   value outside 1..K (0 = unmatched) skips the pixel: every output 0, flag SKIPPED.  Outputs, column-major, every one nullable: qmap Npix x Q fp64
 *   (refined columns theta_q(t), the others the last centre's lut value, NaN -> 0 as in the match);  pd Npix complex doubles = rho (the match's
 *   convention: x ~ pd * unnormalised atom);  res Npix = sqrt(f / ||x||^2);  t Npix x P;  centre Npix int32, 1-based;  flags Npix int32.
 *   DEGENERATE: ||x||^2 or d(0) . d(0) zero or not finite; the pixel gets the centre's grid values, t = 0, pd = 0, res = 0.
 *   A pixel's bits depend on nothing but that pixel: not on Npix, the other pixels or their order.
 * Not built: wide dictionaries (s > 16), cross terms t_q t_r in the model, refinement inside the qmri_recon_batch* workers (qmri_problem is frozen),
 *   a sub-grid B1 inside qmri_b1_estimate, uncertainty maps from H^-1. */
enum { QMRI_RF_FLAG_SKIPPED = 1, QMRI_RF_FLAG_MOVED = 2, QMRI_RF_FLAG_BOUND = 4, QMRI_RF_FLAG_CAP = 8, QMRI_RF_FLAG_STALLED = 16, QMRI_RF_FLAG_DEGENERATE = 32 };
typedef struct {
    int32_t P, K, s;         /* refined columns, atoms and channels in force */
    int32_t reserved;
    int32_t count[3][3];     /* per refined column: atoms with 0, 1 and 2 neighbours */
    int32_t reserved2[3];
} qmri_refine_info;
int qmri_dict_lines(int K, int Q, const float* lut, const float* normD, int P, const int32_t* cols, int32_t* nbr_out, int32_t* info);
/* Builds the lines from the host copy of the dictionary set by qmri_set_dictionary and uploads nbr and the fp64 table of unnormalised atoms
 * [K][16] (one 128-byte row per atom).  info nullable; P = 0 clears (cols may be NULL).  qmri_set_dictionary drops the state.  A failed call leaves
 * the earlier state working.  Everything is decided on the host before the device is touched.  Refusals: P outside 0..3, NULL cols, a column repeated or
 * out of range, a column without lines: QMRI_ERR_INVALID_ARG (the first two also with ctx == NULL); no dictionary: QMRI_ERR_STATE; a wide
 * dictionary (s > 16): QMRI_ERR_UNSUPPORTED.  Setting the state changes nothing about any match. */
int qmri_set_refine(qmri_ctx* ctx, int P, const int32_t* cols, qmri_refine_info* info);
/* The fit on host arrays; returns after the kernel has finished.  Refusals, decided before the device is touched: Npix < 1, NULL X or dm:
 * QMRI_ERR_INVALID_ARG (also with ctx == NULL); no refinement set: QMRI_ERR_STATE. */
int qmri_dict_refine(qmri_ctx* ctx, const void* X, int Npix, const int32_t* dm, double* qmap, double* pd, double* res, double* t, int32_t* centre,
                     int32_t* flags);
/* The same on device arrays, asynchronous on ctx's stream.  d_X as for qmri_dict_match_dev. */
int qmri_dict_refine_dev(qmri_ctx* ctx, const void* d_X, int Npix, const int32_t* d_dm, double* d_qmap, double* d_pd, double* d_res, double* d_t,
                         int32_t* d_centre, int32_t* d_flags);

/* ---- TSMI synthesis from quantitative maps: main_synthesize_tsmis.m:54,82-100 (mode 'real') ------------ */
/* I = knnsearch(KDTreeSearcher(dict.lut), qm(:,1:2)); X = real(dict.D(I,:)) .* dict.normD(I) .* abs(qm(:,3)); X .* sign(X(:,:,1)).
 * qmap: Npix x 3 doubles column-major (T1, T2, PD, in the units of dict.lut); X_out: Npix x s singles column-major;
 * idx_out (nullable): the 1-based nearest entry.  Uses the dictionary of qmri_set_dictionary (Q >= 2). */
int qmri_synthesize_tsmi(qmri_ctx* ctx, const double* qmap, int Npix, float* X_out, int32_t* idx_out);
/* mode 'complex' of the same script (main_synthesize_tsmis.m:27,100-103): X = real(dict.D(I,:)) .* dict.normD(I) .* qm(:,3) with a complex
 * PD, no abs and no sign alignment, stored as cat(3, real(X), imag(X)).  qmap: Npix x 3 (T1, T2, real(PD)); pd_imag: Npix or NULL
 * (imaginary part of PD); X_out: Npix x 2s singles column-major (the s real channels, then the s imaginary ones). */
int qmri_synthesize_tsmi_complex(qmri_ctx* ctx, const double* qmap, const double* pd_imag, int Npix, float* X_out, int32_t* idx_out);

/* ---- slice batches over several GPUs of one node (slices are independent; no collective) ------------ */
typedef struct {
    int32_t N, M, s, T;
    const double* V;                 /* T x s */
    const int32_t* frame_ptr;        /* T+1 */
    const int32_t* kidx;             /* m */
    const qmri_net_desc* net;
    const float* weights;
    size_t weights_nbytes;
    int32_t K, Q;                    /* dictionary (K == 0: skip the match) */
    const float* D;
    const float* normD;
    const float* lut;
    qmri_admm_params admm;
    int32_t slices_per_launch;       /* slices batched through the denoiser on one GPU (>= 1) */
} qmri_problem;
/* Y: nslices x m complex (host).  X_out: nslices x N*M*s complex.  qmap_out: nslices x Npix x Q or NULL,
 * pd_out: nslices x Npix complex single or NULL.  One host thread + one context per device in devs[]. */
int qmri_recon_batch(int ndev, const int* devs, int nslices, const qmri_problem* prob, const void* Y,
                     void* X_out, float* qmap_out, float* pd_out, char* errbuf, size_t errbuf_len);
/* Multi-coil extension of qmri_recon_batch (no reference counterpart, parity unpinned): maps nslices x ncoil x N*M, Y_mc nslices x ncoil x m
 * complex doubles, each slice with its own maps; the same workers, pipelining and shared-device rules, each launch one qmri_pnp_admm_mc_dev call
 * (LSQR solver only).  X_out / qmap_out / pd_out as qmri_recon_batch. */
int qmri_recon_batch_mc(int ndev, const int* devs, int nslices, const qmri_problem* prob, int ncoil, const void* maps, const void* Y_mc,
                        void* X_out, float* qmap_out, float* pd_out, char* errbuf, size_t errbuf_len);

/* ---- coil compression (multi-coil extension, no reference counterpart, parity unpinned) -------------------------- */
/* One linear map on the coil index turns ncoil coils into nv virtual coils, applied alike to the data and to the maps (Buehrer et al. 2007,
 * Huang et al. 2008), optionally after pre-whitening with a noise covariance Psi = L L^H (Cholesky, lower triangle of Psi read):
 *   K = sum_i L^-1 y_i (L^-1 y_i)^H over the m samples of a slice (or of the stack: shared),  K = U diag(lambda) U^H, lambda descending, every
 *   column of U scaled so that its entry of largest magnitude (lowest index on ties) is real and positive;  W = L^-H U(:, 1:nv)  (U(:, 1:nv)
 *   without Psi);  y' = W^H y,  maps' = W^H maps.  nv: p->nv, or (nv == 0) the smallest nv with sum_{l<nv} lambda_l >= energy sum lambda,
 *   the largest over the slices of a stack.  ncoil <= 128 (QMRI_ERR_UNSUPPORTED above).  Layouts as the _mc_batch calls: y_mc nslices x ncoil x m,
 *   maps nslices x ncoil x N*M (m, N, M of qmri_set_operator); Psi ncoil x ncoil column-major. */
typedef struct {
    int32_t nv;          /* > 0: keep nv virtual coils; 0: choose by energy */
    double  energy;      /* (0, 1], used when nv == 0 */
    int32_t shared;      /* 0: one W per slice; 1: one W for the stack */
} qmri_cc_params;
/* Outputs are written compactly with the chosen nv: y_out nslices x nv x m, maps_out nslices x nv x N*M, W_out nmat x ncoil x nv (column-major per
 * matrix), eig_out nmat x ncoil (nmat = 1 when shared, else nslices).  A caller who lets energy choose sizes them for nv = ncoil.  maps_out is
 * nullable iff maps is; W_out and eig_out are nullable. */
int qmri_coil_compress(qmri_ctx* ctx, int nslices, int ncoil, const void* y_mc, const void* maps, const void* noise_cov, const qmri_cc_params* p,
                       int* nv_out, void* y_out, void* maps_out, void* W_out, double* eig_out);
/* The same on device arrays of ctx's device (y_mc, maps, noise_cov, y_out, maps_out, W_out); eig_out stays a host array (the eigensolve runs on
 * the host).  Returns after its kernels have finished. */
int qmri_coil_compress_dev(qmri_ctx* ctx, int nslices, int ncoil, const void* d_y_mc, const void* d_maps, const void* d_noise_cov, const qmri_cc_params* p,
                           int* nv_out, void* d_y_out, void* d_maps_out, void* d_W_out, double* eig_out);
/* Host only, no context: the eigensolver of the coil compression (cyclic Jacobi) on the Hermitian n x n matrix whose upper triangle `herm` holds
 * (column-major complex doubles), 1 <= n <= 128.  evals: n, descending; evecs: n x n column-major, phase rule as above. */
int qmri_coil_eig(int n, const void* herm, double* evals, void* evecs);
/* qmri_recon_batch_mc with every launch's slices compressed on the device (qmri_coil_compress_dev) before qmri_pnp_admm_mc_dev: cc->nv > 0 coils per
 * slice, one W per slice (energy and shared are refused: a stack is split over workers and launches).  noise_cov: host ncoil x ncoil or NULL. */
int qmri_recon_batch_mc_cc(int ndev, const int* devs, int nslices, const qmri_problem* prob, int ncoil, const void* maps, const void* Y_mc,
                           void* X_out, float* qmap_out, float* pd_out, char* errbuf, size_t errbuf_len, const void* noise_cov, const qmri_cc_params* cc);

/* ---- coil sensitivity maps from calibration data (multi-coil extension, no reference counterpart, parity unpinned) ---- */
/* The adaptive-combine estimator of Walsh, Gmitro & Marcellin (MRM 2000) on the device, the step between qmri_coil_compress and a qmri_*_mc call.
 * Needs qmri_set_operator (gridded or trajectory): the inverse transform runs on the operator's dense FFT passes max_batch coil images at a time, so
 * N and M must be the operator's.
 * Per slice, ncoil <= 128 coils on the N x M grid:
 *   kind QMRI_CSM_IMAGES: calib is nslices x ncoil x N*M complex doubles in the layout of `maps`: the calibration images I_j, used as given.
 *   kind QMRI_CSM_KSPACE: calib is nslices x ncoil x cM x cN (column-major cN x cM per coil, cN along N), a centred block of k-space in the
 *     operator's convention -- the centre crop of fftshift(fft2(C_j x)) / sqrt(N M), block index (cN/2, cM/2) is k = 0; cN, cM even, 8 <= cN <= N,
 *     8 <= cM <= M.  I_j = sqrt(N M) ifft2(ifftshift(P(w .* calib_j))): P zero-pads so that block index (cN/2, cM/2) lands on grid index (N/2, M/2),
 *     w(a1, a2) = h_cN(a1) h_cM(a2), h_c(a) = (1 + cos(2 pi (a - c/2) / c)) / 2 (Hann; window = 0: w = 1).  An untapered full-size block inverts fft2.
 *   1. R(r) = sum_{d in [-patch, patch]^2} I(r + d) I(r + d)^H, terms outside the grid dropped (ncoil x ncoil Hermitian, never stored)
 *   2. lambda_1(r), u(r): its largest eigenvalue and unit eigenvector (power iteration from I(r), per pixel until no entry moves by more than
 *      1e-13, at most 256 iterations)
 *   3. phase_ref QMRI_CSM_PHASE_OBJECT: C(r) = u(r) e^{i arg(u(r)^H I(r))} -- C^H I is real and non-negative, the object's phase lives in the maps
 *      (what the real-mode denoiser, real(x + u) of PnP_ADMM.m:115, needs);  QMRI_CSM_PHASE_COIL: C(r) = u(r) e^{-i arg(u_ref(r))}, ref the coil with
 *      the largest sum_r |I_j(r)|^2 (lowest index on ties) -- the object's phase stays in x (complex TSMIs).  A modulus of exactly 0: phase factor 1.
 *   4. thresh > 0: C(r) = 0 where lambda_1(r) < thresh^2 max_r lambda_1(r); |C(r)|_2 = 1 on the pixels kept (thresh = 0: everywhere).
 * A slice's outputs are the same bits alone, at any position of a stack and with any max_batch.  ESPIRiT is not built. */
enum { QMRI_CSM_KSPACE = 0, QMRI_CSM_IMAGES = 1 };
enum { QMRI_CSM_PHASE_OBJECT = 0, QMRI_CSM_PHASE_COIL = 1 };
typedef struct {
    int kind;            /* QMRI_CSM_KSPACE / QMRI_CSM_IMAGES */
    int cN, cM;          /* KSPACE: sides of the calibration block (ignored for IMAGES) */
    int patch;           /* half-width p of the (2p + 1) x (2p + 1) patch, 0..4 */
    int window;          /* KSPACE: 1 = Hann taper, 0 = none */
    int phase_ref;       /* QMRI_CSM_PHASE_OBJECT / QMRI_CSM_PHASE_COIL */
    double thresh;       /* >= 0; 0 keeps every pixel */
} qmri_csm_params;
/* kspace input of a cN x cM block, 7 x 7 patch, Hann taper, object phase, no mask */
#define QMRI_CSM_PARAMS_DEFAULT(cN_, cM_) { QMRI_CSM_KSPACE, (cN_), (cM_), 3, 1, QMRI_CSM_PHASE_OBJECT, 0.0 }
typedef struct {
    int32_t max_iters;       /* the largest iteration count any pixel of the call needed */
    int32_t not_converged;   /* pixels that reached 256 iterations without meeting the stop rule */
} qmri_csm_info;
/* Host arrays.  maps_out: nslices x ncoil x N*M (feeds qmri_set_coils / the *_mc_batch calls directly); img_out (nullable): nslices x N*M complex,
 * C^H I; lambda_out (nullable): nslices x N*M doubles, lambda_1 (unmasked); info (nullable).  Refusals are decided on the host before the device is
 * selected (ctx == NULL: the message of the first failing check in qmri_last_error(NULL)): NULL arrays or params, nslices < 1, ncoil < 1, an odd or
 * out-of-range cN / cM, patch outside 0..4, an unknown kind / phase_ref, window outside {0, 1}, a negative or non-finite thresh: QMRI_ERR_INVALID_ARG;
 * an N or M outside the supported sides of qmri_set_operator: QMRI_ERR_INVALID_ARG; ncoil > 128: QMRI_ERR_UNSUPPORTED; then no operator:
 * QMRI_ERR_STATE; N, M not the operator's: QMRI_ERR_INVALID_ARG. */
int qmri_coil_maps(qmri_ctx* ctx, int nslices, int ncoil, int N, int M, const void* calib, const qmri_csm_params* p, void* maps_out, void* img_out,
                   double* lambda_out, qmri_csm_info* info);
/* The same on device arrays of ctx's device (calib, maps_out, img_out, lambda_out; info stays a host struct); d_maps_out must not alias d_calib.
 * Returns after its kernels have finished. */
int qmri_coil_maps_dev(qmri_ctx* ctx, int nslices, int ncoil, int N, int M, const void* d_calib, const qmri_csm_params* p, void* d_maps_out,
                       void* d_img_out, double* d_lambda_out, qmri_csm_info* info);

/* ---- dictionary compression to its SVD subspace (extension, no reference counterpart, parity unpinned) ---------- */
/* The reference ships its dictionaries already compressed (SVD_dict_FISP_cut*.mat) and never computes the compression.  This call takes what a
 * Bloch / EPG simulator writes -- F, K fingerprints of T frames, real, column-major K x T (frame t contiguous over the atoms, as D of
 * qmri_set_dictionary), fp64 (f_is_f64 = 1) or fp32 (0) -- and returns what qmri_set_operator and qmri_set_dictionary take:
 *   1. G = F^T F in fp64 (fp32 input widened exactly; split over fixed chunks of atoms added in chunk order, no atomics: the same bits from call to
 *      call).  A non-finite trace is QMRI_ERR_INVALID_ARG.
 *   2. lambda_1 >= lambda_2 >= ... and orthonormal v_1 .. v_b, the dominant eigenpairs of G (block subspace iteration with Rayleigh-Ritz, block
 *      b = min(T, s_cap + 8), s_cap = p->s or p->s_max; stopped when every one of the s_cap leading residuals |G v_c - lambda_c v_c|_2 is
 *      <= tol lambda_1, or after maxit iterations).  Every vector's entry of largest magnitude (lowest index on ties) is positive.
 *   3. s = p->s (1..16), or with p->s == 0 the smallest s <= p->s_max (1..16, cut to min(T, K)) with sum_{c<s} lambda_c >= p->energy trace(G); if
 *      s_max does not reach the energy, s = s_max and info->energy_reached = 0.  p->s > min(T, K) is QMRI_ERR_INVALID_ARG.  Note that the operator
 *      (qmri_set_operator) takes s <= 10.
 *   4. Dc = F V (fp64, frames ascending), normD_k = |Dc_k|_2, D_k = Dc_k / normD_k, both rounded once to fp32; an atom of zero norm gives D_k = 0 and
 *      normD_k = 0.
 * 1 <= T <= 1024, K >= 1.  Needs neither an operator, a denoiser nor a dictionary. */
typedef struct {
    int32_t s;           /* 1..16: the rank; 0: choose by energy */
    int32_t s_max;       /* 1..16, used when s == 0 */
    double  energy;      /* (0, 1], used when s == 0 */
    double  tol;         /* residual bound relative to lambda_1, in [0, 1); 0 -> 1e-13 */
    int32_t maxit;       /* >= 0; 0 -> 200 */
} qmri_dsvd_params;
typedef struct {
    int32_t s;               /* the rank used */
    int32_t iters;           /* subspace iterations taken */
    int32_t converged;       /* 0: maxit was reached before the stop rule held */
    int32_t energy_reached;  /* 0: energy mode, and s_max vectors hold less than the energy asked for */
    double  max_resid;       /* the largest |G v_c - lambda_c v_c|_2 / lambda_1 over the s_cap leading pairs */
    double  energy_kept;     /* sum_{c<s} lambda_c / trace(G) */
} qmri_dsvd_info;
/* Host arrays.  V_out: T x s fp64 column-major; D_out: K x s fp32 column-major; normD_out: K; eig_out (nullable): the s leading lambda; info
 * (nullable).  The outputs are written compactly with the chosen s; a caller who lets energy choose sizes them for s = 16.  Refusals are decided on
 * the host before the device is selected (ctx == NULL: the message of the first failing check in qmri_last_error(NULL)): NULL arrays or params,
 * K < 1, T outside 1..1024, f_is_f64 outside {0, 1}, s / s_max / energy / tol / maxit out of range: QMRI_ERR_INVALID_ARG. */
int qmri_dict_compress(qmri_ctx* ctx, int K, int T, const void* F, int f_is_f64, const qmri_dsvd_params* p, int* s_out, double* V_out, float* D_out,
                       float* normD_out, double* eig_out, qmri_dsvd_info* info);
/* The same on device arrays of ctx's device (F, V_out, D_out, normD_out); s_out, eig_out and info stay on the host.  Same bits as the host-array
 * call.  Returns after its kernels have finished. */
int qmri_dict_compress_dev(qmri_ctx* ctx, int K, int T, const void* d_F, int f_is_f64, const qmri_dsvd_params* p, int* s_out, double* d_V_out,
                           float* d_D_out, float* d_normD_out, double* eig_out, qmri_dsvd_info* info);

/* ---- FISP dictionary simulation by extended phase graphs (extension, no reference counterpart, parity unpinned) ---- */
/* The reference ships its dictionaries already simulated and compressed and has no simulator.  This call makes the fingerprints that
 * qmri_dict_compress takes, from a flip-angle train and a list of atoms, by the extended-phase-graph recursion of the FISP-MRF sequence (Jiang et al.
 * 2015; Weigel 2015).  Per atom k, with T1_k, T2_k in seconds and a transmit scale b1_k, the state is three REAL vectors of S = nstates entries,
 * F+_n, F-_n, Z_n for n = 0 .. S-1, all zero at the start except Z_0 = 1 (the pulses rotate about y, which keeps every state real).
 *   Inversion (inversion = 1): Z_0 <- -inv_eff Z_0, then relaxation over TI: Z_0 <- Z_0 e + (1 - e), e = exp(-TI / T1).
 *   Then for each frame t = 0 .. T-1, in this order:
 *   1. RF.  a = alpha_t b1_k, c = cos a, s = sin a, c2 = (1 + c) / 2, s2 = (1 - c) / 2; for every n, all three from the old values:
 *        F+ <- c2 F+ - s2 F- + s Z,   F- <- -s2 F+ + c2 F- + s Z,   Z <- -(s / 2) (F+ + F-) + c Z.
 *   2. Relaxation over TE_t: F+- <- F+- exp(-TE_t / T2), Z <- Z exp(-TE_t / T1) for every n, then Z_0 += 1 - exp(-TE_t / T1).
 *   3. Signal: F[k, t] = F+_0.
 *   4. Relaxation over TR_t - TE_t, in the same way as step 2.
 *   5. Spoiler, one dephasing unit: F+_n <- F+_{n-1} for n >= 1 (the old F+_{S-1} is dropped), F+_0 <- old F-_1 (0 when S = 1),
 *      F-_n <- old F-_{n+1}, F-_{S-1} <- 0, F-_0 <- the new F+_0.
 * The truncation at S states is part of the result (it moves the fingerprints by 1e-3 at S = 32 when T2 reaches 0.6 s): S is the caller's to
 * choose.  No slice profile, no diffusion, no off-resonance.  All arithmetic is fp64, sin / cos / exp included; there is no reduction across atoms
 * and there are no atomics: equal inputs give equal bits.  1 <= T <= 1024 (the limit of qmri_dict_compress), K >= 1.  Needs neither an operator, a
 * denoiser nor a dictionary. */
typedef struct {
    int32_t nstates;      /* S, 1..256 */
    int32_t inversion;    /* 0 / 1 */
    double  ti;           /* s, >= 0, used when inversion */
    double  inv_eff;      /* (0, 1], used when inversion; 1 = ideal */
    int32_t out_is_f64;   /* 1: F fp64, 0: F rounded once to fp32 */
} qmri_epg_params;
/* Host arrays, all fp64: alpha[T] radians, tr[T] and te[T] seconds, t1[K], t2[K], b1[K] (nullable: 1).  F_out: K x T column-major (frame t
 * contiguous over the atoms: the layout qmri_dict_compress takes), fp64 or fp32 as p->out_is_f64 says.  Refusals are decided on the host before
 * the device is selected (ctx == NULL: the message of the first failing check in qmri_last_error(NULL)): a NULL array or params, K < 1, T outside
 * 1..1024, nstates outside 1..256, inversion / out_is_f64 outside {0, 1}, ti or inv_eff out of range when inversion, a non-finite or negative alpha,
 * TR or TE, TR_t <= 0, TE_t > TR_t, a T1 or T2 that is non-finite or <= 0, a b1 that is non-finite or negative (b1 = 0 is allowed):
 * QMRI_ERR_INVALID_ARG.  Returns after its kernels have finished.  qmri_dict_simulate_sp / qmri_dict_simulate_sp_dev below are the same simulation
 * integrated over a slice profile. */
int qmri_dict_simulate(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2,
                       const double* b1, const qmri_epg_params* p, void* F_out);
/* The same with t1, t2, b1 and F_out on ctx's device; alpha, tr, te and p stay on the host.  Same bits as the host-array call.  This route cannot
 * read its atoms on the host: for an atom whose T1 or T2 is non-finite or <= 0, or whose b1 is non-finite or negative, the kernel writes NaN in
 * every frame of that atom (and of no other).  F_out feeds qmri_dict_compress_dev as it is. */
int qmri_dict_simulate_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1, const double* d_t2,
                           const double* d_b1, const qmri_epg_params* p, void* d_F_out);

/* ---- slice-profile-aware FISP dictionary simulation (extension, no reference counterpart, parity unpinned) ---- */
/* A slice-selective pulse turns the magnetisation by a flip angle that varies through the slice; a voxel's signal is the integral over that
 * distribution (Ma et al. 2017; Buonincontri and Sawiak 2016).  The slice is cut into Q = nq sub-slices, 1 <= Q <= 64, with weights weight[Q] and
 * flip-angle scales prof: [Q], the same in every frame (per_frame = 0), or [T][Q] with q fastest (per_frame = 1).  Every entry of weight and prof
 * is finite and >= 0 and the weights sum to more than 0; they are NOT normalised here.  For atom k and sub-slice q the recursion of
 * qmri_dict_simulate runs unchanged, except that step 1 uses a = (alpha_t b1_k) prof[t, q], in that product order; with f_q[t] its step-3 signal,
 *   F[k, t] = sum_q weight[q] f_q[t],
 * the sum starting from 0 and running in ascending q, all in fp64, stored as fp64 or rounded once to fp32 as p->out_is_f64 says.  So Q = 1,
 * weight = {1}, prof = {1} gives the bits of qmri_dict_simulate; a zero weight contributes nothing; and with per_frame = 0 the result is
 * sum_q weight[q] x (qmri_dict_simulate with b1 prof[q]) up to the one-ulp difference in the product order of a.  The sum is taken on the chip: the
 * only device memory beyond the outputs is the schedule ((3 + Q) T + Q doubles); no atomics, and an atom's bits depend neither on K nor on its
 * position in the call. */
typedef struct {
    int32_t nq;             /* Q, 1..64 */
    int32_t per_frame;      /* 0: prof[Q]; 1: prof[T][Q], q fastest */
    const double* prof;     /* host array, flip-angle scales, finite and >= 0 */
    const double* weight;   /* host array [Q], finite and >= 0, sum > 0 */
} qmri_epg_profile;
/* The arguments, layout and refusals of qmri_dict_simulate, plus: a NULL profile struct, nq outside 1..64, per_frame outside {0, 1}, a NULL prof or
 * weight, a non-finite or negative entry of either, weights that do not sum to more than 0: QMRI_ERR_INVALID_ARG, decided on the host before the
 * device is selected (ctx == NULL: the message of the first failing check in qmri_last_error(NULL)).  Returns after its kernel has finished. */
int qmri_dict_simulate_sp(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2,
                          const double* b1, const qmri_epg_params* p, const qmri_epg_profile* sp, void* F_out);
/* The same with t1, t2, b1 and F_out on ctx's device; alpha, tr, te, p, sp and the arrays sp points to stay on the host.  Same bits as the
 * host-array call.  An atom this route cannot refuse (see qmri_dict_simulate_dev) gets NaN in every frame of that atom (and of no other). */
int qmri_dict_simulate_sp_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1, const double* d_t2,
                              const double* d_b1, const qmri_epg_params* p, const qmri_epg_profile* sp, void* d_F_out);

/* ---- EPG fingerprint derivatives and their Cramer-Rao bound (extension, no reference counterpart, parity unpinned) ---- */
/* The fingerprints of qmri_dict_simulate together with their derivatives with respect to theta = (T1, T2) (nparams P = 2) or (T1, T2, b1) (P = 3),
 * by forward-mode differentiation of that recursion, and the Cramer-Rao bound they give per atom -- in ONE launch, so that no K x T x (1 + P) array
 * has to exist for the bound.  Next to F+, F-, Z every parameter carries a tangent of the same shape, real and zero at the start:
 *   Inversion: with e = exp(-TI / T1) and e' = e TI / T1^2 the T1 tangent's Z_0 <- (-inv_eff) e' - e'.
 *   1. RF.  Every tangent takes the rotation of the state.  The b1 tangent adds, from the state (p, m, z) before the pulse,
 *        alpha_t (-(s / 2) (p + m) + c z) to F+ and to F-,   alpha_t (-(c / 2) (p + m) - s z) to Z.
 *   2., 4. Relaxation over D.  With E1 = exp(-D / T1), E2 = exp(-D / T2), E1' = E1 D / T1^2, E2' = E2 D / T2^2 the tangents scale by E2 / E2 / E1
 *      as the state does; the T2 tangent adds E2' (F+, F-) and the T1 tangent E1' Z of the state before its scaling, and the T1 tangent's Z_0
 *      subtracts E1'.
 *   3. Signal: dF[q][k, t] = the F+_0 of tangent q.    5. Spoiler: the lane moves of the state on every tangent.
 * F has the bits of qmri_dict_simulate.  The bound: per atom J = [F, d_1 F, ..., d_P F], T x (1 + P); with a real subspace V [T x s] (s > 0; the V
 * of qmri_dict_compress) J <- V^T J, s x (1 + P).  G = J^T J, every sum in ascending row order from 0; d = sqrt(diag G); Gn = G / (d d^T); Cholesky of
 * Gn.  An atom with a diagonal entry of G that is non-finite or <= 0, or a pivot (the number under a square root) that is not > 1e-10, is SINGULAR:
 * flag 1 and every bound +inf.  Otherwise flag 0 and crb[k][q] = [Gn^-1]_qq / d_q^2, q = 0 .. P, entry 0 the proton density's.  For a pixel
 * x = rho a_k + noise of variance sigma^2 per real and imaginary part and channel (a_k the unnormalised, compressed atom; rho the match's pd):
 *   sigma(theta_q) >= sigma sqrt(crb[k][q]) / |rho|,   sigma(Re rho) >= sigma sqrt(crb[k][0]).
 * s < 1 + P is not refused: it yields SINGULAR atoms.  All arithmetic is fp64; no atomics; an atom's bits depend neither on K nor on its position
 * in the call, and the bound's bits do not depend on which of the other outputs are asked for.  Integration over a slice profile
 * (qmri_dict_simulate_sp) is out of scope: there is no _sp form of this call. */
typedef struct {
    int32_t nparams;       /* P: 2 (T1, T2) or 3 (T1, T2, b1) */
    int32_t s;             /* 0: the bound of the uncompressed fingerprints; 1..16: of their projection on V */
    const double* V;       /* host array, T x s column-major, finite; used when s > 0 */
    int32_t reserved[4];   /* zero */
} qmri_epg_grad_params;
/* Host arrays.  The inputs of qmri_dict_simulate; F_out (nullable): K x T column-major; dF_out (nullable): P arrays of K x T, parameter q at
 * q K T; both fp64 or rounded once to fp32 as p->out_is_f64 says; crb_out (nullable): K x (1 + P) fp64, atom k at k (1 + P); flags_out: K.  At
 * least one output is given; crb_out and flags_out go together.  Refusals: those of qmri_dict_simulate (F_out's replaced by: all outputs NULL,
 * crb_out without flags_out or the reverse), and a NULL grad-params struct, nparams outside {2, 3}, s outside 0..16, s > 0 with a NULL V, a
 * non-finite entry of V: QMRI_ERR_INVALID_ARG, decided on the host before the device is selected (ctx == NULL: the message of the first failing
 * check in qmri_last_error(NULL)).  Returns after its kernel has finished. */
int qmri_dict_simulate_grad(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2,
                            const double* b1, const qmri_epg_params* p, const qmri_epg_grad_params* gp, void* F_out, void* dF_out, double* crb_out,
                            int32_t* flags_out);
/* The same with t1, t2, b1 and the four outputs on ctx's device; alpha, tr, te, p, gp and gp->V stay on the host.  Same bits as the host-array
 * call.  For an atom this route cannot refuse (see qmri_dict_simulate_dev) the kernel writes NaN in every frame of F and dF, NaN in its crb, and
 * flag 2 -- for that atom and no other. */
int qmri_dict_simulate_grad_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1,
                                const double* d_t2, const double* d_b1, const qmri_epg_params* p, const qmri_epg_grad_params* gp, void* d_F_out,
                                void* d_dF_out, double* d_crb_out, int32_t* d_flags_out);

/* ---- EPG simulation of prepared, repeated FISP trains (extension, no reference counterpart, parity unpinned) ---- */
/* qmri_dict_simulate describes one experiment: equilibrium, at most one inversion, one uninterrupted train.  3-D, interleaved multi-slice and SMS
 * MRF play the same train many times with a pause in between, so that the first recorded frame meets a driven steady state; cardiac MRF (Hamilton
 * et al. 2017) plays, heartbeat after heartbeat, an inversion, nothing, a T2 preparation, ... each followed by a wait.  This call simulates such a
 * schedule: the train is cut into B blocks, block b owning the next nframes_b entries of alpha / tr / te (the nframes sum to T), and the block list
 * is played C = ncycles times, of which only the last is recorded.  Per atom the state starts at equilibrium as in qmri_dict_simulate (every F+-_n
 * and Z_n zero except Z_0 = 1); then for cycle = 0 .. C-1 and for each block in order:
 *   a. Wait (only if wait > 0).  E1 = exp(-wait / T1), E2 = exp(-wait / T2); for every n: F+-_n <- F+-_n E2, Z_n <- Z_n E1; then Z_0 += 1 - E1.
 *      Free relaxation: no dephasing and no crusher.
 *   b. Preparation.
 *      inversion (prep = 1): e = exp(-TI / T1), TI = prep_time, eff = prep_eff.  Z_0 <- (-eff Z_0) e + (1 - e); Z_n <- (-eff Z_n) e for n >= 1;
 *        every F+-_n <- 0 (a crusher follows the pulse).
 *      T2 preparation (prep = 2): e2 = exp(-prep_time / T2).  Z_n <- (eff Z_n) e2 for every n; every F+-_n <- 0.  This is the IDEALISED tip-down /
 *        refocus / tip-up module: T1 relaxation during the module is neglected, the pulses are perfect up to the scale eff, a crusher follows.
 *      Preparations are NOT scaled by b1 (adiabatic pulses).
 *   c. Frames: nframes frames, each of them steps 1 to 5 of qmri_dict_simulate verbatim.  In the last cycle step 3 writes F[k, t].
 * All arithmetic is fp64; no atomics; an atom's bits depend neither on K nor on its position in the call.  One block {T, inversion, wait 0, ti,
 * inv_eff} (or {T, none, 0, 0, 1}) with C = 1 gives the numbers of qmri_dict_simulate with the corresponding qmri_epg_params -- equal as numbers;
 * the sign of a zero is not pinned --; and when C T <= 1024, C cycles give the numbers of the last T frames of one cycle on the C-fold tiled train
 * and block list.  The only device memory beyond the outputs is the schedule (3 T doubles and at most T / 16 + B segment records of 40 bytes).
 * Out of scope: a slice profile (qmri_dict_simulate_sp), derivatives and a Cramer-Rao bound (qmri_dict_simulate_grad) for this schedule, complex
 * RF phase, diffusion. */
typedef struct {
    int32_t nframes;     /* frames acquired in this block, >= 1 */
    int32_t prep;        /* 0 none, 1 inversion, 2 T2 preparation */
    double  wait;        /* s, >= 0: free relaxation in front of the preparation */
    double  prep_time;   /* s, >= 0: inversion: TI; T2 preparation: its echo time; prep none: must be 0 */
    double  prep_eff;    /* in (0, 1]: inversion efficiency / T2-preparation scale; prep none: must be 1 */
} qmri_epg_block;
typedef struct {
    int32_t nblocks;     /* B, 1..64 */
    int32_t ncycles;     /* C, 1..16: the block list is played C times, only the last is recorded */
    const qmri_epg_block* blocks;   /* host array [B] */
    int32_t reserved[4]; /* zero */
} qmri_epg_seq;
/* The arrays, the layout of F_out, T <= 1024, nstates <= 256 and out_is_f64 of qmri_dict_simulate.  p->inversion must be 0: inversions are stated
 * in the blocks (p->ti and p->inv_eff are not read).  Refusals, decided on the host before the device is selected (ctx == NULL: the message of the
 * first failing check in qmri_last_error(NULL)): everything qmri_dict_simulate refuses; then p->inversion != 0; a NULL seq or seq->blocks; nblocks
 * outside 1..64; ncycles outside 1..16; a non-zero reserved; and per block nframes < 1, prep outside 0..2, a non-finite or negative wait or
 * prep_time, prep_eff outside (0, 1], prep_time != 0 or prep_eff != 1 on a block with prep none; then nframes that do not sum to T:
 * QMRI_ERR_INVALID_ARG, and nothing is written to F_out.  Returns after its kernel has finished. */
int qmri_dict_simulate_seq(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* t1, const double* t2,
                           const double* b1, const qmri_epg_params* p, const qmri_epg_seq* seq, void* F_out);
/* The same with t1, t2, b1 and F_out on ctx's device; alpha, tr, te, p, seq and seq->blocks stay on the host.  Same bits as the host-array call.
 * For an atom this route cannot refuse (see qmri_dict_simulate_dev) the kernel writes NaN in every frame of that atom (and of no other).  F_out
 * feeds qmri_dict_compress_dev as it is. */
int qmri_dict_simulate_seq_dev(qmri_ctx* ctx, int K, int T, const double* alpha, const double* tr, const double* te, const double* d_t1,
                               const double* d_t2, const double* d_b1, const qmri_epg_params* p, const qmri_epg_seq* seq, void* d_F_out);

/* ---- field map from multi-echo images (extension, no reference counterpart, parity unpinned) ---- */
/* qmri_set_field_map takes its map f from the caller; this call makes one from L gradient-echo images per slice, by the regularised estimator of
 * Funai, Fessler, Yeo, Olafsson and Noll (IEEE TMI 2008): a penalised cosine fit over all echo pairs and coils, minimised by separable quadratic
 * surrogates with a FIXED iteration count (no stopping rule, so the bits do not depend on what else is in the batch).
 *   Model: y_{l,c}[n] = x_c[n] exp(sigma i 2 pi f[n] t_l); sigma = phase_sign, default -1 = the sign of qmri_set_field_map's operator.
 *   Pairs (a < b), P = L (L - 1) / 2 of them in the order (0,1), (0,2), ..., (L-2, L-1):
 *     s_ab[n] = sum_c y_{a,c}[n] conj(y_{b,c}[n]), coils ascending (sigma = +1: conj(y_a) y_b);  phi_ab = atan2(Im s_ab, Re s_ab);
 *     d_ab = 2 pi (t_b - t_a);  w_ab[n] = |s_ab[n]| / W,  W = max_n sum_ab |s_ab[n]| over the slice (W = 0: every weight 0).
 *   Cost: Psi(f) = sum_n sum_ab w_ab[n] (1 - cos(phi_ab[n] - d_ab f[n])) + (B / 2) sum_edges (f[n] - f[n'])^2, the edges being the horizontal and
 *     vertical neighbour pairs inside the grid, each once; B = beta (2 pi (t_{L-1} - t_0))^2.
 *   Start: f0[n] = phi_01[n] / d_01, or the caller's f_init.
 *   Iteration, all of f^{k+1} from f^k, per pixel with pairs in their order and the neighbours in the order n1-1, n1+1, n2-1, n2+1:
 *     u_ab = phi_ab - d_ab f, wrapped by u - 2 pi rint(u / 2 pi);  kappa(u) = sin(u) / u (1 for |u| < 1e-8);
 *     g = -sum w_ab d_ab sin u_ab;  c = sum w_ab d_ab^2 kappa(u_ab);  lap = nb f - sum of the nb in-grid neighbours;  den = c + 2 B nb;
 *     f <- f - (g + B lap) / den  (unchanged when den <= 0).
 * Psi does not increase.  All arithmetic is fp64 with explicit fused multiply-adds in one order, no atomics: a slice has the same bits alone, at
 * any position of a stack and for any nslices.  N, M >= 2 are free (no FFT is involved; at most 4096 each).  Needs neither an operator, a
 * denoiser nor a dictionary. */
typedef struct {
    int32_t iters;        /* 1..100000; 0: the default 200 */
    double  beta;         /* dimensionless, finite, >= 0; 0: the default 0.01 (so 0 cannot mean "no regulariser") */
    int32_t phase_sign;   /* -1 (also 0): y_l = x exp(-i 2 pi f t_l), the operator's sign; +1: the other convention */
    int32_t reserved[4];  /* must be 0 */
} qmri_fieldmap_params;
typedef struct {
    double  cost0, cost;      /* Psi before the first and after the last iteration (fixed-order sums) */
    double  f_min, f_max;     /* of the returned map, Hz */
    int32_t iters;            /* iterations run */
    int32_t reserved;
    double  unwrap_limit_hz;  /* 1 / (2 (t_1 - t_0)): the start wraps beyond it */
} qmri_fieldmap_info;
/* Host arrays.  Y: complex fp64, [slice][echo][coil][n1 + N n2]; t_s[nechoes] seconds, finite and strictly increasing; f_init (nullable) and f_out:
 * [slice][n1 + N n2] fp64 Hz, one slice plane being what qmri_set_field_map reads; trust_out (nullable): sum_ab w_ab in the same layout; info
 * (nullable): nslices entries; p (nullable): the defaults.  Refusals are decided on the host before the device is selected (ctx == NULL: the
 * message of the first failing check in qmri_last_error(NULL)): a NULL Y / t_s / f_out, nslices outside 1..4096, nechoes outside 2..8, ncoil < 1,
 * N or M outside 2..4096, a non-finite or non-increasing t_s, a negative or non-finite beta, iters outside 0..100000, phase_sign outside
 * {0, -1, +1}, reserved != 0, a non-finite value in Y or f_init: QMRI_ERR_INVALID_ARG; ncoil > 128: QMRI_ERR_UNSUPPORTED.  Returns after its
 * kernels have finished. */
int qmri_field_map_estimate(qmri_ctx* ctx, int nslices, int nechoes, int ncoil, int N, int M, const void* Y, const double* t_s, const double* f_init,
                            const qmri_fieldmap_params* p, double* f_out, double* trust_out, qmri_fieldmap_info* info);
/* The same with Y, f_init, f_out and trust_out on ctx's device; t_s, p and info stay on the host.  Same bits as the host-array call.  Runs on the
 * context's stream and returns after its kernels have finished.  This route cannot read its images on the host: for a slice whose Y or f_init
 * holds a non-finite value the whole plane of f_out (and of trust_out) of that slice, and of no other, is NaN. */
int qmri_field_map_estimate_dev(qmri_ctx* ctx, int nslices, int nechoes, int ncoil, int N, int M, const void* d_Y, const double* t_s,
                                const double* d_f_init, const qmri_fieldmap_params* p, double* d_f_out, double* d_trust_out, qmri_fieldmap_info* info);

/* ---- locally low-rank regulariser (extension, no reference counterpart, parity unpinned) ---- */
/* The proximal step of the locally low-rank (LLR) penalty of subspace MR fingerprinting (Zhang et al., Tamir et al., Asslaender et al.): the
 * singular values of every b x b spatial block of the coefficient images are soft-thresholded.  It needs no trained weights, is defined for
 * complex images and does not involve the operator.
 *   X: N x M x s complex fp64, [n1 + N n2 + N M c] per slice, slices outermost.  b = block in {4, 8, 16}, b | N and b | M; 0 <= o1, o2 < b.
 *   Block (i, j), i < N / b, j < M / b, holds the pixels ((o1 + i b + p) mod N, (o2 + j b + q) mod M), p, q < b (circular wrap: every block is full).
 *   The b^2 x s Casorati matrix A of a block becomes U max(S - tau, 0) V^H.  tau = 0 is the identity up to rounding; a zero block stays zero.
 *   sigma_max of a slice = the largest singular value over its blocks before thresholding.
 *   Real mode works on real(X); its output has an imaginary part that is exactly 0.
 * The device route: G = A^H A, its eigenpairs by cyclic Jacobi sweeps in a fixed pivot order (at most 24 sweeps), W = V diag(f) V^H with
 * f_k = max(0, 1 - tau / sigma_k), sigma_k = sqrt(max(lambda_k, 0)), out = A W.  All fp64, every sum in one fixed order, no atomics: a slice has
 * the same bits alone, at any position of a stack and for any nslices.  A non-finite value makes the output of its block (and of no other) non-finite. */
typedef struct {
    double  tau;          /* threshold on the singular values, in the units of the TSMI, >= 0 */
    int32_t block;        /* 4, 8 or 16; 0 = 8 */
    int32_t shift;        /* 0: blocks always at offset (0,0); 1: the offsets cycle with the ADMM iteration */
    int32_t reserved[5];  /* must be zero */
} qmri_llr_params;
/* Host arrays.  x: [slice][c][n2][n1], complex fp64 (x_is_complex = 1) or real fp64 (x_is_complex = 0: real mode); out: complex fp64 in the same
 * layout; sigma_max_out (nullable): nslices doubles.  p->shift is ignored (the offsets are arguments).  Needs neither an operator, a denoiser nor a
 * dictionary.  Refusals are decided on the host before the device is selected (ctx == NULL: the message of the first failing check in
 * qmri_last_error(NULL)): a NULL x / p / out, nslices < 1, s outside 1..16, a block outside {0, 4, 8, 16}, N or M not a positive multiple of
 * the block, an offset outside 0..block-1, a negative or non-finite tau, reserved != 0: QMRI_ERR_INVALID_ARG.  Returns after its kernels have finished. */
int qmri_llr_prox(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* x, int x_is_complex, const qmri_llr_params* p, int o1, int o2,
                  void* out, double* sigma_max_out);
/* The same with d_x and d_out (complex fp64 both) on ctx's device; x_is_complex = 0: real mode, the real part of d_x is taken.  d_out may alias
 * d_x.  sigma_max_out (nullable) stays a host array.  Same bits as the host-array call.  Runs on the context's stream and returns after its
 * kernels have finished. */
int qmri_llr_prox_dev(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* d_x, int x_is_complex, const qmri_llr_params* p, int o1, int o2,
                      void* d_out, double* sigma_max_out);
/* Selects the LLR step as Step 2 of the PnP-ADMM loops (p == NULL: back to the network).  While set, qmri_pnp_admm, _dev, _batch, qmri_pnp_admm_mc,
 * _mc_batch and _mc_dev compute v = LLR_tau(x + uold) -- of the complex x + uold with QMRI_DENOISER_COMPLEX, else of real(x + uold) as the
 * reference's Step 2 -- and need no denoiser; the multi_level bit and noise_std are ignored (denoiser_type keeps its range 0..3).  ADMM iteration
 * `it` (0-based) uses the offsets (0, 0) with shift = 0, else q = it mod b^2, o1 = q mod b, o2 = (q div b + q) mod b: every offset once per b^2
 * iterations, both coordinates moving each iteration.  The gridded loop runs its unfused launch sequence; the solvers, the diagnostics and the
 * stage timers work as before, the prox time goes to ms_denoiser.  b must divide N and M of the operator in force at the ADMM call, which
 * otherwise returns QMRI_ERR_INVALID_ARG.  qmri_recon_batch* build their own contexts and are not affected.  Refusals (host only): the checks of
 * qmri_llr_prox on tau, block and reserved, shift outside {0, 1}. */
int qmri_set_llr(qmri_ctx* ctx, const qmri_llr_params* p);

/* ---- joint wavelet soft-thresholding (extension, no reference counterpart, parity unpinned) ---- */
/* The proximal step of the l1-wavelet penalty on the coefficient images of subspace MR fingerprinting, thresholded jointly over the subspace
 * channels: an orthogonal, periodic, L-level 2-D wavelet transform of every channel plane, a shrink of the detail coefficients, the inverse.
 * It needs no trained weights, is defined for complex images and does not involve the operator.
 *   X: N x M x s complex fp64, [n1 + N n2 + N M c] per slice, slices outermost; 1 <= s <= 16.
 *   Filters, T taps: Haar, T = 2, h = [1, 1] / sqrt 2; Daubechies-2, T = 4, h = [1 + sqrt 3, 3 + sqrt 3, 3 - sqrt 3, 1 - sqrt 3] / (4 sqrt 2);
 *   high-pass g[j] = (-1)^j h[T-1-j].  One level on a length-n axis (n even, n >= T): a[k] = sum_j h[j] x[(2k+j) mod n] and
 *   d[k] = sum_j g[j] x[(2k+j) mod n], k < n / 2; synthesis x[(2k+j) mod n] += h[j] a[k] + g[j] d[k].
 *   Level l = 1 .. L acts on the top-left (N / 2^(l-1)) x (M / 2^(l-1)) corner, axis 0 (N) first, approximation coefficients in the low half of
 *   each axis (Mallat layout); synthesis is the exact reverse.  1 <= L <= 4, 2^L | N, 2^L | M, N / 2^(L-1) >= T and M / 2^(L-1) >= T.
 *   Shift: with P = 2^L and 0 <= o1, o2 < P the transform is taken of Xs[n1, n2] = X[(n1 + o1) mod N, (n2 + o2) mod M] and the result shifted back.
 *   Shrink, at every coefficient position outside the final (N / 2^L) x (M / 2^L) approximation corner: m = sqrt(sum_c |C_c|^2) over the channels
 *   (joint = 1) or |C_c| (joint = 0); C <- f C with f = m > tau ? 1 - tau / m : 0.  The approximation corner is never thresholded.
 *   cmax of a slice = the largest m over its detail positions before thresholding (joint = 0: over the channels as well).
 *   Real mode works on real(X); its output has an imaginary part that is exactly 0.
 * tau = 0 is the identity up to rounding; a zero image stays exactly zero.  All fp64, every sum in one fixed order, no atomics: a slice has the
 * same bits alone, at any position of a stack and for any nslices.  A non-finite m gives a non-finite f: a non-finite value reaches the outputs
 * its coefficients reach (Haar: its own shifted 2^L x 2^L block) and no other slice. */
#define QMRI_WAVELET_HAAR 0
#define QMRI_WAVELET_DB2  1
typedef struct {
    double  tau;          /* threshold, in the units of the TSMI, >= 0 and finite */
    int32_t levels;       /* 1 .. 4; 0 = 3 */
    int32_t filter;       /* QMRI_WAVELET_HAAR, QMRI_WAVELET_DB2 */
    int32_t joint;        /* 0: per channel, 1: jointly over the s channels */
    int32_t shift;        /* 0: always the offsets (0,0); 1: the offsets cycle with the ADMM iteration */
    int32_t reserved[4];  /* must be zero */
} qmri_wavelet_params;    /* 40 bytes */
/* Host arrays.  x: [slice][c][n2][n1], complex fp64 (x_is_complex = 1) or real fp64 (x_is_complex = 0: real mode); out: complex fp64 in the same
 * layout; cmax_out (nullable): nslices doubles.  p->shift is ignored (the offsets are arguments).  Needs neither an operator, a denoiser nor a
 * dictionary.  Refusals are decided on the host before the device is selected (ctx == NULL: the message of the first failing check in
 * qmri_last_error(NULL)): a NULL x / p / out, nslices < 1, s outside 1..16, levels outside 0..4, an unknown filter, joint outside
 * {0, 1}, a negative or non-finite tau, reserved != 0, a side that breaks the size rule, an offset outside 0..2^L-1: QMRI_ERR_INVALID_ARG.
 * Returns after its kernels have finished. */
int qmri_wavelet_prox(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* x, int x_is_complex, const qmri_wavelet_params* p, int o1,
                      int o2, void* out, double* cmax_out);
/* The same with d_x and d_out (complex fp64 both) on ctx's device; x_is_complex = 0: real mode, the real part of d_x is taken.  d_out may alias
 * d_x.  cmax_out (nullable) stays a host array.  Same bits as the host-array call.  Runs on the context's stream and returns after its kernels
 * have finished. */
int qmri_wavelet_prox_dev(qmri_ctx* ctx, int N, int M, int s, int nslices, const void* d_x, int x_is_complex, const qmri_wavelet_params* p,
                          int o1, int o2, void* d_out, double* cmax_out);
/* Selects the wavelet step as Step 2 of the PnP-ADMM loops (p == NULL: back to the network), with the conventions of qmri_set_llr: while set,
 * qmri_pnp_admm, _dev, _batch, qmri_pnp_admm_mc, _mc_batch and _mc_dev compute v = Wav_tau(x + uold) -- of the complex x + uold with
 * QMRI_DENOISER_COMPLEX, else of real(x + uold) -- and need no denoiser; the multi_level bit and noise_std are ignored.  ADMM iteration `it`
 * (0-based) uses the offsets (0, 0) with shift = 0, else, with P = 2^L, q = it mod P^2, o1 = q mod P, o2 = (q div P + q) mod P.  The gridded loop
 * runs its unfused launch sequence; the prox time goes to ms_denoiser.  The size rule is tested against the operator in force at the ADMM call,
 * which otherwise returns QMRI_ERR_INVALID_ARG.  qmri_recon_batch* are not affected.  One regulariser at a time: a non-NULL p while the LLR step
 * is set returns QMRI_ERR_STATE (clear it with qmri_set_llr(ctx, NULL) first), and qmri_set_llr with a non-NULL p while the wavelet step is set
 * returns QMRI_ERR_STATE (clear it with qmri_set_wavelet(ctx, NULL) first); a failing call leaves the state as it was.  Refusals (host only): the
 * checks of qmri_wavelet_prox on tau, levels, filter, joint and reserved, shift outside {0, 1}. */
int qmri_set_wavelet(qmri_ctx* ctx, const qmri_wavelet_params* p);

/* ---- simultaneous multi-slice (SMS) groups: an EXTENSION, no reference counterpart, parity unpinned -------------------
 * Z slices excited together with a known phase per frame and slice (SMS-MRF with RF phase cycling): the receiver sees their sum,
 *     y_j[i] = sum_{b < Z} E[t(i), b] (A (C_{b,j} . x_b))[i]          i sample, t(i) its frame, j coil, b slice, A the context's operator
 * and the Z slices of a group are solved jointly.  qmri_set_sms attaches E to the operator in force (gridded or trajectory): T x Z complex
 * doubles, E[t + T*b], every value finite, any modulus; 1 <= Z <= 8 and T*Z <= 8192.  Z = 0 or E = NULL clears it; replacing the operator drops it,
 * as the sample weights.  No existing entry point reads it.  Host work only.  Refusals: Z outside 0..8, T*Z > 8192, a non-finite E:
 * QMRI_ERR_INVALID_ARG; no operator: QMRI_ERR_STATE; an operator with a field map attached (one map cannot serve Z slices): QMRI_ERR_UNSUPPORTED,
 * as is every _sms call while a map is attached.
 *
 * Layouts extend the _mc_batch calls by a group index: maps G x Z x ncoil x N*M, y G x ncoil x m (the ABI's frame-major order, one set of samples
 * per group), x / z / x0 / x_out G x Z x N*M*s (complex doubles).
 *     A_sms x   = [ sum_b E[t(i), b] (A (C_{g,b,j} . x_{g,b}))_i ]_{g,j}
 *     A_sms^H y = [ sum_j conj(C_{g,b,j}) . A^H (conj(E[t(.), b]) . y_{g,j}) ]_{g,b}
 * slice b added after slice b - 1 and coil j after coil j - 1, in fp64, whatever max_batch is.
 * qmri_xupdate_sms: x = lsqr(@afun, [y; sqrt(r) z], tol, maxit, [], [], x0), afun = [A_sms; sqrt(r) I], over the Z slices of a group jointly, with
 * the recurrences, stop rules (flags 0 / 1 / 3) and order of qmri_xupdate_mc_batch; one iteration count and flag per GROUP (iters_out / flags_out:
 * G entries, nullable).  A group's result is the same bits alone, at any position of any call, at any G and max_batch; with Z = 1 and E = 1 it
 * is qmri_xupdate_mc_batch's, bit for bit.
 * qmri_pnp_admm_sms: the loop of qmri_pnp_admm_mc_batch with that x-update, groups_per_launch groups at a time (groups_per_launch * Z <=
 * max_batch of the operator and the denoiser); x0 = NULL: A_sms^H y; Step 2 runs on the G Z slice images as in every other loop (network in real
 * or complex mode, qmri_set_llr, qmri_set_wavelet); lsqr_iters_out: G x prm->iters (nullable).  prm->solver must be QMRI_SOLVER_LSQR: TOEPLITZ
 * (its normal operator would need Z^2 point-spread functions) and DIRECT are QMRI_ERR_UNSUPPORTED.  _dev: device arrays, G * Z <= max_batch,
 * d_x_out must not alias d_x0.
 * Refusals, decided on the host before the device is selected (ctx == NULL: QMRI_ERR_INVALID_ARG, message in qmri_last_error(NULL)): a NULL
 * array, G < 1, ncoil outside 1..1024, r <= 0, maxit < 0, groups_per_launch < 1 or groups_per_launch * Z > max_batch: QMRI_ERR_INVALID_ARG; no
 * operator, no qmri_set_sms, no Step 2 configured: QMRI_ERR_STATE. */
int qmri_set_sms(qmri_ctx* ctx, int Z, const void* E);
int qmri_forward_sms(qmri_ctx* ctx, int G, int ncoil, const void* maps, const void* x, int x_is_complex, void* y);
int qmri_adjoint_sms(qmri_ctx* ctx, int G, int ncoil, const void* maps, const void* y, void* x);
int qmri_xupdate_sms(qmri_ctx* ctx, int G, int ncoil, const void* maps, const void* y, const void* z, double r, double tol, int maxit, const void* x0,
                     void* x_out, int32_t* iters_out, int32_t* flags_out);
int qmri_pnp_admm_sms(qmri_ctx* ctx, int G, int groups_per_launch, int ncoil, const void* maps, const void* y, const qmri_admm_params* prm,
                      const void* x0, void* x_out, int32_t* lsqr_iters_out);
int qmri_pnp_admm_sms_dev(qmri_ctx* ctx, int G, int ncoil, const void* d_maps, const void* d_y, const qmri_admm_params* prm, const void* d_x0,
                          void* d_x_out, int32_t* lsqr_iters_out);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------------ */
typedef struct {
    double ms_xupdate, ms_denoiser, ms_elementwise, ms_diag, ms_match;   /* hipEvent time per stage */
    double ms_conv3x3;          /* level 2: summed duration of the 3x3 convolution launches, each taken from its own dispatch timestamps: one
                                 * launch per layer (a split-K layer: from the convolution's start to its reduce kernel's end), or one
                                 * resident-tile launch of a whole run of layers (with whatever else rides in it) as ONE unit */
    int64_t n_conv3x3;          /* number of those units */
    int64_t lsqr_iters;         /* LSQR iterations executed */
    int64_t admm_iters;
    double ms_tv_iter;          /* LRTV: summed duration of the prox_tv iteration kernel's launches (level 2) */
    int64_t n_tv_iter;
    double flop_conv3x3;        /* fp32-equivalent algorithmic work of the units in ms_conv3x3: 2 Cout Cin taps Hout Wout B per layer inside them */
    double ms_conv2x2;          /* level 2: the 2x2 / stride-2 (transposed) convolutions launched on their own */
    int64_t n_conv2x2;
    double flop_conv2x2;
    double ms_lsqr_kernels;     /* level 2: the LSQR iteration kernels alone (k_ks_a start -> k_ks_b end per iteration, or a whole k_ks_persist launch) */
    int64_t n_lsqr_launches;
    double ms_net_forward;      /* level 2: whole forward passes of the network, first launch to last (stream events) */
    int64_t n_net_forward;
} qmri_profile;
int qmri_profile_enable(qmri_ctx* ctx, int level);   /* 0 off, 1 per stage (synchronises at every stage boundary), 2 also per conv3x3 launch,
                                                        3 stage MARKS: event records at the stage boundaries that are read only after the call's own final
                                                        synchronisation -- the stage split of a timed run without a wait inside it (batches; an event record
                                                        between two dependent kernels costs a few microseconds, so not for the one-slice headline) */
int qmri_profile_get(qmri_ctx* ctx, qmri_profile* out, int reset);

/* Health of a context (no counterpart in the reference, which reconstructs one slice per run -- main_recon_tsmis_FFT.m:37-38 -- and has no
 * alternative paths): which of the library's self-checking fast paths are armed, how often one of them gave up and the work was repeated on the
 * slower path, and what the most recent qmri_pnp_admm_dev call cost.  A reconstruction that is slow for one of THESE reasons says so here; the
 * results are the same either way (every fallback is tested for bits).  Counters run from qmri_create; the denoiser's from qmri_set_denoiser. */
typedef struct {
    int denoiser_scheme;        /* 2 = f16 x 3 products, 3 = bf16 x 6 products, 0 = no denoiser set */
    int denoiser_fallbacks;     /* switches f16 -> bf16 by the range / low-magnitude guards since qmri_set_denoiser */
    int resident_armed;         /* 1 = the resident-tile launch of the full-resolution ResBlocks is in use (one slice per launch only) */
    int resident_timeouts;      /* ring hand-offs that timed out since qmri_set_denoiser (each: the forward pass was repeated, one launch per layer) */
    int lsqr_one_launch;        /* 1 = the one-launch LSQR iteration is armed, 0 = switched off (by a time-out or by the caller), -1 = not decided yet */
    int lsqr_timeouts;          /* one-launch LSQR kernels that gave up waiting for a partial sum (each: the solve or the reconstruction was repeated) */
    int repeated_calls;         /* qmri_pnp_admm* calls that ran their reconstruction twice (any of the reasons above) */
    int reserved;
    double last_call_wall_ms;   /* host wall clock of the most recent qmri_pnp_admm_dev call, entry to return */
    double last_call_stage_ms[4]; /* its x-update / denoiser / elementwise / diagnostics stages on the device (profile level 1 or 3 only, else zeros) */
    double set_denoiser_ms[3];  /* the most recent qmri_set_denoiser on the host clock: weight splitting, packing and upload of all layers / tensors and
                                   buffers / the two-pass calibration probe (the reference loads its network once per run: main_recon_tsmis_FFT.m:138-152) */
} qmri_health;
int qmri_get_health(const qmri_ctx* ctx, qmri_health* out);

/* Diagnostics (no counterpart in the reference): in-kernel 100 MHz phase stamps, recorded only when the library was
 * started with the knobs lsqr_stamps / conv_stamps set (qmri_debug_knob, QMRI_DEBUG; otherwise QMRI_ERR_STATE).  `out` receives 2*512*16 and 4096*11
 * 64-bit values; layouts are those read by tools/lsqr_stamps.py and tools/conv6_stamps.py. */
int qmri_debug_lsqr_stamps(qmri_ctx* ctx, unsigned long long* out);
int qmri_debug_conv_stamps(qmri_ctx* ctx, unsigned long long* out, int reserved);
/* Test / A-B hook: the LSQR x-update (PnP_ADMM.m:102) runs all its iterations in ONE launch where the operator's work units are resident at
 * once (default; same bits as the two-launch iteration); on = 0 selects the two-launch iteration (also the knob lsqr_persist = 0); on = 2 makes
 * the one-launch kernel lose a partial sum on purpose: its waits time out, the library reports it on stderr and repeats the solve with the
 * two-launch iteration (the recovery path, tested). */
int qmri_debug_lsqr_persist(qmri_ctx* ctx, int on);
/* Test / A-B hook for the dictionary match (mrf_dtm_cpu.m:91-92): on = 1 (default) puts the f16 filter in front of the exact single-precision
 * products (the result is the same, bit for bit: the filter only decides which 32-atom tiles need the exact products), on = 0 computes
 * every product exactly.  margin_scale (default 1) multiplies the filter's margin: the tests shrink it to measure how far the proven
 * margin is from the first wrong answer. */
int qmri_debug_dict_filter(qmri_ctx* ctx, int on, float margin_scale);
/* Test / A-B hook for the denoiser's convolutions: on = 1 (default) runs the ResBlocks of the full-resolution level of a one-slice forward pass as
 * ONE launch with LDS-resident tiles (same bits as one launch per layer); on = 0 selects one launch per layer (also the knob conv_resident = 0); on = 2
 * makes one tile withhold its hand-off on purpose: its neighbours' waits time out, the library reports it on stderr, repeats the call with one
 * launch per layer and keeps the resident form off (the recovery path, tested).  timeouts_out (or NULL): hand-off time-outs seen so far. */
int qmri_debug_conv_resident(qmri_ctx* ctx, int on, int* timeouts_out);
/* Test / timing hook of the dictionary compression: step 1 alone, G = F^T F (T x T fp64 column-major, both triangles) as qmri_dict_compress forms
 * it.  on_device = 0: F and G_out are host arrays; 1: device arrays of ctx's device.  Returns after its kernels have finished. */
int qmri_debug_dsvd_gram(qmri_ctx* ctx, int K, int T, const void* F, int f_is_f64, int on_device, double* G_out);
/* Test hook of the dictionary simulation: step 5 (the spoiler) alone, nshift times, on one atom's given state with the lane layout
 * qmri_dict_simulate uses for S states.  in / out: host arrays of 3 S doubles, F+ [S], F- [S], Z [S] (Z is copied).  1 <= S <= 256, 0 <= nshift <= 4096. */
int qmri_debug_epg_shift(qmri_ctx* ctx, int S, int nshift, const double* in, double* out);
/* The one entry point of the process-wide A/B and diagnostic switches ("knobs": tile configurations, the fused launches, in-kernel stamps of the
 * diagnostic builds ...; names and defaults: csrc/api_core.cpp g_knob_defs).  The same switches can be set at start-up through the library's
 * only environment variable, QMRI_DEBUG="name=value,name=value".  Every default is the product's behaviour; an unknown name is
 * QMRI_ERR_INVALID_ARG (message: qmri_last_error(NULL)).  Knobs are read when a plan is made or a launch is issued: set them before
 * qmri_set_operator / qmri_set_denoiser. */
int qmri_debug_knob(const char* name, int value);
/* Diagnostic: the library's device and pinned allocations, counted process-wide where they are made (csrc/dev_mem.h): how many are live, their
 * bytes, and how many were made since the process started.  Takes no context, so it also reads after qmri_destroy: a process that has destroyed
 * all its contexts reads zero live allocations.  out == NULL: QMRI_ERR_INVALID_ARG. */
typedef struct {
    long long dev_live, dev_bytes, dev_total;           /* hipMalloc */
    long long pinned_live, pinned_bytes, pinned_total;  /* hipHostMalloc */
} qmri_mem_stats;
int qmri_debug_mem_stats(qmri_mem_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* QMRI_H */
