"""Host-side mirror of the reference's plugin surface for the hot path (same names, argument meaning and error
behaviour as the MATLAB functions), implemented on top of the C ABI.  MATLAB itself is not available in this
pipeline, so this Python mirror is the executable counterpart of the `.m` wrappers in `matlab/`.

    P   = setup_subsampling_spiralgrided(N, M, S, V)        # setup_subsampling_spiralgrided.m:1
    P   = setup_subsampling_epi(N, M, percentage, V)        # setup_subsampling_epi.m:1
    P   = setup_subsampling_spiral_exact(N, M, S, V)        # the same spiral before its rounding (a trajectory)
    F   = make_F(P)                                         # F.forward / F.adjoint, main_recon_tsmis_FFT.m:228-229
    net = make_net(weights, denoiser_type, residual_noise)  # param.net, main_recon_tsmis_FFT.m:164
    net = make_llr(F, tau, tau_rel, block, shift)           # param.net without a network: the locally low-rank regulariser
    net = make_wavelet(F, tau, tau_rel, levels, filter, joint, shift)   # ... or joint wavelet soft-thresholding
    x   = PnP_ADMM(y, param)                                # PnP_ADMM.m:1, param = dict with the reference's field names
    out = mrf_dtm_cpu(dict, data, par)                      # mrf_dtm_cpu.m:1 (name kept; it runs on the GPU)
    x   = FISTA_deep(data, param)                           # LRTV option, FISTA_deep.m:1 (+ TV_operator, prox_tv, norm_tv)
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import engine as E

_engines = {}


def _engine(device=0) -> E.Engine:
    if device not in _engines:
        _engines[device] = E.Engine(device)
    return _engines[device]


def release():
    for e in _engines.values():
        e.close()
    _engines.clear()


def setup_subsampling_spiralgrided(N, M, S, V):
    """Gridded spiral masks (setup_subsampling_spiralgrided.m:7-34).  The reference returns closures over the sparse
    matrix P; here P is its defining data (masks + V) and the products happen inside F."""
    if int(N) != int(M):
        raise ValueError(f"the spiral mask is square (setup_subsampling_spiralgrided.m:28-31): N = {N} != M = {M}")
    V = np.real(np.asarray(V, dtype=np.complex128)).astype(np.float64)        # V = real(dict.V), main_recon_tsmis_FFT.m:129
    fp, k = E.build_spiral(int(N), int(S), V.shape[0])
    return SimpleNamespace(N=int(N), M=int(M), V=V, frame_ptr=fp, kidx=k, pattern="Spiral")


def setup_subsampling_epi(N, M, percentage, V):
    """Multi-shot EPI comb masks (setup_subsampling_epi.m:20-33)."""
    V = np.real(np.asarray(V, dtype=np.complex128)).astype(np.float64)
    fp, k = E.build_epi(int(N), int(M), float(percentage), V.shape[0])
    return SimpleNamespace(N=int(N), M=int(M), V=V, frame_ptr=fp, kidx=k, pattern="EPI")


def setup_subsampling_spiral_exact(N, M, S, V):
    """The spiral of setup_subsampling_spiralgrided.m:7-27 WITHOUT the rounding onto the grid: every sample at its exact position
    (qmri_build_spiral_traj); make_F turns it into the NUFFT operator (qmri_set_operator_nufft).  No reference counterpart."""
    if int(N) != int(M):
        raise ValueError(f"the spiral is square (setup_subsampling_spiralgrided.m:28-31): N = {N} != M = {M}")
    V = np.real(np.asarray(V, dtype=np.complex128)).astype(np.float64)
    fp, om = E.build_spiral_traj(int(N), int(S), V.shape[0])
    return SimpleNamespace(N=int(N), M=int(M), V=V, frame_ptr=fp, omega=om, pattern="SpiralExact", S=int(S))


def make_F(P, device=0, field_map=None, readout_s=None, field_echoes=None, field_echo_times=None):
    """F.forward = @(x) P.for(reshape(fft2(x),[],1))/sqrt(N*M);  F.adjoint = @(x) ifft2(reshape(P.adj(x),N,M,[]))*sqrt(N*M).
    A P with a trajectory (setup_subsampling_spiral_exact) gives the same two maps at the exact sample positions; field_map (N x M, Hz) with
    readout_s (the length of one spiral readout, seconds) then attaches the off-resonance correction (an extension):
    F.forward / F.adjoint and PnP_ADMM carry exp(-i 2 pi f tau).  F.field_info is what Engine.set_field_map reported, or None.
    field_echoes ([L, N, M] or [L, C, N, M] gradient-echo images) with field_echo_times ([L] seconds) instead of field_map (or with
    field_map="estimate"): the map is estimated from them on the device first (Engine.estimate_field_map) and attached in
    the same way; F.field_map is the map in use and F.field_map_info what the estimate reported (None for a caller's map)."""
    if (field_echoes is None) != (field_echo_times is None):
        raise ValueError("field_echoes and field_echo_times go together")
    if isinstance(field_map, str) and (field_map != "estimate" or field_echoes is None):
        raise ValueError('field_map is an N x M array, or "estimate" with field_echoes and field_echo_times')
    if field_echoes is not None and not (field_map is None or isinstance(field_map, str)):
        raise ValueError("give field_echoes or a field_map, not both")
    fm_info = None
    if field_echoes is not None:
        if readout_s is None:
            raise ValueError("field_map and readout_s go together")
        if getattr(P, "omega", None) is None:
            raise ValueError("field_map needs a trajectory operator (setup_subsampling_spiral_exact): a gridded mask has no readout times")
        if np.asarray(field_echoes).ndim not in (3, 4):
            raise ValueError("field_echoes must be [L, N, M] or [L, C, N, M]: one map per operator")
        field_map, fm_info = _engine(device).estimate_field_map(field_echoes, field_echo_times, return_info=True)
    if (field_map is None) != (readout_s is None):
        raise ValueError("field_map and readout_s go together")
    if field_map is not None and getattr(P, "omega", None) is None:
        raise ValueError("field_map needs a trajectory operator (setup_subsampling_spiral_exact): a gridded mask has no readout times")
    eng = _engine(device)
    info = None
    if getattr(P, "omega", None) is not None:
        eng.set_trajectory(P.N, P.M, P.V, P.frame_ptr, P.omega)
        if field_map is not None:
            info = eng.set_field_map(field_map, E.spiral_readout_times(P.S, P.V.shape[0], readout_s))
    else:
        eng.set_operator(P.N, P.M, P.V, P.frame_ptr, P.kidx)
    return SimpleNamespace(forward=eng.forward, adjoint=eng.adjoint, _engine=eng, _P=P, field_info=info, field_map=field_map, field_map_info=fm_info)


def denoiseImage_PnP_ADMM(A, net, onnx_dagnetwork=True, residual_noise=False):
    """I = denoiseImage_PnP_ADMM(A, net, onnx_dagnetwork, residual_noise)  (denoiseImage_PnP_ADMM.m:1).
    `net` is the handle returned by make_net; input validation follows validateInputImage (:119-127)."""
    A = np.asarray(A)
    if np.iscomplexobj(A):
        raise TypeError("Expected A to be real.")                            # validateattributes 'real'
    if A.size == 0:
        raise ValueError("Expected A to be nonempty.")
    if not np.all(np.isfinite(A)):
        raise ValueError("Expected A to be finite.")                         # 'nonnan','finite'
    if A.ndim > 4:
        raise ValueError("images:denoiseImage:invalidImageFormat")
    if bool(residual_noise) != bool(net._residual_noise):
        raise ValueError("residual_noise differs from the value the network handle was created with")
    return net._engine.denoise(A)


def make_net(weights, denoiser_type="single_level", residual_noise=False, H=224, W=224, nc=(64, 128, 256, 512), nb=4,
             out_nc=10, device=0, tsmi_domain="real"):
    """param.net = @(x) denoiseImage_PnP_ADMM(x, Net, true, residual_noise)  (main_recon_tsmis_FFT.m:138-164).
    out_nc: the network's output channels -- s for real TSMIs; tsmi_domain "complex": 2s, the cat(3, real, imag) layout of complex TSMIs."""
    if denoiser_type not in ("single_level", "multi_level"):
        raise ValueError(f"unknown denoiser_type {denoiser_type}")
    from .engine import denoiser_type as _dtype
    _dtype(False, tsmi_domain)                                     # (checks tsmi_domain)
    if tsmi_domain == "complex" and out_nc % 2:
        raise ValueError(f"a denoiser of complex TSMIs has an even number of output channels (2s), not {out_nc}")
    eng = _engine(device)
    in_nc = out_nc + (1 if denoiser_type == "multi_level" else 0)
    eng.set_denoiser(weights, H, W, in_nc=in_nc, out_nc=out_nc, nc=nc, nb=nb, residual_noise=residual_noise)

    def net(x):
        return denoiseImage_PnP_ADMM(x, net, True, residual_noise)

    net._engine, net._residual_noise, net._denoiser_type, net._tsmi_domain = eng, bool(residual_noise), denoiser_type, tsmi_domain
    return net


def make_llr(F, tau=None, tau_rel=0.02, block=8, shift=True):
    """param.net without a network (an extension): Step 2 of PnP_ADMM becomes the locally low-rank proximal step
    v = LLR_tau(x + uold) on block x block patches (Engine.set_llr), which needs no trained weights and fits every operator of make_F.
    tau: the threshold on the singular values in the units of the TSMI; None: tau_rel times sigma_max of the loop's start image (Engine.llr_prox
    with tau = 0 gives sigma_max).  shift: the block offsets cycle with the iteration.  The threshold a PnP_ADMM call used is .tau afterwards."""
    if not hasattr(F, "_engine"):
        raise TypeError("F must come from make_F of this package")
    if block not in (4, 8, 16):
        raise ValueError("block must be 4, 8 or 16")
    if tau is not None and not (float(tau) >= 0 and np.isfinite(tau)):
        raise ValueError("tau must be finite and >= 0")
    if tau is None and not (float(tau_rel) >= 0 and np.isfinite(tau_rel)):
        raise ValueError("tau_rel must be finite and >= 0")
    return SimpleNamespace(_engine=F._engine, _llr=True, _denoiser_type="single_level", _tsmi_domain="real", _residual_noise=False,
                           tau=None if tau is None else float(tau), tau_given=None if tau is None else float(tau), tau_rel=float(tau_rel),
                           block=int(block), shift=bool(shift), sigma_max=None)


def _llr_arm(F, net, param, y, x0, tsmi_domain):
    """Sets the engine's LLR step for one PnP_ADMM call; the threshold comes from the start image unless the caller gave one."""
    eng = F._engine
    if net.tau_given is None:
        start = x0 if x0 is not None else F.adjoint(y)
        _, net.sigma_max = eng.llr_prox(start, 0.0, block=net.block, real=tsmi_domain != "complex")
        net.tau = net.tau_rel * net.sigma_max
    eng.set_llr(net.tau, block=net.block, shift=net.shift)


WAVELET_TAU_REL = 0.05      # of cmax of the start image: the choice of DESIGN.md section 29 (tests/test_gpu_wavelet.py::test_it_regularises)


def make_wavelet(F, tau=None, tau_rel=WAVELET_TAU_REL, levels=3, filter="db2", joint=True, shift=True):
    """param.net without a network (an extension): Step 2 of PnP_ADMM becomes joint wavelet soft-thresholding
    v = Wav_tau(x + uold) (Engine.set_wavelet), which needs no trained weights and fits every operator of make_F.  tau: the threshold on the
    detail coefficients in the units of the TSMI; None: tau_rel times cmax of the loop's start image (Engine.wavelet_prox with tau = 0 gives
    cmax).  levels 1..4, filter "haar" or "db2", joint: the s channels are thresholded together; shift: the offsets cycle with the iteration.
    The threshold a PnP_ADMM call used is .tau afterwards."""
    if not hasattr(F, "_engine"):
        raise TypeError("F must come from make_F of this package")
    if levels not in (1, 2, 3, 4):
        raise ValueError("levels must be 1, 2, 3 or 4")
    if filter not in E.WAVELET_FILTERS:
        raise ValueError(f'filter must be one of {sorted(E.WAVELET_FILTERS)}, not {filter!r}')
    if tau is not None and not (float(tau) >= 0 and np.isfinite(tau)):
        raise ValueError("tau must be finite and >= 0")
    if tau is None and not (float(tau_rel) >= 0 and np.isfinite(tau_rel)):
        raise ValueError("tau_rel must be finite and >= 0")
    return SimpleNamespace(_engine=F._engine, _wavelet=True, _denoiser_type="single_level", _tsmi_domain="real", _residual_noise=False,
                           tau=None if tau is None else float(tau), tau_given=None if tau is None else float(tau), tau_rel=float(tau_rel),
                           levels=int(levels), filter=filter, joint=bool(joint), shift=bool(shift), cmax=None)


def _wavelet_arm(F, net, param, y, x0, tsmi_domain):
    """Sets the engine's wavelet step for one PnP_ADMM call; the threshold comes from the start image unless the caller gave one."""
    eng = F._engine
    if net.tau_given is None:
        start = x0 if x0 is not None else F.adjoint(y)
        _, net.cmax = eng.wavelet_prox(start, 0.0, levels=net.levels, filter=net.filter, joint=net.joint, real=tsmi_domain != "complex")
        net.tau = net.tau_rel * net.cmax
    eng.set_wavelet(net.tau, levels=net.levels, filter=net.filter, joint=net.joint, shift=net.shift)


def build_noise_map(noise_std, rows, cols):
    """noise_map = repmat(noise_std, rows, cols)  (build_noise_map.m:19)."""
    return np.full((rows, cols), float(noise_std))


def PnP_ADMM(y, param):
    """x = PnP_ADMM(y, param)  (PnP_ADMM.m:1).  param: dict with iter, gamma, F, cg_tol, gt_tsmi, net, denoiser_type,
    noise_map (multi_level), X0 (PnP_ADMM.m:62-76).  F and net must be the handles made by make_F / make_net on the same
    device: the whole loop then runs on the GPU with one boundary crossing.  param["tsmi_domain"] (default: the net's, "real"):
    "complex" runs the denoiser step on cat(3, real, imag) of x + uold.  param["x0"] = "dcf" (an extension for a
    trajectory F): the start image is the density-compensated adjoint of y instead of param["X0"]; the weights are
    computed here if none are attached yet.  param["field_normal"] (an extension for a trajectory F with a field map): True,
    or a dict with nseg / tol, builds the field-aware Toeplitz normal operator before the loop (Engine.prepare_normal_field), which
    param["solver"] = "toeplitz" then needs; what it reported is PnP_ADMM.last_field_normal."""
    F, net = param["F"], param["net"]
    if not hasattr(F, "_engine") or not hasattr(net, "_engine") or F._engine is not net._engine:
        raise TypeError("param.F and param.net must come from make_F / make_net of this package (same device)")
    PnP_ADMM.last_field_normal = _field_normal(F, param.get("field_normal"))
    llr = getattr(net, "_llr", False)                               # (make_llr: Step 2 is the locally low-rank prox)
    wavelet = getattr(net, "_wavelet", False)                       # (make_wavelet: joint wavelet soft-thresholding)
    multi = param.get("denoiser_type", net._denoiser_type) == "multi_level" and not llr and not wavelet
    noise_std = float(np.asarray(param["noise_map"]).ravel()[0]) if multi else 0.01
    traj = getattr(F._P, "omega", None) is not None                 # (a trajectory computes no per-iteration diagnostics: last_diagnostics is None)
    tsmi_domain = param.get("tsmi_domain", getattr(net, "_tsmi_domain", "real"))
    x0 = _dcf_x0(F, param, y)
    if llr:
        _llr_arm(F, net, param, y, x0, tsmi_domain)
    if wavelet:
        _wavelet_arm(F, net, param, y, x0, tsmi_domain)
    try:
        x, diag, li = F._engine.pnp_admm(y, gamma=param["gamma"], iters=int(param["iter"]), cg_tol=param["cg_tol"], cg_maxit=100,
                                         solver=param.get("solver", "lsqr"), multi_level=multi, noise_std=noise_std,
                                         tsmi_domain=tsmi_domain,
                                         x0=x0, gt=None if traj else param.get("gt_tsmi"),
                                         want_diag=param.get("gt_tsmi") is not None and not traj)
    finally:
        if llr:
            F._engine.clear_llr()
        if wavelet:
            F._engine.clear_wavelet()
    PnP_ADMM.last_diagnostics, PnP_ADMM.last_lsqr_iters = diag, li
    return x


def _field_normal(F, fn):
    """param["field_normal"]: None / False: nothing; True: the defaults; a dict: its nseg and tol."""
    if fn is None or fn is False:
        return None
    if fn is True:
        fn = {}
    if not isinstance(fn, dict) or set(fn) - {"nseg", "tol"}:
        raise ValueError("field_normal must be True or a dict with nseg and / or tol")
    return F._engine.prepare_normal_field(nseg=fn.get("nseg", 0), tol=fn.get("tol", 0.0))


def _dcf_x0(F, param, y):
    """The start image of PnP_ADMM: param["X0"], or with param["x0"] == "dcf" the engine's density-compensated adjoint of y.  Whether weights
    are attached is the engine's to say (QMRI_ERR_STATE): weights the caller attached are used as they are, and only an operator without any
    gets the Pipe-Menon weights of density_weights()."""
    x0 = param.get("x0")
    if x0 is None:
        return param.get("X0")
    if x0 != "dcf":
        raise ValueError(f'param["x0"] must be "dcf" or absent, not {x0!r}')
    if getattr(F._P, "omega", None) is None:
        raise ValueError('param["x0"] = "dcf" needs a trajectory operator (setup_subsampling_spiral_exact)')
    try:
        return F._engine.adjoint(y, weighted=True)
    except E.QmriError as err:
        if err.code != -2:                                          # (QMRI_ERR_STATE: no sample weights attached)
            raise
    F._engine.density_weights()
    return F._engine.adjoint(y, weighted=True)


def FISTA_deep(data, param):
    """[x] = FISTA_deep(data, param)  (FISTA_deep.m:1): data = dict(N, M, L, y, F, D), param = dict(K, iter, step, tol,
    backtrack, usegpu) as main_recon_tsmis_FFT.m:274-281 builds them.  F must come from make_F; the whole loop runs on the
    GPU (param.usegpu is ignored)."""
    F = data["F"]
    if not hasattr(F, "_engine"):
        raise TypeError("data.F must come from make_F of this package")
    eng = F._engine
    if (data["N"], data["M"], data["L"]) != (eng.N, eng.M, eng.s) and (data["M"], data["M"], data["L"]) != (eng.N, eng.M, eng.s):
        raise ValueError("data.N / M / L do not match the operator")       # (the script passes data.N = M, :281)
    x, info = eng.lrtv(data["y"], K=param["K"], iters=int(param["iter"]), step=param.get("step"), tol=param["tol"],
                       backtrack=param.get("backtrack", 1))
    FISTA_deep.last_info = info
    return x


def TV_operator(mode="2D", usegpu=0, device=0):
    """J = TV_operator('2D', usegpu)  (TV_operator.m:1): J.norm / J.prox applied slice by slice along the third dimension."""
    if mode != "2D":
        raise NotImplementedError("only the 2-D operator is on the path (main_recon_tsmis_FFT.m:280)")
    eng = _engine(device)

    def norm(x2):
        x2 = np.asarray(x2, dtype=np.float64)
        x2 = x2[:, :, None] if x2.ndim == 2 else x2
        return float(sum(eng.norm_tv(x2[:, :, i]) for i in range(x2.shape[2])))

    def prox(x2, gamma):
        x2 = np.asarray(x2, dtype=np.float64)
        squeeze = x2.ndim == 2
        x2 = x2[:, :, None] if squeeze else x2
        out = np.stack([eng.prox_tv(x2[:, :, i], gamma)[0] for i in range(x2.shape[2])], axis=2)
        return out[:, :, 0] if squeeze else out

    return SimpleNamespace(norm=norm, prox=prox)


def mrf_dtm_cpu(dict_, data, par, device=0):
    """out = mrf_dtm_cpu(dict, data, par)  (mrf_dtm_cpu.m:1): dict.{D,normD,lut}, data.X, par.f.{qout,pdout,mtout,dmout,Xout}."""
    eng = _engine(device)
    eng.set_dictionary(dict_["D"], dict_["normD"], dict_["lut"])
    f = par.get("f", {})
    r = eng.dict_match(data["X"], want_mt=True, want_dm=True, want_xfit=bool(f.get("Xout", 0)))
    out = {}
    if f.get("qout", 1):
        out["qmap"], out["mask"] = r["qmap"], np.ones(np.asarray(data["X"]).shape[:-1], bool)
    if f.get("pdout", 1):
        out["pd"] = r["pd"]
    if f.get("mtout", 0):
        out["mt"] = r["mt"]
    if f.get("dmout", 0):
        out["dm"] = r["dm"].astype(np.float32)
    if f.get("Xout", 0):                                      # mrf_dtm_cpu.m:129-134: the scaled matched atoms and the input
        out["Xfit"], out["X"] = r["Xfit"], data["X"]
    return out
