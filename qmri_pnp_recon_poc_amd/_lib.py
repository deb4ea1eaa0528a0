"""ctypes loader for libqmri.so (include/qmri.h).

The product path has no CPU fallback: if the shared library is missing it is built with hipcc (which
cross-compiles gfx950 without a GPU); if that fails, or a symbol is absent, loading raises.  Compute entry
points additionally need a gfx950 device and fail with QMRI_ERR_HIP otherwise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libqmri.so")
CSRC = os.path.join(_PKG, "csrc")

# every symbol include/qmri.h declares (checked at load time and by tests/test_abi.py)
SYMBOLS = [
    "qmri_abi_version", "qmri_create", "qmri_destroy", "qmri_last_error", "qmri_set_stream", "qmri_synchronize",
    "qmri_build_spiral", "qmri_build_epi", "qmri_build_spiral_traj", "qmri_set_operator", "qmri_set_operator_nufft", "qmri_nufft_prepare_normal", "qmri_normal", "qmri_normal_dev",
    "qmri_nufft_dcf", "qmri_set_sample_weights", "qmri_adjoint_w", "qmri_adjoint_w_dev", "qmri_adjoint_w_mc", "qmri_set_field_map", "qmri_nufft_prepare_normal_fm", "qmri_operator_m", "qmri_forward", "qmri_adjoint",
    "qmri_forward_f32", "qmri_adjoint_f32", "qmri_forward_dev", "qmri_adjoint_dev", "qmri_set_coils", "qmri_forward_mc", "qmri_adjoint_mc", "qmri_xupdate_mc", "qmri_pnp_admm_mc", "qmri_xupdate_mc_batch", "qmri_pnp_admm_mc_batch", "qmri_pnp_admm_mc_dev", "qmri_xupdate", "qmri_net_nparams", "qmri_set_denoiser", "qmri_denoise",
    "qmri_net_forward_dev", "qmri_denoiser_scheme", "qmri_pnp_admm", "qmri_pnp_admm_dev", "qmri_pnp_admm_batch", "qmri_set_dictionary", "qmri_dict_match",
    "qmri_dict_match_dev", "qmri_dict_match_xfit", "qmri_dict_match_xfit_dev", "qmri_set_dictionary_groups", "qmri_dict_group_assign", "qmri_dict_match_grouped",
    "qmri_dict_match_grouped_dev", "qmri_dict_group_scores", "qmri_dict_group_scores_dev", "qmri_b1_pool", "qmri_b1_pool_dev", "qmri_b1_estimate",
    "qmri_b1_estimate_dev", "qmri_set_components", "qmri_dict_unmix", "qmri_dict_unmix_dev", "qmri_dict_lines", "qmri_set_refine", "qmri_dict_refine",
    "qmri_dict_refine_dev", "qmri_recon_batch", "qmri_recon_batch_mc",
    "qmri_coil_compress", "qmri_coil_compress_dev", "qmri_coil_eig", "qmri_recon_batch_mc_cc", "qmri_coil_maps", "qmri_coil_maps_dev", "qmri_dict_compress", "qmri_dict_compress_dev", "qmri_dict_simulate", "qmri_dict_simulate_dev", "qmri_dict_simulate_sp", "qmri_dict_simulate_sp_dev", "qmri_dict_simulate_grad", "qmri_dict_simulate_grad_dev", "qmri_dict_simulate_seq", "qmri_dict_simulate_seq_dev", "qmri_field_map_estimate", "qmri_field_map_estimate_dev", "qmri_llr_prox", "qmri_llr_prox_dev", "qmri_set_llr", "qmri_wavelet_prox", "qmri_wavelet_prox_dev", "qmri_set_wavelet", "qmri_set_sms", "qmri_forward_sms", "qmri_adjoint_sms", "qmri_xupdate_sms", "qmri_pnp_admm_sms", "qmri_pnp_admm_sms_dev", "qmri_profile_enable", "qmri_profile_get", "qmri_get_health",
    "qmri_debug_lsqr_stamps", "qmri_debug_conv_stamps", "qmri_debug_lsqr_persist", "qmri_debug_dict_filter", "qmri_debug_conv_resident", "qmri_debug_dsvd_gram", "qmri_debug_epg_shift", "qmri_debug_knob", "qmri_debug_mem_stats",
    "qmri_onnx_read_unetres",
    "qmri_lrtv", "qmri_prox_tv", "qmri_norm_tv", "qmri_synthesize_tsmi", "qmri_synthesize_tsmi_complex",
]


class NetDesc(C.Structure):
    _fields_ = [("arch", C.c_int32), ("in_nc", C.c_int32), ("out_nc", C.c_int32), ("nc", C.c_int32 * 4),
                ("nb", C.c_int32), ("residual_noise", C.c_int32)]


class AdmmParams(C.Structure):
    _fields_ = [("gamma", C.c_double), ("iters", C.c_int32), ("cg_tol", C.c_double), ("cg_maxit", C.c_int32),
                ("solver", C.c_int32), ("denoiser_type", C.c_int32), ("noise_std", C.c_double), ("want_diag", C.c_int32)]


class Problem(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("s", C.c_int32), ("T", C.c_int32),
                ("V", C.POINTER(C.c_double)), ("frame_ptr", C.POINTER(C.c_int32)), ("kidx", C.POINTER(C.c_int32)),
                ("net", C.POINTER(NetDesc)), ("weights", C.POINTER(C.c_float)), ("weights_nbytes", C.c_size_t),
                ("K", C.c_int32), ("Q", C.c_int32), ("D", C.POINTER(C.c_float)), ("normD", C.POINTER(C.c_float)),
                ("lut", C.POINTER(C.c_float)), ("admm", AdmmParams), ("slices_per_launch", C.c_int32)]


class CcParams(C.Structure):
    _fields_ = [("nv", C.c_int32), ("energy", C.c_double), ("shared", C.c_int32)]


class CsmParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("cN", C.c_int), ("cM", C.c_int), ("patch", C.c_int), ("window", C.c_int), ("phase_ref", C.c_int), ("thresh", C.c_double)]


class CsmInfo(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("not_converged", C.c_int32)]


class DsvdParams(C.Structure):
    _fields_ = [("s", C.c_int32), ("s_max", C.c_int32), ("energy", C.c_double), ("tol", C.c_double), ("maxit", C.c_int32)]


class DsvdInfo(C.Structure):
    _fields_ = [("s", C.c_int32), ("iters", C.c_int32), ("converged", C.c_int32), ("energy_reached", C.c_int32),
                ("max_resid", C.c_double), ("energy_kept", C.c_double)]


class EpgParams(C.Structure):
    _fields_ = [("nstates", C.c_int32), ("inversion", C.c_int32), ("ti", C.c_double), ("inv_eff", C.c_double), ("out_is_f64", C.c_int32)]


class EpgProfile(C.Structure):
    _fields_ = [("nq", C.c_int32), ("per_frame", C.c_int32), ("prof", C.c_void_p), ("weight", C.c_void_p)]


class EpgGradParams(C.Structure):
    _fields_ = [("nparams", C.c_int32), ("s", C.c_int32), ("V", C.c_void_p), ("reserved", C.c_int32 * 4)]


class EpgBlock(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("prep", C.c_int32), ("wait", C.c_double), ("prep_time", C.c_double), ("prep_eff", C.c_double)]


class EpgSeq(C.Structure):
    _fields_ = [("nblocks", C.c_int32), ("ncycles", C.c_int32), ("blocks", C.POINTER(EpgBlock)), ("reserved", C.c_int32 * 4)]


class NufftParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("reserved", C.c_int32 * 7)]


class DcfParams(C.Structure):
    _fields_ = [("niter", C.c_int32), ("tol", C.c_double), ("reserved", C.c_int32 * 6)]


class DcfInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("dev", C.c_double), ("clamped", C.c_int32), ("split_tiles", C.c_int32), ("reserved", C.c_int32 * 4)]


class OffresParams(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("nbins", C.c_int32), ("tol", C.c_double), ("reserved", C.c_int32 * 4)]


class OffresInfo(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("tol_reached", C.c_int32), ("fit_max", C.c_double), ("fit_rms", C.c_double), ("f_min", C.c_double),
                ("f_max", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double), ("reserved", C.c_int32 * 4)]


class OffresNormalParams(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("tol", C.c_double), ("reserved", C.c_int32 * 4)]


class OffresNormalInfo(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("tol_reached", C.c_int32), ("fit_max", C.c_double), ("fit_rms", C.c_double), ("khat_bytes", C.c_uint64),
                ("reserved", C.c_int32 * 4)]


class FieldmapParams(C.Structure):
    _fields_ = [("iters", C.c_int32), ("beta", C.c_double), ("phase_sign", C.c_int32), ("reserved", C.c_int32 * 4)]


class FieldmapInfo(C.Structure):
    _fields_ = [("cost0", C.c_double), ("cost", C.c_double), ("f_min", C.c_double), ("f_max", C.c_double), ("iters", C.c_int32), ("reserved", C.c_int32),
                ("unwrap_limit_hz", C.c_double)]


class LlrParams(C.Structure):
    _fields_ = [("tau", C.c_double), ("block", C.c_int32), ("shift", C.c_int32), ("reserved", C.c_int32 * 5)]


class WaveletParams(C.Structure):
    _fields_ = [("tau", C.c_double), ("levels", C.c_int32), ("filter", C.c_int32), ("joint", C.c_int32), ("shift", C.c_int32),
                ("reserved", C.c_int32 * 4)]


WAVELET_FILTERS = {"haar": 0, "db2": 1}


class PvInfo(C.Structure):
    _fields_ = [("min_pivot", C.c_double), ("C", C.c_int32), ("s", C.c_int32), ("reserved", C.c_int32 * 4)]


class RefineInfo(C.Structure):
    _fields_ = [("P", C.c_int32), ("K", C.c_int32), ("s", C.c_int32), ("reserved", C.c_int32), ("count", (C.c_int32 * 3) * 3), ("reserved2", C.c_int32 * 3)]


class B1estParams(C.Structure):
    _fields_ = [("half_window", C.c_int32), ("reserved", C.c_int32 * 7)]


class B1estInfo(C.Structure):
    _fields_ = [("n_estimated", C.c_int32), ("n_unmatched", C.c_int32), ("mean_conf", C.c_double), ("reserved", C.c_int32 * 4)]


class LrtvParams(C.Structure):
    _fields_ = [("K", C.c_double), ("iters", C.c_int32), ("step", C.c_double), ("tol", C.c_double), ("backtrack", C.c_int32),
                ("prox_tol", C.c_double), ("prox_maxit", C.c_int32)]


class LrtvInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("halvings", C.c_int32), ("step", C.c_double), ("obj", C.c_double),
                ("prox_calls", C.c_int32), ("prox_iters_total", C.c_int32)]


class Profile(C.Structure):
    _fields_ = [("ms_xupdate", C.c_double), ("ms_denoiser", C.c_double), ("ms_elementwise", C.c_double),
                ("ms_diag", C.c_double), ("ms_match", C.c_double), ("ms_conv3x3", C.c_double),
                ("n_conv3x3", C.c_int64), ("lsqr_iters", C.c_int64), ("admm_iters", C.c_int64),
                ("ms_tv_iter", C.c_double), ("n_tv_iter", C.c_int64),
                ("flop_conv3x3", C.c_double), ("ms_conv2x2", C.c_double), ("n_conv2x2", C.c_int64), ("flop_conv2x2", C.c_double),
                ("ms_lsqr_kernels", C.c_double), ("n_lsqr_launches", C.c_int64), ("ms_net_forward", C.c_double), ("n_net_forward", C.c_int64)]


class Health(C.Structure):
    _fields_ = [("denoiser_scheme", C.c_int32), ("denoiser_fallbacks", C.c_int32), ("resident_armed", C.c_int32), ("resident_timeouts", C.c_int32),
                ("lsqr_one_launch", C.c_int32), ("lsqr_timeouts", C.c_int32), ("repeated_calls", C.c_int32), ("reserved", C.c_int32),
                ("last_call_wall_ms", C.c_double), ("last_call_stage_ms", C.c_double * 4), ("set_denoiser_ms", C.c_double * 3)]


class MemStats(C.Structure):
    _fields_ = [("dev_live", C.c_longlong), ("dev_bytes", C.c_longlong), ("dev_total", C.c_longlong),
                ("pinned_live", C.c_longlong), ("pinned_bytes", C.c_longlong), ("pinned_total", C.c_longlong)]


def build(force: bool = False) -> str:
    """Compile libqmri.so for gfx950 with hipcc (in-tree, next to this file)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h")) or f == "Makefile"]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "qmri.h"))
    stale = force or not os.path.exists(LIB_PATH)
    if not stale:
        t = os.path.getmtime(LIB_PATH)
        stale = any(os.path.getmtime(s) > t for s in srcs)
    if stale:
        subprocess.run(["make", "-C", CSRC, "-s", "-j4"], check=True)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # QMRI_LIBQMRI: another build of the same library (A/B timing of two builds on one box, tools/ab_build.sh); default: in-tree
    path = os.environ.get("QMRI_LIBQMRI") or LIB_PATH
    if path == LIB_PATH and not os.path.exists(LIB_PATH):
        build()
    L = C.CDLL(path)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    if missing:
        raise ImportError(f"libqmri.so lacks symbols declared in include/qmri.h: {missing}")
    vp, ip, dp, fp, i = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int
    L.qmri_abi_version.restype = i
    L.qmri_create.argtypes = [i, C.POINTER(vp)]
    L.qmri_destroy.argtypes = [vp]
    L.qmri_last_error.restype = C.c_char_p
    L.qmri_last_error.argtypes = [vp]
    L.qmri_set_stream.argtypes = [vp, vp]
    L.qmri_synchronize.argtypes = [vp]
    L.qmri_build_spiral.argtypes = [vp, i, i, i, ip, ip, i, C.POINTER(i)]
    L.qmri_build_epi.argtypes = [vp, i, i, C.c_double, i, ip, ip, i, C.POINTER(i)]
    L.qmri_set_operator.argtypes = [vp, i, i, i, i, dp, ip, ip, i]
    L.qmri_build_spiral_traj.argtypes = [vp, i, i, i, ip, dp, i, C.POINTER(i)]
    L.qmri_set_operator_nufft.argtypes = [vp, i, i, i, i, dp, ip, dp, i, C.POINTER(NufftParams)]
    L.qmri_nufft_prepare_normal.argtypes = [vp]
    L.qmri_normal.argtypes = [vp, vp, i, vp]
    L.qmri_normal_dev.argtypes = [vp, vp, vp, i]
    L.qmri_nufft_dcf.argtypes = [vp, C.POINTER(DcfParams), dp, C.POINTER(DcfInfo)]
    L.qmri_set_sample_weights.argtypes = [vp, dp]
    L.qmri_adjoint_w.argtypes = [vp, vp, vp]
    L.qmri_adjoint_w_dev.argtypes = [vp, vp, vp, i]
    L.qmri_adjoint_w_mc.argtypes = [vp, vp, vp]
    L.qmri_set_field_map.argtypes = [vp, dp, dp, C.POINTER(OffresParams), C.POINTER(OffresInfo)]
    L.qmri_nufft_prepare_normal_fm.argtypes = [vp, C.POINTER(OffresNormalParams), C.POINTER(OffresNormalInfo)]
    L.qmri_operator_m.argtypes = [vp, C.POINTER(i)]
    L.qmri_forward.argtypes = [vp, vp, i, vp]
    L.qmri_adjoint.argtypes = [vp, vp, vp]
    L.qmri_forward_f32.argtypes = [vp, fp, i, fp]
    L.qmri_adjoint_f32.argtypes = [vp, fp, fp]
    L.qmri_forward_dev.argtypes = [vp, vp, vp, i]
    L.qmri_adjoint_dev.argtypes = [vp, vp, vp, i]
    L.qmri_set_coils.argtypes = [vp, i, vp]
    L.qmri_forward_mc.argtypes = [vp, vp, i, vp]
    L.qmri_adjoint_mc.argtypes = [vp, vp, vp]
    L.qmri_xupdate_mc.argtypes = [vp, vp, vp, C.c_double, C.c_double, i, vp, vp, ip, ip]
    L.qmri_pnp_admm_mc.argtypes = [vp, vp, C.POINTER(AdmmParams), vp, vp, ip]
    L.qmri_xupdate_mc_batch.argtypes = [vp, i, i, vp, vp, vp, C.c_double, C.c_double, i, vp, vp, ip, ip]
    L.qmri_pnp_admm_mc_batch.argtypes = [vp, i, i, i, vp, vp, C.POINTER(AdmmParams), vp, vp, ip]
    L.qmri_pnp_admm_mc_dev.argtypes = [vp, i, i, vp, vp, C.POINTER(AdmmParams), vp, vp, ip]
    L.qmri_xupdate.argtypes = [vp, vp, vp, C.c_double, C.c_double, i, i, vp, ip, ip]
    L.qmri_net_nparams.restype = C.c_size_t
    L.qmri_net_nparams.argtypes = [C.POINTER(NetDesc)]
    L.qmri_set_denoiser.argtypes = [vp, C.POINTER(NetDesc), fp, C.c_size_t, i, i, i]
    L.qmri_denoise.argtypes = [vp, dp, i, i, i, i, dp]
    L.qmri_onnx_read_unetres.argtypes = [C.c_char_p, C.POINTER(NetDesc), fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.qmri_net_forward_dev.argtypes = [vp, vp, i, vp]
    L.qmri_denoiser_scheme.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.qmri_get_health.argtypes = [vp, C.POINTER(Health)]
    L.qmri_pnp_admm.argtypes = [vp, vp, C.POINTER(AdmmParams), vp, vp, vp, dp, ip]
    L.qmri_pnp_admm_dev.argtypes = [vp, i, vp, C.POINTER(AdmmParams), vp, vp, vp, dp, ip]
    L.qmri_pnp_admm_batch.argtypes = [vp, i, i, vp, C.POINTER(AdmmParams), vp, vp, vp, dp, ip]
    L.qmri_lrtv.argtypes = [vp, vp, C.POINTER(LrtvParams), vp, C.POINTER(LrtvInfo)]
    L.qmri_prox_tv.argtypes = [vp, dp, i, i, C.c_double, C.c_double, i, dp, ip, dp]
    L.qmri_norm_tv.argtypes = [vp, dp, i, i, dp]
    L.qmri_synthesize_tsmi.argtypes = [vp, dp, i, fp, ip]
    L.qmri_synthesize_tsmi_complex.argtypes = [vp, dp, dp, i, fp, ip]
    L.qmri_set_dictionary.argtypes = [vp, i, i, i, fp, fp, fp]
    L.qmri_dict_match.argtypes = [vp, vp, i, fp, fp, fp, ip]
    L.qmri_dict_match_dev.argtypes = [vp, vp, i, vp, vp, vp, vp]
    L.qmri_dict_match_xfit.argtypes = [vp, vp, i, fp, fp, fp, ip, fp]
    L.qmri_dict_match_xfit_dev.argtypes = [vp, vp, i, vp, vp, vp, vp, vp]
    L.qmri_set_dictionary_groups.argtypes = [vp, i, ip, dp]
    L.qmri_dict_group_assign.argtypes = [i, dp, i, dp, ip]
    L.qmri_dict_match_grouped.argtypes = [vp, vp, i, dp, fp, fp, fp, ip, ip, fp]
    L.qmri_dict_match_grouped_dev.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp]
    L.qmri_dict_group_scores.argtypes = [vp, vp, i, fp]
    L.qmri_dict_group_scores_dev.argtypes = [vp, vp, i, vp]
    L.qmri_b1_pool.argtypes = [vp, i, dp, i, i, i, fp, vp, i, dp, ip, dp]
    L.qmri_b1_pool_dev.argtypes = [vp, i, dp, i, i, i, vp, vp, i, vp, vp, vp]
    L.qmri_b1_estimate.argtypes = [vp, vp, i, i, i, vp, C.POINTER(B1estParams), dp, ip, dp, C.POINTER(B1estInfo)]
    L.qmri_b1_estimate_dev.argtypes = [vp, vp, i, i, i, vp, C.POINTER(B1estParams), vp, vp, vp, C.POINTER(B1estInfo)]
    L.qmri_set_components.argtypes = [vp, i, ip, C.POINTER(PvInfo)]
    L.qmri_dict_unmix.argtypes = [vp, vp, i, i, dp, dp, dp, dp, ip]
    L.qmri_dict_unmix_dev.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp]
    L.qmri_dict_lines.argtypes = [i, i, fp, fp, i, ip, ip, ip]
    L.qmri_set_refine.argtypes = [vp, i, ip, C.POINTER(RefineInfo)]
    L.qmri_dict_refine.argtypes = [vp, vp, i, ip, dp, dp, dp, dp, ip, ip]
    L.qmri_dict_refine_dev.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp]
    L.qmri_recon_batch.argtypes = [i, C.POINTER(i), i, C.POINTER(Problem), vp, vp, fp, fp, C.c_char_p, C.c_size_t]
    L.qmri_recon_batch_mc.argtypes = [i, C.POINTER(i), i, C.POINTER(Problem), i, vp, vp, vp, fp, fp, C.c_char_p, C.c_size_t]
    L.qmri_recon_batch_mc_cc.argtypes = [i, C.POINTER(i), i, C.POINTER(Problem), i, vp, vp, vp, fp, fp, C.c_char_p, C.c_size_t, vp, C.POINTER(CcParams)]
    L.qmri_coil_compress.argtypes = [vp, i, i, vp, vp, vp, C.POINTER(CcParams), C.POINTER(i), vp, vp, vp, dp]
    L.qmri_coil_compress_dev.argtypes = [vp, i, i, vp, vp, vp, C.POINTER(CcParams), C.POINTER(i), vp, vp, vp, dp]
    L.qmri_coil_maps.argtypes = [vp, i, i, i, i, vp, C.POINTER(CsmParams), vp, vp, vp, C.POINTER(CsmInfo)]
    L.qmri_coil_maps_dev.argtypes = [vp, i, i, i, i, vp, C.POINTER(CsmParams), vp, vp, vp, C.POINTER(CsmInfo)]
    L.qmri_coil_eig.argtypes = [i, vp, dp, vp]
    L.qmri_dict_compress.argtypes = [vp, i, i, vp, i, C.POINTER(DsvdParams), C.POINTER(i), vp, vp, vp, vp, C.POINTER(DsvdInfo)]
    L.qmri_dict_compress_dev.argtypes = [vp, i, i, vp, i, C.POINTER(DsvdParams), C.POINTER(i), vp, vp, vp, vp, C.POINTER(DsvdInfo)]
    L.qmri_debug_dsvd_gram.argtypes = [vp, i, i, vp, i, i, vp]
    L.qmri_dict_simulate.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), vp]
    L.qmri_dict_simulate_dev.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), vp]
    L.qmri_dict_simulate_sp.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), C.POINTER(EpgProfile), vp]
    L.qmri_dict_simulate_sp_dev.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), C.POINTER(EpgProfile), vp]
    L.qmri_dict_simulate_grad.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), C.POINTER(EpgGradParams), vp, vp, vp, vp]
    L.qmri_dict_simulate_grad_dev.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), C.POINTER(EpgGradParams), vp, vp, vp, vp]
    L.qmri_dict_simulate_seq.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), C.POINTER(EpgSeq), vp]
    L.qmri_dict_simulate_seq_dev.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(EpgParams), C.POINTER(EpgSeq), vp]
    L.qmri_debug_epg_shift.argtypes = [vp, i, i, vp, vp]
    L.qmri_field_map_estimate.argtypes = [vp, i, i, i, i, i, vp, dp, vp, C.POINTER(FieldmapParams), vp, vp, C.POINTER(FieldmapInfo)]
    L.qmri_field_map_estimate_dev.argtypes = [vp, i, i, i, i, i, vp, dp, vp, C.POINTER(FieldmapParams), vp, vp, C.POINTER(FieldmapInfo)]
    L.qmri_llr_prox.argtypes = [vp, i, i, i, i, vp, i, C.POINTER(LlrParams), i, i, vp, dp]
    L.qmri_llr_prox_dev.argtypes = [vp, i, i, i, i, vp, i, C.POINTER(LlrParams), i, i, vp, dp]
    L.qmri_set_llr.argtypes = [vp, C.POINTER(LlrParams)]
    L.qmri_wavelet_prox.argtypes = [vp, i, i, i, i, vp, i, C.POINTER(WaveletParams), i, i, vp, dp]
    L.qmri_wavelet_prox_dev.argtypes = [vp, i, i, i, i, vp, i, C.POINTER(WaveletParams), i, i, vp, dp]
    L.qmri_set_wavelet.argtypes = [vp, C.POINTER(WaveletParams)]
    L.qmri_set_sms.argtypes = [vp, i, vp]
    L.qmri_forward_sms.argtypes = [vp, i, i, vp, vp, i, vp]
    L.qmri_adjoint_sms.argtypes = [vp, i, i, vp, vp, vp]
    L.qmri_xupdate_sms.argtypes = [vp, i, i, vp, vp, vp, C.c_double, C.c_double, i, vp, vp, ip, ip]
    L.qmri_pnp_admm_sms.argtypes = [vp, i, i, i, vp, vp, C.POINTER(AdmmParams), vp, vp, ip]
    L.qmri_pnp_admm_sms_dev.argtypes = [vp, i, i, vp, vp, C.POINTER(AdmmParams), vp, vp, ip]
    L.qmri_debug_knob.argtypes = [C.c_char_p, i]
    L.qmri_debug_mem_stats.argtypes = [C.POINTER(MemStats)]
    L.qmri_profile_enable.argtypes = [vp, i]
    L.qmri_profile_get.argtypes = [vp, C.POINTER(Profile), i]
    if L.qmri_abi_version() != 1:
        raise ImportError("libqmri.so ABI version mismatch")
    _lib = L
    return L
