"""numpy-facing wrapper of one libqmri context (include/qmri.h).

Arrays follow MATLAB conventions: `X[h, w, c]` (any memory order; copied into column-major interleaved-complex
buffers at the boundary), measurement vectors frame-major.  Every failure raises `QmriError` carrying the
library's message -- the Python analogue of the MATLAB exceptions the reference's plugins throw.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import AdmmParams, CcParams, CsmInfo, CsmParams, DcfInfo, DcfParams, DsvdInfo, DsvdParams, EpgBlock, EpgGradParams, EpgParams, EpgProfile, EpgSeq, FieldmapInfo, FieldmapParams, LlrParams, LrtvInfo, LrtvParams, NetDesc, NufftParams, OffresInfo, OffresNormalInfo, OffresNormalParams, OffresParams, Profile, WAVELET_FILTERS, WaveletParams

ARCH_UNETRES, ARCH_SEQ_CONV = 0, 1
SOLVER_LSQR, SOLVER_DIRECT = 0, 1


DENOISER_COMPLEX = 2      # include/qmri.h QMRI_DENOISER_COMPLEX


def denoiser_type(multi_level=False, tsmi_domain="real"):
    """qmri_admm_params.denoiser_type: bit 0 multi_level, bit 1 complex TSMIs.  tsmi_domain "real" is the reference's denoiser step
    (v = real(x + uold)); "complex" feeds the network cat(3, real(x + uold), imag(x + uold)), 2s (+1) -> 2s channels."""
    if tsmi_domain not in ("real", "complex"):
        raise ValueError(f'tsmi_domain must be "real" or "complex", not {tsmi_domain!r}')
    return int(bool(multi_level)) | (DENOISER_COMPLEX if tsmi_domain == "complex" else 0)


SOLVER_TOEPLITZ = 2       # include/qmri.h QMRI_SOLVER_TOEPLITZ


def solver_code(solver):
    """qmri_admm_params.solver: "lsqr" the reference's, "toeplitz" CG on the Toeplitz normal operator of a trajectory;
    any other string is the DIRECT solver, as before."""
    return SOLVER_LSQR if solver == "lsqr" else SOLVER_TOEPLITZ if solver == "toeplitz" else SOLVER_DIRECT


class QmriError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libqmri error {code}: {msg}")
        self.code = code


def _mc_solver(solver):
    if solver not in ("lsqr", "toeplitz"):
        raise ValueError('the multi-coil reconstruction takes solver="lsqr" or "toeplitz"')
    return solver_code(solver)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _cbuf(a):
    """complex array -> 1-D complex128 in column-major (MATLAB) element order."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.complex128).ravel(order="F"))


def real_dictionary_array(a, name: str, dtype):
    """`dict.D` / `dict.V` as the real array the kernels take.  MATLAB may hold them complex-typed (the reference takes
    real(dict.V), main_recon_tsmis_FFT.m:129, and real(dict.D(...)), main_synthesize_tsmis.m:89, explicitly, while
    mrf_dtm_cpu.m:91 multiplies by dict.D as stored): a complex-typed array whose imaginary part is zero is accepted, one
    with a non-zero imaginary part is refused -- it is never silently truncated."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        if np.any(a.imag != 0):
            raise ValueError(f"{name} is complex with a non-zero imaginary part: the dictionary match implements real atoms "
                             f"(dict.D real, as in the reference's real_fisp dictionaries); pass real({name}) if that is what is meant")
        a = a.real
    return np.asarray(a, dtype=dtype)


def simulation_arguments(alpha, tr, te, t1, t2, b1, nstates, inversion, ti, inv_eff, dtype):
    """The arguments of Engine.simulate_dictionary as the library takes them: (alpha [T], tr [T], te [T], t1 [K], t2 [K], b1 [K] or None, EpgParams),
    contiguous float64.  A scalar tr or te is broadcast to T; t1, t2 and b1 are broadcast against each other and flattened."""
    a = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).ravel())
    T = a.size
    if not (1 <= T <= 1024):
        raise ValueError("alpha must hold 1 <= T <= 1024 flip angles")
    sched = []
    for name, v in (("tr", tr), ("te", te)):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.size != T):
            raise ValueError(f"{name} must be a scalar or hold one value per frame ({T})")
        sched.append(np.ascontiguousarray(np.broadcast_to(v, (T,))))
    if np.iscomplexobj(t1) or np.iscomplexobj(t2) or np.iscomplexobj(b1) or np.iscomplexobj(alpha):
        raise ValueError("alpha, t1, t2 and b1 must be real")
    atoms = [np.asarray(t1, dtype=np.float64), np.asarray(t2, dtype=np.float64)] + ([np.asarray(b1, dtype=np.float64)] if b1 is not None else [])
    atoms = [np.ascontiguousarray(x.ravel()) for x in np.broadcast_arrays(*atoms)]
    if atoms[0].size < 1:
        raise ValueError("t1 and t2 must hold at least one atom")
    if int(nstates) != nstates or not (1 <= int(nstates) <= 256):
        raise ValueError("nstates must be an integer in 1..256")
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype must be float64 or float32")
    if inversion and (not (float(ti) >= 0.0 and np.isfinite(ti)) or not (0.0 < float(inv_eff) <= 1.0)):
        raise ValueError("ti must be >= 0 and inv_eff in (0, 1]")
    p = EpgParams(int(nstates), 1 if inversion else 0, float(ti), float(inv_eff), int(np.dtype(dtype) == np.dtype(np.float64)))
    return a, sched[0], sched[1], atoms[0], atoms[1], atoms[2] if b1 is not None else None, p


def slice_profile_arguments(slice_profile, slice_weights, T):
    """The slice profile of Engine.simulate_dictionary as the library takes it: (prof buffer, weight buffer, EpgProfile), or None without one.
    slice_profile is [Q] (the same flip-angle scale in every frame) or [T, Q] (one row per frame), 1 <= Q <= 64; slice_weights is [Q] and
    defaults to 1 / Q.  Every entry is finite and >= 0 and the weights sum to more than 0; they are not normalised.  The two buffers must outlive
    the call that takes the EpgProfile."""
    if slice_profile is None:
        if slice_weights is not None:
            raise ValueError("slice_weights needs a slice_profile")
        return None
    if np.iscomplexobj(slice_profile) or np.iscomplexobj(slice_weights):
        raise ValueError("slice_profile and slice_weights must be real")
    prof = np.asarray(slice_profile, dtype=np.float64)
    if prof.ndim not in (1, 2) or (prof.ndim == 2 and prof.shape[0] != T):
        raise ValueError(f"slice_profile must have shape [Q] or [T, Q] with T = {T}")
    prof = np.ascontiguousarray(prof)
    Q = prof.shape[-1]
    if not (1 <= Q <= 64):
        raise ValueError("slice_profile must hold 1 <= Q <= 64 sub-slices")
    w = np.full(Q, 1.0 / Q) if slice_weights is None else np.ascontiguousarray(np.asarray(slice_weights, dtype=np.float64))
    if w.shape != (Q,):
        raise ValueError(f"slice_weights must have shape [Q] = [{Q}]")
    if not (np.all(np.isfinite(prof)) and np.all(prof >= 0) and np.all(np.isfinite(w)) and np.all(w >= 0) and w.sum() > 0):
        raise ValueError("slice_profile and slice_weights must be finite and >= 0, and the weights must sum to more than 0")
    return prof, w, EpgProfile(Q, int(prof.ndim == 2), prof.ctypes.data, w.ctypes.data)


def grad_arguments(wrt, V, outputs, T):
    """The derivative arguments of Engine.simulate_dictionary_grad as the library takes them: (V buffer or None, EpgGradParams, outputs as a set).
    wrt is ("t1", "t2") or ("t1", "t2", "b1"); V is None or a real [T, s] subspace with 1 <= s <= 16 (the V of compress_dictionary), finite;
    outputs is a non-empty subset of ("F", "dF", "crb").  The buffer must outlive the call that takes the EpgGradParams."""
    wrt = tuple(wrt)
    if wrt not in (("t1", "t2"), ("t1", "t2", "b1")):
        raise ValueError('wrt must be ("t1", "t2") or ("t1", "t2", "b1")')
    outs = {outputs} if isinstance(outputs, str) else set(outputs)
    if not outs or not outs <= {"F", "dF", "crb"}:
        raise ValueError('outputs must be a non-empty subset of ("F", "dF", "crb")')
    if V is None:
        return None, EpgGradParams(len(wrt), 0, None), outs
    if np.iscomplexobj(V):
        raise ValueError("V must be real")
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2 or V.shape[0] != T or not (1 <= V.shape[1] <= 16):
        raise ValueError(f"V must have shape [T, s] with T = {T} and 1 <= s <= 16")
    if not np.all(np.isfinite(V)):
        raise ValueError("V must be finite")
    Vb = np.ascontiguousarray(V.ravel(order="F"))
    return Vb, EpgGradParams(len(wrt), V.shape[1], Vb.ctypes.data), outs


EPG_PREPS = {"none": 0, "inversion": 1, "t2": 2}


def sequence_arguments(blocks, ncycles, T):
    """The schedule of Engine.simulate_dictionary_seq as the library takes it: (EpgBlock array, EpgSeq).  blocks is a sequence of
    dict(nframes=, prep="none" | "inversion" | "t2", wait=0.0, prep_time=0.0, prep_eff=1.0), 1..64 of them, whose nframes sum to T; ncycles is an
    integer in 1..16.  The ranges of the numbers are the library's to refuse (include/qmri.h qmri_dict_simulate_seq).  The array must outlive the
    call that takes the EpgSeq."""
    blocks = list(blocks)
    if not (1 <= len(blocks) <= 64):
        raise ValueError("blocks must hold 1..64 blocks")
    if int(ncycles) != ncycles or not (1 <= int(ncycles) <= 16):
        raise ValueError("ncycles must be an integer in 1..16")
    arr = (EpgBlock * len(blocks))()
    for i, b in enumerate(blocks):
        extra = set(b) - {"nframes", "prep", "wait", "prep_time", "prep_eff"}
        if extra or "nframes" not in b:
            raise ValueError(f"block {i} must be a dict with nframes and optionally prep, wait, prep_time, prep_eff" + (f", not {sorted(extra)}" if extra else ""))
        prep = b.get("prep", "none")
        if prep not in EPG_PREPS:
            raise ValueError(f'block {i}: prep must be "none", "inversion" or "t2"')
        if int(b["nframes"]) != b["nframes"] or int(b["nframes"]) < 1:
            raise ValueError(f"block {i}: nframes must be an integer >= 1")
        arr[i] = EpgBlock(int(b["nframes"]), EPG_PREPS[prep], float(b.get("wait", 0.0)), float(b.get("prep_time", 0.0)), float(b.get("prep_eff", 1.0)))
    if sum(a.nframes for a in arr) != T:
        raise ValueError(f"the nframes of the blocks must sum to the T = {T} frames of alpha")
    return arr, EpgSeq(len(blocks), int(ncycles), arr)


def fieldmap_arguments(Y, echo_times, iters=0, beta=0.0, phase_sign=-1, f_init=None):
    """The arguments of Engine.estimate_field_map as the library takes them: (Y buffer [S][L][C][n1 + N n2] complex128, t [L] float64, f_init buffer
    or None, FieldmapParams, (S, L, C, N, M), stacked).  Y is [L, N, M], [L, C, N, M] or [S, L, C, N, M]; stacked says whether it carried a slice axis
    (the results then keep it).  f_init is [N, M], or [S, N, M] for a stack."""
    Y = np.asarray(Y)
    if Y.ndim not in (3, 4, 5):
        raise ValueError(f"Y must be [L, N, M], [L, C, N, M] or [S, L, C, N, M], not {Y.ndim}-dimensional")
    stacked = Y.ndim == 5
    Y5 = Y[None, :, None] if Y.ndim == 3 else Y[None] if Y.ndim == 4 else Y
    S, L, Cc, N, M = Y5.shape
    t = np.asarray(echo_times)
    if np.iscomplexobj(t):
        raise ValueError("the echo times must be real (seconds)")
    t = np.ascontiguousarray(t, dtype=np.float64).ravel()
    if t.size != L:
        raise ValueError(f"echo_times must hold one time per echo ({L}), not {t.size}")
    if not (2 <= L <= 8):
        raise ValueError("the estimate takes 2 <= L <= 8 echoes")
    if S < 1 or Cc < 1 or N < 2 or M < 2:
        raise ValueError("Y needs at least one slice and coil and a grid of at least 2 x 2")
    if not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
        raise ValueError("echo_times must be finite and strictly increasing")
    if int(iters) != iters or not (0 <= int(iters) <= 100000):
        raise ValueError("iters must be an integer in 1..100000 (0: the default 200)")
    if not (np.isfinite(beta) and beta >= 0):
        raise ValueError("beta must be finite and >= 0 (0: the default 0.01)")
    if phase_sign not in (-1, 0, 1):
        raise ValueError("phase_sign must be -1 or +1")
    Yb = np.ascontiguousarray(np.swapaxes(np.asarray(Y5, dtype=np.complex128), 3, 4))       # [S][L][C][n2][n1]: n1 fastest
    fb = None
    if f_init is not None:
        f = np.asarray(f_init)
        if np.iscomplexobj(f):
            raise ValueError("f_init must be real (Hz)")
        if f.shape != ((S, N, M) if stacked else (N, M)):
            raise ValueError(f"f_init must be {'[S, N, M]' if stacked else '[N, M]'} = {(S, N, M) if stacked else (N, M)}, not {f.shape}")
        fb = np.ascontiguousarray(np.swapaxes(np.asarray(f, dtype=np.float64).reshape(S, N, M), 1, 2))
    return Yb, t, fb, FieldmapParams(int(iters), float(beta), int(phase_sign)), (S, L, Cc, N, M), stacked


def fieldmap_info(info):
    return {"cost0": float(info.cost0), "cost": float(info.cost), "f_min": float(info.f_min), "f_max": float(info.f_max), "iters": int(info.iters),
            "unwrap_limit_hz": float(info.unwrap_limit_hz)}


def group_arguments(group_ptr, group_val):
    """(group_ptr [G + 1] int32, group_val [G] float64) as qmri_set_dictionary_groups takes them; the library checks their contents."""
    gp, gv = np.asarray(group_ptr), np.asarray(group_val, dtype=np.float64)
    if gp.ndim != 1 or gv.ndim != 1 or gp.size != gv.size + 1 or gv.size < 1 or not np.issubdtype(gp.dtype, np.integer):
        raise ValueError("group_ptr must be G + 1 integers and group_val G values, G >= 1")
    return np.ascontiguousarray(gp, dtype=np.int32), np.ascontiguousarray(gv)


def component_arguments(atoms, K=None):
    """atoms [C] int32 (1-based) as qmri_set_components takes them: 1 <= C <= 8 integers, distinct, and inside 1..K when K is known; the library
    checks the atoms themselves."""
    a = np.asarray(atoms)
    if a.ndim != 1 or not (1 <= a.size <= 8) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("atoms must be 1 to 8 integer atom indices (1-based)")
    if len(set(a.tolist())) != a.size:
        raise ValueError("atoms must be distinct")
    if a.min() < 1 or (K is not None and a.max() > K):
        raise ValueError("atoms are 1-based indices" + ("" if K is None else f" into the dictionary's {K} atoms"))
    return np.ascontiguousarray(a, dtype=np.int32)


def unmix_mode(mode):
    """"real" / "phase" -> QMRI_PV_REAL / QMRI_PV_PHASE."""
    if mode not in ("real", "phase"):
        raise ValueError(f'mode must be "real" or "phase", not {mode!r}')
    return 0 if mode == "real" else 1


def b1_window(window):
    """The half window h of the B1 estimate as an int, 0 <= h <= 32 (the window is (2h + 1) x (2h + 1) pixels)."""
    if isinstance(window, bool) or not isinstance(window, (int, float, np.integer, np.floating)) or int(window) != window or not (0 <= int(window) <= 32):
        raise ValueError(f"window must be an integer half window in 0..32, not {window!r}")
    return int(window)


def b1_pool_arguments(score, group_val, mask=None):
    """(score [G, npix] float32 C-contiguous, group_val [G] float64, mask [npix] uint8 or None, (N, M, nslices)) as qmri_b1_pool takes them.
    score is [G, N, M] or [G, N, M, nslices], pixel i + N j of a slice (the first image axis contiguous); mask has the image's shape.  The
    library checks group_val's contents."""
    sc = np.asarray(score)
    gv = np.asarray(group_val, dtype=np.float64)
    if sc.ndim not in (3, 4) or gv.ndim != 1 or gv.size != sc.shape[0] or gv.size < 1:
        raise ValueError("score must be [G, N, M] or [G, N, M, nslices] with one group_val per group, G >= 1")
    if np.iscomplexobj(sc):
        raise ValueError("score must be real")
    lead = sc.shape[1:]
    if min(lead) < 1:
        raise ValueError("score must have at least one pixel")
    N, M, nsl = lead[0], lead[1], (lead[2] if len(lead) == 3 else 1)
    sb = np.ascontiguousarray(np.asarray(sc, dtype=np.float32).reshape((gv.size, -1), order="F"))
    mb = None
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != lead:
            raise ValueError(f"mask must have the image's shape {lead}, not {m.shape}")
        mb = np.ascontiguousarray((m != 0).ravel(order="F").astype(np.uint8))
    return sb, np.ascontiguousarray(gv), mb, (int(N), int(M), int(nsl))


def dict_group_assign(group_val, sel):
    """The group of each selector value as the grouped dictionary match assigns it (qmri_dict_group_assign, host only): the lowest g minimising
    |sel - group_val[g]| in float64, 1-based; 0 for a non-finite value (unmatched).  Returns int32 in the shape of sel."""
    from . import _lib
    gv = np.ascontiguousarray(group_val, dtype=np.float64).ravel()
    b = np.ascontiguousarray(sel, dtype=np.float64)
    out = np.zeros(b.size, np.int32)
    st = _lib.lib().qmri_dict_group_assign(gv.size, gv.ctypes.data_as(C.POINTER(C.c_double)), b.size, b.ravel().ctypes.data_as(C.POINTER(C.c_double)),
                                           out.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != 0:
        raise QmriError(st, _lib.lib().qmri_last_error(None).decode())
    return out.reshape(b.shape)


def refine_columns(cols, Q=None):
    """cols [P] int32 as qmri_set_refine takes them: 1 <= P <= 3 distinct lut columns (0-based), inside 0..Q-1 when Q is known."""
    c = np.asarray(cols)
    if c.ndim != 1 or not (1 <= c.size <= 3) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("cols must be 1 to 3 integer lut columns (0-based)")
    if len(set(c.tolist())) != c.size:
        raise ValueError("cols must be distinct")
    if c.min() < 0 or (Q is not None and c.max() >= Q):
        raise ValueError("cols are 0-based lut columns" + ("" if Q is None else f" of the dictionary's {Q}"))
    return np.ascontiguousarray(c, dtype=np.int32)


def dict_lines(lut, normD, cols=(0, 1)):
    """The lines of a gridded dictionary (qmri_dict_lines, host only): for every atom and every column of cols its lower and
    upper neighbour along that column, all other lut columns equal.  lut [K, Q], normD [K] -> (nbr [K, P, 2] int32, 0-based, -1 = none;
    count [P, 3] = atoms with 0, 1 and 2 neighbours per column)."""
    from . import _lib
    lut = np.asarray(lut, dtype=np.float32)
    nd = np.ascontiguousarray(normD, dtype=np.float32).ravel()
    if lut.ndim != 2 or lut.shape[0] < 1 or lut.shape[1] < 1 or nd.size != lut.shape[0]:
        raise ValueError("lut must be [K, Q] with one normD per atom")
    K, Q = lut.shape
    c = refine_columns(cols, Q)
    lf = np.ascontiguousarray(lut.ravel(order="F"))
    nbr = np.empty((K, c.size, 2), np.int32)
    count = np.zeros((c.size, 3), np.int32)
    f, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    st = _lib.lib().qmri_dict_lines(K, Q, lf.ctypes.data_as(f), nd.ctypes.data_as(f), c.size, c.ctypes.data_as(ip), nbr.ctypes.data_as(ip),
                                    count.ctypes.data_as(ip))
    if st != 0:
        raise QmriError(st, _lib.lib().qmri_last_error(None).decode())
    return nbr, count


REFINE_FLAGS = {"skipped": 1, "moved": 2, "bound": 4, "cap": 8, "stalled": 16, "degenerate": 32}


def nearest_atoms(lut, points):
    """The 1-based row of lut [K, >= 2] whose (T1, T2) is nearest each row of points [n, 2]: squared distance in float64, the first minimum wins."""
    lut = np.asarray(lut, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64)
    if lut.ndim != 2 or lut.shape[1] < 2 or pts.ndim != 2 or pts.shape[1] != 2 or not np.all(np.isfinite(pts)):
        raise ValueError("points must be [n, 2] finite (T1, T2) pairs and the lut [K, >= 2]")
    d = (lut[None, :, 0] - pts[:, None, 0]) ** 2 + (lut[None, :, 1] - pts[:, None, 1]) ** 2
    return (np.argmin(d, axis=1) + 1).astype(np.int32)


def caipi_phases(T: int, Z: int):
    """E [T, Z] of a simultaneous multi-slice acquisition with a CAIPIRINHA-style RF phase cycle: E[t, b] = exp(2 pi i b (t mod Z) / Z)."""
    T, Z = int(T), int(Z)
    if T < 1 or not (1 <= Z <= 8):
        raise ValueError("T >= 1 and 1 <= Z <= 8 required")
    t, b = np.meshgrid(np.arange(T) % Z, np.arange(Z), indexing="ij")
    return np.exp(2j * np.pi * b * t / Z)


def _hip_runtime():
    """The HIP runtime through ctypes, for the few calls that keep an intermediate result on the device between two library calls."""
    import os
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def build_spiral(N: int, S: int, T: int):
    """setup_subsampling_spiralgrided.m:7-34 -> (frame_ptr[T+1], kidx[m]) int32 (0-based column-major k)."""
    L = _lib.lib()
    fp = np.zeros(T + 1, np.int32)
    k = np.zeros(S * T, np.int32)
    m = C.c_int(0)
    st = L.qmri_build_spiral(None, N, S, T, fp.ctypes.data_as(C.POINTER(C.c_int32)), k.ctypes.data_as(C.POINTER(C.c_int32)), k.size, C.byref(m))
    if st != 0:
        raise QmriError(st, L.qmri_last_error(None).decode())
    return fp, k[: m.value].copy()


def build_epi(N: int, M: int, percentage: float, T: int):
    """setup_subsampling_epi.m:20-33 -> (frame_ptr[T+1], kidx[m])."""
    L = _lib.lib()
    step = int(np.floor(1.0 / percentage + 0.5))
    cap = max((N // step) * M * T, 1)
    fp = np.zeros(T + 1, np.int32)
    k = np.zeros(cap, np.int32)
    m = C.c_int(0)
    st = L.qmri_build_epi(None, N, M, float(percentage), T, fp.ctypes.data_as(C.POINTER(C.c_int32)), k.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(m))
    if st != 0:
        raise QmriError(st, L.qmri_last_error(None).decode())
    return fp, k[: m.value].copy()


def build_spiral_traj(N: int, S: int, T: int):
    """The spiral of setup_subsampling_spiralgrided.m:7-27 before rounding -> (frame_ptr[T+1] int32, omega[m, 2] float64 radians per pixel),
    m = S * T, frame-major; omega[:, 0] runs along N (the first index), omega[:, 1] along M."""
    L = _lib.lib()
    fp = np.zeros(T + 1, np.int32)
    om = np.zeros((S * T, 2), np.float64)
    m = C.c_int(0)
    st = L.qmri_build_spiral_traj(None, int(N), int(S), int(T), fp.ctypes.data_as(C.POINTER(C.c_int32)), om.ctypes.data_as(C.POINTER(C.c_double)),
                                  om.shape[0], C.byref(m))
    if st != 0:
        raise QmriError(st, L.qmri_last_error(None).decode())
    return fp, om[: m.value].copy()


def spiral_readout_times(S: int, T: int, readout_s: float):
    """Readout times of build_spiral_traj's samples for set_field_map: sample j of every frame is measured at tau = j * readout_s / S seconds after
    the frame's excitation -> t_s [S * T] float64, frame-major as y."""
    if int(S) != S or int(T) != T or S < 1 or T < 1:
        raise ValueError("S and T must be positive integers")
    if not (np.isfinite(readout_s) and readout_s >= 0):
        raise ValueError("readout_s must be finite and >= 0 (seconds)")
    return np.tile(np.arange(int(S), dtype=np.float64) * (float(readout_s) / int(S)), int(T))


def read_onnx_unetres(path):
    """Weights of the ONNX file main_recon_tsmis_FFT.m:138 imports, through the library's own reader
    (qmri_onnx_read_unetres) -> (flat fp32 weights, dict(in_nc, out_nc, nc, nb))."""
    L = _lib.lib()
    d, n = NetDesc(), C.c_size_t(0)
    st = L.qmri_onnx_read_unetres(str(path).encode(), C.byref(d), None, 0, C.byref(n))
    if st != 0:
        raise QmriError(st, L.qmri_last_error(None).decode())
    w = np.empty(n.value, np.float32)
    st = L.qmri_onnx_read_unetres(str(path).encode(), C.byref(d), w.ctypes.data_as(C.POINTER(C.c_float)), w.size, C.byref(n))
    if st != 0:
        raise QmriError(st, L.qmri_last_error(None).decode())
    return w, {"in_nc": int(d.in_nc), "out_nc": int(d.out_nc), "nc": tuple(int(v) for v in d.nc), "nb": int(d.nb)}


class Engine:
    """One device context: operator + denoiser + dictionary + workspaces."""

    def __init__(self, device: int = 0):
        self.L = _lib.lib()
        h = C.c_void_p()
        st = self.L.qmri_create(int(device), C.byref(h))
        if st != 0:
            raise QmriError(st, self.L.qmri_last_error(None).decode())
        self.h = h
        self.device = device
        self.N = self.M = self.s = self.T = self.m = 0
        self.net_desc = None
        self.dict_shape = None
        self.components = None
        self.refine_cols = None

    def close(self):
        if getattr(self, "h", None):
            self.L.qmri_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise QmriError(st, self.L.qmri_last_error(self.h).decode())

    # -- stream / sync ---------------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr: int | None):
        self._check(self.L.qmri_set_stream(self.h, C.c_void_p(hip_stream_ptr) if hip_stream_ptr else None))

    def synchronize(self):
        self._check(self.L.qmri_synchronize(self.h))

    # -- operator ----------------------------------------------------------------------------------
    def set_operator(self, N, M, V, frame_ptr, kidx, max_batch=1):
        V = real_dictionary_array(V, "V", np.float64)
        if V.ndim != 2:
            raise ValueError("V must be T x s")
        T, s = V.shape
        Vf = np.ascontiguousarray(V.ravel(order="F"))
        fp = np.ascontiguousarray(frame_ptr, dtype=np.int32)
        k = np.ascontiguousarray(kidx, dtype=np.int32)
        self._check(self.L.qmri_set_operator(self.h, int(N), int(M), int(s), int(T), Vf.ctypes.data_as(C.POINTER(C.c_double)),
                                             fp.ctypes.data_as(C.POINTER(C.c_int32)), k.ctypes.data_as(C.POINTER(C.c_int32)), int(max_batch)))
        self.N, self.M, self.s, self.T, self.m = int(N), int(M), int(s), int(T), int(fp[-1])
        self.sms_Z = 0                     # (the library drops the simultaneous multi-slice phases with the operator)

    def set_trajectory(self, N, M, V, frame_ptr, omega, max_batch=1, width=0):
        """A non-Cartesian operator (qmri_set_operator_nufft): omega is m x 2 radians per pixel in [-pi, pi] (column 0 along N, column 1 along M),
        frame-major as y; width = NUFFT kernel width (0: the default).  forward / adjoint / pnp_admm / the _mc methods then run on it."""
        V = real_dictionary_array(V, "V", np.float64)
        if V.ndim != 2:
            raise ValueError("V must be T x s")
        T, s = V.shape
        Vf = np.ascontiguousarray(V.ravel(order="F"))
        fp = np.ascontiguousarray(frame_ptr, dtype=np.int32)
        om = np.ascontiguousarray(omega, dtype=np.float64)
        if fp.ndim != 1 or fp.size != T + 1:
            raise ValueError(f"frame_ptr must have T + 1 = {T + 1} entries")
        if om.ndim != 2 or om.shape[1] != 2 or om.shape[0] != int(fp[-1]):
            raise ValueError(f"omega must be m x 2 with m = frame_ptr[-1] = {int(fp[-1])}")
        p = NufftParams(int(width))
        self._check(self.L.qmri_set_operator_nufft(self.h, int(N), int(M), int(s), int(T), Vf.ctypes.data_as(C.POINTER(C.c_double)),
                                                   fp.ctypes.data_as(C.POINTER(C.c_int32)), om.ctypes.data_as(C.POINTER(C.c_double)), int(max_batch),
                                                   C.byref(p)))
        self.N, self.M, self.s, self.T, self.m = int(N), int(M), int(s), int(T), int(fp[-1])
        self.sms_Z = 0                     # (the library drops the simultaneous multi-slice phases with the operator)

    def forward(self, x):
        """y = F.forward(x)  (main_recon_tsmis_FFT.m:228).  x: [N,M,s] real or complex; single-precision input (float32 /
        complex64, a MATLAB `single` array) goes through the _f32 entry point and comes back as complex64."""
        x = np.asarray(x)
        if x.shape != (self.N, self.M, self.s):
            raise ValueError(f"x must be {self.N}x{self.M}x{self.s}")
        if x.dtype in (np.float32, np.complex64):
            cx = np.iscomplexobj(x)
            xb = np.ascontiguousarray(x.ravel(order="F"))
            y = np.empty(self.m, np.complex64)
            fp = C.POINTER(C.c_float)
            self._check(self.L.qmri_forward_f32(self.h, xb.view(np.float32).ctypes.data_as(fp), int(cx), y.view(np.float32).ctypes.data_as(fp)))
            return y
        y = np.empty(self.m, np.complex128)
        if np.iscomplexobj(x):
            xb = _cbuf(x)
            self._check(self.L.qmri_forward(self.h, _vp(xb), 1, _vp(y)))
        else:
            xb = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel(order="F"))
            self._check(self.L.qmri_forward(self.h, _vp(xb), 0, _vp(y)))
        return y

    def prepare_normal(self):
        """Build the Toeplitz normal operator of the trajectory now (qmri_nufft_prepare_normal) instead of on the first call that needs it."""
        self._check(self.L.qmri_nufft_prepare_normal(self.h))

    def normal(self, x):
        """A^H A x of a trajectory operator without a gather (qmri_normal).  x: [N,M,s] real or complex -> complex128."""
        x = np.asarray(x)
        if x.shape != (self.N, self.M, self.s):
            raise ValueError(f"x must be {self.N}x{self.M}x{self.s}")
        out = np.empty(self.N * self.M * self.s, np.complex128)
        if np.iscomplexobj(x):
            xb = _cbuf(x)
            self._check(self.L.qmri_normal(self.h, _vp(xb), 1, _vp(out)))
        else:
            xb = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel(order="F"))
            self._check(self.L.qmri_normal(self.h, _vp(xb), 0, _vp(out)))
        return out.reshape((self.N, self.M, self.s), order="F")

    # -- density compensation of a trajectory operator (extension, no reference counterpart) ------------------
    def density_weights(self, niter=0, tol=0.0):
        """Pipe-Menon density weights of the trajectory on the operator's own kernel (qmri_nufft_dcf): niter iterations (1..200, 0: the default
        20), stopped after the first one whose max |d - 1| is <= tol (0: never), scaled so that A^H W A has unit transfer for orthonormal V.
        The weights are attached to the operator (adjoint(y, weighted=True) uses them).  Returns (w [m] float64, dict(iters, dev, clamped, split_tiles:
        the tiles of the plan that were spread in segments and reduced))."""
        if int(niter) != niter or not (0 <= int(niter) <= 200):
            raise ValueError("niter must be an integer in 1..200 (0: the default 20)")
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("tol must be finite and >= 0")
        p, info = DcfParams(int(niter), float(tol)), DcfInfo()
        w = np.empty(max(self.m, 1), np.float64)
        self._check(self.L.qmri_nufft_dcf(self.h, C.byref(p), w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info)))
        return w[: self.m], {"iters": int(info.iters), "dev": float(info.dev), "clamped": int(info.clamped),
                              "split_tiles": int(info.split_tiles)}

    def set_sample_weights(self, w):
        """Attach the caller's own sample weights (qmri_set_sample_weights): m finite values >= 0, the order of y; None clears them."""
        if w is None:
            self._check(self.L.qmri_set_sample_weights(self.h, None))
            return
        w = np.asarray(w)
        if np.iscomplexobj(w):
            raise ValueError("the sample weights must be real")
        wb = np.ascontiguousarray(w, dtype=np.float64).ravel()
        if wb.size != self.m:
            raise ValueError(f"w must have {self.m} elements")
        self._check(self.L.qmri_set_sample_weights(self.h, wb.ctypes.data_as(C.POINTER(C.c_double))))

    # -- off-resonance correction of a trajectory operator (extension, no reference counterpart) ----------------
    def set_field_map(self, f_hz, t_s=None, nseg=0, nbins=0, tol=0.0):
        """Attach a field map to the trajectory operator (qmri_set_field_map): f_hz [N, M] real, Hz; t_s [m] the readout time of every sample in
        seconds, the order of y (spiral_readout_times makes them for the project's spiral).  The operator then carries exp(-i 2 pi f[n] t_i), by time
        segmentation with nseg segments (1..16; 0: the smallest whose fit_max <= tol, tol 0: 1e-4) fitted over an nbins-bin histogram (16..1024; 0:
        256).  forward / adjoint / the _mc methods / xupdate / pnp_admm all run the corrected operator; normal, prepare_normal and solver="toeplitz"
        are refused while a map is attached, until prepare_normal_field builds the field-aware normal operator for it.  None clears the map.  One map per operator (every coil, every slice).
        Returns dict(nseg, tol_reached, fit_max, fit_rms, f_min, f_max, t_min, t_max), or None after clearing."""
        if f_hz is None:
            self._check(self.L.qmri_set_field_map(self.h, None, None, None, None))
            return None
        f = np.asarray(f_hz)
        if np.iscomplexobj(f):
            raise ValueError("the field map must be real (Hz)")
        if f.shape != (self.N, self.M):
            raise ValueError(f"f_hz must be {self.N}x{self.M}")
        if t_s is None:
            raise ValueError("t_s (the readout time of every sample, seconds) is needed with a field map")
        t = np.asarray(t_s)
        if np.iscomplexobj(t):
            raise ValueError("the readout times must be real (seconds)")
        tb = np.ascontiguousarray(t, dtype=np.float64).ravel()
        if tb.size != self.m:
            raise ValueError(f"t_s must have {self.m} elements")
        if int(nseg) != nseg or not (0 <= int(nseg) <= 16):
            raise ValueError("nseg must be an integer in 1..16 (0: automatic)")
        if int(nbins) != nbins or not (int(nbins) == 0 or 16 <= int(nbins) <= 1024):
            raise ValueError("nbins must be an integer in 16..1024 (0: the default 256)")
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("tol must be finite and >= 0")
        fb = np.ascontiguousarray(np.asarray(f, dtype=np.float64).ravel(order="F"))
        p, info = OffresParams(int(nseg), int(nbins), float(tol)), OffresInfo()
        dp = C.POINTER(C.c_double)
        self._check(self.L.qmri_set_field_map(self.h, fb.ctypes.data_as(dp), tb.ctypes.data_as(dp), C.byref(p), C.byref(info)))
        return {"nseg": int(info.nseg), "tol_reached": int(info.tol_reached), "fit_max": float(info.fit_max), "fit_rms": float(info.fit_rms),
                "f_min": float(info.f_min), "f_max": float(info.f_max), "t_min": float(info.t_min), "t_max": float(info.t_max)}

    def prepare_normal_field(self, nseg=0, tol=0.0):
        """Build the Toeplitz normal operator of the trajectory operator WITH its attached field map (qmri_nufft_prepare_normal_fm; DESIGN.md section
        23): A_f^H A_f ~ sum over nseg segments of the difference phase (2..32; 0: the smallest whose fit_max <= tol, tol 0: 1e-4).  After it normal,
        xupdate(..., solver="toeplitz") and the pnp_admm* methods with that solver run the field-aware normal operator; set_field_map (a new map or
        None) drops it.  A constant map reports nseg = 1 and is the plain normal operator.
        Returns dict(nseg, tol_reached, fit_max, fit_rms, khat_bytes)."""
        if int(nseg) != nseg or not (int(nseg) == 0 or 2 <= int(nseg) <= 32):
            raise ValueError("nseg must be an integer in 2..32 (0: automatic)")
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("tol must be finite and >= 0")
        p, info = OffresNormalParams(int(nseg), float(tol)), OffresNormalInfo()
        self._check(self.L.qmri_nufft_prepare_normal_fm(self.h, C.byref(p), C.byref(info)))
        return {"nseg": int(info.nseg), "tol_reached": int(info.tol_reached), "fit_max": float(info.fit_max), "fit_rms": float(info.fit_rms),
                "khat_bytes": int(info.khat_bytes)}

    # -- field map from multi-echo images (extension, no reference counterpart) ------------------------------
    def estimate_field_map(self, Y, echo_times, *, iters=0, beta=0.0, phase_sign=-1, f_init=None, return_info=False, return_trust=False):
        """The field map in Hz of L gradient-echo images per slice, by the regularised estimator of Funai et al. on the device
        (qmri_field_map_estimate): Y [L, N, M], [L, C, N, M] or [S, L, C, N, M] complex, echo_times [L] seconds, strictly increasing.  iters
        iterations (0: 200; there is no stopping rule), beta the dimensionless smoothness weight (0: 0.01), phase_sign -1: y_l = x exp(-i 2 pi f
        t_l), the sign of set_field_map's operator; +1 the other convention.  f_init ([N, M], or [S, N, M] for a stack) replaces the start
        phi_01 / d_01.  Returns f [N, M] ([S, N, M] for a stack): what set_field_map takes; with return_info also dict(cost0, cost, f_min, f_max,
        iters, unwrap_limit_hz) (a list of them for a stack), with return_trust also sum_ab w_ab in the shape of f.  Needs no operator."""
        Yb, t, fb, p, (S, L, Cc, N, M), stacked = fieldmap_arguments(Y, echo_times, iters, beta, phase_sign, f_init)
        f = np.empty((S, M, N), np.float64)
        trust = np.empty((S, M, N), np.float64) if return_trust else None
        info = (FieldmapInfo * S)()
        self._check(self.L.qmri_field_map_estimate(self.h, S, L, Cc, N, M, _vp(Yb), t.ctypes.data_as(C.POINTER(C.c_double)), _vp(fb), C.byref(p), _vp(f),
                                                   _vp(trust), info))
        shape = (lambda a: np.ascontiguousarray(np.swapaxes(a, 1, 2)) if stacked else np.ascontiguousarray(a[0].T))
        out = [shape(f)]
        if return_info:
            out.append([fieldmap_info(i) for i in info] if stacked else fieldmap_info(info[0]))
        if return_trust:
            out.append(shape(trust))
        return out[0] if len(out) == 1 else tuple(out)

    def estimate_field_map_dev(self, d_Y: int, dims, echo_times, d_f_out: int, *, iters=0, beta=0.0, phase_sign=-1, d_f_init: int = 0, d_trust_out: int = 0):
        """qmri_field_map_estimate_dev: device pointers (Y [S][L][C][n1 + N n2] complex double, f / trust [S][n1 + N n2] double), dims = (S, L, C, N,
        M); runs on the engine's stream and returns after completion.  Returns the list of S info dicts."""
        S, L, Cc, N, M = (int(v) for v in dims)
        t = np.ascontiguousarray(echo_times, dtype=np.float64).ravel()
        if t.size != L:
            raise ValueError(f"echo_times must hold one time per echo ({L}), not {t.size}")
        p, info = FieldmapParams(int(iters), float(beta), int(phase_sign)), (FieldmapInfo * max(S, 1))()
        self._check(self.L.qmri_field_map_estimate_dev(self.h, S, L, Cc, N, M, C.c_void_p(d_Y), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                       C.c_void_p(d_f_init or None), C.byref(p), C.c_void_p(d_f_out), C.c_void_p(d_trust_out or None), info))
        return [fieldmap_info(i) for i in info[:S]]

    def adjoint(self, y, weighted=False):
        """x = F.adjoint(y)  (main_recon_tsmis_FFT.m:229); complex64 in -> complex64 out (the _f32 entry point).
        weighted=True: x = A^H (w .* y) with the attached sample weights of a trajectory operator (qmri_adjoint_w; complex128)."""
        if weighted:
            yb = _cbuf(y)
            if yb.size != self.m:
                raise ValueError(f"y must have {self.m} elements")
            x = np.empty(self.N * self.M * self.s, np.complex128)
            self._check(self.L.qmri_adjoint_w(self.h, _vp(yb), _vp(x)))
            return x.reshape((self.N, self.M, self.s), order="F")
        if np.asarray(y).dtype == np.complex64:
            y32 = np.ascontiguousarray(np.asarray(y).ravel(order="F"))
            if y32.size != self.m:
                raise ValueError(f"y must have {self.m} elements")
            x = np.empty(self.N * self.M * self.s, np.complex64)
            fp = C.POINTER(C.c_float)
            self._check(self.L.qmri_adjoint_f32(self.h, y32.view(np.float32).ctypes.data_as(fp), x.view(np.float32).ctypes.data_as(fp)))
            return x.reshape((self.N, self.M, self.s), order="F")
        yb = _cbuf(y)
        if yb.size != self.m:
            raise ValueError(f"y must have {self.m} elements")
        x = np.empty(self.N * self.M * self.s, np.complex128)
        self._check(self.L.qmri_adjoint(self.h, _vp(yb), _vp(x)))
        return x.reshape((self.N, self.M, self.s), order="F")

    # -- multi-coil extension (BASELINE configs[4]; no reference counterpart: README.md:63, single coil) -------------------
    def set_coils(self, maps):
        """maps: [N, M, ncoil] complex coil sensitivities (None clears them)."""
        if maps is None:
            self._check(self.L.qmri_set_coils(self.h, 0, None))
            self.ncoil = 0
            return
        maps = np.asarray(maps)
        if maps.ndim != 3 or maps.shape[:2] != (self.N, self.M):
            raise ValueError(f"maps must be {self.N}x{self.M}xncoil")
        mb = _cbuf(maps)
        self._check(self.L.qmri_set_coils(self.h, int(maps.shape[2]), _vp(mb)))
        self.ncoil = int(maps.shape[2])

    def forward_mc(self, x):
        """y[:, j] = F.forward(maps[..., j] * x): [m, ncoil] complex."""
        x = np.asarray(x)
        if x.shape != (self.N, self.M, self.s):
            raise ValueError(f"x must be {self.N}x{self.M}x{self.s}")
        y = np.empty(self.m * max(getattr(self, "ncoil", 0), 1), np.complex128)
        xb = _cbuf(x)
        self._check(self.L.qmri_forward_mc(self.h, _vp(xb), 1, _vp(y)))
        return y.reshape((self.m, -1), order="F")

    def adjoint_mc(self, y, weighted=False):
        """x = sum_j conj(maps[..., j]) * F.adjoint(y[:, j]); weighted=True: of w .* y[:, j] with the attached sample weights (qmri_adjoint_w_mc)."""
        yb = _cbuf(y)
        nc = getattr(self, "ncoil", 0)
        if nc and yb.size != self.m * nc:                        # (no maps set: the library says so, QMRI_ERR_STATE)
            raise ValueError(f"y must be {self.m} x {nc}")
        x = np.empty(self.N * self.M * self.s, np.complex128)
        self._check((self.L.qmri_adjoint_w_mc if weighted else self.L.qmri_adjoint_mc)(self.h, _vp(yb), _vp(x)))
        return x.reshape((self.N, self.M, self.s), order="F")

    def xupdate_mc(self, y_mc, z, r, tol=1e-4, maxit=100, x0=None):
        """Multi-coil extension (no reference counterpart): x = lsqr(afun_mc, [y_mc; sqrt(r) z], tol, maxit, [], [], x0).  y_mc [m, ncoil].  Returns (x, iters, flag)."""
        yb, zb = _cbuf(y_mc), _cbuf(z)
        nc = getattr(self, "ncoil", 0)
        if nc and yb.size != self.m * nc:
            raise ValueError(f"y_mc must be {self.m} x {nc}")
        x0b = _cbuf(x0) if x0 is not None else None
        x = np.empty(self.N * self.M * self.s, np.complex128)
        it, fl = C.c_int32(0), C.c_int32(0)
        self._check(self.L.qmri_xupdate_mc(self.h, _vp(yb), _vp(zb), float(r), float(tol), int(maxit), _vp(x0b), _vp(x), C.byref(it), C.byref(fl)))
        return x.reshape((self.N, self.M, self.s), order="F"), it.value, fl.value

    def pnp_admm_mc(self, y_mc, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, multi_level=False, noise_std=0.01, x0=None, tsmi_domain="real",
                    solver="lsqr"):
        """Multi-coil extension: PnP_ADMM(y, param) with F replaced by the SENSE operator of set_coils.  Returns (x, lsqr_iters).
        x0 = "dcf": the start image is adjoint_mc(y_mc, weighted=True) (a trajectory operator with attached sample weights).
        solver: "lsqr", or "toeplitz" on a trajectory operator."""
        p = AdmmParams(float(gamma), int(iters), float(cg_tol), int(cg_maxit), _mc_solver(solver), denoiser_type(multi_level, tsmi_domain), float(noise_std), 0)
        yb = _cbuf(y_mc)
        nc = getattr(self, "ncoil", 0)
        if nc and yb.size != self.m * nc:
            raise ValueError(f"y_mc must be {self.m} x {nc}")
        if isinstance(x0, str):
            x0 = self._dcf_start(x0, lambda: self.adjoint_mc(y_mc, weighted=True))
        x0b = _cbuf(x0) if x0 is not None else None
        x = np.empty(self.N * self.M * self.s, np.complex128)
        li = np.zeros(max(iters, 1), np.int32)
        self._check(self.L.qmri_pnp_admm_mc(self.h, _vp(yb), C.byref(p), _vp(x0b), _vp(x), li.ctypes.data_as(C.POINTER(C.c_int32))))
        return x.reshape((self.N, self.M, self.s), order="F"), li[:iters]

    @staticmethod
    def _dcf_start(x0, weighted_adjoint):
        """x0 = "dcf" of pnp_admm / pnp_admm_mc: the density-compensated adjoint of y as the start image (the attached weights of
        density_weights / set_sample_weights).  Nothing else is a valid string."""
        if x0 != "dcf":
            raise ValueError(f'x0 must be an array, None (the adjoint of y) or "dcf" (the density-compensated adjoint), not {x0!r}')
        return weighted_adjoint()

    def _mc_stack(self, maps, y_mc):
        """maps [S, N, M, ncoil], y_mc [S, m, ncoil] -> slice-major column-major buffers (S, ncoil, maps, y)."""
        maps, y_mc = np.asarray(maps), np.asarray(y_mc)
        if maps.ndim != 4 or maps.shape[1:3] != (self.N, self.M):
            raise ValueError(f"maps must be [slices, {self.N}, {self.M}, ncoil]")
        S, nc = maps.shape[0], maps.shape[3]
        if y_mc.shape != (S, self.m, nc):
            raise ValueError(f"y_mc must be [{S}, {self.m}, {nc}]")
        mb = np.concatenate([_cbuf(maps[b]) for b in range(S)])
        yb = np.concatenate([_cbuf(y_mc[b]) for b in range(S)])
        return S, nc, mb, yb

    def _image_stack(self, a, S):
        if a is None:
            return None
        a = np.asarray(a)
        if a.shape != (S, self.N, self.M, self.s):
            raise ValueError(f"image stack must be [{S}, {self.N}, {self.M}, {self.s}]")
        return np.concatenate([_cbuf(a[b]) for b in range(S)])

    def xupdate_mc_batch(self, maps, y_mc, z, r, tol=1e-4, maxit=100, x0=None):
        """Multi-coil x-update of a slice stack, each slice with its own maps (extension, no reference counterpart): maps [S, N, M, ncoil],
        y_mc [S, m, ncoil], z / x0 [S, N, M, s].  Does not use or change the maps of set_coils.  Returns (x [S, N, M, s], iters [S], flags [S])."""
        S, nc, mb, yb = self._mc_stack(maps, y_mc)
        zb, x0b = self._image_stack(z, S), self._image_stack(x0, S)
        n = self.N * self.M * self.s
        x = np.empty(S * n, np.complex128)
        it, fl = np.zeros(S, np.int32), np.zeros(S, np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self.L.qmri_xupdate_mc_batch(self.h, S, nc, _vp(mb), _vp(yb), _vp(zb), float(r), float(tol), int(maxit), _vp(x0b), _vp(x),
                                                 it.ctypes.data_as(ip), fl.ctypes.data_as(ip)))
        return np.stack([x[b * n:(b + 1) * n].reshape((self.N, self.M, self.s), order="F") for b in range(S)]), it, fl

    def pnp_admm_mc_batch(self, maps, y_mc, slices_per_launch=1, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, multi_level=False, noise_std=0.01,
                          x0=None, tsmi_domain="real", solver="lsqr"):
        """Multi-coil PnP-ADMM of a slice stack, slices_per_launch at a time, each slice with its own maps (extension): maps [S, N, M, ncoil],
        y_mc [S, m, ncoil].  Returns (X [S, N, M, s], lsqr_iters [S, iters]).  solver: "lsqr", or "toeplitz" on a trajectory operator."""
        S, nc, mb, yb = self._mc_stack(maps, y_mc)
        x0b = self._image_stack(x0, S)
        p = AdmmParams(float(gamma), int(iters), float(cg_tol), int(cg_maxit), _mc_solver(solver), denoiser_type(multi_level, tsmi_domain), float(noise_std), 0)
        n = self.N * self.M * self.s
        x = np.empty(S * n, np.complex128)
        li = np.zeros((S, max(iters, 1)), np.int32)
        self._check(self.L.qmri_pnp_admm_mc_batch(self.h, S, int(slices_per_launch), nc, _vp(mb), _vp(yb), C.byref(p), _vp(x0b), _vp(x),
                                                  li.ctypes.data_as(C.POINTER(C.c_int32))))
        return np.stack([x[b * n:(b + 1) * n].reshape((self.N, self.M, self.s), order="F") for b in range(S)]), li.reshape(-1)[: S * iters].reshape(S, iters)

    # -- simultaneous multi-slice groups (extension, no reference counterpart) ---------------------------
    def set_sms(self, E):
        """E [T, Z] complex: the phase of slice b of a group in frame t (qmri_set_sms; caipi_phases makes the usual cycle).  1 <= Z <= 8, every value
        finite, any modulus.  Attached to the operator in force and dropped when it is replaced; refused on an operator with a field map."""
        E = np.asarray(E)
        if E.ndim != 2 or E.shape[0] != self.T or not (1 <= E.shape[1] <= 8):
            raise ValueError(f"E must be [{self.T}, Z] with 1 <= Z <= 8")
        if not np.all(np.isfinite(E)):
            raise ValueError("every value of E must be finite")
        eb = _cbuf(E)
        self._check(self.L.qmri_set_sms(self.h, int(E.shape[1]), _vp(eb)))
        self.sms_Z = int(E.shape[1])

    def clear_sms(self):
        self._check(self.L.qmri_set_sms(self.h, 0, None))
        self.sms_Z = 0

    def _sms_stack(self, maps, y=None):
        """maps [G, Z, N, M, ncoil], y [G, m, ncoil] -> (G, Z, ncoil, maps buffer, y buffer) in the library's group-major layouts."""
        maps = np.asarray(maps)
        if maps.ndim != 5 or maps.shape[2:4] != (self.N, self.M) or maps.shape[0] < 1:
            raise ValueError(f"maps must be [groups, Z, {self.N}, {self.M}, ncoil]")
        G, Z, nc = maps.shape[0], maps.shape[1], maps.shape[4]
        if Z != getattr(self, "sms_Z", 0):
            raise ValueError(f"maps hold {Z} slices per group, set_sms was given {getattr(self, 'sms_Z', 0)}")
        mb = np.concatenate([_cbuf(maps[g, b]) for g in range(G) for b in range(Z)])
        yb = None
        if y is not None:
            y = np.asarray(y)
            if y.shape != (G, self.m, nc):
                raise ValueError(f"y must be [{G}, {self.m}, {nc}]")
            yb = np.concatenate([_cbuf(y[g]) for g in range(G)])
        return G, Z, nc, mb, yb

    def _sms_images(self, a, G, Z, real_ok=False):
        if a is None:
            return None
        a = np.asarray(a)
        if a.shape != (G, Z, self.N, self.M, self.s):
            raise ValueError(f"images must be [{G}, {Z}, {self.N}, {self.M}, {self.s}]")
        if real_ok and not np.iscomplexobj(a):
            return np.concatenate([np.ascontiguousarray(np.asarray(a[g, b], np.float64).ravel(order="F")) for g in range(G) for b in range(Z)])
        return np.concatenate([_cbuf(a[g, b]) for g in range(G) for b in range(Z)])

    def _sms_unstack(self, x, G, Z):
        n = self.N * self.M * self.s
        return np.stack([np.stack([x[(g * Z + b) * n:(g * Z + b + 1) * n].reshape((self.N, self.M, self.s), order="F") for b in range(Z)])
                         for g in range(G)])

    def forward_sms(self, maps, x):
        """y[g, :, j] = sum_b E[t(.), b] F.forward(maps[g, b, ..., j] * x[g, b]): maps [G, Z, N, M, ncoil], x [G, Z, N, M, s] (real or complex)
        -> [G, m, ncoil] complex (qmri_forward_sms)."""
        G, Z, nc, mb, _ = self._sms_stack(maps)
        xb = self._sms_images(x, G, Z, real_ok=True)
        y = np.empty(G * nc * self.m, np.complex128)
        self._check(self.L.qmri_forward_sms(self.h, G, nc, _vp(mb), _vp(xb), int(np.iscomplexobj(xb)), _vp(y)))
        return np.stack([y[g * nc * self.m:(g + 1) * nc * self.m].reshape((self.m, nc), order="F") for g in range(G)])

    def adjoint_sms(self, maps, y):
        """x[g, b] = sum_j conj(maps[g, b, ..., j]) * F.adjoint(conj(E[t(.), b]) * y[g, :, j]): [G, Z, N, M, s] (qmri_adjoint_sms)."""
        G, Z, nc, mb, yb = self._sms_stack(maps, y)
        x = np.empty(G * Z * self.N * self.M * self.s, np.complex128)
        self._check(self.L.qmri_adjoint_sms(self.h, G, nc, _vp(mb), _vp(yb), _vp(x)))
        return self._sms_unstack(x, G, Z)

    def xupdate_sms(self, maps, y, z, r, tol=1e-4, maxit=100, x0=None):
        """The joint x-update of G groups of Z simultaneously excited slices: x = lsqr(afun_sms, [y; sqrt(r) z], tol, maxit, [], [], x0) per group.
        maps [G, Z, N, M, ncoil], y [G, m, ncoil], z / x0 [G, Z, N, M, s].  Returns (x [G, Z, N, M, s], iters [G], flags [G])."""
        G, Z, nc, mb, yb = self._sms_stack(maps, y)
        zb, x0b = self._sms_images(z, G, Z), self._sms_images(x0, G, Z)
        if zb is None:
            raise ValueError("z must be given")
        x = np.empty(G * Z * self.N * self.M * self.s, np.complex128)
        it, fl = np.zeros(G, np.int32), np.zeros(G, np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self.L.qmri_xupdate_sms(self.h, G, nc, _vp(mb), _vp(yb), _vp(zb), float(r), float(tol), int(maxit), _vp(x0b), _vp(x),
                                            it.ctypes.data_as(ip), fl.ctypes.data_as(ip)))
        return self._sms_unstack(x, G, Z), it, fl

    def pnp_admm_sms(self, maps, y, groups_per_launch=1, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, multi_level=False, noise_std=0.01, x0=None,
                     tsmi_domain="real", solver="lsqr"):
        """PnP-ADMM of G groups of Z simultaneously excited slices, groups_per_launch at a time (qmri_pnp_admm_sms): the loop of pnp_admm_mc_batch
        with the joint x-update.  x0 None: adjoint_sms(maps, y).  Returns (X [G, Z, N, M, s], lsqr_iters [G, iters]).  Only solver="lsqr" is built."""
        G, Z, nc, mb, yb = self._sms_stack(maps, y)
        x0b = self._sms_images(x0, G, Z)
        p = AdmmParams(float(gamma), int(iters), float(cg_tol), int(cg_maxit), solver_code(solver), denoiser_type(multi_level, tsmi_domain), float(noise_std), 0)
        x = np.empty(G * Z * self.N * self.M * self.s, np.complex128)
        li = np.zeros((G, max(iters, 1)), np.int32)
        self._check(self.L.qmri_pnp_admm_sms(self.h, G, int(groups_per_launch), nc, _vp(mb), _vp(yb), C.byref(p), _vp(x0b), _vp(x),
                                             li.ctypes.data_as(C.POINTER(C.c_int32))))
        return self._sms_unstack(x, G, Z), li.reshape(-1)[: G * iters].reshape(G, iters)

    def coil_compress(self, y_mc, maps=None, noise_cov=None, nv=0, energy=0.99, shared=False):
        """Coil compression of a stack (extension, no reference counterpart; include/qmri.h qmri_coil_compress): y_mc [S, m, ncoil], maps
        [S, N, M, ncoil] or None, noise_cov [ncoil, ncoil] Hermitian positive definite or None (pre-whitening); nv > 0 keeps nv virtual coils,
        nv = 0 takes the smallest nv holding `energy` of the eigenvalue sum (the largest over the slices); shared: one W for the whole stack.
        Returns dict(y [S, m, nv], maps [S, N, M, nv] or None, W [S or 1, ncoil, nv], eig [S or 1, ncoil], nv)."""
        y_mc = np.asarray(y_mc)
        if y_mc.ndim != 3 or y_mc.shape[1] != self.m or y_mc.shape[0] < 1:
            raise ValueError(f"y_mc must be [slices, {self.m}, ncoil]")
        S, nc = y_mc.shape[0], y_mc.shape[2]
        if maps is not None:
            maps = np.asarray(maps)
            if maps.shape != (S, self.N, self.M, nc):
                raise ValueError(f"maps must be [{S}, {self.N}, {self.M}, {nc}]")
        if noise_cov is not None:
            noise_cov = np.asarray(noise_cov)
            if noise_cov.shape != (nc, nc):
                raise ValueError(f"noise_cov must be [{nc}, {nc}]")
        if not (0 <= int(nv) <= nc):
            raise ValueError(f"nv must satisfy 0 <= nv <= ncoil = {nc}")
        yb = np.concatenate([_cbuf(y_mc[b]) for b in range(S)])
        mb = np.concatenate([_cbuf(maps[b]) for b in range(S)]) if maps is not None else None
        pb = _cbuf(noise_cov) if noise_cov is not None else None
        p = CcParams(int(nv), float(energy), int(bool(shared)))
        nmat = 1 if shared else S
        plane = self.N * self.M
        yo = np.empty(S * nc * self.m, np.complex128)
        mo = np.empty(S * nc * plane, np.complex128) if maps is not None else None
        W = np.empty(nmat * nc * nc, np.complex128)
        eig = np.empty(nmat * nc, np.float64)
        got = C.c_int(0)
        self._check(self.L.qmri_coil_compress(self.h, S, nc, _vp(yb), _vp(mb), _vp(pb), C.byref(p), C.byref(got), _vp(yo), _vp(mo), _vp(W),
                                              eig.ctypes.data_as(C.POINTER(C.c_double))))
        k = got.value
        m = self.m
        out = {"nv": k, "eig": eig.reshape(nmat, nc),
               "y": np.stack([yo[b * k * m:(b + 1) * k * m].reshape((m, k), order="F") for b in range(S)]),
               "W": np.stack([W[j * nc * k:(j + 1) * nc * k].reshape((nc, k), order="F") for j in range(nmat)]),
               "maps": None}
        if maps is not None:
            out["maps"] = np.stack([mo[b * k * plane:(b + 1) * k * plane].reshape((self.N, self.M, k), order="F") for b in range(S)])
        return out

    def coil_maps(self, calib, kind="kspace", patch=3, window=True, phase_ref="object", thresh=0.0):
        """Coil sensitivity maps from calibration data (adaptive combine; extension, no reference counterpart; include/qmri.h qmri_coil_maps).
        calib: kind "kspace": a centred k-space block [cN, cM, ncoil] (or a stack [S, cN, cM, ncoil]) in the operator's convention, cN and cM even,
        8 <= cN <= N, 8 <= cM <= M; kind "images": calibration images [N, M, ncoil] (or [S, N, M, ncoil]).  patch: half-width 0..4; window: Hann
        taper of the block; phase_ref: "object" (C^H I real and non-negative) or "coil" (the strongest coil real and non-negative); thresh: pixels
        with lambda_1 < thresh^2 max lambda_1 are zeroed.  Returns (maps, img, lambda1, info) shaped as the input (slice or stack):
        maps [.., N, M, ncoil], img [.., N, M] = C^H I, lambda1 [.., N, M], info = dict(max_iters, not_converged)."""
        kinds, refs = {"kspace": 0, "images": 1}, {"object": 0, "coil": 1}
        if kind not in kinds:
            raise ValueError('kind must be "kspace" or "images"')
        if phase_ref not in refs:
            raise ValueError('phase_ref must be "object" or "coil"')
        if not (0 <= int(patch) <= 4) or int(patch) != patch:
            raise ValueError("patch must be an integer 0..4")
        if not (np.isfinite(thresh) and thresh >= 0):
            raise ValueError("thresh must be finite and >= 0")
        calib = np.asarray(calib)
        if calib.ndim not in (3, 4):
            raise ValueError("calib must be [n1, n2, ncoil] or [slices, n1, n2, ncoil]")
        one = calib.ndim == 3
        c4 = calib[None] if one else calib
        S, c1, c2, nc = c4.shape
        if S < 1 or nc < 1 or nc > 128:
            raise ValueError("calib needs at least one slice and 1..128 coils")
        if kind == "images":
            if (c1, c2) != (self.N, self.M):
                raise ValueError(f"calibration images must be [.., {self.N}, {self.M}, ncoil]")
        elif c1 % 2 or c2 % 2 or not (8 <= c1 <= self.N) or not (8 <= c2 <= self.M):
            raise ValueError(f"the calibration block must have even sides with 8 <= cN <= {self.N}, 8 <= cM <= {self.M}")
        cb = np.concatenate([_cbuf(c4[b]) for b in range(S)])
        p = CsmParams(kinds[kind], int(c1), int(c2), int(patch), int(bool(window)), refs[phase_ref], float(thresh))
        plane = self.N * self.M
        mo = np.empty(S * nc * plane, np.complex128)
        io = np.empty(S * plane, np.complex128)
        lo = np.empty(S * plane, np.float64)
        info = CsmInfo(0, 0)
        self._check(self.L.qmri_coil_maps(self.h, S, nc, self.N, self.M, _vp(cb), C.byref(p), _vp(mo), _vp(io), _vp(lo), C.byref(info)))
        maps = np.stack([mo[b * nc * plane:(b + 1) * nc * plane].reshape((self.N, self.M, nc), order="F") for b in range(S)])
        img = np.stack([io[b * plane:(b + 1) * plane].reshape((self.N, self.M), order="F") for b in range(S)])
        lam = np.stack([lo[b * plane:(b + 1) * plane].reshape((self.N, self.M), order="F") for b in range(S)])
        inf = {"max_iters": int(info.max_iters), "not_converged": int(info.not_converged)}
        return (maps[0], img[0], lam[0], inf) if one else (maps, img, lam, inf)

    def xupdate(self, y, z, r, tol=1e-4, maxit=100, x0=None, solver="lsqr"):
        """The x-update of PnP_ADMM.m:102 alone.  Returns (x, iters, flag)."""
        yb, zb = _cbuf(y), _cbuf(z)
        x = _cbuf(x0 if x0 is not None else np.zeros((self.N, self.M, self.s))).copy()
        it, fl = C.c_int32(0), C.c_int32(0)
        self._check(self.L.qmri_xupdate(self.h, _vp(yb), _vp(zb), float(r), float(tol), int(maxit),
                                        solver_code(solver), _vp(x), C.byref(it), C.byref(fl)))
        return x.reshape((self.N, self.M, self.s), order="F"), it.value, fl.value

    # -- denoiser ------------------------------------------------------------------------------------
    def set_denoiser(self, weights, H, W, in_nc=10, out_nc=10, nc=(64, 128, 256, 512), nb=4, arch=ARCH_UNETRES,
                     residual_noise=False, max_batch=1):
        d = NetDesc(int(arch), int(in_nc), int(out_nc), (C.c_int32 * 4)(*[int(v) for v in nc]), int(nb), int(bool(residual_noise)))
        w = np.ascontiguousarray(weights, dtype=np.float32)
        self._check(self.L.qmri_set_denoiser(self.h, C.byref(d), w.ctypes.data_as(C.POINTER(C.c_float)), w.nbytes, int(H), int(W), int(max_batch)))
        self.net_desc = d
        self.net_hw = (int(H), int(W))

    def lsqr_persist(self, on: bool):
        """Test / A-B hook (qmri_debug_lsqr_persist): all LSQR iterations of an x-update in one launch (default) or two launches per iteration."""
        self._check(self.L.qmri_debug_lsqr_persist(self.h, 2 if on == 2 else int(bool(on))))

    def dict_filter(self, on: bool = True, margin_scale: float = 1.0):
        """Test / A-B hook (qmri_debug_dict_filter): f16 filter in front of the exact dictionary products (default on; same results)."""
        self.L.qmri_debug_dict_filter.argtypes = [C.c_void_p, C.c_int, C.c_float]
        self._check(self.L.qmri_debug_dict_filter(self.h, int(bool(on)), float(margin_scale)))

    def conv_resident(self, on=True):
        """Test / A-B hook (qmri_debug_conv_resident): the full-resolution ResBlocks as one launch with LDS-resident tiles (default) or one
        launch per layer; on = 2: a tile withholds its hand-off (recovery path).  Returns the hand-off time-outs seen so far."""
        n = C.c_int(0)
        self.L.qmri_debug_conv_resident.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self._check(self.L.qmri_debug_conv_resident(self.h, 2 if on == 2 else int(bool(on)), C.byref(n)))
        return n.value

    def denoiser_scheme(self):
        """(scheme, fallbacks): 2 = f16 x 3 products, 3 = bf16 x 6 products; how often a run-time guard switched 2 -> 3."""
        sc, fb = C.c_int(0), C.c_int(0)
        self._check(self.L.qmri_denoiser_scheme(self.h, C.byref(sc), C.byref(fb)))
        return sc.value, fb.value

    def health(self) -> dict:
        """qmri_get_health: which self-checking fast paths are armed, how often one gave up (the work was then repeated on the slower path, same
        results), and wall clock + stage times of the most recent qmri_pnp_admm_dev call (stages: profile level 1 or 3)."""
        from ._lib import Health
        h = Health()
        self._check(self.L.qmri_get_health(self.h, C.byref(h)))
        st = list(h.last_call_stage_ms)
        return {"denoiser_scheme": {0: None, 2: "f16x3", 3: "bf16x6"}.get(h.denoiser_scheme, str(h.denoiser_scheme)),
                "denoiser_fallbacks": h.denoiser_fallbacks, "resident_tile_launch_armed": bool(h.resident_armed),
                "resident_tile_timeouts": h.resident_timeouts, "lsqr_one_launch": {-1: "undecided", 0: "off", 1: "armed"}.get(h.lsqr_one_launch, "armed"),
                "lsqr_one_launch_timeouts": h.lsqr_timeouts, "repeated_calls": h.repeated_calls,
                "last_call_wall_ms": round(h.last_call_wall_ms, 3),
                "last_call_stage_ms": {"xupdate": round(st[0], 3), "denoiser": round(st[1], 3), "elementwise": round(st[2], 3), "diagnostics": round(st[3], 3)},
                "set_denoiser_ms": {"pack_and_upload": round(h.set_denoiser_ms[0], 2), "tensors_and_buffers": round(h.set_denoiser_ms[1], 2),
                                    "calibration_probe": round(h.set_denoiser_ms[2], 2)}}

    def denoise(self, x):
        """I = denoiseImage_PnP_ADMM(x, net, true, residual_noise): x [H,W,C] or [H,W,C,B] double."""
        x = np.asarray(x, dtype=np.float64)
        squeeze = x.ndim == 3
        if squeeze:
            x = x[..., None]
        if x.ndim != 4:
            raise ValueError("input must be H x W x C (x N)")       # images:denoiseImage:invalidImageFormat
        H, W, Cc, B = x.shape
        xb = np.ascontiguousarray(x.ravel(order="F"))
        out_nc = self.net_desc.out_nc if self.net_desc is not None else 1    # unset: the library reports QMRI_ERR_STATE
        out = np.empty(H * W * out_nc * B, np.float64)
        self._check(self.L.qmri_denoise(self.h, xb.ctypes.data_as(C.POINTER(C.c_double)), H, W, Cc, B, out.ctypes.data_as(C.POINTER(C.c_double))))
        out = out.reshape((H, W, out_nc, B), order="F")
        return out[..., 0] if squeeze else out

    # -- locally low-rank regulariser ------------------------------------------
    def llr_prox(self, x, tau, block=8, offset=(0, 0), real=False):
        """The locally low-rank proximal step (qmri_llr_prox): the singular values of every block x block patch of x are soft-thresholded by
        tau.  x: [N, M, s] or a stack [S, N, M, s], N and M multiples of block (4, 8 or 16), s <= 16; offset = (o1, o2) shifts the blocks
        (circular wrap); real: work on real(x).  Needs no operator.  Returns (out complex128 like x, sigma_max: a float, or [S] for a stack)."""
        x = np.asarray(x)
        one = x.ndim == 3
        xs = x[None] if one else x
        if xs.ndim != 4:
            raise ValueError("x must be [N, M, s] or [slices, N, M, s]")
        S, N, M, s = xs.shape
        p = LlrParams(float(tau), int(block), 0)
        if real:
            xb = np.concatenate([np.ascontiguousarray(np.asarray(xs[b].real, np.float64).ravel(order="F")) for b in range(S)])
        else:
            xb = np.concatenate([_cbuf(xs[b]) for b in range(S)])
        out = np.empty(S * N * M * s, np.complex128)
        sm = np.zeros(S, np.float64)
        self._check(self.L.qmri_llr_prox(self.h, N, M, s, S, _vp(xb), 0 if real else 1, C.byref(p), int(offset[0]), int(offset[1]), _vp(out),
                                         sm.ctypes.data_as(C.POINTER(C.c_double))))
        n = N * M * s
        out = np.stack([out[b * n:(b + 1) * n].reshape((N, M, s), order="F") for b in range(S)])
        return (out[0], float(sm[0])) if one else (out, sm)

    def llr_prox_dev(self, d_x: int, dims, tau, d_out: int, block=8, offset=(0, 0), real=False, want_sigma_max=True):
        """qmri_llr_prox_dev on device arrays (complex fp64, [slice][c][n2][n1]); dims = (N, M, s, slices); d_out may be d_x.  Returns sigma_max [slices]."""
        N, M, s, S = (int(v) for v in dims)
        p = LlrParams(float(tau), int(block), 0)
        sm = np.zeros(S, np.float64)
        self._check(self.L.qmri_llr_prox_dev(self.h, N, M, s, S, C.c_void_p(d_x), 0 if real else 1, C.byref(p), int(offset[0]), int(offset[1]),
                                             C.c_void_p(d_out), sm.ctypes.data_as(C.POINTER(C.c_double)) if want_sigma_max else None))
        return sm

    def set_llr(self, tau, block=8, shift=True):
        """Step 2 of every pnp_admm* call of this engine becomes v = LLR_tau(x + uold) (qmri_set_llr) until clear_llr: no denoiser is needed.
        tsmi_domain="complex" thresholds the complex x + uold, "real" its real part.  shift: the block offsets cycle with the iteration."""
        p = LlrParams(float(tau), int(block), int(bool(shift)))
        self._check(self.L.qmri_set_llr(self.h, C.byref(p)))

    def clear_llr(self):
        self._check(self.L.qmri_set_llr(self.h, None))

    # -- joint wavelet soft-thresholding ---------------------------------------
    @staticmethod
    def _wavelet_params(tau, levels, filter, joint, shift):
        if isinstance(filter, str):
            if filter not in WAVELET_FILTERS:
                raise ValueError(f'filter must be one of {sorted(WAVELET_FILTERS)}, not {filter!r}')
            filter = WAVELET_FILTERS[filter]
        return WaveletParams(float(tau), int(levels), int(filter), int(bool(joint)), int(bool(shift)))

    def wavelet_prox(self, x, tau, levels=3, filter="db2", joint=True, offset=(0, 0), real=False):
        """Joint wavelet soft-thresholding (qmri_wavelet_prox): the detail coefficients of a `levels`-level periodic orthogonal wavelet transform
        ("haar" or "db2") of every channel plane are shrunk by tau, jointly over the channels (joint) or each on its own.  x: [N, M, s] or a
        stack [S, N, M, s], N and M multiples of 2^levels, s <= 16; offset = (o1, o2) < 2^levels shifts the transform (cycle spinning); real:
        work on real(x).  Needs no operator.  Returns (out complex128 like x, cmax: a float, or [S] for a stack)."""
        x = np.asarray(x)
        one = x.ndim == 3
        xs = x[None] if one else x
        if xs.ndim != 4:
            raise ValueError("x must be [N, M, s] or [slices, N, M, s]")
        S, N, M, s = xs.shape
        p = self._wavelet_params(tau, levels, filter, joint, False)
        if real:
            xb = np.concatenate([np.ascontiguousarray(np.asarray(xs[b].real, np.float64).ravel(order="F")) for b in range(S)])
        else:
            xb = np.concatenate([_cbuf(xs[b]) for b in range(S)])
        out = np.empty(S * N * M * s, np.complex128)
        cm = np.zeros(S, np.float64)
        self._check(self.L.qmri_wavelet_prox(self.h, N, M, s, S, _vp(xb), 0 if real else 1, C.byref(p), int(offset[0]), int(offset[1]), _vp(out),
                                             cm.ctypes.data_as(C.POINTER(C.c_double))))
        n = N * M * s
        out = np.stack([out[b * n:(b + 1) * n].reshape((N, M, s), order="F") for b in range(S)])
        return (out[0], float(cm[0])) if one else (out, cm)

    def wavelet_prox_dev(self, d_x: int, dims, tau, d_out: int, levels=3, filter="db2", joint=True, offset=(0, 0), real=False, want_cmax=True):
        """qmri_wavelet_prox_dev on device arrays (complex fp64, [slice][c][n2][n1]); dims = (N, M, s, slices); d_out may be d_x.  Returns cmax [slices]."""
        N, M, s, S = (int(v) for v in dims)
        p = self._wavelet_params(tau, levels, filter, joint, False)
        cm = np.zeros(S, np.float64)
        self._check(self.L.qmri_wavelet_prox_dev(self.h, N, M, s, S, C.c_void_p(d_x), 0 if real else 1, C.byref(p), int(offset[0]), int(offset[1]),
                                                 C.c_void_p(d_out), cm.ctypes.data_as(C.POINTER(C.c_double)) if want_cmax else None))
        return cm

    def set_wavelet(self, tau, levels=3, filter="db2", joint=True, shift=True):
        """Step 2 of every pnp_admm* call of this engine becomes v = Wav_tau(x + uold) (qmri_set_wavelet) until clear_wavelet: no denoiser is
        needed.  tsmi_domain="complex" thresholds the complex x + uold, "real" its real part.  shift: the offsets cycle with the iteration.
        Refused while the LLR step is set (one regulariser at a time)."""
        p = self._wavelet_params(tau, levels, filter, joint, shift)
        self._check(self.L.qmri_set_wavelet(self.h, C.byref(p)))

    def clear_wavelet(self):
        self._check(self.L.qmri_set_wavelet(self.h, None))

    # -- PnP-ADMM ------------------------------------------------------------------------------------
    def pnp_admm(self, y, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, solver="lsqr", multi_level=False,
                 noise_std=0.01, x0=None, gt=None, want_diag=False, tsmi_domain="real"):
        """x = PnP_ADMM(y, param)  (PnP_ADMM.m:1).  Returns (x [N,M,s] complex, diag [iters,2] or None, lsqr_iters).
        x0: an array, None (F.adjoint(y)) or, on a trajectory operator with attached sample weights, "dcf": adjoint(y, weighted=True).
        tsmi_domain="complex": the denoiser step on cat(3, real, imag) of x + uold (a 2s (+1) -> 2s network; see denoiser_type)."""
        p = AdmmParams(float(gamma), int(iters), float(cg_tol), int(cg_maxit), solver_code(solver),
                       denoiser_type(multi_level, tsmi_domain), float(noise_std), int(bool(want_diag)))
        yb = _cbuf(y)
        if yb.size != self.m:
            raise ValueError(f"y must have {self.m} elements")
        if isinstance(x0, str):
            x0 = self._dcf_start(x0, lambda: self.adjoint(y, weighted=True))
        x0b = _cbuf(x0) if x0 is not None else None
        gtb = _cbuf(gt) if gt is not None else None
        x = np.empty(self.N * self.M * self.s, np.complex128)
        diag = np.zeros(2 * max(iters, 1), np.float64) if want_diag else None
        li = np.zeros(max(iters, 1), np.int32)
        self._check(self.L.qmri_pnp_admm(self.h, _vp(yb), C.byref(p), _vp(x0b), _vp(gtb), _vp(x),
                                         diag.ctypes.data_as(C.POINTER(C.c_double)) if diag is not None else None,
                                         li.ctypes.data_as(C.POINTER(C.c_int32))))
        return (x.reshape((self.N, self.M, self.s), order="F"),
                diag[: 2 * iters].reshape(iters, 2) if diag is not None else None, li[:iters])

    def pnp_admm_batch(self, ys, slices_per_launch=15, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, solver="lsqr", multi_level=False,
                       noise_std=0.01, tsmi_domain="real"):
        """A slice stack ys [S, m] through this context, slices_per_launch at a time (qmri_pnp_admm_batch; what `PnP_ADMM_hip(Y, param)` calls
        for a measurement matrix).  Returns (X [S,N,M,s] complex, lsqr_iters [S, iters])."""
        p = AdmmParams(float(gamma), int(iters), float(cg_tol), int(cg_maxit), solver_code(solver),
                       denoiser_type(multi_level, tsmi_domain), float(noise_std), 0)
        yb = np.ascontiguousarray(np.asarray(ys, np.complex128))
        if yb.ndim != 2 or yb.shape[1] != self.m:
            raise ValueError(f"ys must be [slices, {self.m}]")
        S, n = yb.shape[0], self.N * self.M * self.s
        x = np.empty((S, n), np.complex128)
        li = np.zeros((S, max(iters, 1)), np.int32)
        self._check(self.L.qmri_pnp_admm_batch(self.h, S, int(slices_per_launch), _vp(yb), C.byref(p), None, None, _vp(x), None,
                                               li.ctypes.data_as(C.POINTER(C.c_int32))))
        return np.stack([x[i].reshape((self.N, self.M, self.s), order="F") for i in range(S)]), li[:, :iters]

    # -- dictionary ----------------------------------------------------------------------------------
    def set_dictionary(self, D, normD, lut):
        D = real_dictionary_array(D, "dict.D", np.float32)
        lut = np.asarray(lut, dtype=np.float32)
        K, s = D.shape
        Q = lut.shape[1]
        Df = np.ascontiguousarray(D.ravel(order="F"))
        lf = np.ascontiguousarray(lut.ravel(order="F"))
        nd = np.ascontiguousarray(normD, dtype=np.float32)
        f = C.POINTER(C.c_float)
        self._check(self.L.qmri_set_dictionary(self.h, K, s, Q, Df.ctypes.data_as(f), nd.ctypes.data_as(f), lf.ctypes.data_as(f)))
        self.dict_shape = (K, s, Q)
        self._lut = np.asarray(lut, dtype=np.float64)
        self.components = None                                   # (qmri_set_dictionary drops them)
        self.dict_groups = None                                  # (... and the groups)
        self.refine_cols = None                                  # (... and the refinement)

    # -- sub-grid refinement of a match (extension, no reference counterpart) --
    def set_refine(self, cols=(0, 1)):
        """The lut columns dict_refine moves off the grid (include/qmri.h qmri_set_refine): 1 to 3 distinct 0-based columns of the set narrow
        dictionary's lut, (0, 1) = (T1, T2).  Builds every atom's neighbours along each column (dict_lines) and uploads them with the fp64 table of
        unnormalised atoms.  Returns dict(P, K, s, count [P, 3] = atoms with 0, 1, 2 neighbours per column).  set_dictionary drops the state."""
        from ._lib import RefineInfo
        if getattr(self, "dict_shape", None) is None:
            raise ValueError("set_dictionary first")
        c = refine_columns(cols, self.dict_shape[2])
        info = RefineInfo()
        self._check(self.L.qmri_set_refine(self.h, c.size, c.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info)))
        self.refine_cols = c.copy()
        return {"P": int(info.P), "K": int(info.K), "s": int(info.s), "count": np.array([[info.count[q][j] for j in range(3)] for q in range(c.size)], np.int32)}

    def clear_refine(self):
        self._check(self.L.qmri_set_refine(self.h, 0, None, None))
        self.refine_cols = None

    def dict_refine(self, X, dm, want_pd=True, want_res=True, want_t=True, want_centre=True):
        """Every pixel of X [..., s] complex fitted to the quadratic through its start atom dm [...] (1-based, from any match; 0 = skipped) and that
        atom's neighbours along the set_refine columns (qmri_dict_refine): dict(qmap [..., Q] float64 -- the refined columns off the grid, the
        others the final centre's lut value --, flags [...] int32 (REFINE_FLAGS), pd [...] complex128, res [...] = ||x - pd d|| / ||x||,
        t [..., P] the position between the neighbours in [-1, 1], centre [...] the 1-based atom the result is expressed around)."""
        if getattr(self, "refine_cols", None) is None:
            raise ValueError("set_refine first")
        X = np.asarray(X, dtype=np.complex128)
        K, s, Q = self.dict_shape
        if X.ndim < 1 or X.shape[-1] != s:
            raise ValueError("last dimension of X must equal the dictionary's channel count")
        lead = X.shape[:-1]
        dm = np.asarray(dm)
        if dm.shape != lead or not np.issubdtype(dm.dtype, np.integer):
            raise ValueError(f"dm must be integers in the leading shape of X, {lead}")
        npix, P = int(np.prod(lead)), int(self.refine_cols.size)
        xb = np.ascontiguousarray(X.reshape((npix, s), order="F").ravel(order="F"))
        db = np.ascontiguousarray(dm.ravel(order="F"), dtype=np.int32)
        qmap = np.empty(npix * Q, np.float64)
        pd = np.empty(2 * npix, np.float64) if want_pd else None
        res = np.empty(npix, np.float64) if want_res else None
        t = np.empty(npix * P, np.float64) if want_t else None
        centre = np.empty(npix, np.int32) if want_centre else None
        flags = np.empty(npix, np.int32)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self._check(self.L.qmri_dict_refine(self.h, _vp(xb), npix, db.ctypes.data_as(ip), qmap.ctypes.data_as(dp), pd.ctypes.data_as(dp) if want_pd else None,
                                            res.ctypes.data_as(dp) if want_res else None, t.ctypes.data_as(dp) if want_t else None,
                                            centre.ctypes.data_as(ip) if want_centre else None, flags.ctypes.data_as(ip)))
        out = {"qmap": qmap.reshape(lead + (Q,), order="F"), "flags": flags.reshape(lead, order="F")}
        if want_pd:
            out["pd"] = pd.view(np.complex128).reshape(lead, order="F")
        if want_res:
            out["res"] = res.reshape(lead, order="F")
        if want_t:
            out["t"] = t.reshape(lead + (P,), order="F")
        if want_centre:
            out["centre"] = centre.reshape(lead, order="F")
        return out

    def dict_refine_dev(self, d_X: int, npix: int, d_dm: int, d_qmap: int = 0, d_pd: int = 0, d_res: int = 0, d_t: int = 0, d_centre: int = 0, d_flags: int = 0):
        """qmri_dict_refine_dev: device pointers (X Npix x s complex double column-major, dm Npix int32; outputs as qmri.h lays them out),
        asynchronous on the engine's stream."""
        self._check(self.L.qmri_dict_refine_dev(self.h, C.c_void_p(d_X), int(npix), C.c_void_p(d_dm), C.c_void_p(d_qmap or None), C.c_void_p(d_pd or None),
                                                C.c_void_p(d_res or None), C.c_void_p(d_t or None), C.c_void_p(d_centre or None), C.c_void_p(d_flags or None)))

    def set_components(self, atoms):
        """The components of tissue_fractions (extension, no reference counterpart; include/qmri.h qmri_set_components):
        1 <= C <= 8 distinct atoms (1-based, like dm) of the set narrow dictionary, e.g. nearest_atoms([(T1, T2) of white matter, grey matter,
        CSF]).  Returns dict(min_pivot, C, s): min_pivot in (0, 1] is the smallest Cholesky pivot of the unit-diagonal Gram matrix of the
        components (1: orthogonal; near 0: nearly dependent, fractions ill-determined).  set_dictionary drops the components."""
        from ._lib import PvInfo
        if self.dict_shape is None:
            raise ValueError("set_dictionary first")
        a = component_arguments(atoms, self.dict_shape[0])
        info = PvInfo()
        self._check(self.L.qmri_set_components(self.h, a.size, a.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info)))
        self.components = a.copy()
        return {"min_pivot": float(info.min_pivot), "C": int(info.C), "s": int(info.s)}

    def clear_components(self):
        self._check(self.L.qmri_set_components(self.h, 0, None, None))
        self.components = None

    def nearest_atoms(self, points):
        """The 1-based atom whose first two lut columns are nearest each (T1, T2) of points [n, 2], squared distance in float64, the first minimum
        winning (the rule of synth.synthesize_tsmi's knnsearch) -> int32 [n]."""
        if self.dict_shape is None:
            raise ValueError("set_dictionary first")
        return nearest_atoms(self._lut, points)

    def tissue_fractions(self, X, mode="real", want_frac=True, want_pd=True, want_res=True):
        """Every pixel of X [..., s] complex as a non-negative combination of the set components (qmri_dict_unmix): dict(w [..., C] float64 in the
        units of PD, flags [...] int32 (bit 0: iteration cap, bit 1: non-finite pixel, outputs 0), frac [..., C] = w / sum w, pd [...] complex128 =
        (sum w) e^{i phi}, res [...] = ||x e^{-i phi} - A w|| / ||x||).  mode "real" fits Re x; "phase" first removes the pixel's own phase."""
        m = unmix_mode(mode)
        if self.components is None:
            raise ValueError("set_components first")
        X = np.asarray(X, dtype=np.complex128)
        K, s, Q = self.dict_shape
        if X.ndim < 1 or X.shape[-1] != s:
            raise ValueError("last dimension of X must equal the dictionary's channel count")
        lead = X.shape[:-1]
        npix, nc = int(np.prod(lead)), int(self.components.size)
        xb = np.ascontiguousarray(X.reshape((npix, s), order="F").ravel(order="F"))
        w = np.empty(npix * nc, np.float64)
        frac = np.empty(npix * nc, np.float64) if want_frac else None
        pd = np.empty(2 * npix, np.float64) if want_pd else None
        res = np.empty(npix, np.float64) if want_res else None
        flags = np.empty(npix, np.int32)
        dp = C.POINTER(C.c_double)
        self._check(self.L.qmri_dict_unmix(self.h, _vp(xb), npix, m, w.ctypes.data_as(dp), frac.ctypes.data_as(dp) if want_frac else None,
                                           pd.ctypes.data_as(dp) if want_pd else None, res.ctypes.data_as(dp) if want_res else None,
                                           flags.ctypes.data_as(C.POINTER(C.c_int32))))
        out = {"w": w.reshape(lead + (nc,), order="F"), "flags": flags.reshape(lead, order="F")}
        if want_frac:
            out["frac"] = frac.reshape(lead + (nc,), order="F")
        if want_pd:
            out["pd"] = pd.view(np.complex128).reshape(lead, order="F")
        if want_res:
            out["res"] = res.reshape(lead, order="F")
        return out

    def tissue_fractions_dev(self, d_X: int, npix: int, mode="real", d_w: int = 0, d_frac: int = 0, d_pd: int = 0, d_res: int = 0, d_flags: int = 0):
        """qmri_dict_unmix_dev: device pointers (X Npix x s complex double column-major; outputs as qmri.h lays them out), asynchronous on the
        engine's stream."""
        self._check(self.L.qmri_dict_unmix_dev(self.h, C.c_void_p(d_X), int(npix), unmix_mode(mode), C.c_void_p(d_w or None), C.c_void_p(d_frac or None),
                                               C.c_void_p(d_pd or None), C.c_void_p(d_res or None), C.c_void_p(d_flags or None)))

    def set_dictionary_groups(self, group_ptr, group_val):
        """Groups of the set dictionary (extension, no reference counterpart; include/qmri.h qmri_set_dictionary_groups): group g holds atoms
        group_ptr[g] .. group_ptr[g + 1] - 1 (0-based) and has the selector value group_val[g] (e.g. its b1), ascending.  dict_match(X, sel=...) then
        matches every pixel against the atoms of its own group.  group_ptr = None clears.  set_dictionary drops the groups."""
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        if group_ptr is None:
            self._check(self.L.qmri_set_dictionary_groups(self.h, 0, None, None))
            self.dict_groups = None
            return
        gp, gv = group_arguments(group_ptr, group_val)
        self._check(self.L.qmri_set_dictionary_groups(self.h, gv.size, gp.ctypes.data_as(ip), gv.ctypes.data_as(dp)))
        self.dict_groups = gv.copy()

    # -- the B1 map from the fingerprints (extension, no reference counterpart) --
    def _group_count(self):
        gv = getattr(self, "dict_groups", None)
        if getattr(self, "dict_shape", None) is None or gv is None:
            raise ValueError("set_dictionary and set_dictionary_groups first")
        return int(gv.size)

    def group_scores(self, X):
        """qmri_dict_group_scores: X [..., s] complex -> score [G, ...] float32, score[g] the mt of dict_match(X, sel=group_val[g]) for every
        group g, bit for bit.  Needs a dictionary of s <= 16 channels with groups."""
        G = self._group_count()
        X = np.asarray(X, dtype=np.complex128)
        s = self.dict_shape[1]
        if X.ndim < 2 or X.shape[-1] != s:
            raise ValueError("last dimension of X must equal the dictionary's channel count")
        lead = X.shape[:-1]
        npix = int(np.prod(lead))
        xb = np.ascontiguousarray(X.reshape((npix, s), order="F").ravel(order="F"))
        score = np.empty((G, npix), np.float32)
        self._check(self.L.qmri_dict_group_scores(self.h, _vp(xb), npix, score.ctypes.data_as(C.POINTER(C.c_float))))
        return score.reshape((G,) + lead, order="F")

    def group_scores_dev(self, d_X: int, npix: int, d_score: int):
        """qmri_dict_group_scores_dev: device pointers (X Npix x s complex double column-major, score G x Npix float32), asynchronous on the
        engine's stream."""
        self._check(self.L.qmri_dict_group_scores_dev(self.h, C.c_void_p(d_X), int(npix), C.c_void_p(d_score or None)))

    def b1_pool(self, score, group_val, mask=None, window=4, want_b1=True, want_grp=True, want_conf=True):
        """qmri_b1_pool: score [G, N, M] or [G, N, M, nslices] -> dict(b1 float64 (NaN where nothing was estimated), grp int32 (1-based, 0 none),
        conf float64) in the image's shape: per pixel the lowest group with the largest energy score^2 summed over the (2 window + 1)^2 window, in
        fp64 as include/qmri.h states it.  mask: non-zero = foreground.  Needs no dictionary."""
        sb, gv, mb, (N, M, nsl) = b1_pool_arguments(score, group_val, mask)
        h = b1_window(window)
        lead = np.asarray(score).shape[1:]
        n = N * M * nsl
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        b1 = np.empty(n, np.float64) if want_b1 else None
        grp = np.empty(n, np.int32) if want_grp else None
        conf = np.empty(n, np.float64) if want_conf else None
        self._check(self.L.qmri_b1_pool(self.h, gv.size, gv.ctypes.data_as(dp), N, M, nsl, sb.ctypes.data_as(C.POINTER(C.c_float)),
                                        _vp(mb) if mb is not None else None, h, b1.ctypes.data_as(dp) if want_b1 else None,
                                        grp.ctypes.data_as(ip) if want_grp else None, conf.ctypes.data_as(dp) if want_conf else None))
        out = {}
        for k, v in (("b1", b1), ("grp", grp), ("conf", conf)):
            if v is not None:
                out[k] = v.reshape(lead, order="F")
        return out

    def b1_pool_dev(self, group_val, N: int, M: int, nslices: int, d_score: int, d_mask: int = 0, window=4, d_b1: int = 0, d_grp: int = 0, d_conf: int = 0):
        """qmri_b1_pool_dev: device pointers (group_val stays a host array), asynchronous on the engine's stream."""
        gv = np.ascontiguousarray(group_val, dtype=np.float64).ravel()
        self._check(self.L.qmri_b1_pool_dev(self.h, gv.size, gv.ctypes.data_as(C.POINTER(C.c_double)), int(N), int(M), int(nslices), C.c_void_p(d_score or None),
                                            C.c_void_p(d_mask or None), b1_window(window), C.c_void_p(d_b1 or None), C.c_void_p(d_grp or None),
                                            C.c_void_p(d_conf or None)))

    def estimate_b1(self, X, mask=None, window=4):
        """qmri_b1_estimate: X [N, M, s] or [N, M, nslices, s] complex -> dict(b1, grp, conf in the image's shape, info = dict(n_estimated,
        n_unmatched, mean_conf)): group_scores then b1_pool with the dictionary's own groups, bit for bit, a run of slices at a time."""
        from ._lib import B1estInfo, B1estParams
        self._group_count()
        h = b1_window(window)
        X = np.asarray(X, dtype=np.complex128)
        s = self.dict_shape[1]
        if X.ndim not in (3, 4) or X.shape[-1] != s:
            raise ValueError("X must be [N, M, s] or [N, M, nslices, s] with the dictionary's channel count")
        lead = X.shape[:-1]
        if min(lead) < 1:
            raise ValueError("X must have at least one pixel")
        N, M, nsl = lead[0], lead[1], (lead[2] if len(lead) == 3 else 1)
        n = N * M * nsl
        mb = None
        if mask is not None:
            m = np.asarray(mask)
            if m.shape != lead:
                raise ValueError(f"mask must have the image's shape {lead}, not {m.shape}")
            mb = np.ascontiguousarray((m != 0).ravel(order="F").astype(np.uint8))
        xb = np.ascontiguousarray(X.reshape((n, s), order="F").ravel(order="F"))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        b1, grp, conf = np.empty(n, np.float64), np.empty(n, np.int32), np.empty(n, np.float64)
        p, info = B1estParams(h), B1estInfo()
        self._check(self.L.qmri_b1_estimate(self.h, _vp(xb), N, M, nsl, _vp(mb) if mb is not None else None, C.byref(p), b1.ctypes.data_as(dp),
                                            grp.ctypes.data_as(ip), conf.ctypes.data_as(dp), C.byref(info)))
        return {"b1": b1.reshape(lead, order="F"), "grp": grp.reshape(lead, order="F"), "conf": conf.reshape(lead, order="F"),
                "info": {"n_estimated": int(info.n_estimated), "n_unmatched": int(info.n_unmatched), "mean_conf": float(info.mean_conf)}}

    def estimate_b1_dev(self, d_X: int, N: int, M: int, nslices: int, d_mask: int = 0, window=4, d_b1: int = 0, d_grp: int = 0, d_conf: int = 0):
        """qmri_b1_estimate_dev: device pointers, asynchronous on the engine's stream."""
        from ._lib import B1estParams
        p = B1estParams(b1_window(window))
        self._check(self.L.qmri_b1_estimate_dev(self.h, C.c_void_p(d_X), int(N), int(M), int(nslices), C.c_void_p(d_mask or None), C.byref(p),
                                                C.c_void_p(d_b1 or None), C.c_void_p(d_grp or None), C.c_void_p(d_conf or None), None))

    def compress_dictionary(self, F, s=None, energy=None, s_max=16, tol=0.0, maxit=0):
        """A simulated dictionary compressed to its SVD subspace on the device (extension, no reference counterpart; include/qmri.h
        qmri_dict_compress).  F [K, T]: K real fingerprints of T <= 1024 frames, float64 or float32 (float32 stays float32 on its way to the
        device and is widened there); a complex F with a non-zero imaginary part is refused.  Exactly one of s (the rank, 1..16) and energy (the
        fraction of trace(F^T F) to keep, with at most s_max <= 16 vectors) is given.  tol: residual bound of the eigenpairs relative to lambda_1
        (0: 1e-13); maxit: cap on the subspace iterations (0: 200).  Returns dict(V [T, s] float64 for set_operator, D [K, s] float32 and normD [K]
        float32 for set_dictionary, eig [s], info = dict(s, iters, converged, energy_reached, max_resid, energy_kept)).  Needs no operator."""
        if (s is None) == (energy is None):
            raise ValueError("give exactly one of s and energy")
        F = real_dictionary_array(F, "F", np.float32 if np.asarray(F).dtype == np.float32 else np.float64)
        if F.ndim != 2 or F.shape[0] < 1 or not (1 <= F.shape[1] <= 1024):
            raise ValueError("F must be [K, T] with K >= 1 and 1 <= T <= 1024")
        K, T = F.shape
        if s is not None and (int(s) != s or not (1 <= int(s) <= min(16, K, T))):
            raise ValueError(f"s must be an integer with 1 <= s <= min(16, K, T) = {min(16, K, T)}")
        if s is None and (int(s_max) != s_max or not (1 <= int(s_max) <= 16) or not (0.0 < float(energy) <= 1.0)):
            raise ValueError("energy must be in (0, 1] and s_max an integer in 1..16")
        if not (0.0 <= float(tol) < 1.0) or int(maxit) != maxit or int(maxit) < 0:
            raise ValueError("tol must be in [0, 1) and maxit an integer >= 0")
        Fb = np.ascontiguousarray(F.ravel(order="F"))
        p = DsvdParams(0 if s is None else int(s), int(s_max), 0.0 if energy is None else float(energy), float(tol), int(maxit))
        V = np.empty(T * 16, np.float64)
        D = np.empty(K * 16, np.float32)
        nd = np.empty(K, np.float32)
        eig = np.empty(16, np.float64)
        got, info = C.c_int(0), DsvdInfo()
        self._check(self.L.qmri_dict_compress(self.h, K, T, _vp(Fb), int(F.dtype == np.float64), C.byref(p), C.byref(got), _vp(V), _vp(D), _vp(nd), _vp(eig),
                                              C.byref(info)))
        r = got.value
        return {"V": V[: T * r].reshape((T, r), order="F"), "D": D[: K * r].reshape((K, r), order="F"), "normD": nd, "eig": eig[:r].copy(),
                "info": {"s": int(info.s), "iters": int(info.iters), "converged": int(info.converged), "energy_reached": int(info.energy_reached),
                         "max_resid": float(info.max_resid), "energy_kept": float(info.energy_kept)}}

    def simulate_dictionary(self, alpha, tr, te, t1, t2, b1=None, nstates=32, inversion=True, ti=0.0, inv_eff=1.0, dtype=np.float64,
                            slice_profile=None, slice_weights=None):
        """The fingerprints of a FISP-MRF sequence by extended phase graphs on the device (extension, no reference counterpart; include/qmri.h
        qmri_dict_simulate).  alpha [T] flip angles in radians, T <= 1024; tr, te in seconds, scalars (broadcast to T) or [T]; t1, t2 (seconds)
        and b1 (transmit scale, None: 1) are broadcast against each other and flattened to the K atoms.  nstates: configuration states kept
        (1..256; the truncation is part of the result).  inversion: an inversion pulse of efficiency inv_eff, TI = ti before the train.
        slice_profile [Q] or [T, Q] (with slice_weights [Q], default 1 / Q): the simulation integrated over a slice profile (qmri_dict_simulate_sp;
        DESIGN.md section 26) -- F = sum_q w_q x the fingerprint with flip angles alpha_t b1 slice_profile[t, q]; synth.rf_slice_profile makes one.
        Returns F [K, T] in dtype (float64, or float32: the float64 result rounded once).  Needs no operator."""
        a, trv, tev, T1, T2, B1, p = simulation_arguments(alpha, tr, te, t1, t2, b1, nstates, inversion, ti, inv_eff, dtype)
        K, T = T1.size, a.size
        sp = slice_profile_arguments(slice_profile, slice_weights, T)
        F = np.empty(K * T, np.float64 if p.out_is_f64 else np.float32)
        if sp is None:
            self._check(self.L.qmri_dict_simulate(self.h, K, T, _vp(a), _vp(trv), _vp(tev), _vp(T1), _vp(T2), _vp(B1), C.byref(p), _vp(F)))
        else:
            self._check(self.L.qmri_dict_simulate_sp(self.h, K, T, _vp(a), _vp(trv), _vp(tev), _vp(T1), _vp(T2), _vp(B1), C.byref(p), C.byref(sp[2]), _vp(F)))
        return F.reshape((K, T), order="F")

    def simulate_dictionary_grad(self, alpha, tr, te, t1, t2, b1=None, wrt=("t1", "t2"), V=None, outputs=("F", "dF", "crb"), nstates=32, inversion=True,
                                 ti=0.0, inv_eff=1.0, dtype=np.float64):
        """The fingerprints of simulate_dictionary with their derivatives and the Cramer-Rao bound they give, in one launch (extension, no
        reference counterpart; include/qmri.h qmri_dict_simulate_grad).  The sequence and atom arguments are
        simulate_dictionary's (no slice profile).  wrt: ("t1", "t2") or ("t1", "t2", "b1"), the P parameters.  V [T, s], s <= 16: the bound is that
        of the fingerprints projected on V (the V of compress_dictionary); None: of the uncompressed ones.  outputs: which of "F", "dF", "crb" to
        compute and return.  Returns dict(F [K, T] -- the bits of simulate_dictionary --, dF [P, K, T], both in dtype; crb [K, 1 + P] float64: a
        pixel rho x atom k + noise of deviation sigma per real and imaginary part and channel has sigma(theta_q) >= sigma sqrt(crb[k, 1 + q]) /
        |rho| and sigma(Re rho) >= sigma sqrt(crb[k, 0]); flags [K] int32: 0, or 1 for an atom whose Fisher matrix is singular (its crb is +inf)).
        Entries that were not asked for are None.  Needs no operator."""
        a, trv, tev, T1, T2, B1, p = simulation_arguments(alpha, tr, te, t1, t2, b1, nstates, inversion, ti, inv_eff, dtype)
        K, T = T1.size, a.size
        Vb, gp, outs = grad_arguments(wrt, V, outputs, T)
        P, dt = gp.nparams, np.float64 if p.out_is_f64 else np.float32
        F = np.empty(K * T, dt) if "F" in outs else None
        dF = np.empty(P * K * T, dt) if "dF" in outs else None
        crb = np.empty(K * (1 + P), np.float64) if "crb" in outs else None
        flags = np.empty(K, np.int32) if "crb" in outs else None
        self._check(self.L.qmri_dict_simulate_grad(self.h, K, T, _vp(a), _vp(trv), _vp(tev), _vp(T1), _vp(T2), _vp(B1), C.byref(p), C.byref(gp), _vp(F),
                                                   _vp(dF), _vp(crb), _vp(flags)))
        return {"F": None if F is None else F.reshape((K, T), order="F"),
                "dF": None if dF is None else np.stack([dF[q * K * T:(q + 1) * K * T].reshape((K, T), order="F") for q in range(P)]),
                "crb": None if crb is None else crb.reshape(K, 1 + P), "flags": flags}

    def simulate_dictionary_seq(self, alpha, tr, te, t1, t2, blocks, ncycles=1, b1=None, nstates=32, dtype=np.float64):
        """The fingerprints of a prepared, repeated FISP train (extension, no reference counterpart; include/qmri.h qmri_dict_simulate_seq;
        DESIGN.md section 33).  alpha, tr, te, t1, t2, b1, nstates, dtype: as in simulate_dictionary.  blocks: a sequence of dict(nframes=,
        prep="none" | "inversion" | "t2", wait=0.0, prep_time=0.0, prep_eff=1.0) whose nframes sum to T -- in front of its frames a block waits
        `wait` seconds (free relaxation), then plays its preparation (inversion: TI = prep_time, efficiency prep_eff; T2 preparation: echo time
        prep_time, scale prep_eff; idealised, not scaled by b1).  The block list is played ncycles times from equilibrium and the last cycle is
        recorded.  synth.repeated_train_blocks and synth.cmrf_blocks make block lists.  Returns F [K, T] in dtype.  Needs no operator."""
        a, trv, tev, T1, T2, B1, p = simulation_arguments(alpha, tr, te, t1, t2, b1, nstates, False, 0.0, 1.0, dtype)
        K, T = T1.size, a.size
        arr, seq = sequence_arguments(blocks, ncycles, T)
        F = np.empty(K * T, np.float64 if p.out_is_f64 else np.float32)
        self._check(self.L.qmri_dict_simulate_seq(self.h, K, T, _vp(a), _vp(trv), _vp(tev), _vp(T1), _vp(T2), _vp(B1), C.byref(p), C.byref(seq), _vp(F)))
        return F.reshape((K, T), order="F")

    def dictionary_crb(self, alpha, tr, te, t1, t2, b1=None, wrt=("t1", "t2"), V=None, nstates=32, inversion=True, ti=0.0, inv_eff=1.0):
        """The Cramer-Rao bound of simulate_dictionary_grad alone: no K x T array is made, on the device or the host.  Returns dict(crb [K, 1 + P],
        flags [K])."""
        r = self.simulate_dictionary_grad(alpha, tr, te, t1, t2, b1=b1, wrt=wrt, V=V, outputs=("crb",), nstates=nstates, inversion=inversion, ti=ti,
                                          inv_eff=inv_eff)
        return {"crb": r["crb"], "flags": r["flags"]}

    def simulate_compress_dictionary(self, alpha, tr, te, t1, t2, b1=None, s=None, energy=None, s_max=16, nstates=32, inversion=True, ti=0.0,
                                     inv_eff=1.0, slice_profile=None, slice_weights=None, blocks=None, ncycles=1):
        """simulate_dictionary followed by compress_dictionary on the same device buffer: the K x T float64 fingerprints never leave the device.
        slice_profile / slice_weights: as in simulate_dictionary.  blocks / ncycles: the fingerprints are those of simulate_dictionary_seq
        (qmri_dict_simulate_seq_dev on the same buffer); inversions are then stated in the blocks and inversion / ti / inv_eff are not used; not
        available with a slice profile.  Returns what compress_dictionary returns."""
        if (s is None) == (energy is None):
            raise ValueError("give exactly one of s and energy")
        if blocks is not None and (slice_profile is not None or slice_weights is not None):
            raise ValueError("blocks are not available with a slice profile")
        if blocks is not None:
            inversion, ti, inv_eff = False, 0.0, 1.0
        a, trv, tev, T1, T2, B1, p = simulation_arguments(alpha, tr, te, t1, t2, b1, nstates, inversion, ti, inv_eff, np.float64)
        K, T = T1.size, a.size
        sp = slice_profile_arguments(slice_profile, slice_weights, T)
        sq = None if blocks is None else sequence_arguments(blocks, ncycles, T)
        if s is not None and (int(s) != s or not (1 <= int(s) <= min(16, K, T))):
            raise ValueError(f"s must be an integer with 1 <= s <= min(16, K, T) = {min(16, K, T)}")
        if s is None and (int(s_max) != s_max or not (1 <= int(s_max) <= 16) or not (0.0 < float(energy) <= 1.0)):
            raise ValueError("energy must be in (0, 1] and s_max an integer in 1..16")
        q = DsvdParams(0 if s is None else int(s), int(s_max), 0.0 if energy is None else float(energy), 0.0, 0)
        V, D, nd, eig = np.empty(T * 16, np.float64), np.empty(K * 16, np.float32), np.empty(K, np.float32), np.empty(16, np.float64)
        got, info = C.c_int(0), DsvdInfo()
        hip = _hip_runtime()
        bufs = [C.c_void_p() for _ in range(7)]
        d_t1, d_t2, d_b1, d_F, d_V, d_D, d_n = bufs
        try:
            for d, nb in ((d_t1, K * 8), (d_t2, K * 8), (d_b1, K * 8), (d_F, K * T * 8), (d_V, V.nbytes), (d_D, D.nbytes), (d_n, nd.nbytes)):
                if hip.hipMalloc(C.byref(d), nb) != 0:
                    raise MemoryError(f"hipMalloc of {nb} bytes failed")
            for d, h in ((d_t1, T1), (d_t2, T2)) + (((d_b1, B1),) if B1 is not None else ()):
                if hip.hipMemcpy(d, _vp(h), h.nbytes, 1) != 0:
                    raise RuntimeError("hipMemcpy to the device failed")
            if sq is not None:
                self._check(self.L.qmri_dict_simulate_seq_dev(self.h, K, T, _vp(a), _vp(trv), _vp(tev), d_t1, d_t2, d_b1 if B1 is not None else None, C.byref(p),
                                                              C.byref(sq[1]), d_F))
            elif sp is None:
                self._check(self.L.qmri_dict_simulate_dev(self.h, K, T, _vp(a), _vp(trv), _vp(tev), d_t1, d_t2, d_b1 if B1 is not None else None, C.byref(p), d_F))
            else:
                self._check(self.L.qmri_dict_simulate_sp_dev(self.h, K, T, _vp(a), _vp(trv), _vp(tev), d_t1, d_t2, d_b1 if B1 is not None else None, C.byref(p),
                                                             C.byref(sp[2]), d_F))
            self._check(self.L.qmri_dict_compress_dev(self.h, K, T, d_F, 1, C.byref(q), C.byref(got), d_V, d_D, d_n, _vp(eig), C.byref(info)))
            for d, h in ((d_V, V), (d_D, D), (d_n, nd)):
                if hip.hipMemcpy(_vp(h), d, h.nbytes, 2) != 0:
                    raise RuntimeError("hipMemcpy from the device failed")
        finally:
            for d in bufs:
                if d.value:
                    hip.hipFree(d)
        r = got.value
        return {"V": V[: T * r].reshape((T, r), order="F").copy(), "D": D[: K * r].reshape((K, r), order="F").copy(), "normD": nd, "eig": eig[:r].copy(),
                "info": {"s": int(info.s), "iters": int(info.iters), "converged": int(info.converged), "energy_reached": int(info.energy_reached),
                         "max_resid": float(info.max_resid), "energy_kept": float(info.energy_kept)}}

    def synthesize_tsmi(self, qmap, mode="real"):
        """TSMI of a quantitative map (main_synthesize_tsmis.m:82-103): qmap [..., 3] (T1, T2, PD) ->
        (X, idx [...] 1-based nearest dictionary entry).  mode 'real' (:91-98): X [..., s] float32, |PD| and the sign of channel 1
        folded in; mode 'complex' (:100-103): PD may be complex, X [..., 2s] = the real parts of the s channels, then the imaginary
        ones.  Needs set_dictionary."""
        if mode not in ("real", "complex"):
            raise ValueError("mode must be 'real' or 'complex'")
        qmap = np.asarray(qmap)
        if qmap.shape[-1] != 3:
            raise ValueError("qmap must have T1, T2, PD along its last dimension")
        if getattr(self, "dict_shape", None) is None:
            raise ValueError("dictionary not set")
        if mode == "real" and np.iscomplexobj(qmap):
            qmap = np.concatenate([qmap[..., :2].real, np.abs(qmap[..., 2:3])], axis=-1)     # abs(qm(:,3)), :92
        shp = qmap.shape[:-1]
        pd_im = np.ascontiguousarray(qmap[..., 2].imag.reshape(-1, order="F"), dtype=np.float64) if np.iscomplexobj(qmap) else None
        q = np.ascontiguousarray(np.asarray(qmap.real, dtype=np.float64).reshape(-1, 3, order="F").ravel(order="F"))
        npix, s = q.size // 3, self.dict_shape[1]
        nch = s if mode == "real" else 2 * s
        X = np.empty(npix * nch, np.float32)
        idx = np.empty(npix, np.int32)
        dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        if mode == "real":
            self._check(self.L.qmri_synthesize_tsmi(self.h, q.ctypes.data_as(dp), npix, X.ctypes.data_as(fp), idx.ctypes.data_as(ip)))
        else:
            self._check(self.L.qmri_synthesize_tsmi_complex(self.h, q.ctypes.data_as(dp), pd_im.ctypes.data_as(dp) if pd_im is not None else None,
                                                            npix, X.ctypes.data_as(fp), idx.ctypes.data_as(ip)))
        return X.reshape(shp + (nch,), order="F"), idx.reshape(shp, order="F")

    # -- LRTV option ---------------------------------------------------------------------------------
    def lrtv(self, y, K=4e-5, iters=200, step=None, tol=1e-4, backtrack=True, prox_tol=None, prox_maxit=None):
        """x = FISTA_deep(data, param)  (FISTA_deep.m:1, parameters of main_recon_tsmis_FFT.m:274-281).
        Returns (x [N,M,s] complex, info dict)."""
        if not hasattr(self, "N"):
            raise ValueError("operator not set")
        N, M, s = self.N, self.M, self.s
        p = LrtvParams(float(K), int(iters), float(step) if step else 0.0, float(tol), int(bool(backtrack)),
                       float(prox_tol) if prox_tol else 0.0, int(prox_maxit) if prox_maxit else 0)
        yb = _cbuf(y)
        if yb.size != self.m:
            raise ValueError(f"y must have {self.m} elements")
        x = np.empty(N * M * s, np.complex128)
        info = LrtvInfo()
        self._check(self.L.qmri_lrtv(self.h, _vp(yb), C.byref(p), _vp(x), C.byref(info)))
        return x.reshape((N, M, s), order="F"), {k: getattr(info, k) for k, _ in LrtvInfo._fields_}

    def prox_tv(self, b, gamma, tol=10e-4, maxit=200):
        """[sol, info] = prox_tv(b, gamma)  (unlocbox/prox/prox_tv.m:1) on a real 2-D image.  Returns (sol, iters, obj)."""
        b = np.asfortranarray(b, dtype=np.float64)
        if b.ndim != 2:
            raise ValueError("b must be a 2-D image")
        sol = np.empty_like(b, order="F")
        it, obj = C.c_int32(0), C.c_double(0.0)
        dp = C.POINTER(C.c_double)
        self._check(self.L.qmri_prox_tv(self.h, b.ctypes.data_as(dp), b.shape[0], b.shape[1], float(gamma), float(tol), int(maxit),
                                        sol.ctypes.data_as(dp), C.byref(it), C.byref(obj)))
        return sol, int(it.value), float(obj.value)

    def norm_tv(self, I):
        """y = norm_tv(I)  (unlocbox/utils/norm_tv.m:1)."""
        I = np.asfortranarray(I, dtype=np.float64)
        if I.ndim != 2:
            raise ValueError("I must be a 2-D image")
        out = C.c_double(0.0)
        self._check(self.L.qmri_norm_tv(self.h, I.ctypes.data_as(C.POINTER(C.c_double)), I.shape[0], I.shape[1], C.byref(out)))
        return float(out.value)

    def dict_match(self, X, sel=None, want_mt=True, want_dm=True, want_xfit=False, refine=False):
        """out = mrf_dtm_cpu(dict, data, par)  (mrf_dtm_cpu.m:1).  X [..., s] complex -> dict of arrays; want_xfit adds Xfit [..., s]
        complex64 (par.f.Xout, :95,129-134).  sel (the leading shape of X, e.g. a measured B1 map): the grouped match (extension;
        set_dictionary_groups) -- every pixel against the atoms of the group nearest its value, "grp" (1-based, 0 = unmatched: a non-finite value,
        all outputs zero) added to the result.  refine=True (extension; set_refine): the match, then dict_refine started at its dm --
        "qmap_refined", "pd_refined", "refine_res", "refine_t" and "refine_flags" added, everything else unchanged."""
        if refine:
            if getattr(self, "refine_cols", None) is None:
                raise ValueError("set_refine first")
            out = self.dict_match(X, sel=sel, want_mt=want_mt, want_dm=True, want_xfit=want_xfit)
            r = self.dict_refine(X, out["dm"], want_centre=False)
            out.update(qmap_refined=r["qmap"], pd_refined=r["pd"], refine_res=r["res"], refine_t=r["t"], refine_flags=r["flags"])
            if not want_dm:
                del out["dm"]
            return out
        X = np.asarray(X, dtype=np.complex128)
        K, s, Q = self.dict_shape
        if X.shape[-1] != s:
            raise ValueError("last dimension of X must equal the dictionary's channel count")
        lead = X.shape[:-1]
        npix = int(np.prod(lead))
        xb = np.ascontiguousarray(X.reshape((npix, s), order="F").ravel(order="F"))
        qmap = np.empty(npix * Q, np.float32)
        pd = np.empty(2 * npix, np.float32)
        mt = np.empty(npix, np.float32) if want_mt else None
        dm = np.empty(npix, np.int32) if want_dm else None
        xfit = np.empty(2 * npix * s, np.float32) if want_xfit else None
        f, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        outs = (qmap.ctypes.data_as(f), pd.ctypes.data_as(f), mt.ctypes.data_as(f) if mt is not None else None, dm.ctypes.data_as(ip) if dm is not None else None)
        xf = xfit.ctypes.data_as(f) if xfit is not None else None
        grp = None
        if sel is None:
            self._check(self.L.qmri_dict_match_xfit(self.h, _vp(xb), npix, *outs, xf))
        else:
            sel = np.asarray(sel, dtype=np.float64)
            if sel.shape != lead:
                raise ValueError(f"sel must have the leading shape of X, {lead}, not {sel.shape}")
            sb = np.ascontiguousarray(sel.ravel(order="F"))
            grp = np.empty(npix, np.int32)
            self._check(self.L.qmri_dict_match_grouped(self.h, _vp(xb), npix, sb.ctypes.data_as(C.POINTER(C.c_double)), *outs, grp.ctypes.data_as(ip), xf))
        out = {"qmap": qmap.reshape(lead + (Q,), order="F"), "pd": pd.view(np.complex64).reshape(lead, order="F")}
        if grp is not None:
            out["grp"] = grp.reshape(lead, order="F")
        if xfit is not None:
            out["Xfit"] = xfit.view(np.complex64).reshape(lead + (s,), order="F")
        if mt is not None:
            out["mt"] = mt.reshape(lead, order="F")
        if dm is not None:
            out["dm"] = dm.reshape(lead, order="F")
        return out

    def dict_match_dev(self, d_X: int, npix: int, d_qmap: int = 0, d_pd: int = 0, d_mt: int = 0, d_dm: int = 0, d_xfit: int = 0, d_sel: int = 0, d_grp: int = 0):
        """qmri_dict_match_xfit_dev: device pointers (X Npix x s complex double column-major; outputs as qmri.h lays them out), asynchronous on
        the engine's stream.  d_sel (Npix doubles): the grouped match, qmri_dict_match_grouped_dev, with d_grp (Npix int32) as a further output."""
        if d_sel:
            self._check(self.L.qmri_dict_match_grouped_dev(self.h, C.c_void_p(d_X), int(npix), C.c_void_p(d_sel), C.c_void_p(d_qmap or None), C.c_void_p(d_pd or None),
                                                           C.c_void_p(d_mt or None), C.c_void_p(d_dm or None), C.c_void_p(d_grp or None), C.c_void_p(d_xfit or None)))
            return
        self._check(self.L.qmri_dict_match_xfit_dev(self.h, C.c_void_p(d_X), int(npix), C.c_void_p(d_qmap or None), C.c_void_p(d_pd or None),
                                                    C.c_void_p(d_mt or None), C.c_void_p(d_dm or None), C.c_void_p(d_xfit or None)))

    # -- profiling -----------------------------------------------------------------------------------
    def profile_enable(self, level: int):
        self._check(self.L.qmri_profile_enable(self.h, int(level)))

    def profile_get(self, reset=True) -> dict:
        p = Profile()
        self._check(self.L.qmri_profile_get(self.h, C.byref(p), int(reset)))
        return {k: getattr(p, k) for k, _ in Profile._fields_}
