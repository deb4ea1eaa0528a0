"""Slice batches: the only parallelism the hot path has.

Slices are independent (`PnP_ADMM.m:76-146` touches only its own y, x, v, u), so a batch is sharded over GPUs
with no collective: `shard_slices` is the rank -> slice assignment used by bench.py under torchrun (one process
per GPU), `recon_batch` drives `qmri_recon_batch` (one host thread + one context per device inside one process,
the shape a single MATLAB session needs).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import AdmmParams, CcParams, NetDesc, Problem


def shard_slices(nslices: int, world: int, rank: int) -> list:
    """Static block partition of slice ids over ranks: contiguous, sizes differ by at most one."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError("bad world / rank")
    base, extra = divmod(nslices, world)
    start = rank * base + min(rank, extra)
    return list(range(start, start + base + (1 if rank < extra else 0)))


def recon_batch(devices, Y, N, M, V, frame_ptr, kidx, weights, in_nc=10, out_nc=10, nc=(64, 128, 256, 512), nb=4,
                dictionary=None, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, solver="lsqr", multi_level=False,
                noise_std=0.01, slices_per_launch=1, coil_maps=None, coil_compress=None, noise_cov=None, tsmi_domain="real"):
    """Reconstruct Y[nslices, m] on the given devices; returns dict(X [nslices,N,M,s], qmap, pd).

    coil_maps [nslices, N, M, ncoil] (multi-coil extension, no reference counterpart): Y is then [nslices, m, ncoil], every slice is reconstructed
    with its own maps through qmri_recon_batch_mc (LSQR solver only).  Without coil_maps nothing changes.

    coil_compress (with coil_maps): an int nv, or a dict of qmri_cc_params fields (nv, energy, shared), and noise_cov [ncoil, ncoil] (or None):
    every launch compresses its slices to nv virtual coils on the device, one W per slice (whitened by noise_cov), before the reconstruction
    (qmri_recon_batch_mc_cc; the library refuses energy and shared there).  Without coil_compress nothing changes.

    tsmi_domain "complex": complex TSMIs (engine.denoiser_type); the network then has in_nc = 2s (+1) and out_nc = 2s."""
    from .engine import denoiser_type
    dtype = denoiser_type(multi_level, tsmi_domain)
    L = _lib.lib()
    ncoil, Mb = 0, None
    cc = None
    if coil_compress is not None or noise_cov is not None:
        if coil_maps is None:
            raise ValueError("coil_compress / noise_cov need coil_maps (multi-coil stacks)")
        if coil_compress is None:
            raise ValueError("noise_cov is used by the coil compression: give coil_compress too")
        d = {"nv": int(coil_compress)} if np.isscalar(coil_compress) else dict(coil_compress)
        if set(d) - {"nv", "energy", "shared"}:
            raise ValueError("coil_compress takes the fields nv, energy, shared")
        cc = CcParams(int(d.get("nv", 0)), float(d.get("energy", 0.0)), int(bool(d.get("shared", False))))
    if coil_maps is not None:
        from .engine import _cbuf
        cm, Yc = np.asarray(coil_maps), np.asarray(Y)
        if cm.ndim != 4 or cm.shape[1:3] != (N, M) or Yc.ndim != 3 or Yc.shape[0] != cm.shape[0] or Yc.shape[2] != cm.shape[3]:
            raise ValueError("coil_maps must be [nslices, N, M, ncoil] and Y [nslices, m, ncoil]")
        if solver != "lsqr":                                           # (the workers plan gridded masks only: no trajectory for "toeplitz" to run on)
            raise ValueError("the multi-coil reconstruction uses the LSQR solver")
        ncoil = int(cm.shape[3])
        Mb = np.ascontiguousarray(np.concatenate([_cbuf(cm[b]) for b in range(cm.shape[0])]))
        Y = np.stack([_cbuf(Yc[b]) for b in range(Yc.shape[0])])
        if noise_cov is not None:
            noise_cov = np.asarray(noise_cov)
            if noise_cov.shape != (ncoil, ncoil):
                raise ValueError(f"noise_cov must be [{ncoil}, {ncoil}]")
            noise_cov = _cbuf(noise_cov)
    Y = np.ascontiguousarray(Y, dtype=np.complex128)
    nsl, m = Y.shape
    m //= max(ncoil, 1)
    from .engine import real_dictionary_array
    V = real_dictionary_array(V, "V", np.float64)
    T, s = V.shape
    Vf = np.ascontiguousarray(V.ravel(order="F"))
    fp = np.ascontiguousarray(frame_ptr, dtype=np.int32)
    kk = np.ascontiguousarray(kidx, dtype=np.int32)
    if int(fp[-1]) != m:
        raise ValueError("Y does not match the operator's measurement count")
    w = np.ascontiguousarray(weights, dtype=np.float32)
    desc = NetDesc(0, in_nc, out_nc, (C.c_int32 * 4)(*[int(v) for v in nc]), nb, 0)
    f, d, i32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pb = Problem()
    pb.N, pb.M, pb.s, pb.T = N, M, s, T
    pb.V, pb.frame_ptr, pb.kidx = Vf.ctypes.data_as(d), fp.ctypes.data_as(i32), kk.ctypes.data_as(i32)
    pb.net = C.pointer(desc)
    pb.weights, pb.weights_nbytes = w.ctypes.data_as(f), w.nbytes
    keep = []
    if dictionary is not None:
        D = np.ascontiguousarray(real_dictionary_array(dictionary["D"], "dict.D", np.float32).ravel(order="F"))
        lut = np.asarray(dictionary["lut"], np.float32)
        lf = np.ascontiguousarray(lut.ravel(order="F"))
        nd = np.ascontiguousarray(dictionary["normD"], dtype=np.float32)
        keep += [D, lf, nd]
        pb.K, pb.Q = int(np.asarray(dictionary["D"]).shape[0]), int(lut.shape[1])
        pb.D, pb.normD, pb.lut = D.ctypes.data_as(f), nd.ctypes.data_as(f), lf.ctypes.data_as(f)
    else:
        pb.K, pb.Q = 0, 0
    pb.admm = AdmmParams(float(gamma), int(iters), float(cg_tol), int(cg_maxit), 0 if solver == "lsqr" else 1,
                         dtype, float(noise_std), 0)
    pb.slices_per_launch = int(slices_per_launch)
    n = N * M * s
    X = np.empty((nsl, n), np.complex128)
    qmap = np.empty((nsl, N * M * max(pb.Q, 1)), np.float32) if dictionary is not None else None
    pd = np.empty((nsl, N * M), np.complex64) if dictionary is not None else None
    devs = (C.c_int * len(devices))(*[int(v) for v in devices])
    err = C.create_string_buffer(1024)
    outs = (X.ctypes.data_as(C.c_void_p), qmap.ctypes.data_as(f) if qmap is not None else None, pd.ctypes.data_as(f) if pd is not None else None,
            err, len(err))
    if cc is not None:
        st = L.qmri_recon_batch_mc_cc(len(devices), devs, nsl, C.byref(pb), ncoil, Mb.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p), *outs,
                                      noise_cov.ctypes.data_as(C.c_void_p) if noise_cov is not None else None, C.byref(cc))
    elif ncoil:
        st = L.qmri_recon_batch_mc(len(devices), devs, nsl, C.byref(pb), ncoil, Mb.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p), *outs)
    else:
        st = L.qmri_recon_batch(len(devices), devs, nsl, C.byref(pb), Y.ctypes.data_as(C.c_void_p), *outs)
    if st != 0:
        from .engine import QmriError
        raise QmriError(st, err.value.decode())
    out = {"X": X.reshape((nsl, N, M, s), order="C").copy()}
    out["X"] = np.stack([X[i].reshape((N, M, s), order="F") for i in range(nsl)])
    if dictionary is not None:
        out["qmap"] = np.stack([qmap[i].reshape((N, M, pb.Q), order="F") for i in range(nsl)])
        out["pd"] = np.stack([pd[i].reshape((N, M), order="F") for i in range(nsl)])
    return out
