"""The harness around the hot path: what `main_recon_tsmis_FFT.m` does before and after `PnP_ADMM` / `mrf_dtm_cpu`
 -- load the `.mat` inputs, crop, subsample + noise, reconstruct, match, and the metrics
the script prints -- so that someone holding the reference's data files gets the script's numbers from this engine.
Host logic in numpy/scipy; the reconstruction and the match run on the GPU through `reference_api`.

  load_mat(path)                       `load(...)` of a MATLAB file: v5/v7 (scipy.io) or -v7.3 (HDF5; mat73.py, no HDF5 library needed)
  load_dictionary(path)                `load(dict_dir); V = real(dict.V)`                     main_recon_tsmis_FFT.m:121-130
  compress_dictionary(dic, s | energy) an uncompressed (s = T) dictionary -> the SVD-compressed fields, on the GPU (extension)
  simulate_dictionary(alpha, tr, te, t1_grid, t2_grid, s | energy)  a FISP dictionary by extended phase graphs, simulated and compressed on the GPU
                                       (extension)
  load_tsmi(path) / crop_tsmi(X)       `load(tsmi_dir); X0 = X((4:227),(4:227),:)`            :199-212
  load_qmaps(path, slice)              qmap(slice,:,:,:) -> N x M x 3, cropped the same way   :177-189
  getmask_fromPD(PD, thresh)           foreground mask                                         getmask_fromPD.m:9-15
  awgn_measured(y, snr_db, seed)       `awgn(Y, snr, 'measured')` with an explicit seed       :243
  psnr(A, ref) / ssim(A, ref)          MATLAB `psnr` / `ssim` defaults for double images [MathWorks]   :352-372
  metrics(qmap, qmap0, mask, X, X0)    the block :327-374 as a dict
  synthesize_tsmis(qmap, dictionary)   main_synthesize_tsmis.m:76-100: quantitative maps -> TSMIs (GPU)
  training_volume / save_training_pickle   the `.mat` -> training-pickle layout of main_save_python_tsmis.py:132-190
  recon_tsmis(...)                     the script's main flow for recon_method 'SVD_MRF' | 'LRTV' | 'PnP_ADMM'  :263-319

[MathWorks] functions are restated from their documented defaults (no MATLAB here: parity unpinned for them, see
DESIGN.md section 10): psnr peak value 1 for class double; ssim with an isotropic Gaussian of sigma 1.5 truncated at
radius ceil(3 sigma) = 5 (11 x 11), border replication, exponents 1, C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = 1 for double,
mean over all pixels; imfill(I, 8, 'holes') followed by `> 0` = every zero pixel that is not 8-connected to the border
through zeros becomes foreground.
"""
from __future__ import annotations

import numpy as np

__all__ = ["load_mat", "load_dictionary", "compress_dictionary", "simulate_dictionary", "uncertainty_maps", "estimate_b1", "load_tsmi", "crop_tsmi", "load_qmaps", "getmask_fromPD", "awgn_measured",
           "psnr", "ssim", "metrics", "recon_tsmis", "synthesize_tsmis", "training_volume", "save_training_pickle"]

CROP = slice(3, 227)          # MATLAB (4:227): 230 -> 224                                       main_recon_tsmis_FFT.m:189,212


# ------------------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------------------
def load_mat(path):
    """dict of the variables in a MATLAB file; structs become objects with attribute access.  v5 / v7 files go through scipy.io,
    -v7.3 files (HDF5 containers) through the dependency-free reader in mat73.py -- same shapes, same squeezing."""
    from . import mat73
    if mat73.is_mat73(path):
        return mat73.load_mat73(path, squeeze_me=True)
    import scipy.io
    return {k: v for k, v in scipy.io.loadmat(path, squeeze_me=True, struct_as_record=False).items() if not k.startswith("__")}


def load_dictionary(path):
    """`load(dict_dir)` -> the fields the path uses: V (T x s, real part taken as in :129), D (K x s), normD (K), lut (K x Q)."""
    d = load_mat(path)
    if "dict" not in d:
        raise KeyError(f"{path} holds no variable 'dict'")
    s = d["dict"]
    from .engine import real_dictionary_array
    # V: real(dict.V) as :129 takes it.  D: used as stored by mrf_dtm_cpu.m:91 -- a complex-typed D must have a zero imaginary part
    out = {"V": np.real(np.asarray(s.V)).astype(np.float64), "D": real_dictionary_array(s.D, "dict.D", np.float32),
           "lut": np.asarray(s.lut, dtype=np.float32)}
    out["normD"] = np.asarray(s.normD, dtype=np.float32).ravel() if hasattr(s, "normD") else np.linalg.norm(out["D"], axis=1).astype(np.float32)
    return out


def compress_dictionary(dic, s=None, energy=None, s_max=16, device=0):
    """An uncompressed dictionary -- D K x T unit-norm fingerprints with normD and lut, as synth.make_dictionary(uncompressed=True) and the s = T
    files give it -- compressed to its SVD subspace on the GPU (Engine.compress_dictionary; an extension, the reference only loads compressed
    files).  The fingerprints are re-scaled to F = normD .* D first.  Give the rank s or the energy to keep.  Returns the fields of
    load_dictionary (V, D, normD, lut) plus eig and info; recon_tsmis runs on the result unchanged."""
    from .engine import Engine, real_dictionary_array
    D = real_dictionary_array(dic["D"], "dict.D", np.float64)
    nd = np.asarray(dic["normD"], dtype=np.float64).ravel() if dic.get("normD") is not None else np.ones(D.shape[0])
    if D.ndim != 2 or nd.shape != (D.shape[0],):
        raise ValueError("the dictionary must hold D [K, T] and normD [K]")
    eng = Engine(device)
    try:
        out = eng.compress_dictionary(D * nd[:, None], s=s, energy=energy, s_max=s_max)
    finally:
        eng.close()
    return {"V": out["V"], "D": out["D"], "normD": out["normD"], "lut": np.asarray(dic["lut"], dtype=np.float32), "eig": out["eig"], "info": out["info"]}


def simulate_dictionary(alpha, tr, te, t1_grid, t2_grid, s=None, energy=None, nstates=32, inversion=True, ti=0.0, inv_eff=1.0, b1=None, s_max=16,
                        device=0, b1_grid=None, slice_profile=None, slice_weights=None, crb=False, blocks=None, ncycles=1):
    """A FISP-MRF dictionary from a flip-angle train: the fingerprints of every (T1, T2) of the grid by extended phase graphs
    (Engine.simulate_dictionary), then their SVD compression (Engine.compress_dictionary) on the same device buffer -- the K x T fingerprints
    never cross to the host.  An extension; the reference only loads compressed files.  The atoms are the ij-meshgrid of t1_grid and t2_grid as
    synth.make_dictionary orders it (T2 fastest), lut = (T1, T2).  Atoms with T2 > T1 are kept: a caller who wants only the physical ones filters
    the grid (or the result) itself.  b1: one transmit scale for all atoms, or None.  Give the rank s or the energy to keep.  Returns the fields
    of load_dictionary (V, D, normD, lut) plus eig and info; recon_tsmis runs on the result unchanged.
    b1_grid (ascending transmit scales, instead of b1): a B1-resolved dictionary -- the (T1, T2) atoms of b1_grid[0], then
    those of b1_grid[1], ... in one simulation with one joint SVD; lut = (T1, T2, b1) and the result carries group_ptr and group_val, which
    recon_tsmis(..., b1_map=...) hands to the grouped match.
    slice_profile [Q] or [T, Q], slice_weights [Q] (default 1 / Q): every atom is integrated over that slice profile (Engine.simulate_dictionary;
    DESIGN.md section 26).  It composes with b1 and b1_grid -- the flip angle of sub-slice q is alpha_t b1 slice_profile[t, q] -- and leaves the
    atom order, lut and groups unchanged.
    crb=True: after the compression the Cramer-Rao bound of every atom in the dictionary's own subspace V (Engine.dictionary_crb, DESIGN.md
    section 32; with respect to (T1, T2), and b1 as well with b1_grid) is added as crb [K, 1 + P] and crb_flags [K]; uncertainty_maps turns them
    into per-pixel standard deviations.  Not available with a slice profile.  The default returns exactly the dict described above.
    blocks (with ncycles): the fingerprints are those of a prepared, repeated train (Engine.simulate_dictionary_seq; DESIGN.md section 33;
    synth.repeated_train_blocks and synth.cmrf_blocks make block lists) -- inversions are then stated in the blocks and inversion / ti / inv_eff
    are not used; everything after the simulation (compression, b1_grid groups, lut) is unchanged.  The schedule has neither a slice-profile nor a
    derivative form: blocks together with slice_profile or crb=True is refused."""
    from .engine import Engine
    if blocks is not None and (slice_profile is not None or slice_weights is not None):
        raise ValueError("blocks are not available with a slice profile: qmri_dict_simulate_seq has no slice-profile form")
    if blocks is not None and crb:
        raise ValueError("blocks are not available with crb=True: qmri_dict_simulate_seq has no derivative form")
    if crb and (slice_profile is not None or slice_weights is not None):
        raise ValueError("crb=True is not available with a slice profile")
    t1g, t2g = np.asarray(t1_grid, dtype=np.float64).ravel(), np.asarray(t2_grid, dtype=np.float64).ravel()
    T1, T2 = (a.ravel() for a in np.meshgrid(t1g, t2g, indexing="ij"))
    groups = {}
    if b1_grid is not None:
        if b1 is not None:
            raise ValueError("give b1 or b1_grid, not both")
        bg = np.asarray(b1_grid, dtype=np.float64).ravel()
        if bg.size < 1 or bg.size > 256 or not np.all(np.isfinite(bg)) or np.any(bg < 0) or np.any(np.diff(bg) <= 0):
            raise ValueError("b1_grid must hold 1..256 finite, non-negative, strictly ascending values")
        n = T1.size
        T1, T2, b1 = np.tile(T1, bg.size), np.tile(T2, bg.size), np.repeat(bg, n)                # group-major
        groups = {"group_ptr": (np.arange(bg.size + 1) * n).astype(np.int32), "group_val": bg.copy()}
    sp = {} if slice_profile is None and slice_weights is None else {"slice_profile": slice_profile, "slice_weights": slice_weights}
    if blocks is not None:
        sp = {"blocks": blocks, "ncycles": ncycles}
    eng = Engine(device)
    try:
        out = eng.simulate_compress_dictionary(alpha, tr, te, T1, T2, b1=b1, s=s, energy=energy, s_max=s_max, nstates=nstates, inversion=inversion,
                                               ti=ti, inv_eff=inv_eff, **sp)
        bound = {}
        if crb:
            c = eng.dictionary_crb(alpha, tr, te, T1, T2, b1=b1, wrt=("t1", "t2", "b1") if groups else ("t1", "t2"), V=out["V"], nstates=nstates,
                                   inversion=inversion, ti=ti, inv_eff=inv_eff)
            bound = {"crb": c["crb"], "crb_flags": c["flags"]}
    finally:
        eng.close()
    cols = [T1, T2] + ([b1] if groups else [])
    return {"V": out["V"], "D": out["D"], "normD": out["normD"], "lut": np.ascontiguousarray(np.stack(cols, axis=1).astype(np.float32)),
            "eig": out["eig"], "info": out["info"], **groups, **bound}


def uncertainty_maps(dictionary, dm, pd, sigma):
    """Per-pixel lower bounds on the standard deviation of matched maps, from a dictionary that carries crb and crb_flags
    (simulate_dictionary(..., crb=True)): dm [N, M] the match's 1-based atom indices (0: no atom), pd [N, M] its proton density (real or complex),
    sigma the noise's standard deviation per real and per imaginary part and channel of the TSMI that was matched.  Returns dict(std [N, M, P]:
    sigma sqrt(crb[dm - 1, 1 + q]) / |pd| for q = T1, T2 (, b1); std_pd [N, M]: sigma sqrt(crb[dm - 1, 0])).  A host gather; pixels with dm = 0,
    pd = 0 or an atom flagged singular are NaN."""
    if "crb" not in dictionary or "crb_flags" not in dictionary:
        raise ValueError("uncertainty_maps needs a dictionary with crb and crb_flags (simulate_dictionary(..., crb=True))")
    c, fl = np.asarray(dictionary["crb"], dtype=np.float64), np.asarray(dictionary["crb_flags"])
    dm, pd = np.asarray(dm), np.asarray(pd)
    if c.ndim != 2 or fl.shape != (c.shape[0],) or dm.shape != pd.shape or not (np.isfinite(sigma) and float(sigma) >= 0):
        raise ValueError("crb must be [K, 1 + P] with crb_flags [K], dm and pd of one shape, sigma finite and >= 0")
    if dm.size and (dm.min() < 0 or dm.max() > c.shape[0]):
        raise ValueError("dm must hold 1-based atom indices of the dictionary, or 0")
    k = np.maximum(dm.astype(np.int64) - 1, 0)
    ok = (dm > 0) & (pd != 0) & (fl[k] == 0)
    ck = c[k]
    with np.errstate(all="ignore"):
        std = float(sigma) * np.sqrt(ck[..., 1:]) / np.abs(pd)[..., None]
        std_pd = float(sigma) * np.sqrt(ck[..., 0])
    return {"std": np.where(ok[..., None], std, np.nan), "std_pd": np.where(ok, std_pd, np.nan)}


def crop_tsmi(X):
    """X0((4:227),(4:227),:)"""
    X = np.asarray(X)
    if X.shape[0] < 227 or X.shape[1] < 227:
        raise ValueError(f"cannot crop (4:227, 4:227) out of {X.shape}")
    return X[CROP, CROP, ...]


def load_tsmi(path, crop=True):
    d = load_mat(path)
    if "X" not in d:
        raise KeyError(f"{path} holds no variable 'X'")
    X = np.asarray(d["X"])
    return crop_tsmi(X) if crop else X


def load_qmaps(path, slice_index, crop=True):
    """qmap (slices x 3 x W x H in the file, :180 'Batch x C x W x H') -> N x M x 3 of one slice (1-based index as in the script).
    The script's permute/reshape chain (:182-186) amounts to moving the channel axis last."""
    d = load_mat(path)
    if "qmap" not in d:
        raise KeyError(f"{path} holds no variable 'qmap'")
    q = np.asarray(d["qmap"])
    if q.ndim != 4:
        raise ValueError(f"qmap has {q.ndim} dimensions, expected slices x 3 x N x M")
    q = np.transpose(q[slice_index - 1], (1, 2, 0))
    return q[CROP, CROP, :] if crop else q


# ------------------------------------------------------------------------------------------------------------
# small image-processing pieces
# ------------------------------------------------------------------------------------------------------------
def getmask_fromPD(PD, thresh):
    """getmask_fromPD.m:9-15: |PD| scaled to unit maximum, values below thresh zeroed, holes filled (8-connected
    background), then binarised."""
    from scipy import ndimage
    pd = np.abs(np.asarray(PD)).astype(np.float64)
    mx = pd.max()
    pd = pd / mx if mx > 0 else pd
    fg = pd >= thresh                                          # pd(pd < thresh) = 0 ; later mask(mask > 0) = 1
    fg &= pd > 0
    # zero pixels reachable from the border through zeros (8-connectivity) stay background, every other pixel is filled
    lab, n = ndimage.label(~fg, structure=np.ones((3, 3), bool))
    border = np.unique(np.concatenate([lab[0, :], lab[-1, :], lab[:, 0], lab[:, -1]]))
    outside = np.isin(lab, border[border > 0])
    return (~outside).astype(np.float64)


def awgn_measured(y, snr_db, seed=0):
    """`awgn(Y, snr, 'measured')` for complex Y: noise power = mean(|y|^2) / 10^(snr/10), split equally between the real
    and imaginary parts.  MATLAB draws from its global stream; here the stream is numpy's PCG64 with an explicit seed."""
    y = np.asarray(y, dtype=np.complex128)
    p = np.mean(np.abs(y) ** 2) / (10.0 ** (snr_db / 10.0))
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)
    return y + np.sqrt(p / 2.0) * n


def psnr(A, ref, peakval=1.0):
    """MATLAB psnr(A, ref) for double inputs: 10 log10(peakval^2 / mean((A - ref)^2)), peakval = 1."""
    A, ref = np.asarray(A, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if A.shape != ref.shape:
        raise ValueError("A and ref must have the same size")     # images:validate:unequalSizeMatrices
    mse = np.mean((A - ref) ** 2)
    return float("inf") if mse == 0 else float(10.0 * np.log10(peakval * peakval / mse))


def _gauss_kernel(sigma=1.5):
    r = int(np.ceil(3 * sigma))
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2 * sigma * sigma))
    return g / g.sum()


def _gfilt(img, g):
    """separable Gaussian with border replication (imfilter(..., 'replicate'))"""
    from scipy import ndimage
    return ndimage.correlate1d(ndimage.correlate1d(img, g, axis=0, mode="nearest"), g, axis=1, mode="nearest")


def ssim(A, ref, dynamic_range=1.0, sigma=1.5, K=(0.01, 0.03)):
    """MATLAB ssim(A, ref) defaults for 2-D double images; returns the global value (mean of the local map)."""
    A, ref = np.asarray(A, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if A.shape != ref.shape or A.ndim != 2:
        raise ValueError("A and ref must be 2-D images of the same size")
    g = _gauss_kernel(sigma)
    C1, C2 = (K[0] * dynamic_range) ** 2, (K[1] * dynamic_range) ** 2
    mux, muy = _gfilt(A, g), _gfilt(ref, g)
    sxx = np.maximum(_gfilt(A * A, g) - mux * mux, 0.0)
    syy = np.maximum(_gfilt(ref * ref, g) - muy * muy, 0.0)
    sxy = _gfilt(A * ref, g) - mux * muy
    num = (2 * mux * muy + C1) * (2 * sxy + C2)
    den = (mux * mux + muy * muy + C1) * (sxx + syy + C2)
    return float(np.mean(num / den))


def metrics(qmap, qmap0, foreground_mask, X=None, X0=None):
    """main_recon_tsmis_FFT.m:327-374.  qmap / qmap0: N x M x 3 (T1, T2, PD; PD may be complex), mask N x M.
    MAE inside the mask, PSNR / SSIM over the whole masked images, TSMI PSNR / SSIM as channel means of |X|."""
    qmap, qmap0 = np.asarray(qmap), np.asarray(qmap0)
    m = np.asarray(foreground_mask, dtype=np.float64)
    ind = m > 0
    out = {}
    maps = {}
    for i, name in enumerate(("t1", "t2")):
        maps[name] = (np.real(qmap[:, :, i]).astype(np.float64) * m, np.real(qmap0[:, :, i]).astype(np.float64) * m)
    pd, pd_ref = np.abs(qmap[:, :, 2] * m), np.abs(qmap0[:, :, 2] * m)
    maps["pd"] = (pd / pd.max() if pd.max() > 0 else pd, pd_ref / pd_ref.max() if pd_ref.max() > 0 else pd_ref)   # :339-342
    for name, (a, r) in maps.items():
        out[f"{name}_mae"] = float(np.mean(np.abs(a[ind] - r[ind]))) if ind.any() else float("nan")
        out[f"{name}_psnr"] = psnr(a, r)
        out[f"{name}_ssim"] = ssim(a, r)
    if X is not None and X0 is not None:
        X, X0 = np.asarray(X), np.asarray(X0)
        out["tsmi_mean_psnr"] = float(np.mean([psnr(np.abs(X[:, :, c]), np.abs(X0[:, :, c])) for c in range(X0.shape[2])]))
        out["tsmi_mean_ssim"] = float(np.mean([ssim(np.abs(X[:, :, c]), np.abs(X0[:, :, c])) for c in range(X0.shape[2])]))
    return out


def tsmi_from_stack(X):
    """The stored TSMIs of the complex synthesis mode, cat(3, real(X), imag(X)) (main_synthesize_tsmis.m:100-103): N x M x 2s real ->
    N x M x s complex (double).  Also takes a leading slice axis: [..., 2s] -> [..., s]."""
    X = np.asarray(X)
    if np.iscomplexobj(X) or X.ndim < 3 or X.shape[-1] % 2:
        raise ValueError(f"a complex-mode TSMI stack is real with an even channel count (2s) along its last axis, not {X.dtype} {X.shape}")
    s = X.shape[-1] // 2
    return X[..., :s].astype(np.float64) + 1j * X[..., s:].astype(np.float64)


def synthesize_tsmis(qmap, dictionary, device=0, mode="real"):
    """main_synthesize_tsmis.m:76-103 for one volume: qmap slices x 3 x N x M (the file layout, :180) -> X slices x N x M x C single.
    mode 'real' (:27,91-98): C = s, |PD| folded in, first SVD channel non-negative; mode 'complex' (:100-103): PD may be complex,
    C = 2s (real parts of the s channels, then the imaginary parts).  Runs on the GPU (exhaustive nearest-entry search)."""
    from . import reference_api as R
    q = np.asarray(qmap)
    q = q.astype(np.complex128 if np.iscomplexobj(q) else np.float64)
    if q.ndim != 4 or q.shape[1] != 3:
        raise ValueError("qmap must be slices x 3 x N x M")
    eng = R._engine(device)
    eng.set_dictionary(dictionary["D"], dictionary["normD"], dictionary["lut"])
    return np.stack([eng.synthesize_tsmi(np.transpose(q[i], (1, 2, 0)), mode=mode)[0] for i in range(q.shape[0])])


def training_volume(X_slices, channels_to_save=None):
    """PyTorch_Denoiser/main_save_python_tsmis.py:132-166: the TSMIs of one volume (slices x N x M x C, as synthesize_tsmis
    returns them or as loaded from the per-slice `.mat` files) -> the float64 array slices x C x N x M the training kit
    pickles (`data_slice` transposed (2,1,0) then (0,2,1), i.e. channel first); optionally only the first channels."""
    v = np.moveaxis(np.asarray(X_slices, dtype=np.float64), 3, 1)
    return np.ascontiguousarray(v if channels_to_save is None else v[:, :channels_to_save])


def save_training_pickle(path, X_slices, channels_to_save=None):
    """pickle.dump(vol_data, f) of main_save_python_tsmis.py:184-190 (file naming is the caller's)."""
    import pickle
    with open(path, "wb") as f:
        pickle.dump(training_volume(X_slices, channels_to_save), f)


def estimate_field_map(Y, echo_times, device=0, **kw):
    """The field map in Hz of multi-echo gradient-echo images, estimated on the device (Engine.estimate_field_map; an extension, DESIGN.md section
    24): Y [L, N, M], [L, C, N, M] or [S, L, C, N, M] complex, echo_times [L] seconds.  Keywords: iters, beta, phase_sign, f_init, return_info,
    return_trust.  The result is what recon_tsmis(field_map=...) and Engine.set_field_map take."""
    from . import reference_api as R
    return R._engine(device).estimate_field_map(Y, echo_times, **kw)


def resolve_components(dictionary, components):
    """components of recon_tsmis / unmix_tsmi -> 1-based atom indices int32 [C]: integers are taken as they are, (T1, T2) pairs stand for the atom whose
    first two lut columns are nearest (engine.nearest_atoms)."""
    from .engine import component_arguments, nearest_atoms
    c = np.asarray(components)
    K = np.asarray(dictionary["D"]).shape[0]
    if c.ndim == 1 and np.issubdtype(c.dtype, np.integer):
        return component_arguments(c, K)
    if c.ndim != 2 or c.shape[1] != 2 or not (1 <= c.shape[0] <= 8):
        raise ValueError("components must be 1 to 8 atom indices (integers, 1-based) or (T1, T2) pairs")
    return component_arguments(nearest_atoms(dictionary["lut"], c), K)


def unmix_tsmi(dictionary, X, components, mode="real", device=0):
    """Tissue-fraction maps of a TSMI X [N, M, s]: dict(fractions [N, M, C], component_atoms [C], unmix_res [N, M],
    unmix_weights [N, M, C], unmix_pd [N, M] complex, unmix_flags [N, M])."""
    from . import reference_api as R
    atoms = resolve_components(dictionary, components)
    eng = R._engine(device)
    eng.set_dictionary(dictionary["D"], dictionary["normD"], dictionary["lut"])
    eng.set_components(atoms)
    out = eng.tissue_fractions(X, mode=mode)
    return {"fractions": out["frac"], "component_atoms": atoms, "unmix_res": out["res"], "unmix_weights": out["w"], "unmix_pd": out["pd"],
            "unmix_flags": out["flags"]}


def resolve_refine(dictionary, refine):
    """refine of recon_tsmis -> None (False / None: no refinement) or the int32 lut columns: True stands for (0, 1) = (T1, T2)."""
    from .engine import refine_columns
    if refine is None or refine is False:
        return None
    return refine_columns((0, 1) if refine is True else refine, np.asarray(dictionary["lut"]).shape[1])


def refine_tsmi(dictionary, X, cols=(0, 1), sel=None, device=0):
    """Quantitative maps of a TSMI X [N, M, s] below the dictionary's grid: the match, then every pixel fitted to the quadratic
    through its matched atom and that atom's neighbours along the lut columns cols.  sel: the selector map of a grouped match (a dictionary with
    group_ptr / group_val).  Returns dict(qmap_refined [N, M, Q] float64, pd_refined [N, M] complex, refine_res, refine_t [N, M, P], refine_flags,
    dm, qmap, pd: the match's own)."""
    from . import reference_api as R
    from .engine import refine_columns
    c = refine_columns(cols, np.asarray(dictionary["lut"]).shape[1])
    eng = R._engine(device)
    eng.set_dictionary(dictionary["D"], dictionary["normD"], dictionary["lut"])
    if sel is not None:
        eng.set_dictionary_groups(dictionary["group_ptr"], dictionary["group_val"])
    eng.set_refine(c)
    out = eng.dict_match(X, sel=sel, refine=True)
    return {k: out[k] for k in ("qmap_refined", "pd_refined", "refine_res", "refine_t", "refine_flags", "dm", "qmap", "pd")}


def estimate_b1(dictionary, X, mask=None, window=4, device=0):
    """The B1 map of a TSMI X [N, M, s] (or [N, M, nslices, s]) estimated from the fingerprints themselves: per pixel the b1
    group of the dictionary (simulate_dictionary(..., b1_grid=...)) whose best atoms explain the most energy over the (2 window + 1)^2 window;
    T1, T2 and PD stay free per pixel.  mask: non-zero = foreground.  Returns dict(b1 (NaN = no estimate: what recon_tsmis(b1_map=...) treats as
    background), grp (1-based, 0 none), conf, info)."""
    from .engine import b1_window
    if dictionary.get("group_ptr") is None or dictionary.get("group_val") is None:
        raise ValueError("estimate_b1 needs a dictionary with group_ptr and group_val (simulate_dictionary(..., b1_grid=...))")
    b1_window(window)
    X = np.asarray(X)
    if X.ndim not in (3, 4):
        raise ValueError("X must be [N, M, s] or [N, M, nslices, s]")
    if mask is not None and np.asarray(mask).shape != X.shape[:-1]:
        raise ValueError(f"mask must have the image's shape {X.shape[:-1]}")
    from . import reference_api as R
    eng = R._engine(device)
    eng.set_dictionary(dictionary["D"], dictionary["normD"], dictionary["lut"])
    eng.set_dictionary_groups(dictionary["group_ptr"], dictionary["group_val"])
    return eng.estimate_b1(X, mask=mask, window=window)


# ------------------------------------------------------------------------------------------------------------
# the script's main flow
# ------------------------------------------------------------------------------------------------------------
def recon_tsmis(dictionary, X0, qmap0, weights=None, recon_method="PnP_ADMM", subsampling_pattern="Spiral",
                spiral_sampling_curve=771, epi_sampling_rate=1 / 65, measurements_type="noisy", measurements_noise=30,
                denoiser_type="single_level", noise_map_std=0.01, residual_noise=False, iters=100, seed=0, Y=None, device=0,
                net_arch=None, lrtv_iters=None, tsmi_domain="real", solver="lsqr", b1_map=None, density_compensation=False,
                field_map=None, readout_s=None, field_normal=None, field_echoes=None, field_echo_times=None,
                regulariser="net", llr_tau=None, llr_tau_rel=0.02, llr_block=8, wavelet_tau=None, wavelet_tau_rel=None,
                wavelet_levels=3, wavelet_filter="db2", components=None, unmix_mode="real", b1_window=4, refine=False, uncertainty=None):
    """main_recon_tsmis_FFT.m:216-374 on already loaded (and cropped) arrays.

    dictionary  dict(V, D, normD, lut) (load_dictionary);  X0  N x M x s ground-truth TSMI;  qmap0  N x M x 3
    weights     flat fp32 UNetRes weights, or the path of a `.pt` / `.onnx` file (weights.load_denoiser_weights); needed for PnP_ADMM
    Y           precomputed measurements (the script's save / load option, :248-262) instead of subsample + noise
    net_arch    dict(nc=..., nb=...) when `weights` is a flat blob of a non-default UNetRes (files carry their architecture)
    tsmi_domain "complex": X0 may be complex (tsmi_from_stack turns the stored 2s-channel layout into one) and the denoiser takes 2s (+1) ->
                2s channels, cat(3, real, imag); "real" is the reference's loop
    solver      x-update of PnP_ADMM: "lsqr" (the reference's), "direct", or with SpiralExact "toeplitz" 
    b1_map      N x M measured transmit field for a dictionary that carries group_ptr / group_val (simulate_dictionary(..., b1_grid=...)): every
                pixel is matched against the atoms of the b1 nearest its value, NaN = background, all outputs zero.
                b1_map="estimate": the map is estimated from the reconstructed TSMI itself inside the foreground mask, over windows of
                (2 b1_window + 1)^2 pixels (estimate_b1), and then takes the b1_map route unchanged; the result gains
                b1_est and b1_conf
    density_compensation  with SpiralExact: SVD_MRF is the density-compensated adjoint A^H (w .* y) and PnP_ADMM starts from it (Pipe-Menon
                weights); False (default) is the bare adjoint
    field_map, readout_s  with SpiralExact, PnP_ADMM or SVD_MRF: an N x M field map in Hz and the length of one spiral readout in seconds (sample j of a
                frame is measured at j * readout_s / S): the operator carries the off-resonance phase (time segmentation), for
                the measurements it simulates (when Y is not given) and for the reconstruction.  Absent: the operator without a map, bit for bit.
    field_echoes, field_echo_times  with field_map="estimate": [L, N, M] or [L, C, N, M] gradient-echo images and their L echo times in seconds; the
                map is estimated from them on the device first (estimate_field_map) and then takes the field_map route
                unchanged.  The result gains field_map (the estimate) and field_map_info.
    field_normal  with field_map and solver="toeplitz": True, or a dict with nseg / tol, builds the field-aware Toeplitz normal operator before the
                loop (Engine.prepare_normal_field); None or False (default): solver="toeplitz" with a field_map is refused
    regulariser   of PnP_ADMM: "net" (default) is the denoiser of `weights`; "llr" the locally low-rank proximal step, which
                needs no weights and works on every subsampling pattern: llr_block x llr_block patches (4, 8 or 16, dividing N and M), threshold
                llr_tau, or with None llr_tau_rel times sigma_max of the start image.  The result gains llr_tau, the threshold used.
                "wavelet": joint wavelet soft-thresholding, which needs no weights either and works on every subsampling
                pattern: wavelet_levels (1..4, 2^levels dividing N and M) of wavelet_filter ("haar" or "db2"), threshold wavelet_tau, or with
                None wavelet_tau_rel (None: reference_api.WAVELET_TAU_REL) times cmax of the start image.  The result gains wavelet_tau.
    components  tissue-fraction maps after the match: 1..8 (T1, T2) pairs in the units of dict.lut (each stands for the
                nearest atom) or 1-based atom indices; every pixel of the reconstructed TSMI is written as a non-negative mix of those atoms
                (unmix_mode "real": of its real part, "phase": after removing the pixel's phase).  The result gains fractions (N x M x C),
                component_atoms (C, 1-based) and unmix_res (N x M).  Absent: nothing changes.
    refine      True, or the lut columns to refine ((0, 1) = T1, T2): after the match every pixel is fitted to the quadratic through its matched atom
                and that atom's neighbours, started at the match's own dm (Engine.dict_refine).  The result gains
                qmap_refined (N x M x 3: the first two lut columns after the fit and the fit's PD -- the layout of qmap), metrics_refined (metrics
                of it, as `metrics` is of qmap), refine_qmap (N x M x Q: every lut column after the fit, so a refined third column such as b1 is
                there), refine_res and refine_flags.  False (default): nothing changes.
    uncertainty the standard deviation sigma of the noise per real and imaginary part and channel of the reconstructed TSMI, for a dictionary that
                carries crb / crb_flags (simulate_dictionary(..., crb=True)): the result gains qmap_std (N x M x P) and pd_std (N x M), the
                Cramer-Rao lower bounds of uncertainty_maps at every pixel's matched atom and PD.  None (default):
                nothing changes.
    Returns dict(X, qmap (N x M x 3: T1, T2, PD), Y, metrics, foreground_mask); with b1_map also grp (N x M, the 1-based b1 group, 0 = unmatched);
    with field_normal also field_normal_info (what prepare_normal_field reported).
    """
    from . import reference_api as R
    net_arch = dict(net_arch or {})
    if uncertainty is not None and ("crb" not in dictionary or "crb_flags" not in dictionary):
        raise ValueError("uncertainty needs a dictionary with crb and crb_flags (simulate_dictionary(..., crb=True))")
    if regulariser not in ("net", "llr", "wavelet"):
        raise ValueError(f'regulariser must be "net", "llr" or "wavelet", not {regulariser!r}')
    if regulariser != "net" and recon_method != "PnP_ADMM":
        raise ValueError(f'regulariser="{regulariser}" goes with recon_method="PnP_ADMM"')
    from .engine import denoiser_type as _dtype
    _dtype(denoiser_type == "multi_level", tsmi_domain)            # (checks tsmi_domain)
    X0 = np.asarray(X0)
    N, M, s = X0.shape
    if b1_map is not None:                                                           # (refused before anything is reconstructed)
        if dictionary.get("group_ptr") is None or dictionary.get("group_val") is None:
            raise ValueError("b1_map needs a dictionary with group_ptr and group_val (simulate_dictionary(..., b1_grid=...))")
        if isinstance(b1_map, str):
            if b1_map != "estimate":
                raise ValueError(f'b1_map must be an {N} x {M} map or "estimate", not {b1_map!r}')
            from .engine import b1_window as _b1w
            _b1w(b1_window)
        else:
            b1_map = np.asarray(b1_map, dtype=np.float64)
            if b1_map.shape != (N, M):
                raise ValueError(f"b1_map must be {N} x {M}")
    if components is not None:                                                       # (refused before anything is reconstructed)
        component_atoms = resolve_components(dictionary, components)
        from .engine import unmix_mode as _umode
        _umode(unmix_mode)
    refine_cols = resolve_refine(dictionary, refine)                                 # (refused before anything is reconstructed)
    V = np.asarray(dictionary["V"], dtype=np.float64)
    if subsampling_pattern == "Spiral":
        P = R.setup_subsampling_spiralgrided(N, M, spiral_sampling_curve, V)
    elif subsampling_pattern == "EPI":
        P = R.setup_subsampling_epi(N, M, epi_sampling_rate, V)
    elif subsampling_pattern == "SpiralExact":                                       # the spiral at its exact positions (NUFFT)
        if recon_method not in ("PnP_ADMM", "SVD_MRF"):
            raise ValueError(f"subsampling pattern SpiralExact supports PnP_ADMM and SVD_MRF, not {recon_method}")
        P = R.setup_subsampling_spiral_exact(N, M, spiral_sampling_curve, V)
    else:
        raise ValueError(f"unknown subsampling pattern {subsampling_pattern}")
    if density_compensation and subsampling_pattern != "SpiralExact":
        raise ValueError("density_compensation needs the subsampling pattern SpiralExact (a gridded mask has nothing to compensate)")
    extra_fm = {}
    if isinstance(field_map, str) or field_echoes is not None or field_echo_times is not None:
        if not (isinstance(field_map, str) and field_map == "estimate") or field_echoes is None or field_echo_times is None:
            raise ValueError('field_map="estimate", field_echoes and field_echo_times go together')
        if readout_s is None:
            raise ValueError("field_map and readout_s go together")
        if subsampling_pattern != "SpiralExact":
            raise ValueError("field_map needs the subsampling pattern SpiralExact (a gridded mask has no readout times)")
        if np.asarray(field_echoes).ndim not in (3, 4) or np.asarray(field_echoes).shape[-2:] != (N, M):
            raise ValueError(f"field_echoes must be [L, {N}, {M}] or [L, C, {N}, {M}]")
        field_map, fm_info = estimate_field_map(field_echoes, field_echo_times, device=device, return_info=True)
        extra_fm = {"field_map": field_map, "field_map_info": fm_info}
    if (field_map is None) != (readout_s is None):
        raise ValueError("field_map and readout_s go together")
    if field_map is not None and subsampling_pattern != "SpiralExact":
        raise ValueError("field_map needs the subsampling pattern SpiralExact (a gridded mask has no readout times)")
    if field_normal is False:                                                        # (as None: no field-aware normal operator)
        field_normal = None
    if field_normal is not None and (field_map is None or solver != "toeplitz" or recon_method != "PnP_ADMM"):
        raise ValueError('field_normal goes with a field_map, recon_method="PnP_ADMM" and solver="toeplitz"')
    if field_map is not None and solver == "toeplitz" and field_normal is None:
        raise ValueError('with a field_map the x-update is solver="lsqr": the Toeplitz normal operator of the corrected operator is not built')
    extra_fn = {}
    F = R.make_F(P, device=device) if field_map is None else R.make_F(P, device=device, field_map=field_map, readout_s=readout_s)
    if density_compensation:
        F._engine.density_weights()                                                  # (make_F planned the operator afresh: nothing was attached)
    if Y is None:
        Y = F.forward(X0.astype(np.complex128))                                      # :237
        if measurements_type == "noisy":
            Y = awgn_measured(Y, measurements_noise, seed=seed)                      # :243
        elif measurements_type != "clean":
            raise ValueError(f"unknown measurements type {measurements_type}")
    if recon_method == "SVD_MRF":                                                    # :270-271
        Yc = np.asarray(Y, dtype=np.complex128)
        X = F._engine.adjoint(Yc, weighted=True) if density_compensation else F.adjoint(Yc)
    elif recon_method == "PnP_ADMM":                                                 # :284-293
        if weights is None and regulariser == "net":
            raise ValueError("PnP_ADMM needs the denoiser weights")
        arch = {}
        if regulariser != "net":
            pass
        elif isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            from .weights import load_denoiser_weights
            weights, arch = load_denoiser_weights(weights)
            want = (2 * s if tsmi_domain == "complex" else 10) + (0 if denoiser_type == "single_level" else 1)
            if arch["in_nc"] != want:
                raise ValueError(f"the weight file takes {arch['in_nc']} input channels, denoiser type {denoiser_type} "
                                 f"({tsmi_domain} TSMIs) needs {want}")
        out_nc = 2 * s if tsmi_domain == "complex" else s
        if regulariser == "llr":
            net = R.make_llr(F, tau=llr_tau, tau_rel=llr_tau_rel, block=llr_block)
        elif regulariser == "wavelet":
            net = R.make_wavelet(F, tau=wavelet_tau, tau_rel=R.WAVELET_TAU_REL if wavelet_tau_rel is None else wavelet_tau_rel,
                                 levels=wavelet_levels, filter=wavelet_filter)
        else:
            net = R.make_net(weights, denoiser_type, residual_noise, H=N, W=M, out_nc=out_nc, device=device, tsmi_domain=tsmi_domain,
                             **{**net_arch, **({"nc": arch["nc"], "nb": arch["nb"]} if arch else {})})
        param = {"eta": 20, "sigma_squared": 1, "gamma": 1 / 20, "iter": iters, "cg_tol": 1e-4, "F": F, "gt_tsmi": X0,
                 "X0": None if density_compensation else F.adjoint(Y), "net": net, "denoiser_type": denoiser_type, "tsmi_domain": tsmi_domain,
                 "noise_map": R.build_noise_map(noise_map_std, N, M), "solver": solver}   # :166-171
        if density_compensation:
            param["x0"] = "dcf"
        if field_normal is not None:
            param["field_normal"] = field_normal
        X = R.PnP_ADMM(np.asarray(Y, dtype=np.complex128), param)
        if field_normal is not None:
            extra_fn = {"field_normal_info": R.PnP_ADMM.last_field_normal}
        if regulariser == "llr":
            extra_fn["llr_tau"] = net.tau
        if regulariser == "wavelet":
            extra_fn["wavelet_tau"] = net.tau
    elif recon_method == "LRTV":                                                     # :273-282
        param = {"K": 4e-5, "iter": 200 if lrtv_iters is None else int(lrtv_iters), "step": X0.size / np.asarray(Y).size, "tol": 1e-4,
                 "backtrack": 1, "usegpu": 0}
        X = R.FISTA_deep({"N": N, "M": M, "L": s,   # (the script sets data.N = M, :281: the same on its square grid)
                          "y": np.asarray(Y, dtype=np.complex128), "F": F, "D": []}, param)
    else:
        raise ValueError(f"unknown reconstruction method {recon_method}")
    par = {"f": {"qout": 1, "pdout": 1, "mtout": 0, "Xout": 0, "dmout": 0, "Yout": 0, "verbose": 0}, "fp": {"blockSize": 1e9}}   # :302-309
    extra = {**extra_fn, **extra_fm}
    if isinstance(b1_map, str):                                                      # "estimate": from X, inside the foreground mask
        est = estimate_b1(dictionary, X, mask=getmask_fromPD(np.asarray(qmap0)[:, :, 2], 0.15), window=b1_window, device=device)
        b1_map = est["b1"]
        extra["b1_est"], extra["b1_conf"] = est["b1"], est["conf"]
    if b1_map is not None:
        eng = R._engine(device)
        eng.set_dictionary(dictionary["D"], dictionary["normD"], dictionary["lut"])
        eng.set_dictionary_groups(dictionary["group_ptr"], dictionary["group_val"])
        out = eng.dict_match(X, sel=b1_map)
        out["qmap"] = out["qmap"][:, :, :2]                                          # (T1, T2); column 3 of the lut is the group's b1
        extra["grp"] = out["grp"]
    elif refine_cols is not None or uncertainty is not None:                         # what mrf_dtm_cpu does, keeping dm for what follows
        eng = R._engine(device)
        eng.set_dictionary(dictionary["D"], dictionary["normD"], dictionary["lut"])
        out = eng.dict_match(X)
    else:
        out = R.mrf_dtm_cpu(dictionary, {"X": X}, par, device=device)
    qmap = np.concatenate([np.asarray(out["qmap"], dtype=np.complex128), np.asarray(out["pd"]).reshape(N, M, 1)], axis=2)       # :316
    if components is not None:
        extra.update(unmix_tsmi(dictionary, X, component_atoms, mode=unmix_mode, device=device))
    if uncertainty is not None:                                                      # the bound at the matched atom and proton density
        um = uncertainty_maps(dictionary, out["dm"], out["pd"], uncertainty)
        extra.update(qmap_std=um["std"], pd_std=um["std_pd"])
    mask = getmask_fromPD(np.asarray(qmap0)[:, :, 2], 0.15)                          # :192
    if refine_cols is not None:                                                      # the fit, started at the dm of the match above
        eng.set_refine(refine_cols)
        rf = eng.dict_refine(X, out["dm"])
        qr = np.concatenate([np.asarray(rf["qmap"][:, :, :2], dtype=np.complex128), np.asarray(rf["pd"]).reshape(N, M, 1)], axis=2)
        extra.update(qmap_refined=qr, metrics_refined=metrics(qr, qmap0, mask, X, X0), refine_qmap=rf["qmap"], refine_res=rf["res"],
                     refine_flags=rf["flags"])
    return {"X": X, "qmap": qmap, "Y": Y, "foreground_mask": mask, "metrics": metrics(qmap, qmap0, mask, X, X0), **extra}
