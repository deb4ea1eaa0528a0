"""CPU restatement of PnP-ADMM with complex TSMIs (include/qmri.h QMRI_DENOISER_COMPLEX), built on the oracle's
x-update (Operator.lsqr / lsqr_mc) and single-precision network (Net.denoise).  The loop is PnP_ADMM.m:76-146 with Step 2 replaced by

    v = x + uold ; V = cat(3, real(v), imag(v)) ; [V, lo, range] = norm_zero_to_one(V) (one min / max over all 2s planes)
    multi_level: V = cat(3, V, noise_map) ; V = net(V) ; V = V * range + lo ; v = complex(V(:,:,1:s), V(:,:,s+1:2s))
    uold = uold + x - v

tsmi_domain="real" is the reference's own Step 2 (v = real(x + uold)), so the same function gives both sides of a real / complex comparison."""
import numpy as np


def stack(v):
    """N x M x s complex -> N x M x 2s real, cat(3, real(v), imag(v))."""
    return np.concatenate([v.real, v.imag], axis=2)


def normalise(x, u, tsmi_domain="complex", multi_level=False, noise_std=0.01):
    """Step 2 up to the network: (V, lo, range)."""
    w = stack(x + u) if tsmi_domain == "complex" else np.real(x + u)
    lo, hi = w.min(), w.max()
    rng = hi - lo
    V = (w - lo) / rng
    if multi_level:
        V = np.concatenate([V, np.full(V.shape[:2] + (1,), noise_std)], axis=2)
    return V, lo, rng


def unnormalise(I, lo, rng, s, tsmi_domain="complex"):
    """Network output -> v (complex N x M x s)."""
    W = I * rng + lo
    if tsmi_domain == "complex":
        return W[:, :, :s] + 1j * W[:, :, s:2 * s]
    return W[:, :, :s] + 0j


def pnp_admm(op, net, y, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, multi_level=False, noise_std=0.01, x0=None,
             tsmi_domain="complex", maps=None, gt=None, want_diag=False, solver="lsqr"):
    """Returns (x, diag [iters, 2] or None, lsqr_iters).  maps (the layout of oracle.Operator.forward_mc) switches to the multi-coil
    x-update (lsqr_mc); diag follows PnP_ADMM.m:106-107 (||y - Ax|| / ||y||, ||gt - x|| / ||gt||)."""
    s = op.s
    if maps is None:
        x = np.asarray(x0, np.complex128).copy() if x0 is not None else op.adjoint(y)
    else:
        x = np.asarray(x0, np.complex128).copy() if x0 is not None else op.adjoint_mc(y, maps)
    v = x.copy()
    u = np.zeros_like(x)
    li = np.zeros(iters, np.int32)
    diag = np.zeros((iters, 2)) if want_diag else None
    for it in range(iters):
        if solver == "direct":
            x = op.direct(y, v - u, gamma)
        elif maps is None:
            x, li[it], _, _ = op.lsqr(y, v - u, gamma, cg_tol, cg_maxit, x0=x)
        else:
            x, li[it], _ = op.lsqr_mc(y, maps, v - u, gamma, cg_tol, cg_maxit, x0=x)
        if want_diag:
            r = y - (op.forward(x) if maps is None else op.forward_mc(x, maps))
            diag[it, 0] = np.linalg.norm(r) / np.linalg.norm(y)
            diag[it, 1] = np.linalg.norm(gt - x) / np.linalg.norm(gt) if gt is not None else np.nan
        V, lo, rng = normalise(x, u, tsmi_domain, multi_level, noise_std)
        v = unnormalise(net.denoise(V), lo, rng, s, tsmi_domain)
        u = u + x - v
    return x, diag, li
