"""TEST HELPER: numpy restatement of the coil compression (include/qmri.h qmri_coil_compress), the checker of
tests/test_gpu_coil_compress.py.  Written from the definition, not from the kernels: whitening by a triangular solve per sample, K summed over
the samples, numpy.linalg.eigh, the phase rule, the energy rule, W = L^-H U_nv, y' = U_nv^H y~, maps' = W^H maps."""
import numpy as np


def phase_fix(U):
    """Every column scaled so that its entry of largest magnitude (lowest index on ties) is real and positive."""
    U = np.array(U, dtype=np.complex128, copy=True)
    for l in range(U.shape[1]):
        k = int(np.argmax(np.abs(U[:, l])))
        mag = abs(U[k, l])
        if mag > 0:
            U[:, l] *= np.conj(U[k, l]) / mag
            U[k, l] = mag
    return U


def eig_desc(K):
    lam, U = np.linalg.eigh(K)
    order = np.argsort(-lam, kind="stable")
    return lam[order], phase_fix(U[:, order])


def choose_nv(lam, energy):
    c = np.cumsum(lam)
    return int(np.argmax(c >= energy * c[-1])) + 1 if np.any(c >= energy * c[-1]) else len(lam)


def coil_compress(ys, maps=None, noise_cov=None, nv=0, energy=0.99, shared=False):
    """ys [S, m, ncoil], maps [S, N, M, ncoil] or None.  Returns dict(y, maps, W, eig, nv) as Engine.coil_compress."""
    ys = np.asarray(ys, np.complex128)
    S, m, nc = ys.shape
    if noise_cov is not None:
        L = np.linalg.cholesky(noise_cov)
        yt = np.stack([np.linalg.solve(L, ys[b].T).T for b in range(S)])      # y~_i = L^-1 y_i, every sample
    else:
        L, yt = None, ys
    Ks = [yt[b].T @ yt[b].conj() for b in range(S)]                           # K = sum_i y~_i y~_i^H
    if shared:
        Ks = [sum(Ks[1:], Ks[0])]
    eig, Us = zip(*[eig_desc(K) for K in Ks])
    if nv == 0:
        nv = max(choose_nv(l, energy) for l in eig)
    Un = [U[:, :nv] for U in Us]
    Ws = [np.linalg.solve(L.conj().T, U) if L is not None else U for U in Un]
    pick = (lambda b: 0) if shared else (lambda b: b)
    out = {"nv": nv, "eig": np.stack(eig), "W": np.stack(Ws), "maps": None,
           "y": np.stack([yt[b] @ Un[pick(b)].conj() for b in range(S)])}
    if maps is not None:
        maps = np.asarray(maps, np.complex128)
        out["maps"] = np.stack([maps[b] @ Ws[pick(b)].conj() for b in range(S)])
    return out
