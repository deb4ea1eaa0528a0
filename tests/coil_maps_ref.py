"""numpy restatement of the coil-map estimate (include/qmri.h, "coil sensitivity maps from calibration data"): the
adaptive-combine estimator of Walsh, Gmitro & Marcellin (MRM 2000) per slice.  Arrays are [N, M, ncoil] (the Engine's layout); the eigenpair comes
from numpy.linalg.eigh of the explicitly formed R(r), so the device's power iteration is held to the definition, not to an iteration of its own kind."""
import numpy as np


def hann(c):
    a = np.arange(c)
    return 0.5 * (1.0 + np.cos(2.0 * np.pi * (a - c // 2) / c))


def calib_images(block, N, M, window=True):
    """block [cN, cM, ncoil], index (cN/2, cM/2) is k = 0, values fftshift(fft2(.)) / sqrt(NM) -> I [N, M, ncoil] = sqrt(NM) ifft2(ifftshift(P(w block)))."""
    cN, cM, nc = block.shape
    assert cN % 2 == 0 and cM % 2 == 0 and 8 <= cN <= N and 8 <= cM <= M
    w = np.outer(hann(cN), hann(cM)) if window else np.ones((cN, cM))
    P = np.zeros((N, M, nc), np.complex128)
    a0, b0 = N // 2 - cN // 2, M // 2 - cM // 2
    P[a0:a0 + cN, b0:b0 + cM] = block * w[:, :, None]
    return np.sqrt(N * M) * np.fft.ifft2(np.fft.ifftshift(P, axes=(0, 1)), axes=(0, 1))


def centre_block(img, cN, cM):
    """The calibration block of coil images [N, M, ncoil]: the centre crop of fftshift(fft2(.)) / sqrt(NM)."""
    N, M = img.shape[:2]
    K = np.fft.fftshift(np.fft.fft2(img, axes=(0, 1)), axes=(0, 1)) / np.sqrt(N * M)
    a0, b0 = N // 2 - cN // 2, M // 2 - cM // 2
    return K[a0:a0 + cN, b0:b0 + cM]


def patch_cov(I, p):
    """R [N, M, ncoil, ncoil]: R(r) = sum_{d in [-p, p]^2} I(r + d) I(r + d)^H, terms outside the grid dropped."""
    N, M, nc = I.shape
    Q = I[:, :, :, None] * np.conj(I[:, :, None, :])
    Z = np.zeros((N + 2 * p, M + 2 * p, nc, nc), np.complex128)
    Z[p:p + N, p:p + M] = Q
    R = np.zeros_like(Q)
    for d2 in range(2 * p + 1):
        for d1 in range(2 * p + 1):
            R += Z[d1:d1 + N, d2:d2 + M]
    return R


def _unit_phase(z):
    m = np.abs(z)
    return np.where(m > 0, z / np.where(m > 0, m, 1.0), 1.0)


def coil_maps_ref(calib, N, M, kind="kspace", patch=3, window=True, phase_ref="object", thresh=0.0, full=False):
    """-> (maps [N, M, ncoil], img [N, M], lambda1 [N, M]); full: also (lambda2 [N, M], kept [N, M] bool, I, ref coil)."""
    I = calib_images(calib, N, M, window) if kind == "kspace" else np.asarray(calib, np.complex128)
    assert I.shape[:2] == (N, M)
    nc = I.shape[2]
    R = patch_cov(I, patch)
    lam, U = np.linalg.eigh(R)                                  # ascending
    l1, u = lam[..., -1], U[..., -1]
    l2 = lam[..., -2] if nc > 1 else np.zeros_like(l1)
    ref = int(np.argmax(np.sum(np.abs(I) ** 2, axis=(0, 1))))   # lowest index on ties
    if phase_ref == "object":
        ph = _unit_phase(np.sum(np.conj(u) * I, axis=2))
    else:
        ph = np.conj(_unit_phase(u[..., ref]))
    C = u * ph[..., None]
    kept = np.ones((N, M), bool) if thresh <= 0 else ~(l1 < thresh * thresh * l1.max())
    C = np.where(kept[..., None], C, 0.0)
    img = np.sum(np.conj(C) * I, axis=2)
    if full:
        return C, img, l1, l2, kept, I, ref
    return C, img, l1
