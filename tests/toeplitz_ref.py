"""numpy restatement of the Toeplitz normal operator of a trajectory for the tests.

    (A^H A x)_c[n] = sum_c' sum_n' q_{c,c'}[n - n'] x_c'[n'],   q_{c,c'}[d] = (1/NM) sum_i V(t_i, c) V(t_i, c') exp(i omega_i . d)

the point-spread function q from the exact non-uniform DFT, its 2N x 2M embedding K^ (the lines d1 = -N, d2 = -M zero), the apply
crop(ifft2(K^ . fft2(zero-padded x))), and plain conjugate gradients on (A^H A + r I) x = b with the stop rule of include/qmri.h."""
import numpy as np

from nufft_ref import frames_of


def psf(N, M, V, frame_ptr, omega):
    """q [s, s, 2N - 1, 2M - 1], d = (d1 + N - 1, d2 + M - 1) for d1 in [-(N-1), N-1], d2 in [-(M-1), M-1]."""
    om = np.asarray(omega, np.float64)
    Vt = np.asarray(V, np.float64)[frames_of(frame_ptr)]               # m x s
    A = np.exp(1j * np.outer(om[:, 0], np.arange(-(N - 1), N)))        # m x (2N - 1)
    B = np.exp(1j * np.outer(om[:, 1], np.arange(-(M - 1), M)))
    s = Vt.shape[1]
    q = np.empty((s, s, 2 * N - 1, 2 * M - 1), np.complex128)
    for c in range(s):
        for e in range(s):
            q[c, e] = (A * (Vt[:, c] * Vt[:, e])[:, None]).T @ B
    return q / (N * M)


def khat(q, N, M):
    """K^ [s, s, 2N, 2M]: the 2N x 2M DFT of q placed at d mod (2N, 2M), the lines d1 = -N and d2 = -M (index N, M) zero."""
    s = q.shape[0]
    e = np.zeros((s, s, 2 * N, 2 * M), np.complex128)
    d1 = np.arange(-(N - 1), N) % (2 * N)
    d2 = np.arange(-(M - 1), M) % (2 * M)
    e[:, :, d1[:, None], d2[None, :]] = q
    return np.fft.fft2(e, axes=(2, 3))


def normal(x, K):
    """x: N x M x s -> A^H A x: N x M x s."""
    x = np.asarray(x, np.complex128)
    N, M, s = x.shape
    X = np.fft.fft2(x, s=(2 * N, 2 * M), axes=(0, 1))
    Y = np.einsum("cekl,kle->klc", K, X)
    return np.fft.ifft2(Y, axes=(0, 1))[:N, :M]


def cg(apply_normal, b, r, x0, tol, maxit):
    """Plain CG on (A^H A + r I) x = b from x0.  Stops at the first k with ||res_k|| <= tol ||b|| (the recurrence's residual): flag 0; flag 1
    when maxit is reached.  Returns (x, k, flag)."""
    x = np.array(x0, np.complex128)
    res = b - (apply_normal(x) + r * x)
    p = res.copy()
    rr = np.vdot(res, res).real
    tolb = tol * np.linalg.norm(b)
    if np.sqrt(rr) <= tolb:
        return x, 0, 0
    for k in range(1, maxit + 1):
        q = apply_normal(p) + r * p
        alpha = rr / np.vdot(p, q).real
        x = x + alpha * p
        res = res - alpha * q
        rn = np.vdot(res, res).real
        if np.sqrt(rn) <= tolb:
            return x, k, 0
        p = res + (rn / rr) * p
        rr = rn
    return x, maxit, 1
