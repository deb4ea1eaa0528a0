"""numpy restatement of the trajectory operator (qmri_set_operator_nufft) for the tests.

    y_i = (1/sqrt(NM)) sum_c V(t_i, c) a_i^T X_c b_i,   a_i[n1] = exp(-i omega1_i n1),  b_i[n2] = exp(-i omega2_i n2)

computed exactly (a non-uniform DFT, in chunks of samples), its adjoint, and a duck-typed operator whose multi-coil methods, LSQR and the
PnP-ADMM loop are the oracle's own (oracle.Operator.forward_mc / adjoint_mc / lsqr_mc, oracle.pnp_admm_mc) running on it unchanged.
gridded_forward / gridded_adjoint restate the approximation the library computes instead of the exact sum: the 2x oversampled gridding NUFFT at a
given kernel width, on one 2N x 2M FFT."""
import numpy as np

import dcf_ref as D
from oracle import oracle as O

CHUNK = 2048


def frames_of(frame_ptr):
    fp = np.asarray(frame_ptr)
    return np.repeat(np.arange(fp.size - 1), np.diff(fp))


def nudft_forward(x, omega, V, frame_ptr):
    """x: N x M x s complex, omega: m x 2, V: T x s real -> y: m complex (frame-major, the ABI order)."""
    x = np.asarray(x, np.complex128)
    if x.ndim == 2:
        x = x[..., None]
    N, M, s = x.shape
    om = np.asarray(omega, np.float64)
    t = frames_of(frame_ptr)
    Vt = np.asarray(V, np.float64)[t]                                  # m x s
    n1, n2 = np.arange(N), np.arange(M)
    y = np.empty(om.shape[0], np.complex128)
    for i0 in range(0, om.shape[0], CHUNK):
        sl = slice(i0, min(i0 + CHUNK, om.shape[0]))
        A = np.exp(-1j * np.outer(om[sl, 0], n1))                      # chunk x N
        B = np.exp(-1j * np.outer(om[sl, 1], n2))                      # chunk x M
        yc = np.einsum("in,nmc,im->ic", A, x, B)                       # a_i^T X_c b_i
        y[sl] = np.sum(Vt[sl] * yc, axis=1)
    return y / np.sqrt(N * M)


def nudft_adjoint(y, omega, V, frame_ptr, N, M):
    """the exact Hermitian transpose of nudft_forward: y m complex -> N x M x s complex."""
    y = np.asarray(y, np.complex128)
    om = np.asarray(omega, np.float64)
    t = frames_of(frame_ptr)
    Vt = np.asarray(V, np.float64)[t]
    n1, n2 = np.arange(N), np.arange(M)
    x = np.zeros((N, M, Vt.shape[1]), np.complex128)
    for i0 in range(0, om.shape[0], CHUNK):
        sl = slice(i0, min(i0 + CHUNK, om.shape[0]))
        A = np.exp(1j * np.outer(om[sl, 0], n1))
        B = np.exp(1j * np.outer(om[sl, 1], n2))
        x += np.einsum("in,ic,im->nmc", A, Vt[sl] * y[sl, None], B)
    return x / np.sqrt(N * M)


def deapodisation(L, width, beta):
    """1 / Phi(p) at the centred index p = n - L/2, n < L:  Phi(p) = int_{-w/2}^{w/2} phi(u) cos(2 pi u p / (2L)) du by the 200-point
    Gauss-Legendre quadrature of the host plan (deapodisation() of csrc/nufft_plan.h)."""
    gx, gw = np.polynomial.legendre.leggauss(200)
    hw = 0.5 * width
    p = np.arange(L) - L // 2
    Phi = np.sum(gw[None, :] * hw * D.phi(gx * hw, hw, beta)[None, :] * np.cos(2 * np.pi * np.outer(p, gx * hw) / (2 * L)), axis=1)
    return 1.0 / Phi


def _gridding_plan(omega, N, M, width):
    """-> (w, k1 [m, w] and k2 [m, w] wrapped into the 2N x 2M grid, p1 [m, w] and p2 [m, w] = phi(u - k), the samples' phases [m])."""
    w = D.plan_width(width)
    beta, hw = D.plan_beta(w), 0.5 * w
    om = np.asarray(omega, np.float64)
    u1, u2 = om[:, 0] * N / np.pi, om[:, 1] * M / np.pi
    k1 = np.ceil(u1 - hw).astype(np.int64)[:, None] + np.arange(w)[None, :]
    k2 = np.ceil(u2 - hw).astype(np.int64)[:, None] + np.arange(w)[None, :]
    p1, p2 = D.phi(u1[:, None] - k1, hw, beta), D.phi(u2[:, None] - k2, hw, beta)
    ph = np.exp(-1j * (om[:, 0] * (N // 2) + om[:, 1] * (M // 2)))     # the image index is centred: n = p + (N/2, M/2)
    return w, k1 % (2 * N), k2 % (2 * M), p1, p2, ph


def gridded_forward(x, omega, V, frame_ptr, width=0):
    """The library's gridding NUFFT restated plainly, without the sub-grid trick: x / Phi(p) on the centred index p,
    zero-padded to 2N x 2M (at p mod 2N, 2M), np.fft.fft2, then y_i = ph_i sum_k phi(u_i1 - k1) phi(u_i2 - k2) sum_c V(t_i, c) G_c[k] / sqrt(NM) over
    the window k = ceil(u - w/2) ... + w - 1 wrapped into the grid.  x: N x M x s, width 0: the plan's default -> y: m complex."""
    x = np.asarray(x, np.complex128)
    if x.ndim == 2:
        x = x[..., None]
    N, M, s = x.shape
    w, k1, k2, p1, p2, ph = _gridding_plan(omega, N, M, width)
    beta = D.plan_beta(w)
    pad = np.zeros((2 * N, 2 * M, s), np.complex128)
    i1, i2 = (np.arange(N) - N // 2) % (2 * N), (np.arange(M) - M // 2) % (2 * M)
    pad[np.ix_(i1, i2)] = x * (deapodisation(N, w, beta)[:, None] * deapodisation(M, w, beta)[None, :])[:, :, None]
    G = np.fft.fft2(pad, axes=(0, 1))
    Vt = np.asarray(V, np.float64)[frames_of(frame_ptr)]               # m x s
    y = np.empty(k1.shape[0], np.complex128)
    for i0 in range(0, y.size, CHUNK):
        sl = slice(i0, min(i0 + CHUNK, y.size))
        g = G[k1[sl][:, :, None], k2[sl][:, None, :], :]               # chunk x w x w x s
        y[sl] = np.einsum("ia,ib,iabc,ic->i", p1[sl], p2[sl], g, Vt[sl])
    return ph * y / np.sqrt(N * M)


def gridded_adjoint(y, omega, V, frame_ptr, N, M, width=0):
    """the exact transpose of gridded_forward, step by step in reverse: spread conj(ph) V y with the same window and kernel values, the conjugate
    2N x 2M DFT, crop to the centred image, 1 / Phi -> N x M x s complex."""
    y = np.asarray(y, np.complex128)
    w, k1, k2, p1, p2, ph = _gridding_plan(omega, N, M, width)
    beta = D.plan_beta(w)
    Vt = np.asarray(V, np.float64)[frames_of(frame_ptr)]
    s = Vt.shape[1]
    val = (p1[:, :, None] * p2[:, None, :]).reshape(y.size, w * w)
    idx = (k1[:, :, None] * (2 * M) + k2[:, None, :]).reshape(y.size, w * w)
    yc = np.conj(ph) * y
    G = np.empty((2 * N, 2 * M, s), np.complex128)
    for c in range(s):
        v = Vt[:, c] * yc
        G[:, :, c] = (np.bincount(idx.ravel(), weights=(v.real[:, None] * val).ravel(), minlength=4 * N * M)
                      + 1j * np.bincount(idx.ravel(), weights=(v.imag[:, None] * val).ravel(), minlength=4 * N * M)).reshape(2 * N, 2 * M)
    pad = np.fft.ifft2(G, axes=(0, 1)) * (4 * N * M)                   # sum_k G[k] exp(+2 pi i k p / (2N, 2M))
    i1, i2 = (np.arange(N) - N // 2) % (2 * N), (np.arange(M) - M // 2) % (2 * M)
    x = pad[np.ix_(i1, i2)] * (deapodisation(N, w, beta)[:, None] * deapodisation(M, w, beta)[None, :])[:, :, None]
    return x / np.sqrt(N * M)


class NudftOperator:
    """Duck-typed oracle.Operator on a trajectory: forward / adjoint exact, the multi-coil methods and the LSQR borrowed from the oracle."""

    forward_mc = O.Operator.forward_mc
    adjoint_mc = O.Operator.adjoint_mc
    lsqr_mc = O.Operator.lsqr_mc

    def __init__(self, N, M, V, frame_ptr, omega):
        self.N, self.M = int(N), int(M)
        self.V = np.asarray(V, np.float64)
        self.T, self.s = self.V.shape
        self.fp = np.asarray(frame_ptr, np.int32)
        self.omega = np.asarray(omega, np.float64)
        self.m = self.omega.shape[0]

    def forward(self, x):
        return nudft_forward(x, self.omega, self.V, self.fp)

    def adjoint(self, y):
        return nudft_adjoint(y, self.omega, self.V, self.fp, self.N, self.M)


def spiral_traj(N, S, T):
    """setup_subsampling_spiralgrided.m:7-27 before the rounding: theta = 8 linspace(0, 2 pi, S), r = 1.05^theta normalised to [0, 1], frame f
    rotated by f * 7.5 degrees; omega = pi r (cos, sin).  -> (frame_ptr, omega m x 2)."""
    t = np.linspace(0, 2 * np.pi, S)
    theta = 8 * t
    r = 1.05 ** theta
    r = (r - r.min()) / (r.max() - r.min())
    delta = np.pi / 180 * 7.5
    om = np.concatenate([np.stack([np.pi * (r * np.cos(theta + f * delta)), np.pi * (r * np.sin(theta + f * delta))], axis=1) for f in range(T)])
    return np.arange(T + 1, dtype=np.int32) * S, om


def matlab_round(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def grid_mask_from_traj(N, frame_ptr, omega):
    """The reference's rounding of the spiral (setup_subsampling_spiralgrided.m:28-34): round(r cos * N/2) + N/2 + 1 clamped to N, fftshift, unique
    per frame in column-major order -> (frame_ptr, kidx) of the gridded mask."""
    fp_out, kidx = [0], []
    half = N // 2
    for f in range(len(frame_ptr) - 1):
        om = omega[frame_ptr[f]:frame_ptr[f + 1]]
        gx = np.minimum(matlab_round(om[:, 0] / np.pi * N / 2) + N / 2 + 1, N)
        gy = np.minimum(matlab_round(om[:, 1] / np.pi * N / 2) + N / 2 + 1, N)
        r = (gx.astype(int) - 1 + half) % N
        c = (gy.astype(int) - 1 + half) % N
        k = np.unique(c * N + r)
        kidx.extend(k.tolist())
        fp_out.append(len(kidx))
    return np.array(fp_out, np.int32), np.array(kidx, np.int32)


def traj_from_kidx(N, M, kidx):
    """on-grid trajectory of a gridded mask: omega = 2 pi k / (N, M) wrapped into [-pi, pi)."""
    k = np.asarray(kidx)
    k1, k2 = k % N, k // N
    w1 = 2 * np.pi * k1 / N
    w2 = 2 * np.pi * k2 / M
    w1 = np.where(k1 >= N // 2, w1 - 2 * np.pi, w1)
    w2 = np.where(k2 >= M // 2, w2 - 2 * np.pi, w2)
    return np.stack([w1, w2], axis=1)
