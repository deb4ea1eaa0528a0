"""numpy restatement of the trajectory operator (qmri_set_operator_nufft) for the tests.

    y_i = (1/sqrt(NM)) sum_c V(t_i, c) a_i^T X_c b_i,   a_i[n1] = exp(-i omega1_i n1),  b_i[n2] = exp(-i omega2_i n2)

computed exactly (a non-uniform DFT, in chunks of samples), its adjoint, and a duck-typed operator whose multi-coil methods, LSQR and the
PnP-ADMM loop are the oracle's own (oracle.Operator.forward_mc / adjoint_mc / lsqr_mc, oracle.pnp_admm_mc) running on it unchanged."""
import numpy as np

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
