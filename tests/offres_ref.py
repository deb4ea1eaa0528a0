"""numpy restatement of the off-resonance correction of a trajectory operator (qmri_set_field_map) for the tests, fp64.

    exact:      y_i = (1/sqrt(NM)) sum_n (sum_c V x_c[n]) exp(-i omega_i . n) exp(-i 2 pi f[n] tau_i)          and its Hermitian transpose
    segmented:  exp(-i 2 pi f tau) ~ exp(-i 2 pi f0 tau) sum_{l<L} b_l(tau) exp(-i 2 pi (f - f0) tauhat_l)

f0 = (f_min + f_max) / 2, tauhat_l = t_min + l (t_max - t_min) / (L - 1), b(tau_i) the least-squares solution over the nbins-bin histogram (p_h, f_h)
of f - f0 (equal bins on [f_min - f0, f_max - f0], f_h the centres, p_h the fraction of pixels):
    (G^H P G + eps I) b = G^H P e(tau_i),   G_hl = exp(-i 2 pi f_h tauhat_l),   eps = 1e-12 tr(G^H P G) / L.
A constant map is L = 1 with b = 1.  The segmented operator here runs exact NUDFTs per segment (nufft_ref)."""
import numpy as np

import dcf_ref as D
import nufft_ref as R


def field(N, M=None, scale=100.0):
    """the issue's field: f = scale (sin 2 pi a cos pi b + 0.6 b + 0.2) Hz on the phantom's coordinates a, b in [-1/2, 1/2)."""
    M = M or N
    a, b = np.meshgrid((np.arange(N) - N / 2) / N, (np.arange(M) - M / 2) / M, indexing="ij")
    return scale * (np.sin(2 * np.pi * a) * np.cos(np.pi * b) + 0.6 * b + 0.2)


def readout_times(S, T, readout_s):
    return np.tile(np.arange(S) * (readout_s / S), T)


def exact_forward(x, omega, V, frame_ptr, f, tau):
    """one NUDFT per distinct readout time would be the cheap way; the direct sum in chunks of samples is the plain one."""
    x = np.asarray(x, np.complex128)
    if x.ndim == 2:
        x = x[..., None]
    N, M, s = x.shape
    om = np.asarray(omega, np.float64)
    Vt = np.asarray(V, np.float64)[R.frames_of(frame_ptr)]
    n1, n2 = np.arange(N), np.arange(M)
    y = np.empty(om.shape[0], np.complex128)
    CH = 256
    for i0 in range(0, om.shape[0], CH):
        sl = slice(i0, min(i0 + CH, om.shape[0]))
        A = np.exp(-1j * np.outer(om[sl, 0], n1))
        B = np.exp(-1j * np.outer(om[sl, 1], n2))
        Ph = np.exp(-2j * np.pi * tau[sl, None, None] * f[None, :, :])                 # chunk x N x M
        yc = np.einsum("in,inm,nmc,im->ic", A, Ph, x, B, optimize=True)
        y[sl] = np.sum(Vt[sl] * yc, axis=1)
    return y / np.sqrt(N * M)


def exact_adjoint(y, omega, V, frame_ptr, N, M, f, tau):
    y = np.asarray(y, np.complex128)
    om = np.asarray(omega, np.float64)
    Vt = np.asarray(V, np.float64)[R.frames_of(frame_ptr)]
    n1, n2 = np.arange(N), np.arange(M)
    x = np.zeros((N, M, Vt.shape[1]), np.complex128)
    CH = 256
    for i0 in range(0, om.shape[0], CH):
        sl = slice(i0, min(i0 + CH, om.shape[0]))
        A = np.exp(1j * np.outer(om[sl, 0], n1))
        B = np.exp(1j * np.outer(om[sl, 1], n2))
        Ph = np.exp(2j * np.pi * tau[sl, None, None] * f[None, :, :])
        x += np.einsum("in,inm,ic,im->nmc", A, Ph, Vt[sl] * y[sl, None], B, optimize=True)
    return x / np.sqrt(N * M)


class Segmentation:
    """the coefficients exactly as the library specifies them."""

    def __init__(self, f, tau, L, nbins=256):
        f, tau = np.asarray(f, np.float64), np.asarray(tau, np.float64)
        self.f_min, self.f_max, self.t_min, self.t_max = float(f.min()), float(f.max()), float(tau.min()), float(tau.max())
        self.f0 = 0.5 * (self.f_min + self.f_max)
        self.L, self.tau, self.fc = int(L), tau, f - self.f0
        if self.f_max == self.f_min:
            assert L == 1
            self.tauhat = np.array([self.t_min])
            self.b = np.ones((tau.size, 1), np.complex128)
            self.fit_max = self.fit_rms = 0.0
            return
        lo, width = self.f_min - self.f0, (self.f_max - self.f_min) / nbins
        idx = np.clip(np.floor((self.fc.ravel() - lo) / width).astype(np.int64), 0, nbins - 1)
        self.p = np.bincount(idx, minlength=nbins) / f.size
        self.fh = lo + (np.arange(nbins) + 0.5) * width
        self.tauhat = np.full(L, self.t_min) if L == 1 else self.t_min + np.arange(L) * (self.t_max - self.t_min) / (L - 1)
        G = np.exp(-2j * np.pi * np.outer(self.fh, self.tauhat))                       # nbins x L
        A = G.conj().T @ (self.p[:, None] * G)
        A = A + 1e-12 * np.trace(A).real / L * np.eye(L)
        E = np.exp(-2j * np.pi * np.outer(self.fh, tau))                               # nbins x m
        self.b = np.linalg.solve(A, G.conj().T @ (self.p[:, None] * E)).T              # m x L
        res = np.abs(E - G @ self.b.T)[self.p > 0]
        self.fit_max = float(res.max())
        self.fit_rms = float(np.sqrt(np.sum(self.p[self.p > 0][:, None] * res ** 2) / tau.size))

    def phase_maps(self):
        return np.exp(-2j * np.pi * self.fc[None, :, :] * self.tauhat[:, None, None])  # L x N x M

    def sample_factors(self):
        return self.b * np.exp(-2j * np.pi * self.f0 * self.tau)[:, None]              # m x L, the centre frequency folded in

    def approximation_error(self):
        """max over pixels x samples of |exp(-i 2 pi f tau) - the segmented value| (the table of the issue)."""
        fu = np.unique(self.fc)
        ex = np.exp(-2j * np.pi * np.outer(fu, self.tau))
        ap = np.exp(-2j * np.pi * np.outer(fu, self.tauhat)) @ self.b.T
        return float(np.abs(ex - ap).max())


def segmented_forward(x, omega, V, frame_ptr, seg):
    x = np.asarray(x, np.complex128)
    if x.ndim == 2:
        x = x[..., None]
    P, bf = seg.phase_maps(), seg.sample_factors()
    y = np.zeros(np.asarray(omega).shape[0], np.complex128)
    for l in range(seg.L):
        y += bf[:, l] * R.nudft_forward(x * P[l][:, :, None], omega, V, frame_ptr)
    return y


def segmented_adjoint(y, omega, V, frame_ptr, N, M, seg):
    P, bf = seg.phase_maps(), seg.sample_factors()
    x = 0
    for l in range(seg.L):
        x = x + np.conj(P[l])[:, :, None] * R.nudft_adjoint(np.conj(bf[:, l]) * np.asarray(y, np.complex128), omega, V, frame_ptr, N, M)
    return x


def spiral_case(N=32, S=60, T=48, s=1, readout_s=5e-3, seed=0):
    """the 32 x 32 case of the issue: (frame_ptr, omega, V, f, tau); s = 1: V = 1/sqrt(T), else random orthonormal columns."""
    fp, om = R.spiral_traj(N, S, T)
    if s == 1:
        V = np.full((T, 1), 1 / np.sqrt(T))
    else:
        V = np.linalg.qr(np.random.default_rng(seed).standard_normal((T, s)))[0]
    return fp, om, V, field(N), readout_times(S, T, readout_s)


phantom = D.phantom

# eps_ref(L): the restatement's own relative L2 error against the exact operator on vectors(), the larger of forward and adjoint, at nbins = 256
# (measured by eps_ref below, reproduced by tests/test_offres_host.py).  The GPU tests hold the library to twice these.
EPS_REF = {"spiral32": {3: 2.83e-2, 4: 2.28e-3, 5: 1.84e-4, 6: 1.26e-5, 8: 4.68e-7},
           "rect32x64": {3: 2.82e-2, 4: 2.36e-3, 5: 1.90e-4, 6: 1.29e-5, 8: 4.93e-7}}


def rect_case(N=32, M=64, m=700, T=7, s=2, readout_s=5e-3, seed=5):
    """32 x 64, random omega in [-pi, pi]^2 and random tau in [0, readout_s], T frames of m / T samples, random orthonormal V; the field has no
    symmetry between the axes, so a transposed map fails."""
    rng = np.random.default_rng(seed)
    om = rng.uniform(-np.pi, np.pi, (m, 2))
    tau = rng.uniform(0.0, readout_s, m)
    fp = (np.arange(T + 1) * (m // T)).astype(np.int32)
    fp[-1] = m
    V = np.linalg.qr(rng.standard_normal((T, s)))[0]
    return fp, om, V, field(N, M), tau


def vectors(N, M, s, m, seed=11):
    """the x and y every accuracy test uses (so that eps_ref and the library see the same input)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, M, s)) + 1j * rng.standard_normal((N, M, s))
    y = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    return x, y


def eps_ref(case, L, nbins=256):
    """relative L2 error of the restatement's segmented operator against the exact one on test_vectors: (forward, adjoint)."""
    fp, om, V, f, tau = case
    N, M = f.shape
    x, y = vectors(N, M, V.shape[1], om.shape[0])
    sg = Segmentation(f, tau, L, nbins)
    ye, xe = exact_forward(x, om, V, fp, f, tau), exact_adjoint(y, om, V, fp, N, M, f, tau)
    ys, xs = segmented_forward(x, om, V, fp, sg), segmented_adjoint(y, om, V, fp, N, M, sg)
    return float(np.linalg.norm(ys - ye) / np.linalg.norm(ye)), float(np.linalg.norm(xs - xe) / np.linalg.norm(xe))
