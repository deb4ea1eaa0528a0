"""numpy restatement of the field-aware Toeplitz normal operator (qmri_nufft_prepare_normal_fm) for the tests, fp64.

    (A_f^H A_f)[n, n'] carries exp(i 2 pi (f[n] - f[n']) tau_i);   exp(i 2 pi g tau) ~ sum_{l<L} c_l(tau) exp(i 2 pi g tauhat_l),  g = f[n] - f[n']
    A_f^H A_f ~ sum_l P_l^H T_l P_l,   P_l = diag(exp(-i 2 pi (f - f0) tauhat_l)),   T_l = A^H diag(c_l(tau)) A   (A the operator without a map)

f0, f_min, f_max, t_min, t_max and the histogram p_h are those of offres_ref.Segmentation (the attached map's).  The difference histogram is
p~_j = sum_h p_h p_{h-j} over 2 nbins - 1 bins at g_j = j (f_max - f_min) / nbins; tauhat_l = t_min + l (t_max - t_min) / (L - 1); c(tau_i) solves the
REAL system (R + eps I) c = rho(tau_i), R_ll' = sum_j p~_j cos 2 pi g_j (tauhat_l - tauhat_l'), rho_l(tau) = sum_j p~_j cos 2 pi g_j (tau - tauhat_l),
eps = 1e-12 tr(R) / L.  That system is the least-squares problem of the stacked table B = [sqrt(p~) cos 2 pi g tauhat; sqrt(p~) sin 2 pi g tauhat;
sqrt(eps) I] (B^T B = R + eps I, B^T b = rho for b = [sqrt(p~) cos 2 pi g tau; sqrt(p~) sin 2 pi g tau; 0]) and is solved through B's QR, as the
library does: R's condition is the square of B's (3e9 at L = 8 on the spiral fixture), and a Cholesky solve of R in fp64 moves fit_max there by
1e-7 .. 1e-6 relative, which is the whole bound of the auto-mode test; QR, SVD and an orthogonalised-twice Gram-Schmidt agree to 1e-11.
Every T_l here runs exact NUDFTs (nufft_ref)."""
import numpy as np

import nufft_ref as R
import offres_ref as F


def diff_histogram(p):
    """p~_j = sum_h p_h p_{h-j}, j = -(nbins - 1) .. nbins - 1 (the autocorrelation: symmetric in j)."""
    return np.correlate(p, p, mode="full")


class NormalSegmentation:
    def __init__(self, f, tau, L, nbins=256):
        base = F.Segmentation(f, tau, 2, nbins)                        # (its histogram and ranges: the attached map's)
        self.f0, self.fc, self.tau, self.L = base.f0, base.fc, base.tau, int(L)
        self.pt = diff_histogram(base.p)
        self.g = np.arange(-(nbins - 1), nbins) * ((base.f_max - base.f_min) / nbins)
        self.tauhat = base.t_min + np.arange(L) * (base.t_max - base.t_min) / (L - 1)
        ah, at = 2 * np.pi * np.outer(self.g, self.tauhat), 2 * np.pi * np.outer(self.g, self.tau)
        w = np.sqrt(self.pt)[:, None]
        eps = 1e-12 * self.pt.sum()                                    # = 1e-12 tr(R) / L: R_ll = sum_j p~_j
        B = np.vstack([w * np.cos(ah), w * np.sin(ah), np.sqrt(eps) * np.eye(L)])
        b = np.vstack([w * np.cos(at), w * np.sin(at), np.zeros((L, self.tau.size))])
        Q, U = np.linalg.qr(B)
        self.c = _back_substitute(U, Q.T @ b).T                        # m x L, real
        occ = self.pt > 0
        E = np.exp(2j * np.pi * np.outer(self.g[occ], self.tau))
        G = np.exp(2j * np.pi * np.outer(self.g[occ], self.tauhat))
        res = np.abs(E - G @ self.c.T)
        self.fit_max = float(res.max())
        self.fit_rms = float(np.sqrt(np.sum(self.pt[occ][:, None] * res ** 2) / self.tau.size))

    def complex_coefficients(self):
        """the same least-squares problem solved as a complex one (no ridge needed at small L): its imaginary part is rounding alone."""
        G = np.exp(2j * np.pi * np.outer(self.g, self.tauhat))
        E = np.exp(2j * np.pi * np.outer(self.g, self.tau))
        A = G.conj().T @ (self.pt[:, None] * G)
        A = A + 1e-12 * np.trace(A).real / self.L * np.eye(self.L)
        return np.linalg.solve(A, G.conj().T @ (self.pt[:, None] * E)).T

    def phase_maps(self):
        return np.exp(-2j * np.pi * self.fc[None, :, :] * self.tauhat[:, None, None])  # L x N x M


def _back_substitute(U, Y):
    """U c = y with the upper factor U (what the device does per sample)."""
    L = U.shape[0]
    Y = np.array(Y, np.float64)
    for r in range(L - 1, -1, -1):
        Y[r] = (Y[r] - U[r, r + 1:] @ Y[r + 1:]) / U[r, r]
    return Y


def auto(f, tau, tol, nbins=256, Lmax=32):
    """the auto mode: the first L in 2 .. Lmax whose fit_max <= tol."""
    for L in range(2, Lmax + 1):
        sg = NormalSegmentation(f, tau, L, nbins)
        if sg.fit_max <= tol:
            return sg
    return sg


def normal_segmented(x, omega, V, frame_ptr, seg):
    x = np.asarray(x, np.complex128)
    if x.ndim == 2:
        x = x[..., None]
    N, M, _ = x.shape
    P = seg.phase_maps()
    out = 0
    for l in range(seg.L):
        y = seg.c[:, l] * R.nudft_forward(x * P[l][:, :, None], omega, V, frame_ptr)
        out = out + np.conj(P[l])[:, :, None] * R.nudft_adjoint(y, omega, V, frame_ptr, N, M)
    return out


def normal_exact(x, omega, V, frame_ptr, f, tau):
    N, M = f.shape
    return F.exact_adjoint(F.exact_forward(x, omega, V, frame_ptr, f, tau), omega, V, frame_ptr, N, M, f, tau)


# eps_ref_n(L): the restatement's relative L2 error against normal_exact on offres_ref.vectors() at nbins = 256 (measured by eps_ref_n below,
# reproduced by tests/test_offres_normal_host.py).  The GPU tests hold the library to max(2 eps, 1e-9) up to L = 8; beyond
# L ~ 10 the coefficient system is ill-conditioned and the figures are a solver's, not the method's.
EPS_REF_N = {"spiral32": {4: 1.41e-2, 6: 4.94e-4, 8: 7.80e-6, 12: 2.3e-7},
             "rect32x64": {4: 1.82e-2, 6: 3.91e-4, 8: 5.48e-6, 12: 2.7e-7}}


def eps_ref_n(case, L, nbins=256, exact=None):
    fp, om, V, f, tau = case
    N, M = f.shape
    x, _ = F.vectors(N, M, V.shape[1], om.shape[0])
    ne = normal_exact(x, om, V, fp, f, tau) if exact is None else exact
    ns = normal_segmented(x, om, V, fp, NormalSegmentation(f, tau, L, nbins))
    return float(np.linalg.norm(ns - ne) / np.linalg.norm(ne))


# ---- the dense problem of the x-update test: s = 1, V = 1 / sqrt(T), the phantom, data from the exact operator, r = 0.05, z = 0
XUPDATE_R = 0.05
# distance from the dense minimiser of the exact matrix to the dense minimiser under the restatement's segmented normal at L = 8 with the exact
# right-hand side (measured by xupdate_reference below, reproduced by the host test)
D_REF = {8: 3.22e-5}


def exact_matrix(case, with_field=True):
    """A [m, N*M] of the s = 1 case, columns in the layout of one channel plane (n1 + N n2)."""
    fp, om, V, f, tau = case
    N, M = f.shape
    n1, n2 = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    n1, n2, fr = n1.ravel(order="F"), n2.ravel(order="F"), f.ravel(order="F")
    ph = np.outer(om[:, 0], n1) + np.outer(om[:, 1], n2)
    if with_field:
        ph = ph + 2 * np.pi * np.outer(tau, fr)
    Vt = np.asarray(V, np.float64)[R.frames_of(fp)][:, 0]
    return Vt[:, None] * np.exp(-1j * ph) / np.sqrt(N * M)


def xupdate_reference(case, L=8, r=XUPDATE_R):
    """(y, x_exact, x_seg, d_ref): data of the phantom from the exact operator, the dense minimiser of |A_f x - y|^2 + r |x|^2, the one with the
    restatement's segmented normal in place of A_f^H A_f (the right-hand side A_f^H y exact), and their relative distance."""
    fp, om, V, f, tau = case
    N, M = f.shape
    Af, A0 = exact_matrix(case), exact_matrix(case, with_field=False)
    x0 = F.phantom(N).astype(np.complex128).ravel(order="F")
    y = Af @ x0
    rhs = Af.conj().T @ y
    n = N * M
    xe = np.linalg.solve(Af.conj().T @ Af + r * np.eye(n), rhs)
    sg = NormalSegmentation(f, tau, L)
    P = sg.phase_maps().reshape(L, -1, order="F")
    Ns = np.zeros((n, n), np.complex128)
    for l in range(L):
        Ns += np.conj(P[l])[:, None] * (A0.conj().T @ (sg.c[:, l][:, None] * A0)) * P[l][None, :]
    xs = np.linalg.solve(Ns + r * np.eye(n), rhs)
    d = float(np.linalg.norm(xs - xe) / np.linalg.norm(xe))
    return y, xe.reshape((N, M, 1), order="F"), xs.reshape((N, M, 1), order="F"), d
