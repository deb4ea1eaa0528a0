"""numpy restatement of the regularised field-map estimate from multi-echo images (include/qmri.h qmri_field_map_estimate):
the penalised cosine fit of Funai, Fessler, Yeo, Olafsson and Noll (IEEE TMI 2008) over all echo pairs and coils, minimised by separable quadratic
surrogates with a fixed iteration count.  Every function takes a dtype, so the same code runs in np.float64 and np.longdouble.

    model   y_{l,c}[n] = x_c[n] exp(sigma i 2 pi f[n] t_l),  sigma = phase_sign (-1: the sign of qmri_set_field_map's operator)
    pairs   (a < b) in the order (0,1), (0,2), ..., (L-2, L-1):  s_ab = sum_c y_a conj(y_b)  (sigma = +1: conj(y_a) y_b),  phi_ab = angle(s_ab),
            d_ab = 2 pi (t_b - t_a),  w_ab = |s_ab| / W,  W = max_n sum_ab |s_ab[n]|  (W = 0: all weights 0)
    cost    Psi(f) = sum_n sum_ab w_ab (1 - cos(phi_ab - d_ab f)) + (beta_s / 2) sum_edges (f[n] - f[n'])^2,  beta_s = beta (2 pi (t_{L-1} - t_0))^2
    start   f0 = phi_01 / d_01
Images are [N, M] arrays here (the library's plane is their column-major raveling); Y is [L, C, N, M] for one slice."""
import numpy as np

DEFAULT_ITERS, DEFAULT_BETA = 200, 0.01


def pair_list(L):
    return [(a, b) for a in range(L) for b in range(a + 1, L)]


def _cplx(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


def pairs(Y, t, phase_sign=-1, dtype=np.float64):
    """(phi [P, N, M], w [P, N, M], d [P], W) of one slice."""
    Y = np.asarray(Y).astype(_cplx(dtype))
    t = np.asarray(t, dtype=dtype)
    L = Y.shape[0]
    two_pi = 2 * np.pi if np.dtype(dtype) == np.dtype(np.float64) else 2 * np.arctan2(dtype(0), dtype(-1))
    phi, mag, d = [], [], []
    for a, b in pair_list(L):
        s = np.zeros(Y.shape[2:], _cplx(dtype))
        for c in range(Y.shape[1]):                                   # coils ascending
            s = s + (Y[a, c] * np.conj(Y[b, c]) if phase_sign < 0 else np.conj(Y[a, c]) * Y[b, c])
        phi.append(np.arctan2(s.imag, s.real))
        mag.append(np.abs(s))
        d.append(two_pi * (t[b] - t[a]))
    phi, mag, d = np.array(phi, dtype=dtype), np.array(mag, dtype=dtype), np.array(d, dtype=dtype)
    W = mag.sum(axis=0).max()
    w = mag / W if W > 0 else np.zeros_like(mag)
    return phi, w, d, W


def beta_scaled(beta, t, dtype=np.float64):
    t = np.asarray(t, dtype=dtype)
    two_pi = 2 * np.pi if np.dtype(dtype) == np.dtype(np.float64) else 2 * np.arctan2(dtype(0), dtype(-1))
    b = dtype(DEFAULT_BETA if beta == 0 else beta)
    return b * (two_pi * (t[-1] - t[0])) ** 2


def _wrap(u, two_pi):
    return u - two_pi * np.rint(u / two_pi)


def cost(f, phi, w, d, bs):
    """Psi(f): the data term pixel by pixel in pair order, then every horizontal and vertical edge once."""
    dt = f.dtype.type
    data = dt(0)
    for p in range(phi.shape[0]):
        data = data + np.sum(w[p] * (1 - np.cos(phi[p] - d[p] * f)))
    edges = np.sum((f[1:, :] - f[:-1, :]) ** 2) + np.sum((f[:, 1:] - f[:, :-1]) ** 2)
    return data + bs / 2 * edges


def step(f, phi, w, d, bs):
    """one iteration: all of f^{k+1} from f^k."""
    dt = f.dtype.type
    two_pi = 2 * np.pi if f.dtype == np.float64 else 2 * np.arctan2(dt(0), dt(-1))
    g, c = np.zeros_like(f), np.zeros_like(f)
    for p in range(phi.shape[0]):
        u = _wrap(phi[p] - d[p] * f, two_pi)
        small = np.abs(u) < 1e-8
        kappa = np.where(small, dt(1), np.sin(u) / np.where(small, dt(1), u))
        g = g - w[p] * d[p] * np.sin(u)
        c = c + w[p] * d[p] ** 2 * kappa
    nb, nsum = np.zeros_like(f), np.zeros_like(f)
    nb[1:, :] += 1; nsum[1:, :] += f[:-1, :]                          # n1 - 1
    nb[:-1, :] += 1; nsum[:-1, :] += f[1:, :]                         # n1 + 1
    nb[:, 1:] += 1; nsum[:, 1:] += f[:, :-1]                          # n2 - 1
    nb[:, :-1] += 1; nsum[:, :-1] += f[:, 1:]                         # n2 + 1
    lap = nb * f - nsum
    den = c + 2 * bs * nb
    ok = den > 0
    return np.where(ok, f - (g + bs * lap) / np.where(ok, den, dt(1)), f)


def estimate(Y, t, iters=0, beta=0.0, phase_sign=-1, f_init=None, dtype=np.float64, history=False):
    """One slice: Y [L, C, N, M] (or [L, N, M]) -> (f [N, M], info).  info: cost0, cost, f_min, f_max, iters, unwrap_limit_hz, trust [N, M], start
    [N, M], and with history=True the cost after every iteration (costs[k], k = 0 .. iters)."""
    Y = np.asarray(Y)
    if Y.ndim == 3:
        Y = Y[:, None]
    t = np.asarray(t, dtype=dtype)
    n = DEFAULT_ITERS if iters == 0 else int(iters)
    phi, w, d, _ = pairs(Y, t, phase_sign, dtype)
    bs = beta_scaled(beta, t, dtype)
    start = phi[0] / d[0]
    f = start.copy() if f_init is None else np.asarray(f_init).astype(dtype)
    costs = [cost(f, phi, w, d, bs)]
    for _ in range(n):
        f = step(f, phi, w, d, bs)
        if history:
            costs.append(cost(f, phi, w, d, bs))
    if not history:
        costs.append(cost(f, phi, w, d, bs))
    info = {"cost0": costs[0], "cost": costs[-1], "f_min": f.min(), "f_max": f.max(), "iters": n, "unwrap_limit_hz": 1 / (2 * (t[1] - t[0])),
            "trust": w.sum(axis=0), "start": start}
    if history:
        info["costs"] = np.array(costs, dtype=dtype)
    return f, info


def coil_profiles(N, M, C):
    """C smooth complex coil profiles on [N, M]: Gaussians around points of a circle with a linear phase each (deterministic)."""
    a, b = np.meshgrid((np.arange(N) - N / 2) / N, (np.arange(M) - M / 2) / M, indexing="ij")
    out = []
    for c in range(C):
        th = 2 * np.pi * c / C + 0.3
        mag = np.exp(-((a - 0.45 * np.cos(th)) ** 2 + (b - 0.45 * np.sin(th)) ** 2) / (2 * 0.45 ** 2))
        out.append(mag * np.exp(1j * (1.5 * a * np.cos(th) + 1.1 * b * np.sin(th) + 0.4 * c)))
    return np.array(out)


def echoes(x, f, t, C=1, sigma_rel=0.0, phase_sign=-1, seed=0):
    """Y [L, C, N, M]: y_{l,c} = x coil_c exp(phase_sign i 2 pi f t_l) + complex noise whose real and imaginary parts each have the standard
    deviation sigma_rel max|x|."""
    x = np.asarray(x, np.complex128)
    N, M = x.shape
    S = coil_profiles(N, M, C) if C > 1 else np.ones((1, N, M), np.complex128)
    t = np.asarray(t, np.float64)
    Y = x[None, None] * S[None] * np.exp(phase_sign * 2j * np.pi * f[None, None] * t[:, None, None, None])
    if sigma_rel > 0:
        rng = np.random.default_rng(seed)
        sg = sigma_rel * np.abs(x).max()
        Y = Y + sg * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape))
    return Y
