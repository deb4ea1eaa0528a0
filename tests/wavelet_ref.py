"""Joint wavelet soft-thresholding: the numpy restatement that defines qmri_wavelet_prox (include/qmri.h).

X is N x M x s (numpy shape (N, M, s); in the ABI the first side is contiguous and the channel planes are outermost).  Two orthogonal filters with
periodic boundaries: Haar (T = 2) and Daubechies-2 (T = 4), high-pass g[j] = (-1)^j h[T-1-j].  One analysis level on a length-n axis (n even,
n >= T): a[k] = sum_j h[j] x[(2k+j) mod n], d[k] = sum_j g[j] x[(2k+j) mod n], k < n/2; synthesis x[(2k+j) mod n] += h[j] a[k] + g[j] d[k].
Level l = 1..L acts on the top-left (N/2^(l-1)) x (M/2^(l-1)) corner, axis 0 first, approximation coefficients in the low half of each axis (Mallat
layout).  With offsets 0 <= o1, o2 < P = 2^L the transform is taken of Xs[n1, n2] = X[(n1+o1) mod N, (n2+o2) mod M] and the result shifted back.
Every coefficient outside the final (N/2^L) x (M/2^L) corner is scaled by f = 1 - tau/m where m > tau, else 0; m = sqrt(sum_c |C_c|^2) (joint) or
|C_c| (per channel).  cmax is the largest m over those positions before thresholding.  Real mode works on real(X) and returns an imaginary part
that is exactly 0.  A non-finite m gives a non-finite f, so a NaN shows in every coefficient its m reaches.

wavelet_prox is the definition (filter bank by index arithmetic); wavelet_prox_dense is a second route that applies the explicit n x n orthogonal
matrix per level and axis, so that the rounding gap between two correct routes can be measured on the host: SENS holds that gap per fixture family.
"""
import functools

import numpy as np

from llr_ref import tsmi_like  # noqa: F401  (the fixtures of section 25 serve here too)

HAAR, DB2 = 0, 1
FILTERS = {"haar": HAAR, "db2": DB2}
_S3 = np.sqrt(3.0)
LOWPASS = {HAAR: np.array([1.0, 1.0]) / np.sqrt(2.0),
           DB2: np.array([1.0 + _S3, 3.0 + _S3, 3.0 - _S3, 1.0 - _S3]) / (4.0 * np.sqrt(2.0))}
MAX_LEVELS, MAX_S = 4, 16


def filters(filt):
    """(h, g) of a filter id."""
    h = LOWPASS[filt]
    T = len(h)
    g = np.array([(-1.0) ** j * h[T - 1 - j] for j in range(T)])
    return h, g


def sizes_ok(N, M, L, filt):
    T = len(LOWPASS[filt])
    return 1 <= L <= MAX_LEVELS and N % (1 << L) == 0 and M % (1 << L) == 0 and (N >> (L - 1)) >= T and (M >> (L - 1)) >= T


def offsets(it, P, shift=True):
    """The offsets (o1, o2) of ADMM iteration `it` (0-based): section 25's rule with the block side replaced by P = 2^L."""
    if not shift:
        return 0, 0
    q = it % (P * P)
    return q % P, (q // P + q) % P


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one level on axis 0 of an array (n, ...)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _analysis(x, h, g):
    n = x.shape[0]
    k2 = 2 * np.arange(n // 2)
    a = np.zeros((n // 2,) + x.shape[1:], x.dtype)
    d = np.zeros_like(a)
    for j in range(len(h)):
        xj = x[(k2 + j) % n]
        a = a + h[j] * xj
        d = d + g[j] * xj
    return np.concatenate([a, d], 0)


def _synthesis(c, h, g):
    n = c.shape[0]
    a, d = c[:n // 2], c[n // 2:]
    k2 = 2 * np.arange(n // 2)
    x = np.zeros_like(c)
    for j in range(len(h)):
        x[(k2 + j) % n] += h[j] * a + g[j] * d        # (the indices of one j are distinct)
    return x


@functools.lru_cache(maxsize=None)
def analysis_matrix(n, filt):
    """The n x n orthogonal matrix of one periodised level: rows 0..n/2-1 low-pass, n/2..n-1 high-pass."""
    h, g = filters(filt)
    W = np.zeros((n, n))
    for k in range(n // 2):
        for j in range(len(h)):
            W[k, (2 * k + j) % n] += h[j]
            W[n // 2 + k, (2 * k + j) % n] += g[j]
    W.setflags(write=False)
    return W


def _analysis_dense(x, filt):
    return np.tensordot(analysis_matrix(x.shape[0], filt), x, axes=(1, 0))


def _synthesis_dense(c, filt):
    return np.tensordot(analysis_matrix(c.shape[0], filt).T, c, axes=(1, 0))


def _levels(X, L, filt, dense, inverse):
    h, g = filters(filt)
    N, M = X.shape[:2]
    C = X.copy()
    for l in (range(L, 0, -1) if inverse else range(1, L + 1)):
        n, m = N >> (l - 1), M >> (l - 1)
        blk = C[:n, :m]
        if not inverse:
            blk = _analysis_dense(blk, filt) if dense else _analysis(blk, h, g)
            blk = np.swapaxes(blk, 0, 1)
            blk = _analysis_dense(blk, filt) if dense else _analysis(blk, h, g)
            blk = np.swapaxes(blk, 0, 1)
        else:
            blk = np.swapaxes(blk, 0, 1)
            blk = _synthesis_dense(blk, filt) if dense else _synthesis(blk, h, g)
            blk = np.swapaxes(blk, 0, 1)
            blk = _synthesis_dense(blk, filt) if dense else _synthesis(blk, h, g)
        C[:n, :m] = blk
    return C


def dwt2(X, L, filt=DB2, dense=False):
    """L levels of the 2-D transform of X (N x M [x s]) in the Mallat layout."""
    return _levels(np.asarray(X), L, filt, dense, False)


def idwt2(C, L, filt=DB2, dense=False):
    return _levels(np.asarray(C), L, filt, dense, True)


def detail_mask(N, M, L):
    """True at every coefficient position outside the final approximation corner."""
    m = np.ones((N, M), bool)
    m[:N >> L, :M >> L] = False
    return m


def _prox(X, tau, L, filt, joint, offset, real, dense):
    X = np.asarray(X)
    if X.ndim != 3:
        raise ValueError("X must be N x M x s")
    N, M, s = X.shape
    if filt not in LOWPASS or not sizes_ok(N, M, L, filt) or not 1 <= s <= MAX_S:
        raise ValueError("the sizes break the rule of the contract")
    P = 1 << L
    o1, o2 = int(offset[0]), int(offset[1])
    if not (0 <= o1 < P and 0 <= o2 < P):
        raise ValueError("offsets must satisfy 0 <= o < 2^L")
    if not tau >= 0:
        raise ValueError("tau must be >= 0")
    Xc = X.real.astype(np.float64) if (real or not np.iscomplexobj(X)) else X.astype(np.complex128)
    C = dwt2(np.roll(Xc, (-o1, -o2), (0, 1)), L, filt, dense)
    det = detail_mask(N, M, L)
    mag = np.abs(C)
    m = np.sqrt(np.sum(mag * mag, axis=2, keepdims=True)) * np.ones((1, 1, s)) if joint else mag
    md = m[det]
    cmax = float("nan") if np.isnan(md).any() else float(md.max())
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(m > tau, 1.0 - tau / m, np.where(np.isnan(m), m, 0.0))
    f[~det] = 1.0
    out = np.roll(idwt2(C * f, L, filt, dense), (o1, o2), (0, 1))
    return out.real + 0j if not np.iscomplexobj(out) else out, cmax


def wavelet_prox(X, tau, levels=3, filt=DB2, joint=True, offset=(0, 0), real=False):
    """The definition: (out N x M x s complex128, cmax)."""
    return _prox(X, float(tau), int(levels), filt, bool(joint), offset, real, False)


def wavelet_prox_dense(X, tau, levels=3, filt=DB2, joint=True, offset=(0, 0), real=False):
    """The second route: the explicit orthogonal matrix of every level and axis."""
    return _prox(X, float(tau), int(levels), filt, bool(joint), offset, real, True)


def wavelet_prox_stack(X, tau, levels=3, filt=DB2, joint=True, offset=(0, 0), real=False):
    outs = [wavelet_prox(x, tau, levels, filt, joint, offset, real) for x in X]
    return np.stack([o for o, _ in outs]), np.array([m for _, m in outs])


def haar_block_means(X, L, offset=(0, 0), real=False):
    """What Haar with tau > cmax returns: the mean of every shifted 2^L x 2^L block (a closed form that does not go through the filter bank)."""
    X = np.asarray(X, np.complex128)
    if real:
        X = X.real + 0j
    N, M, s = X.shape
    P = 1 << L
    o1, o2 = offset
    Xs = np.roll(X, (-o1, -o2), (0, 1))
    mean = Xs.reshape(N // P, P, M // P, P, s).mean(axis=(1, 3), keepdims=True)
    return np.roll(np.broadcast_to(mean, (N // P, P, M // P, P, s)).reshape(N, M, s), (o1, o2), (0, 1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fixtures and tolerances
# ---------------------------------------------------------------------------------------------------------------------------------------------
FIXTURE_GRIDS = ((16, 16), (32, 32), (32, 64), (64, 32), (48, 80))
FIXTURE_S = (1, 3, 10, 16)
FIXTURE_LEVELS = (1, 3, 4)
FIXTURE_TAUS = (0.0, 1e-3, 0.02, 0.3, 2.0)          # times cmax


def fixture_offsets(L):
    P = 1 << L
    return ((0, 0), (3 % P, 5 % P), (P - 1, P - 1))


def fixture_cases(N, M):
    """(filter, L) pairs the size rule allows on an N x M grid."""
    return [(f, L) for f in (HAAR, DB2) for L in FIXTURE_LEVELS if sizes_ok(N, M, L, f)]


def fixture_key(filt, L, joint, real):
    return (int(filt), int(L), bool(joint), bool(real))


# The measured gap between the filter bank and the dense route: max |difference| / max |X|, the largest over the grids, channel counts, offsets and
# thresholds of the fixture family (filter, L, joint, real), times 2.  tests/test_wavelet_host.py asserts the measured value from above by the entry
# and from below by a quarter of it; the device tolerance of a fixture is 16 x its entry (fused multiply-adds, another summation order).
SENS = {
    (0, 1, False, False): 1.2e-15, (0, 1, False, True): 9.5e-16, (0, 1, True, False): 1.2e-15, (0, 1, True, True): 9.5e-16,
    (0, 3, False, False): 2.3e-15, (0, 3, False, True): 2.3e-15, (0, 3, True, False): 2.3e-15, (0, 3, True, True): 2.3e-15,
    (0, 4, False, False): 2e-15, (0, 4, False, True): 1.8e-15, (0, 4, True, False): 2e-15, (0, 4, True, True): 2.1e-15,
    (1, 1, False, False): 1.6e-15, (1, 1, False, True): 1.4e-15, (1, 1, True, False): 1.6e-15, (1, 1, True, True): 1.4e-15,
    (1, 3, False, False): 3.1e-15, (1, 3, False, True): 2.5e-15, (1, 3, True, False): 3.1e-15, (1, 3, True, True): 2.8e-15,
    (1, 4, False, False): 3.5e-15, (1, 4, False, True): 2.8e-15, (1, 4, True, False): 3.1e-15, (1, 4, True, True): 3.5e-15,
}


def atol(filt, L, joint, real):
    """The device tolerance of a fixture, relative to max |X|."""
    return 16.0 * SENS[fixture_key(filt, L, joint, real)]


def measure_sens(filt, L, joint, real):
    """The gap of one fixture family (before the factor 2)."""
    worst = 0.0
    for N, M in FIXTURE_GRIDS:
        if not sizes_ok(N, M, L, filt):
            continue
        for s in FIXTURE_S:
            X = tsmi_like(N, M, s)
            _, c0 = wavelet_prox(X, 0.0, L, filt, joint, (0, 0), real)
            for off in fixture_offsets(L):
                for tr in FIXTURE_TAUS:
                    a, _ = wavelet_prox(X, tr * c0, L, filt, joint, off, real)
                    b, _ = wavelet_prox_dense(X, tr * c0, L, filt, joint, off, real)
                    worst = max(worst, float(np.abs(a - b).max() / np.abs(X).max()))
    return worst


def pnp_admm_wavelet(op, y, tau, levels=3, filt=DB2, joint=True, shift=True, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, x0=None,
                     tsmi_domain="real", maps=None, solver="lsqr", prox=wavelet_prox):
    """llr_ref.pnp_admm_llr's loop (PnP_ADMM.m:76-146 on the oracle's x-update) with Step 2 replaced by v = Wav_tau(x + uold) at the offsets of the
    iteration; tsmi_domain "real" thresholds real(x + uold).  Returns (x, lsqr_iters)."""
    if maps is None:
        x = np.asarray(x0, np.complex128).copy() if x0 is not None else op.adjoint(y)
    else:
        x = np.asarray(x0, np.complex128).copy() if x0 is not None else op.adjoint_mc(y, maps)
    v = x.copy()
    u = np.zeros_like(x)
    li = np.zeros(iters, np.int32)
    P = 1 << levels
    for it in range(iters):
        if solver == "direct":
            x = op.direct(y, v - u, gamma)
        elif maps is None:
            x, li[it], _, _ = op.lsqr(y, v - u, gamma, cg_tol, cg_maxit, x0=x)
        else:
            x, li[it], _ = op.lsqr_mc(y, maps, v - u, gamma, cg_tol, cg_maxit, x0=x)
        v, _ = prox(x + u, tau, levels, filt, joint, offsets(it, P, shift), real=tsmi_domain != "complex")
        u = u + x - v
    return x, li
