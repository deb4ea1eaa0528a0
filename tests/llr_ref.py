"""Locally low-rank (LLR) proximal step: the numpy restatement that defines qmri_llr_prox (include/qmri.h).

X is N x M x s (numpy shape (N, M, s); in the ABI the first side is contiguous and the channel planes are outermost).  With block side b | N, M and
offsets 0 <= o1, o2 < b, block (i, j) holds the pixels ((o1 + i b + p) mod N, (o2 + j b + q) mod M), p, q < b: the wrap is circular, so every block
is full.  The b^2 x s Casorati matrix A of a block becomes U max(S - tau, 0) V^H.  sigma_max is the largest singular value over the blocks before
thresholding.  Real mode works on real(X) and returns an imaginary part that is exactly 0.

llr_prox is the definition (LAPACK SVD per block); llr_prox_gram is the route the device kernel takes (Gram matrix, Hermitian eigenpairs, A W),
restated so that the gap between the two can be measured on the host: SENS holds that gap per fixture.
"""
import numpy as np

BLOCKS = (4, 8, 16)


def offsets(it, b, shift=True):
    """The block offsets (o1, o2) of ADMM iteration `it` (0-based): (0, 0) without shift, else q = it mod b^2, o1 = q mod b,
    o2 = (q div b + q) mod b: every offset once per b^2 iterations, both coordinates moving each iteration."""
    if not shift:
        return 0, 0
    q = it % (b * b)
    return q % b, (q // b + q) % b


def _check(X, tau, b, offset):
    X = np.asarray(X)
    if X.ndim != 3:
        raise ValueError("X must be N x M x s")
    N, M, s = X.shape
    if b not in BLOCKS or N % b or M % b:
        raise ValueError("block must be 4, 8 or 16 and divide N and M")
    o1, o2 = offset
    if not (0 <= o1 < b and 0 <= o2 < b):
        raise ValueError("offsets must satisfy 0 <= o < block")
    if not tau >= 0:
        raise ValueError("tau must be >= 0")
    return N, M, s, int(o1), int(o2)


def block_index(N, M, b, o1, o2, i, j):
    """Row and column indices (np.ix_ form) of block (i, j)."""
    return np.ix_((o1 + i * b + np.arange(b)) % N, (o2 + j * b + np.arange(b)) % M)


def _apply(X, tau, b, offset, real, block_fn):
    N, M, s, o1, o2 = _check(X, tau, b, offset)
    Xc = np.asarray(X, np.float64).astype(np.complex128) if not np.iscomplexobj(X) else np.asarray(X, np.complex128)
    if real:
        Xc = Xc.real.astype(np.complex128)
    out = np.zeros((N, M, s), np.complex128)
    smax = 0.0
    for j in range(M // b):
        for i in range(N // b):
            r, c = block_index(N, M, b, o1, o2, i, j)
            A = Xc[r, c, :].reshape(b * b, s)
            if real:
                A = A.real
            Bk, sm = block_fn(A, tau)
            out[r, c, :] = Bk.reshape(b, b, s)
            smax = max(smax, sm) if not np.isnan(sm) else np.nan
    if real:
        out = out.real + 0j
    return out, float(smax)


def _svd_block(A, tau):
    if not A.any():
        return np.zeros_like(A), 0.0
    U, S, Vh = np.linalg.svd(A, full_matrices=False)
    return (U * np.maximum(S - tau, 0.0)) @ Vh, float(S[0])


def _gram_block(A, tau):
    G = A.conj().T @ A
    lam, V = np.linalg.eigh(G)
    sig = np.sqrt(np.maximum(lam, 0.0))
    f = np.zeros_like(sig)
    nz = sig > tau
    f[nz] = 1.0 - tau / sig[nz]
    W = (V * f) @ V.conj().T
    return A @ W, float(sig.max())


def llr_prox(X, tau, block=8, offset=(0, 0), real=False):
    """The definition: (out N x M x s complex128, sigma_max)."""
    return _apply(X, float(tau), int(block), offset, real, _svd_block)


def llr_prox_gram(X, tau, block=8, offset=(0, 0), real=False):
    """The kernel's route (G = A^H A, eigenpairs, W = V diag(max(0, 1 - tau / sigma)) V^H, A W) with LAPACK's eigh."""
    return _apply(X, float(tau), int(block), offset, real, _gram_block)


def llr_prox_stack(X, tau, block=8, offset=(0, 0), real=False):
    outs = [llr_prox(x, tau, block, offset, real) for x in X]
    return np.stack([o for o, _ in outs]), np.array([m for _, m in outs])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fixtures: TSMI-like data -- three spatial components mixed into s channels with geometrically decaying energy, plus 1e-3 noise
# ---------------------------------------------------------------------------------------------------------------------------------------------
def tsmi_like(N, M, s, seed=0, complex_=True):
    rng = np.random.default_rng(seed)
    n1, n2 = np.meshgrid(np.arange(N) / N, np.arange(M) / M, indexing="ij")
    comps = np.stack([np.exp(-((n1 - 0.4) ** 2 + (n2 - 0.55) ** 2) * 8.0),
                      np.cos(2 * np.pi * (n1 + 0.5 * n2)) * (n1 > 0.25),
                      ((n1 - 0.6) ** 2 + (n2 - 0.3) ** 2 < 0.06).astype(np.float64)], -1)              # N x M x 3
    mix = rng.standard_normal((3, s)) + (1j * rng.standard_normal((3, s)) if complex_ else 0)
    mix = mix * (0.5 ** np.arange(s))[None, :]
    if complex_:
        comps = comps * np.exp(1j * 2.0 * n1 * n2)[..., None]
    X = comps @ mix
    X = X + 1e-3 * (rng.standard_normal((N, M, s)) + (1j * rng.standard_normal((N, M, s)) if complex_ else 0))
    return X.astype(np.complex128)


FIXTURE_GRIDS = ((32, 32), (32, 64), (64, 32))
FIXTURE_S = (1, 2, 3, 10, 16)
FIXTURE_TAUS = (0.0, 1e-3, 0.02, 0.3, 2.0)          # times sigma_max


def fixture_offsets(b):
    return ((0, 0), (min(3, b - 1), min(5, b - 1)), (b - 1, b - 1))


def fixture_key(s, b, real):
    return (int(s), int(b), bool(real))


# The measured gap between the SVD definition and the Gram route: max |difference| / max |X|, the largest over the grids, offsets and thresholds of
# the fixture family (s, block, real), times 2.  tests/test_llr_host.py asserts the measured value from above by the entry and from below by a
# quarter of it; the device tolerance of a fixture is 16 x its entry (Jacobi instead of LAPACK, fused multiply-adds, another summation order).
SENS = {
    (1, 4, False): 1.4e-15, (1, 4, True): 6.9e-16, (1, 8, False): 2.5e-15, (1, 8, True): 1.6e-15, (1, 16, False): 3e-15, (1, 16, True): 2.2e-15,
    (2, 4, False): 3.1e-14, (2, 4, True): 1.6e-15, (2, 8, False): 4.5e-15, (2, 8, True): 2.5e-15, (2, 16, False): 5e-15, (2, 16, True): 5.3e-15,
    (3, 4, False): 1.6e-14, (3, 4, True): 1.3e-14, (3, 8, False): 1.7e-14, (3, 8, True): 3e-14, (3, 16, False): 1.1e-14, (3, 16, True): 3.3e-15,
    (10, 4, False): 6.5e-14, (10, 4, True): 5.9e-14, (10, 8, False): 3.9e-14, (10, 8, True): 2.2e-14, (10, 16, False): 6.6e-14, (10, 16, True): 1.8e-14,
    (16, 4, False): 7.7e-14, (16, 4, True): 4.3e-14, (16, 8, False): 2.9e-14, (16, 8, True): 2.2e-14, (16, 16, False): 1.1e-13, (16, 16, True): 1.4e-14,
}


def atol(s, b, real):
    """The device tolerance of a fixture, relative to max |X|."""
    return 16.0 * SENS[fixture_key(s, b, real)]


def pnp_admm_llr(op, y, tau, block=8, shift=True, gamma=0.05, iters=100, cg_tol=1e-4, cg_maxit=100, x0=None, tsmi_domain="real", maps=None,
                 solver="lsqr", prox=llr_prox):
    """complex_admm_ref.pnp_admm (PnP_ADMM.m:76-146 on the oracle's x-update) with Step 2 replaced by v = LLR_tau(x + uold) at the offsets of the
    iteration; tsmi_domain "real" thresholds real(x + uold) as the reference's Step 2 takes the real part.  Returns (x, lsqr_iters)."""
    if maps is None:
        x = np.asarray(x0, np.complex128).copy() if x0 is not None else op.adjoint(y)
    else:
        x = np.asarray(x0, np.complex128).copy() if x0 is not None else op.adjoint_mc(y, maps)
    v = x.copy()
    u = np.zeros_like(x)
    li = np.zeros(iters, np.int32)
    for it in range(iters):
        if solver == "direct":
            x = op.direct(y, v - u, gamma)
        elif maps is None:
            x, li[it], _, _ = op.lsqr(y, v - u, gamma, cg_tol, cg_maxit, x0=x)
        else:
            x, li[it], _ = op.lsqr_mc(y, maps, v - u, gamma, cg_tol, cg_maxit, x0=x)
        v, _ = prox(x + u, tau, block, offsets(it, block, shift), real=tsmi_domain != "complex")
        u = u + x - v
    return x, li
