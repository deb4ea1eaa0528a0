"""The gridded operator and its x-update restated in plain numpy (fp64), and the case tables of the gridded sweep.

Written from the reference's definitions, not from the oracle's C: F.forward / F.adjoint of main_recon_tsmis_FFT.m:228-229 (unitary fft2 of every
channel, the rows of the temporal basis V applied at the sampled k locations; k indices are MATLAB's column-major ones, 0-based) and the x-update of
PnP_ADMM.m:102,153-171, x = argmin ||y - A x||^2 + r ||x - z||^2.  A^H A is block-diagonal in k-space -- G_k = sum over the frames t that sample k of
V(t,:)' V(t,:) -- so the minimiser is one s x s solve per k location: (G_k + r I) xhat_k = chat_k + r zhat_k.

tests/test_gridded_ref_host.py holds the oracle to these functions on every case below (CPU); tests/test_gpu_gridded_sweep.py holds the kernels to
both.  Every case carries its seed, so both files run the same inputs; `inputs(name)` builds them once per process."""
import functools

import numpy as np

R = 0.05                     # the x-update's weight in every case (gamma of PnP_ADMM.m)
R_SMALL = 1e-3               # the second weight of the DIRECT r-sweep


# ---- the operator --------------------------------------------------------------------------------------------------------------------------------------
def _frames(fp):
    return np.repeat(np.arange(len(fp) - 1), np.diff(fp))


def forward(x, V, fp, kidx):
    """y[(t, k)] = V[t, :] . fft2(x)[k, :] / sqrt(N M), frame after frame."""
    x = np.asarray(x)
    N, M, s = x.shape
    Xh = np.fft.fft2(x, axes=(0, 1)).reshape(N * M, s, order="F") / np.sqrt(N * M)
    return np.einsum("ic,ic->i", np.asarray(V, np.float64)[_frames(fp)], Xh[np.asarray(kidx)])


def _scatter(y, V, fp, kidx, NM):
    V = np.asarray(V, np.float64)
    Z = np.zeros((NM, V.shape[1]), np.complex128)
    np.add.at(Z, np.asarray(kidx), np.asarray(y)[:, None] * V[_frames(fp)])
    return Z


def adjoint(y, V, fp, kidx, N, M):
    """x = sqrt(N M) ifft2(Zhat), Zhat[k, :] = sum over the samples (t, k) of V[t, :] y[(t, k)]."""
    s = np.asarray(V).shape[1]
    return np.fft.ifft2(_scatter(y, V, fp, kidx, N * M).reshape((N, M, s), order="F"), axes=(0, 1)) * np.sqrt(N * M)


def gram(V, fp, kidx, NM, chunk=1 << 16):
    """G[k] = sum over the samples (t, k) of V[t, :]' V[t, :]   ([N M, s, s]; np.add.at, a chunk of samples at a time)."""
    V = np.asarray(V, np.float64)
    s = V.shape[1]
    tt, kidx = _frames(fp), np.asarray(kidx)
    G = np.zeros((NM, s, s))
    for i in range(0, kidx.size, chunk):
        v = V[tt[i:i + chunk]]
        np.add.at(G, kidx[i:i + chunk], v[:, :, None] * v[:, None, :])
    return G


def minimiser(y, z, r, V, fp, kidx, G=None):
    """argmin_x ||y - A x||^2 + r ||x - z||^2, exactly: per k, (G_k + r I) xhat_k = (A^H y)hat_k + r zhat_k."""
    z = np.asarray(z)
    N, M, s = z.shape
    if G is None:
        G = gram(V, fp, kidx, N * M)
    rhs = _scatter(y, V, fp, kidx, N * M) + r * np.fft.fft2(z, axes=(0, 1)).reshape(N * M, s, order="F") / np.sqrt(N * M)
    xh = np.linalg.solve(G + r * np.eye(s), rhs[:, :, None])[:, :, 0]
    return np.fft.ifft2(xh.reshape((N, M, s), order="F"), axes=(0, 1)) * np.sqrt(N * M)


# ---- masks: (frame_ptr, kidx), kidx 0-based column-major (k = kh + N kw), ascending inside a frame ------------------------------------------------
def _pack(ks):
    fp = np.concatenate([[0], np.cumsum([len(k) for k in ks])]).astype(np.int32)
    return fp, (np.concatenate(ks) if fp[-1] else np.zeros(0)).astype(np.int32)


def user_mask(N, M, T, per_frame, seed, pool=None, skew=1.0):
    """per_frame distinct random k locations per frame, from the whole grid -- or from `pool` random locations of it, drawn with weights that grow
    linearly from 1 to `skew` across the pool (so the locations are sampled unequally often)."""
    rng = np.random.default_rng(seed)
    if pool is None:
        return _pack([np.sort(rng.choice(N * M, per_frame, replace=False)) for _ in range(T)])
    src = np.sort(rng.permutation(N * M)[:pool])
    p = np.linspace(1.0, skew, pool)
    return _pack([np.sort(rng.choice(src, per_frame, replace=False, p=p / p.sum())) for _ in range(T)])


def full_then_k0(N, T, full):
    """Every k of the N x N grid in each of the first `full` frames, then k = 0 alone in the other frames (op_plan_test.cpp's mask of that name)."""
    return _pack([np.arange(N * N) if t < full else np.zeros(1, np.int64) for t in range(T)])


def full_with_short_last_frame(N, T, last):
    """Every k of the N x N grid in every frame but the last, which samples the first `last` k."""
    return _pack([np.arange(last if t == T - 1 else N * N) for t in range(T)])


def spiral_mask(N, S, T):
    """setup_subsampling_spiralgrided.m:7-34: an 8-turn exponential spiral of S points, rotated by 7.5 degrees per frame, rounded onto the grid
    (MATLAB's round), clamped, fftshift-ed; find()'s order inside a frame."""
    j = np.arange(S)
    t = j * (2.0 * np.pi) / (S - 1)
    t[-1] = 2.0 * np.pi
    theta = 8.0 * t
    rad = np.power(1.05, theta)
    rad = (rad - rad.min()) / (rad.max() - rad.min())
    mround = lambda a: np.sign(a) * np.floor(np.abs(a) + 0.5)
    ks = []
    for f in range(T):
        rot = f * (np.pi / 180.0 * 7.5)
        gx = np.minimum(mround(rad * np.cos(theta + rot) * N / 2.0) + N / 2.0 + 1.0, N).astype(np.int64)
        gy = np.minimum(mround(rad * np.sin(theta + rot) * N / 2.0) + N / 2.0 + 1.0, N).astype(np.int64)
        ks.append(np.unique(((gy - 1 + N // 2) % N) * N + (gx - 1 + N // 2) % N))
    return _pack(ks)


def epi_mask(N, M, pct, T):
    """setup_subsampling_epi.m:20-33: a comb of floor(N / step) k-rows, step = round(1 / pct), moved down by one row before every frame."""
    step = int(np.floor(1.0 / pct + 0.5))
    rows = np.arange(0, step * (N // step), step)
    ks = []
    for _ in range(T):
        rows = (rows + 1) % N
        ks.append(np.sort((np.sort(rows)[None, :] + N * np.arange(M)[:, None]).ravel()))
    return _pack(ks)


def empty_rows_and_frames(N, M, T, per_frame, seed):
    """Random k locations on every third k-row only (rows 1, 4, 7, ...: k-row 0 and two rows in three are never sampled); every fourth frame is empty."""
    rng = np.random.default_rng(seed)
    rows = np.arange(1, N, 3)
    allowed = (rows[:, None] + N * np.arange(M)[None, :]).ravel()
    return _pack([np.zeros(0, np.int64) if t % 4 == 3 else np.sort(rng.choice(allowed, per_frame, replace=False)) for t in range(T)])


def busy_row(N, M, T, kh, others, seed):
    """Every frame samples the whole k-row kh (M locations) and `others` random locations of the other rows: M T samples in one row."""
    rng = np.random.default_rng(seed)
    row = kh + N * np.arange(M)
    rest = np.setdiff1d(np.arange(N * M), row)
    return _pack([np.sort(np.concatenate([row, rng.choice(rest, others, replace=False)])) for _ in range(T)])


def single_sample(N, M, T, t, k):
    """One sample in all: frame t samples k, every other frame is empty."""
    return _pack([np.full(1, k, np.int64) if f == t else np.zeros(0, np.int64) for f in range(T)])


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------------------
# name -> dict(N, M, s, T, mask: () -> (fp, kidx), seed, v: "ortho" | "scaled" | "random", sweep: the DIRECT r-sweep runs on it, few_iters: the one
# case whose LSQR may stop before 5 iterations).  v = "ortho": V = Q of a QR (orthonormal columns), inputs as the existing operator tests take them
# (y = A x + noise, x0 = A^H y, z = 0.9 x0).  On the full and busy masks an orthonormal V lets LSQR converge in one or two iterations, which leaves
# the iteration kernels unexercised: v = "scaled" is V = 3 Q diag(logspace(0, -1, s)) with z = x + 0.3 noise and x0 = 0; v = "random" (T < s, no
# orthonormal columns exist) is a plain Gaussian V with the same z and x0.  The dense spiral, the T = 30 EPI mask and the busy k-row take the scaled
# V too.  tests/test_gridded_ref_host.py asserts that the oracle runs at least 5 iterations on every case but single_sample32.
SIDES = (32, 64, 96, 112, 128, 160, 192, 224, 256)
CASES = {}


def _case(table, name, N, M, s, T, mask, seed, v="ortho", sweep=False, few_iters=False):
    assert name not in CASES
    CASES[name] = dict(name=name, N=N, M=M, s=s, T=T, mask=mask, seed=seed, v=v, sweep=sweep, few_iters=few_iters)
    table.append(name)


GRIDS, CHANNELS, VCAP_CASES, MASKS = [], [], [], []
# every side once as N (h axis, contiguous) and once as M (w axis) against 32; the largest square grid
for _n, _m in [(sd, 32) for sd in SIDES] + [(32, sd) for sd in SIDES[1:]] + [(256, 256)]:
    _case(GRIDS, f"grid{_n}x{_m}", _n, _m, 10, 12, functools.partial(user_mask, _n, _m, 12, _n * _m // 16, 1000 * _n + _m), seed=_n + 7 * _m)
for _s in range(1, 11):
    _case(CHANNELS, f"chan{_s}", 64, 32, _s, 20, functools.partial(user_mask, 64, 32, 20, 200, 77 + _s), seed=300 + _s, sweep=_s in (1, 5, 10))
# T s on both sides of DC_VCAP = 2048 doubles of V in LDS.  s = 1: 8 k per frame from a pool of 48 locations sampled about 100 to 600 times each, so
# that G_k (a scalar, about samples / T) is spread over 0.05 .. 0.3 beside r = 0.05 and LSQR does not finish in three steps
for _T, _s, _per, _pool in [(204, 10, 24, None), (205, 10, 24, None), (256, 8, 24, None), (257, 8, 24, None), (300, 7, 24, None),
                            (2048, 1, 8, 48), (2049, 1, 8, 48)]:
    _case(VCAP_CASES, f"vcap_T{_T}_s{_s}", 32, 32, _s, _T, functools.partial(user_mask, 32, 32, _T, _per, 5 * _T + _s, _pool, 6.0), seed=_T + _s)
_case(MASKS, "busy32_T300", 32, 32, 10, 300, functools.partial(full_then_k0, 32, 300, 1), seed=11, v="scaled", sweep=True)       # shape 3 refuses k = 0: shape 0
_case(MASKS, "busy32_T1100", 32, 32, 10, 1100, functools.partial(full_then_k0, 32, 1100, 1), seed=12, v="scaled", sweep=True)   # only shape 2 holds the slot
_case(MASKS, "full32_T300", 32, 32, 10, 300, functools.partial(full_then_k0, 32, 300, 300), seed=13, v="scaled", sweep=True)    # no unsampled k; shape 2
_case(MASKS, "spiral32_S57_T9", 32, 32, 10, 9, functools.partial(spiral_mask, 32, 57, 9), seed=14, v="random")                   # sparse: shape 3
_case(MASKS, "spiral32_S400_T24", 32, 32, 10, 24, functools.partial(spiral_mask, 32, 400, 24), seed=15, v="scaled")              # dense: shape 0
_case(MASKS, "epi160_5th_T9", 160, 160, 10, 9, functools.partial(epi_mask, 160, 160, 0.2, 9), seed=16, v="random")               # shape 1
_case(MASKS, "epi128_5th_T30", 128, 128, 10, 30, functools.partial(epi_mask, 128, 128, 0.2, 30), seed=17, v="scaled")            # shape 1
_case(MASKS, "full32_T8", 32, 32, 10, 8, functools.partial(full_with_short_last_frame, 32, 8, 1024), seed=18, v="random", sweep=True)        # 8 per k: dense
_case(MASKS, "full32_T8_last1023", 32, 32, 10, 8, functools.partial(full_with_short_last_frame, 32, 8, 1023), seed=19, v="random", sweep=True)  # < 8: sparse
_case(MASKS, "empty_rows_frames32", 32, 32, 10, 20, functools.partial(empty_rows_and_frames, 32, 32, 20, 40, 5), seed=20)
_case(MASKS, "busy_row32_T20", 32, 32, 10, 20, functools.partial(busy_row, 32, 32, 20, 5, 10, 6), seed=21, v="scaled", sweep=True)  # 640 > DC_CH in k-row 5
_case(MASKS, "single_sample32", 32, 32, 10, 3, functools.partial(single_sample, 32, 32, 3, 1, 5 + 32 * 7), seed=22, v="random", few_iters=True)
ALL = GRIDS + CHANNELS + VCAP_CASES + MASKS
SWEEP = [n for n in ALL if CASES[n]["sweep"]]

# The oracle's DIRECT against `minimiser` at r = R_SMALL on the r-sweep cases, as tests/test_gridded_ref_host.py measures it (asserted there from
# above, with a factor 2 of room).  The GPU's bound at R_SMALL is max(1e-10, 100 x this entry).
DIRECT_SENS = {
    "chan1": 6e-14, "chan5": 2.1e-13, "chan10": 4.1e-13, "busy32_T300": 9e-14, "busy32_T1100": 3.2e-14, "full32_T300": 1.7e-15,
    "full32_T8": 2.4e-12, "full32_T8_last1023": 3.1e-12,          # (T = 8 < s = 10: G_k is singular, the condition number of G_k + r I is ~ 1 / r)
    "busy_row32_T20": 3.6e-13,
}
assert sorted(DIRECT_SENS) == sorted(SWEEP)


def direct_bound_small_r(name):
    return max(1e-10, 100.0 * DIRECT_SENS[name])


# LSQR at tol 1e-4: the project's bound on x against the oracle is 1e-10 (tests/test_gpu_operator.py), and it stands wherever the iteration is
# well conditioned: there the oracle's own x moves by <= 5e-15 under a one-ulp perturbation of y and z (lsqr_sensitivity; asserted <= 1e-12 on the
# host).  The full / busy / spiral masks with a scaled or Gaussian V are not: A^H A + r I has few distinct eigenvalues (full32_T300: ten)
# or a wide spectrum, the Krylov space is exhausted or Lanczos orthogonality is lost before the stop rule fires, and from there rounding errors
# grow by a factor 10 .. 30 per iteration (measured on the oracle alone, a perturbed against an unperturbed run with the iterations capped:
# busy32_T300 4e-16 after 5 iterations, 1e-11 after 9, 5e-9 after 11; full32_T300 1e-14 after 5, 4e-8 after 10).  For those cases this table
# records the oracle's own movement: the largest of five one-ulp perturbations (it varies 10 x from one perturbation to the next) times 3,
# asserted from above on the host.  The device's bound is 30 x the entry, about 100 x the measured figure: the device differs from the oracle by
# a few ulps in EVERY operation of EVERY iteration (other FFT, other summation orders), not by one ulp of the inputs once.  On its first run the
# device was within 4 x of the measured figure on every case.  The same cases are held to the exact minimiser to 1e-7 at tol 1e-13 and to
# identical bits between the launch forms, which no conditioning excuses.
LSQR_SENS = {
    "busy32_T300": 1.7e-8, "busy32_T1100": 4.1e-8, "full32_T300": 1.4e-7, "spiral32_S57_T9": 1.4e-8, "spiral32_S400_T24": 1.0e-9,
    "full32_T8": 7.3e-10, "full32_T8_last1023": 2.8e-10, "busy_row32_T20": 3.6e-8,
}


def lsqr_bound(name):
    return max(1e-10, 30.0 * LSQR_SENS.get(name, 0.0))


def _cn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The inputs of a case, built once: V, the mask, x / yn (operator test), y, z, x0 (x-update)."""
    c = CASES[name]
    N, M, s, T = c["N"], c["M"], c["s"], c["T"]
    rng = np.random.default_rng(c["seed"])
    fp, k = c["mask"]()
    m = int(fp[-1])
    if c["v"] == "random":
        V = rng.standard_normal((T, s))
    else:
        V = np.linalg.qr(rng.standard_normal((T, s)))[0]
        if c["v"] == "scaled":
            V = 3.0 * V * np.logspace(0.0, -1.0, s)[None, :]
    x, yn = _cn(rng, (N, M, s)), _cn(rng, m)
    if c["v"] == "ortho":
        y = forward(x, V, fp, k) + 0.01 * yn
        x0 = adjoint(y, V, fp, k, N, M)
        z = 0.9 * x0
    else:
        y = forward(x, V, fp, k) + 0.01 * yn
        z = x + 0.3 * _cn(rng, (N, M, s))
        x0 = np.zeros((N, M, s), np.complex128)
    out = dict(c, V=V, fp=fp, k=k, m=m, x=x, yn=yn, xr=rng.standard_normal((N, M, s)), y=y, z=z, x0=x0)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_operator(name):
    """The CPU oracle's operator of a case (the other yardstick: its LSQR gives the iteration count the kernels must reproduce)."""
    from oracle import oracle as O
    c = inputs(name)
    return O.Operator(c["N"], c["M"], c["V"], c["fp"], c["k"])


@functools.lru_cache(maxsize=None)
def oracle_lsqr(name, tol=1e-4, maxit=100, zero_start=False):
    """(x, iters, flag) of the oracle's LSQR x-update on a case's y, z at r = R, from the case's x0 or from 0."""
    c = inputs(name)
    x, it, fl, _ = oracle_operator(name).lsqr(c["y"], c["z"], R, tol, maxit, None if zero_start else c["x0"])
    x.setflags(write=False)
    return x, it, fl


def lsqr_sensitivity(name, trials=5):
    """How far the oracle's own x at tol 1e-4 moves when every element of y and z is perturbed by about one ulp (relative, Gaussian, 2.2e-16): the
    largest relative distance over `trials` perturbations, and whether (iterations, flag) stayed the same in all of them."""
    c = inputs(name)
    op = oracle_operator(name)
    xo, io, flo = oracle_lsqr(name)
    rng = np.random.default_rng(c["seed"] + 4242)
    worst, same = 0.0, True
    for _ in range(trials):
        y = c["y"] * (1.0 + 2.2e-16 * rng.standard_normal(c["m"]))
        z = c["z"] * (1.0 + 2.2e-16 * rng.standard_normal(c["z"].shape))
        xp, ip, flp, _ = op.lsqr(y, z, R, 1e-4, 100, c["x0"])
        worst = max(worst, float(np.linalg.norm(xp - xo) / np.linalg.norm(xo)))
        same = same and (ip, flp) == (io, flo)
    return worst, same


@functools.lru_cache(maxsize=None)
def minimisers(name):
    """{r: minimiser(y, z, r)} of a case: R, and R_SMALL on the r-sweep cases."""
    c = inputs(name)
    G = gram(c["V"], c["fp"], c["k"], c["N"] * c["M"])
    out = {r: minimiser(c["y"], c["z"], r, c["V"], c["fp"], c["k"], G=G) for r in ((R, R_SMALL) if c["sweep"] else (R,))}
    for a in out.values():
        a.setflags(write=False)
    return out
