"""The multi-coil (SENSE) operator and its x-update restated in plain numpy (fp64), and the case table of the multi-coil sweep.

Written from the definition in include/qmri.h and in the header of mc_kernels.hip, on top of gridded_ref.forward / adjoint -- not from the oracle:
    A_mc x = [A (C_j . x)]_j  (m x ncoil),      A_mc^H y = sum_j conj(C_j) . A^H y_j,      x-update: argmin ||y - A_mc x||^2 + r ||x - z||^2.
The coil maps act in image space and couple the k locations, so the per-k dense solve of gridded_ref.minimiser does not exist here: `minimiser_mc`
solves the normal equations (A_mc^H A_mc + r I) x = A_mc^H y + r z by conjugate gradients to a relative residual of 1e-13, checked on the residual
computed from x itself, and raises when that is not reached.

tests/test_mc_ref_host.py holds the oracle (Operator.forward_mc / adjoint_mc / lsqr_mc) to these functions on every case below (CPU) and asserts the
tables LSQR_SENS / TIGHT_SENS / FLAG3_SPREAD from above; tests/test_gpu_mc_sweep.py holds the kernels to both.  Every case carries its seed, so both
files run the same inputs; `inputs(name)` builds them once per process."""
import functools

import numpy as np

import gridded_ref as GR

R = GR.R                     # the x-update's weight in every case


# ---- the operator --------------------------------------------------------------------------------------------------------------------------------------
def forward_mc(x, maps, V, fp, k):
    """y[:, j] = A (C_j . x): [m, nc]."""
    x, maps = np.asarray(x), np.asarray(maps)
    return np.stack([GR.forward(maps[..., j, None] * x, V, fp, k) for j in range(maps.shape[2])], axis=1)


def adjoint_mc(y, maps, V, fp, k, N, M):
    """x = sum_j conj(C_j) . A^H y[:, j]."""
    y, maps = np.asarray(y), np.asarray(maps)
    x = np.zeros((N, M, np.asarray(V).shape[1]), np.complex128)
    for j in range(maps.shape[2]):
        x += np.conj(maps[..., j, None]) * GR.adjoint(y[:, j], V, fp, k, N, M)
    return x


def normal_residual(x, y, maps, z, r, V, fp, k):
    """|| (A_mc^H y + r z) - (A_mc^H A_mc + r I) x || / || A_mc^H y + r z ||  (0 when the right-hand side is 0 and x is)."""
    N, M, _ = np.asarray(z).shape
    b = adjoint_mc(y, maps, V, fp, k, N, M) + r * np.asarray(z)
    res = b - (adjoint_mc(forward_mc(x, maps, V, fp, k), maps, V, fp, k, N, M) + r * np.asarray(x))
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(res) / nb) if nb else float(np.linalg.norm(res))


def normal_mc(v, maps, G):
    """A_mc^H A_mc v with A^H A applied in k-space, where it is block-diagonal (G = gridded_ref.gram: one s x s block per k location):
    sum_j conj(C_j) . ifft2(G fft2(C_j . v)).  The fast route of minimiser_mc's iteration; the host test holds it to adjoint_mc(forward_mc(v))."""
    v, maps = np.asarray(v), np.asarray(maps)
    N, M, s = v.shape
    out = np.zeros((N, M, s), np.complex128)
    for j in range(maps.shape[2]):
        vh = np.fft.fft2(maps[..., j, None] * v, axes=(0, 1)).reshape(N * M, s, order="F")
        out += np.conj(maps[..., j, None]) * np.fft.ifft2(np.einsum("kab,kb->ka", G, vh).reshape((N, M, s), order="F"), axes=(0, 1))
    return out


def minimiser_mc(y, maps, z, r, V, fp, k, rtol=1e-13, maxit=4000, G=None):
    """argmin_x ||y - A_mc x||^2 + r ||x - z||^2 by conjugate gradients on the normal equations, from x = z.  The iteration applies A_mc^H A_mc
    through normal_mc; what ends it is the TRUE residual b - (A_mc^H (A_mc x) + r x), computed through forward_mc and adjoint_mc whenever the
    recurrence's residual (which drifts from the true one by about eps x the condition number) reports rtol: above rtol the iteration restarts from
    the true residual.  The function returns only when that relative residual is <= rtol and raises otherwise."""
    z = np.asarray(z, np.complex128)
    N, M, _ = z.shape
    if G is None:
        G = GR.gram(V, fp, k, N * M)
    H = lambda v: normal_mc(v, maps, G) + r * v
    b = adjoint_mc(y, maps, V, fp, k, N, M) + r * z
    nb = np.linalg.norm(b)
    if nb == 0.0:
        return np.zeros_like(z)
    x = z.copy()
    done = 0
    for _ in range(20):                                           # restarts
        res = b - (adjoint_mc(forward_mc(x, maps, V, fp, k), maps, V, fp, k, N, M) + r * x)
        if np.linalg.norm(res) <= rtol * nb:
            return x
        p, rs = res.copy(), np.vdot(res, res).real
        while done < maxit:
            Hp = H(p)
            a = rs / np.vdot(p, Hp).real
            x = x + a * p
            res = res - a * Hp
            rs_new = np.vdot(res, res).real
            done += 1
            if np.sqrt(rs_new) <= 0.5 * rtol * nb:
                break
            p = res + (rs_new / rs) * p
            rs = rs_new
        if done >= maxit:
            break
    rel = np.linalg.norm(b - (adjoint_mc(forward_mc(x, maps, V, fp, k), maps, V, fp, k, N, M) + r * x)) / nb
    if rel <= rtol:
        return x
    raise RuntimeError(f"minimiser_mc: relative residual {rel:.2e} after {done} iterations, {rtol:.0e} wanted")


# ---- coil maps: [N, M, nc] -------------------------------------------------------------------------------------------------------------------------------
def _grid(N, M):
    return np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")


def maps_smooth(N, M, nc, phase):
    """nc Gaussians centred on the unit circle, each times a smooth phase (the maps of tests/test_gpu_mc_batch.py), normalised to sum_j |C_j|^2 = 1."""
    hh, ww = _grid(N, M)
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                  for a in phase + np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def ellipse(N, M):
    """The support of maps_masked: True inside the ellipse (h / 0.9)^2 + (w / 0.8)^2 <= 1."""
    hh, ww = _grid(N, M)
    return (hh / 0.9) ** 2 + (ww / 0.8) ** 2 <= 1.0


def maps_masked(N, M, nc, phase):
    """maps_smooth with exact zeros outside the ellipse in every coil, as estimated maps have: A_mc has a null space there, the minimiser equals z."""
    return maps_smooth(N, M, nc, phase) * ellipse(N, M)[:, :, None]


def maps_unnormalised(N, M, nc, phase, lo=0.2, hi=3.0):
    """maps_smooth times sqrt(g), g bilinear from lo (the edges h = -1 and w = -1) to hi (the corner h = w = 1): sum_j |C_j|^2 = g."""
    hh, ww = _grid(N, M)
    g = lo + (hi - lo) * (hh + 1.0) * (ww + 1.0) / 4.0
    return maps_smooth(N, M, nc, phase) * np.sqrt(g)[:, :, None]


def maps_constant(N, M, nc, phase):
    """One complex constant per coil, sum_j |c_j|^2 = 1."""
    c = (1.0 + np.arange(nc)) * np.exp(1j * (phase + 1.3 * np.arange(nc)))
    return np.broadcast_to(c / np.linalg.norm(c), (N, M, nc)).copy()


MAPS = {"smooth": maps_smooth, "masked": maps_masked, "unnormalised": maps_unnormalised, "constant": maps_constant}

# ---- the case table -------------------------------------------------------------------------------------------------------------------------------------
# name -> dict(N, M, s, T, mask: () -> (fp, kidx), nc, S, max_batch: the values the GPU runs it under, maps_kind, seed, kind).  V is the orthonormal Q of a QR
# in every case (one V per operator, so per stack).  kind "generic": per slice y = A_mc x + 1 % noise, z = x + 0.1 noise, x0 = A_mc^H y;
# kind "stagger": see _stagger_slices.  A chunk is max_batch consecutive coil images g = b nc + j of the whole stack.
CASES = {}
COILS, STRIDES, MASKS, MAPCASES, STAGGER = [], [], [], [], []


def _case(table, name, N, M, s, T, mask, nc, S, max_batch, seed, maps="smooth", kind="generic"):
    assert name not in CASES and N in GR.SIDES and M in GR.SIDES and T >= s
    CASES[name] = dict(name=name, N=N, M=M, s=s, T=T, mask=mask, nc=nc, S=S, max_batch=tuple(max_batch), seed=seed, maps_kind=maps, kind=kind)
    table.append(name)


_um = lambda N, M, T, per, seed: functools.partial(GR.user_mask, N, M, T, per, seed)
# coil counts and chunkings: 32 x 32, s = 6, T = 24, 100 samples per frame
_case(COILS, "coils1x5", 32, 32, 6, 24, _um(32, 32, 24, 100, 501), 1, 5, (1, 3, 8), seed=41)      # one coil per slice; 3 / 5 whole slices per chunk (nb = cnt)
_case(COILS, "coils2x5", 32, 32, 6, 24, _um(32, 32, 24, 100, 502), 2, 5, (8,), seed=42)           # a chunk over four slices, a short last chunk of one
_case(COILS, "coils3x3", 32, 32, 6, 24, _um(32, 32, 24, 100, 503), 3, 3, (8, 2), seed=43)         # 8: slices 0, 1 and 2/3 of slice 2, then a chunk of ONE image that continues slice 2's sum
_case(COILS, "coils4x3", 32, 32, 6, 24, _um(32, 32, 24, 100, 504), 4, 3, (4, 3), seed=44)         # 4: chunk = slice; 3: chunks start at coil 3, 2, 1 of a slice
_case(COILS, "coils5x3", 32, 32, 6, 24, _um(32, 32, 24, 100, 505), 5, 3, (2, 4, 7), seed=45)      # ragged last chunks (15 = 7 x 2 + 1 = 3 x 4 + 3 = 2 x 7 + 1), mid-slice starts
_case(COILS, "coils8x2", 32, 32, 6, 24, _um(32, 32, 24, 100, 506), 8, 2, (3, 8, 16), seed=46)     # 3: a slice over three chunks; 16 = nc S exactly
_case(COILS, "coils13x1", 32, 32, 6, 24, _um(32, 32, 24, 100, 507), 13, 1, (4,), seed=47)         # one slice through four chunks, the last of one coil
# strides of the streaming kernels: PS NT = 65 536 image elements, PC NT = 16 384 samples
_case(STRIDES, "stride128x64", 128, 64, 10, 12, _um(128, 64, 12, 2048, 511), 3, 2, (4,), seed=51)  # m = 24 576, n = 81 920: every loop runs twice
_case(STRIDES, "stride32x128", 32, 128, 10, 12, _um(32, 128, 12, 256, 512), 2, 2, (3,), seed=52)   # n = 40 960: 160 of 256 partial workgroups hold elements
_case(STRIDES, "stride32x32_s1", 32, 32, 1, 24, _um(32, 32, 24, 100, 513), 4, 2, (3,), seed=53)    # n = 1024: 252 of 256 partials are exact zeros
_case(STRIDES, "stride64x32_s3", 64, 32, 3, 12, _um(64, 32, 12, 200, 514), 3, 1, (2,), seed=54)    # n = 6144 = 24 workgroups, plane = 2048
# masks: 32 x 32 (EPI: 64 x 32), s = 6, 3 coils, 2 slices, chunks of 4 (the second starts inside slice 1)
_case(MASKS, "single_sample", 32, 32, 6, 8, functools.partial(GR.single_sample, 32, 32, 8, 1, 5 + 32 * 7), 3, 2, (4,), seed=61)   # m = 1: 63 of 64 sample partials zero
_case(MASKS, "empty_rows_frames", 32, 32, 6, 24, functools.partial(GR.empty_rows_and_frames, 32, 32, 24, 60, 7), 3, 2, (4,), seed=62)
_case(MASKS, "full_then_k0", 32, 32, 6, 8, functools.partial(GR.full_then_k0, 32, 8, 2), 3, 2, (4,), seed=63)
_case(MASKS, "epi64x32", 64, 32, 6, 12, functools.partial(GR.epi_mask, 64, 32, 1 / 8, 12), 3, 2, (4,), seed=64)
# maps
_case(MAPCASES, "masked32", 32, 32, 6, 24, _um(32, 32, 24, 100, 521), 3, 2, (4,), seed=71, maps="masked")
_case(MAPCASES, "masked64x32", 64, 32, 6, 24, _um(64, 32, 24, 200, 522), 3, 2, (4,), seed=72, maps="masked")
_case(MAPCASES, "unnormalised32", 32, 32, 6, 24, _um(32, 32, 24, 100, 523), 3, 2, (4,), seed=73, maps="unnormalised")
_case(MAPCASES, "constant32", 32, 32, 6, 24, _um(32, 32, 24, 100, 524), 3, 2, (4,), seed=74, maps="constant")
# staggered stops: five slices of one stack that stop at different iterations (see _stagger_slices)
_case(STAGGER, "stagger", 32, 32, 6, 24, _um(32, 32, 24, 100, 531), 4, 5, (3, 20), seed=81, kind="stagger")
ALL = COILS + STRIDES + MASKS + MAPCASES + STAGGER
MASKED = [n for n in ALL if CASES[n]["maps_kind"] == "masked"]
STAGGER_LONG_TOL = 1e-10        # the prediction test's long solve: stagger's slice 3 at this tol
FLAG3_CASE = "stride32x32_s1"   # the stagnation exit: this case's slice 0 at tol = 0, maxit = 300

# LSQR at tol 1e-4 against the oracle: the project's bound on x is 1e-10 (tests/test_gpu_operator.py, tests/test_gpu_mc_batch.py) wherever the
# oracle's own x moves by <= 1e-12 under one-ulp perturbations of y and z (lsqr_sensitivity; asserted on the host).  A case where it moves further
# enters 3 x the largest of five perturbations here and is held to 30 x the entry: the rule, the margins and the reason of gridded_ref.lsqr_bound.
# The host test asserts that at most a quarter of the cases are entered and none of COILS.
# Measured: the oracle's x moves by 2.4e-16 .. 7.2e-16 on every slice of every case (orthonormal V, maps with sum_j |C_j|^2 <= 12), so no case is
# entered and every case takes 1e-10.
LSQR_SENS = {}

# The oracle's lsqr_mc at tol 1e-13, maxit 300 against minimiser_mc, the largest over a case's slices, as tests/test_mc_ref_host.py measures it
# (asserted there from above; entered with a factor 3 of room -- the figure is the rounding of two iterations, the oracle's and minimiser_mc's, whose
# own residual is 3e-14 .. 5e-14).  The device's bound is max(1e-7, 100 x entry), so 1e-7 on every case: the figure tests/test_gpu_operator.py and
# the gridded sweep hold the single-coil tight solve to.
TIGHT_SENS = {
    "coils1x5": 2.7e-13, "coils2x5": 2.3e-13, "coils3x3": 2.0e-13, "coils4x3": 2.5e-13, "coils5x3": 2.6e-13, "coils8x2": 1.9e-13, "coils13x1": 2.5e-13,
    "stride128x64": 3.3e-13, "stride32x128": 1.9e-13, "stride32x32_s1": 3.0e-13, "stride64x32_s3": 2.0e-13,
    "single_sample": 1e-15, "empty_rows_frames": 1.7e-13, "full_then_k0": 4e-15, "epi64x32": 3.0e-13,
    "masked32": 1.3e-13, "masked64x32": 1.5e-13, "unnormalised32": 2.3e-13, "constant32": 2.7e-13,
    "stagger": 5.1e-12,        # (slice 3: sum_j |C_j|^2 up to 12 beside r = 0.05)
}
assert sorted(TIGHT_SENS) == sorted(ALL)

# How far the oracle's count of the flag-3 solve (FLAG3_CASE, tol 0: 42 iterations) moves under the five one-ulp perturbations: it does not (asserted
# from above on the host).  The device's count may differ from the oracle's by this + 2.
FLAG3_SPREAD = 0


def lsqr_bound(name):
    return max(1e-10, 30.0 * LSQR_SENS.get(name, 0.0))


def tight_bound(name):
    return max(1e-7, 100.0 * TIGHT_SENS[name])


def _cn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _generic_slice(rng, c, V, fp, k, maps):
    N, M, s, nc = c["N"], c["M"], c["s"], c["nc"]
    x = _cn(rng, (N, M, s))
    y = forward_mc(x, maps, V, fp, k)
    y = y + 0.01 * _cn(rng, y.shape)
    z = x + 0.1 * _cn(rng, (N, M, s))
    return x, y, z, adjoint_mc(y, maps, V, fp, k, N, M)


def _stagger_slices(rng, c, V, fp, k):
    """Slice 0 generic; slice 1 y = 0, z = x0 = 0 (stops at iteration 0 with x = 0); slice 2 z = x0 = the minimiser of a generic problem and
    y = A_mc of it (the residual is rounding noise: stops at 0); slice 3 strongly unnormalised maps (sum_j |C_j|^2 from 0.02 to 12), z pure noise and
    x0 = 0: many iterations (V belongs to the operator, one per stack, so the spread of this slice's spectrum comes from its maps alone); slice 4
    slice 0's x, noise and z under other maps."""
    N, M, s, nc = c["N"], c["M"], c["s"], c["nc"]
    maps = [maps_smooth(N, M, nc, 0.0), maps_smooth(N, M, nc, 0.4), maps_smooth(N, M, nc, 0.8),
            maps_unnormalised(N, M, nc, 1.2, 0.02, 12.0), maps_smooth(N, M, nc, 1.6)]
    x0_, y0, z0, s0 = _generic_slice(rng, c, V, fp, k, maps[0])
    zero = np.zeros((N, M, s), np.complex128)
    xg, yg, zg, _ = _generic_slice(rng, c, V, fp, k, maps[2])
    xm = minimiser_mc(yg, maps[2], zg, R, V, fp, k)
    x3 = _cn(rng, (N, M, s))
    y3 = forward_mc(x3, maps[3], V, fp, k)
    y3 = y3 + 0.01 * _cn(rng, y3.shape)
    z3 = _cn(rng, (N, M, s))
    y4 = forward_mc(x0_, maps[4], V, fp, k) + (y0 - forward_mc(x0_, maps[0], V, fp, k))
    xs = [x0_, zero, xm, x3, x0_]
    ys = [y0, np.zeros_like(y0), forward_mc(xm, maps[2], V, fp, k), y3, y4]
    zs = [z0, zero, xm, z3, z0]
    x0s = [s0, zero, xm, zero, adjoint_mc(y4, maps[4], V, fp, k, N, M)]
    return maps, xs, ys, zs, x0s


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The inputs of a case, built once: V, the mask, per slice the maps [S, N, M, nc], x, y [S, m, nc], z and x0 [S, N, M, s]; for the operator's
    tests xop [N, M, s] complex, xr real and yn [m, nc].  Read-only."""
    c = CASES[name]
    N, M, s, T, nc, S = c["N"], c["M"], c["s"], c["T"], c["nc"], c["S"]
    rng = np.random.default_rng(c["seed"])
    fp, k = c["mask"]()
    m = int(fp[-1])
    V = np.linalg.qr(rng.standard_normal((T, s)))[0]
    if c["kind"] == "stagger":
        maps, xs, ys, zs, x0s = _stagger_slices(rng, c, V, fp, k)
    else:
        maps = [MAPS[c["maps_kind"]](N, M, nc, 0.7 * b) for b in range(S)]
        xs, ys, zs, x0s = zip(*[_generic_slice(rng, c, V, fp, k, maps[b]) for b in range(S)])
    assert len(maps) == S
    out = dict(c, V=V, fp=fp, k=k, m=m, maps=np.stack(maps), x=np.stack(xs), y=np.stack(ys), z=np.stack(zs), x0=np.stack(x0s), yn=_cn(rng, (m, nc)), xop=_cn(rng, (N, M, s)), xr=rng.standard_normal((N, M, s)))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_operator(name):
    """The CPU oracle's operator of a case (the other yardstick: its lsqr_mc gives the iteration count the kernels must reproduce)."""
    from oracle import oracle as O
    c = inputs(name)
    return O.Operator(c["N"], c["M"], c["V"], c["fp"], c["k"])


@functools.lru_cache(maxsize=None)
def oracle_lsqr(name, b, tol=1e-4, maxit=100):
    """(x, iters, flag) of the oracle's lsqr_mc on slice b of a case at r = R, from the case's x0."""
    c = inputs(name)
    x, it, fl = oracle_operator(name).lsqr_mc(c["y"][b], c["maps"][b], c["z"][b], R, tol=tol, maxit=maxit, x0=c["x0"][b])
    x.setflags(write=False)
    return x, int(it), int(fl)


def perturbed(name, b, trials=5):
    """`trials` copies of slice b's (y, z) with every element perturbed by about one ulp (relative, Gaussian, 2.2e-16), as gridded_ref.lsqr_sensitivity."""
    c = inputs(name)
    rng = np.random.default_rng(c["seed"] + 4242 + b)
    for _ in range(trials):
        yield (c["y"][b] * (1.0 + 2.2e-16 * rng.standard_normal(c["y"][b].shape)), c["z"][b] * (1.0 + 2.2e-16 * rng.standard_normal(c["z"][b].shape)))


def lsqr_sensitivity(name, b, tol=1e-4, maxit=100):
    """How far the oracle's own x moves under the perturbations of `perturbed` (largest relative distance; absolute where x = 0), and the
    (iterations, flag) of every perturbed run."""
    c = inputs(name)
    op = oracle_operator(name)
    xo, _, _ = oracle_lsqr(name, b, tol, maxit)
    worst, counts = 0.0, []
    for y, z in perturbed(name, b):
        xp, ip, flp = op.lsqr_mc(y, c["maps"][b], z, R, tol=tol, maxit=maxit, x0=c["x0"][b])
        worst = max(worst, float(np.linalg.norm(xp - xo) / max(np.linalg.norm(xo), 1e-300)))
        counts.append((int(ip), int(flp)))
    return worst, counts


@functools.lru_cache(maxsize=None)
def minimisers(name):
    """minimiser_mc of every slice of a case at r = R: [S, N, M, s], read-only."""
    c = inputs(name)
    G = GR.gram(c["V"], c["fp"], c["k"], c["N"] * c["M"])
    out = np.stack([minimiser_mc(c["y"][b], c["maps"][b], c["z"][b], R, c["V"], c["fp"], c["k"], G=G) for b in range(c["S"])])
    out.setflags(write=False)
    return out
