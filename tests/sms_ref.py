"""The simultaneous multi-slice (SMS) operator and its joint x-update restated in plain numpy (fp64), and the case table of the SMS tests.

Written from the definition in include/qmri.h, on top of mc_ref.forward_mc / adjoint_mc -- not from the kernels:
    A_sms x   = sum_b E[t(i), b] (A_mc,b x_b)[i]            ([m, nc]; slice b added after slice b - 1)
    A_sms^H y = [ A_mc,b^H (conj(E[t(.), b]) y) ]_b          ([Z, N, M, s])
    x-update: argmin ||y - A_sms x||^2 + r ||x - z||^2 over the Z slices of a group jointly.
`SmsOperator` carries N, M, s and the pair as forward_mc / adjoint_mc, so the oracle's Operator.lsqr_mc -- which is written against exactly those --
restates the solve when called unbound on it.  `minimiser_sms` solves the normal equations by conjugate gradients to 1e-13 on the TRUE residual and
raises otherwise, as mc_ref.minimiser_mc does.

tests/test_sms_host.py measures, on the CPU and with the oracle alone, what the tables below hold; tests/test_gpu_sms.py holds the kernels to them.
A group's arrays: maps [Z, N, M, nc], y [m, nc], x / z / x0 [Z, N, M, s]; a case stacks G groups on a leading axis."""
import functools

import numpy as np

import gridded_ref as GR
import mc_ref as MC

R = GR.R


def caipi(T, Z):
    """E[t, b] = exp(2 pi i b (t mod Z) / Z): [T, Z]."""
    t, b = np.meshgrid(np.arange(T) % Z, np.arange(Z), indexing="ij")
    return np.exp(2j * np.pi * b * t / Z)


def frames(fp):
    """Frame of every sample in the ABI's frame-major order."""
    return np.repeat(np.arange(len(fp) - 1), np.diff(fp))


# ---- the operator ------------------------------------------------------------------------------------------------------------------------------------
def forward_sms(x, maps, E, V, fp, k):
    tf = frames(fp)
    y = E[tf, 0][:, None] * MC.forward_mc(x[0], maps[0], V, fp, k)
    for b in range(1, len(x)):
        y = y + E[tf, b][:, None] * MC.forward_mc(x[b], maps[b], V, fp, k)
    return y


def adjoint_sms(y, maps, E, V, fp, k, N, M):
    tf = frames(fp)
    return np.stack([MC.adjoint_mc(np.conj(E[tf, b])[:, None] * np.asarray(y), maps[b], V, fp, k, N, M) for b in range(len(maps))])


class SmsOperator:
    """What oracle.Operator.lsqr_mc needs of `self`: N, M, s, forward_mc(x, maps), adjoint_mc(y, maps) -- here on a group, x [Z, N, M, s]."""

    def __init__(self, N, M, V, fp, k, E):
        self.N, self.M, self.s = N, M, np.asarray(V).shape[1]
        self.V, self.fp, self.k, self.E = V, fp, k, np.asarray(E)

    def forward_mc(self, x, maps):
        return forward_sms(np.asarray(x), np.asarray(maps), self.E, self.V, self.fp, self.k)

    def adjoint_mc(self, y, maps):
        return adjoint_sms(y, np.asarray(maps), self.E, self.V, self.fp, self.k, self.N, self.M)

    def lsqr(self, y, maps, z, r, tol=1e-4, maxit=100, x0=None):
        """(x, iters, flag) of the oracle's lsqr_mc, statement for statement, on this operator."""
        from oracle import oracle as O
        x0 = np.zeros_like(np.asarray(z), dtype=np.complex128) if x0 is None else x0
        x, it, fl = O.Operator.lsqr_mc(self, y, maps, z, r, tol=tol, maxit=maxit, x0=x0)
        return x, int(it), int(fl)


def minimiser_sms(op, y, maps, z, r, rtol=1e-13, maxit=4000):
    """argmin_x ||y - A_sms x||^2 + r ||x - z||^2 by conjugate gradients on the normal equations, from x = z, restarted from the true residual
    until that is <= rtol relative; raises otherwise."""
    z = np.asarray(z, np.complex128)
    H = lambda v: op.adjoint_mc(op.forward_mc(v, maps), maps) + r * v
    b = op.adjoint_mc(y, maps) + r * z
    nb = np.linalg.norm(b)
    if nb == 0.0:
        return np.zeros_like(z)
    x = z.copy()
    done = 0
    for _ in range(20):
        res = b - H(x)
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
    rel = np.linalg.norm(b - H(x)) / nb
    if rel <= rtol:
        return x
    raise RuntimeError(f"minimiser_sms: relative residual {rel:.2e} after {done} iterations, {rtol:.0e} wanted")


# ---- the case table -----------------------------------------------------------------------------------------------------------------------------------
# name -> dict(N, M, s, T, mask, nc, Z, G, max_batch: the values the GPU runs it under, maps_kind, E_kind, seed, kind).  One V and one E per
# operator.  kind "generic": per group y = A_sms x + 1 % noise, z = x + 0.1 noise, x0 = A_sms^H y; "stagger": see _stagger_groups.  Forward
# chunks are max_batch consecutive images q = (g nc + j) Z + b, adjoint chunks q = (g Z + b) nc + j.
CASES = {}
ALL = []


def _case(name, N, M, s, T, mask, nc, Z, G, max_batch, seed, maps="smooth", E="caipi", kind="generic"):
    assert name not in CASES and N in GR.SIDES and M in GR.SIDES and T >= s and 1 <= Z <= 8
    CASES[name] = dict(name=name, N=N, M=M, s=s, T=T, mask=mask, nc=nc, Z=Z, G=G, max_batch=tuple(max_batch), seed=seed, maps_kind=maps, E_kind=E, kind=kind)
    ALL.append(name)


_um = lambda N, M, T, per, seed: functools.partial(GR.user_mask, N, M, T, per, seed)
_case("z2c4", 32, 32, 6, 24, _um(32, 32, 24, 100, 901), 4, 2, 1, (1, 3, 8), seed=91)
_case("z3c3g2", 32, 32, 6, 24, _um(32, 32, 24, 100, 902), 3, 3, 2, (2, 4, 5, 18), seed=92)      # chunks begin inside a (g, j) sum and inside a slice's coil sum; 18: the whole call
_case("z8c2", 32, 32, 6, 24, _um(32, 32, 24, 100, 903), 2, 8, 1, (3,), seed=93)
_case("z1c4g3", 32, 32, 6, 24, _um(32, 32, 24, 100, 904), 4, 1, 3, (4,), seed=94, E="ones")       # the degenerate case: qmri_xupdate_mc_batch's bits
_case("z4c3masked", 32, 32, 6, 24, _um(32, 32, 24, 100, 905), 3, 4, 1, (4,), seed=95, maps="masked")
_case("genE", 32, 32, 6, 24, _um(32, 32, 24, 100, 906), 4, 2, 1, (3,), seed=96, E="gauss")        # complex Gaussian E, not of unit modulus
_case("stride", 128, 64, 10, 12, _um(128, 64, 12, 2048, 907), 3, 2, 1, (4,), seed=97)             # m = 24 576, Z n = 163 840: every strided loop and partial runs more than once
_case("epi64x32", 64, 32, 6, 12, functools.partial(GR.epi_mask, 64, 32, 1 / 8, 12), 3, 2, 1, (4,), seed=98)
_case("stagger", 32, 32, 6, 24, _um(32, 32, 24, 100, 909), 4, 2, 3, (3, 24), seed=99, kind="stagger")

# LSQR at tol 1e-4 against the oracle: 1e-10 on x wherever the oracle's own x moves by <= 1e-12 under five one-ulp perturbations of (y, z) -- the
# rule of mc_ref.lsqr_bound.  A case that moves further enters 3 x its figure here and is held to 30 x the entry (at most a quarter of the cases).
# Measured by tests/test_sms_host.py on this code base: 3.1e-16 .. 6.0e-16 on the generic groups, 4.6e-15 on stagger's long group and 2.8e-14 on
# z4c3masked (exact zeros in the maps), no count moved: no case is entered and every case takes 1e-10.
LSQR_SENS = {}

# The oracle's solve at tol 1e-13, maxit 300 against minimiser_sms, the largest over a case's groups, as tests/test_sms_host.py measures it, with a
# factor 3 of room.  The device's bound is max(1e-7, 100 x entry).
# Measured: 3.1e-14 .. 1.3e-13 in 50 .. 91 iterations; stagger's long group 1.4e-12 in 127.  So 1e-7 on every case.
TIGHT_SENS = {
    "z2c4": 2.3e-13, "z3c3g2": 2.7e-13, "z8c2": 9.2e-14, "z1c4g3": 2.4e-13, "z4c3masked": 1.9e-13, "genE": 3.1e-13, "stride": 3.7e-13,
    "epi64x32": 3.2e-13, "stagger": 4.2e-12,        # (group 2: sum_j |C_j|^2 up to 12 beside r = 0.05)
}
assert sorted(TIGHT_SENS) == sorted(ALL)


def lsqr_bound(name):
    return max(1e-10, 30.0 * LSQR_SENS.get(name, 0.0))


def tight_bound(name):
    return max(1e-7, 100.0 * TIGHT_SENS[name])


def _cn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _generic_group(rng, c, op, maps):
    x = _cn(rng, (c["Z"], c["N"], c["M"], c["s"]))
    y = op.forward_mc(x, maps)
    y = y + 0.01 * _cn(rng, y.shape)
    z = x + 0.1 * _cn(rng, x.shape)
    return x, y, z, op.adjoint_mc(y, maps)


def _stagger_groups(rng, c, op):
    """Group 0 generic; group 1 y = 0, z = x0 = 0 (stops at iteration 0 with x = 0); group 2 strongly unnormalised maps (sum_j |C_j|^2 from 0.02 to
    12), z pure noise and x0 = 0: it runs long."""
    N, M, nc, Z, s = c["N"], c["M"], c["nc"], c["Z"], c["s"]
    maps = [np.stack([MC.maps_smooth(N, M, nc, 0.7 * b) for b in range(Z)]),
            np.stack([MC.maps_smooth(N, M, nc, 0.7 * (Z + b)) for b in range(Z)]),
            np.stack([MC.maps_unnormalised(N, M, nc, 0.7 * (2 * Z + b), 0.02, 12.0) for b in range(Z)])]
    x0_, y0, z0, s0 = _generic_group(rng, c, op, maps[0])
    zero = np.zeros((Z, N, M, s), np.complex128)
    x2 = _cn(rng, zero.shape)
    y2 = op.forward_mc(x2, maps[2])
    y2 = y2 + 0.01 * _cn(rng, y2.shape)
    z2 = _cn(rng, zero.shape)
    return maps, [x0_, zero, x2], [y0, np.zeros_like(y0), y2], [z0, zero, z2], [s0, zero, zero]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The inputs of a case, built once: V, E, the mask, the operator `op`, per group maps [G, Z, N, M, nc], x, z, x0 [G, Z, N, M, s] and y
    [G, m, nc]; for the operator's tests xop [Z, N, M, s] complex, xr real and yn [m, nc].  Read-only."""
    c = CASES[name]
    N, M, s, T, nc, Z, G = c["N"], c["M"], c["s"], c["T"], c["nc"], c["Z"], c["G"]
    rng = np.random.default_rng(c["seed"])
    fp, k = c["mask"]()
    m = int(fp[-1])
    V = np.linalg.qr(rng.standard_normal((T, s)))[0]
    E = {"caipi": lambda: caipi(T, Z), "ones": lambda: np.ones((T, Z), np.complex128), "gauss": lambda: _cn(rng, (T, Z))}[c["E_kind"]]()
    op = SmsOperator(N, M, V, fp, k, E)
    if c["kind"] == "stagger":
        maps, xs, ys, zs, x0s = _stagger_groups(rng, c, op)
    else:
        maps = [np.stack([MC.MAPS[c["maps_kind"]](N, M, nc, 0.7 * (g * Z + b)) for b in range(Z)]) for g in range(G)]
        xs, ys, zs, x0s = zip(*[_generic_group(rng, c, op, maps[g]) for g in range(G)])
    assert len(maps) == G
    out = dict(c, V=V, E=E, fp=fp, k=k, m=m, op=op, maps=np.stack(maps), x=np.stack(xs), y=np.stack(ys), z=np.stack(zs), x0=np.stack(x0s),
               yn=_cn(rng, (m, nc)), xop=_cn(rng, (Z, N, M, s)), xr=rng.standard_normal((Z, N, M, s)))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_lsqr(name, g, tol=1e-4, maxit=100):
    """(x, iters, flag) of the oracle's lsqr_mc on group g of a case at r = R, from the case's x0."""
    c = inputs(name)
    x, it, fl = c["op"].lsqr(c["y"][g], c["maps"][g], c["z"][g], R, tol, maxit, c["x0"][g])
    x.setflags(write=False)
    return x, it, fl


def lsqr_sensitivity(name, g, tol=1e-4, maxit=100, trials=5):
    """How far the oracle's own x moves when every element of group g's (y, z) is perturbed by about one ulp (relative, Gaussian, 2.2e-16; the
    largest relative distance over `trials` perturbations, absolute where x = 0), and the (iterations, flag) of every perturbed run."""
    c = inputs(name)
    xo, _, _ = oracle_lsqr(name, g, tol, maxit)
    rng = np.random.default_rng(c["seed"] + 4242 + g)
    worst, counts = 0.0, []
    for _ in range(trials):
        y = c["y"][g] * (1.0 + 2.2e-16 * rng.standard_normal(c["y"][g].shape))
        z = c["z"][g] * (1.0 + 2.2e-16 * rng.standard_normal(c["z"][g].shape))
        xp, ip, flp = c["op"].lsqr(y, c["maps"][g], z, R, tol, maxit, c["x0"][g])
        worst = max(worst, float(np.linalg.norm(xp - xo) / max(np.linalg.norm(xo), 1e-300)))
        counts.append((ip, flp))
    return worst, counts


@functools.lru_cache(maxsize=None)
def minimisers(name):
    """minimiser_sms of every group of a case at r = R: [G, Z, N, M, s], read-only."""
    c = inputs(name)
    out = np.stack([minimiser_sms(c["op"], c["y"][g], c["maps"][g], c["z"][g], R) for g in range(c["G"])])
    out.setflags(write=False)
    return out


# ---- the separation fixture ---------------------------------------------------------------------------------------------------------------------------
SEP = dict(N=32, M=32, s=3, T=24, per_frame=200, nc=8, Z=2, r=1e-6, tol=1e-10, maxit=400, seed=77)


def _phantom(N, M, s, which):
    """Two different smooth-edged phantoms: a tilted ellipse with a bright disc, and two rectangles; each channel its own weights of the parts."""
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    soft = lambda d: 0.5 * (1.0 - np.tanh(8.0 * d))
    if which == 0:
        parts = [soft(np.sqrt(((hh + 0.3 * ww) / 0.75) ** 2 + (ww / 0.55) ** 2) - 1.0), soft(np.sqrt((hh - 0.25) ** 2 + (ww + 0.1) ** 2) / 0.22 - 1.0)]
        wts = np.array([[1.0, 0.6], [0.5, -0.4], [0.2 + 0.3j, 0.8]])
    else:
        parts = [soft(np.maximum(np.abs(hh + 0.35) / 0.3, np.abs(ww) / 0.7) - 1.0), soft(np.maximum(np.abs(hh - 0.4) / 0.25, np.abs(ww - 0.2) / 0.4) - 1.0)]
        wts = np.array([[0.7, -0.5], [1.0, 0.3j], [-0.3, 0.9]])
    return np.stack([wts[c % 3, 0] * parts[0] + wts[c % 3, 1] * parts[1] for c in range(s)], axis=2).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def separate():
    """The Z = 2 separation set-up: two different phantoms, 32 x 32, s = 3, T = 24, 200 samples per frame, 8 smooth coils, noise-free data under the
    CAIPI cycle (y) and under E = 1 (y_ones: the control, from which coils alone must separate the slices); r = 1e-6, z = x0 = 0, tol 1e-10, maxit 400."""
    c = dict(SEP)
    N, M, s, T, nc, Z = c["N"], c["M"], c["s"], c["T"], c["nc"], c["Z"]
    rng = np.random.default_rng(c["seed"])
    fp, k = GR.user_mask(N, M, T, c["per_frame"], 977)
    V = np.linalg.qr(rng.standard_normal((T, s)))[0]
    maps = np.stack([MC.maps_smooth(N, M, nc, 0.7 * b) for b in range(Z)])
    x = np.stack([_phantom(N, M, s, b) for b in range(Z)])
    E, ones = caipi(T, Z), np.ones((T, Z), np.complex128)
    op, op1 = SmsOperator(N, M, V, fp, k, E), SmsOperator(N, M, V, fp, k, ones)
    out = dict(c, V=V, fp=fp, k=k, m=int(fp[-1]), maps=maps, x=x, E=E, E_ones=ones, op=op, op_ones=op1, y=op.forward_mc(x, maps), y_ones=op1.forward_mc(x, maps),
               zero=np.zeros_like(x))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def separate_oracle(control=False):
    """(x, iters, flag) of the oracle on the fixture (control: the E = 1 data and operator)."""
    f = separate()
    op, y = (f["op_ones"], f["y_ones"]) if control else (f["op"], f["y"])
    x, it, fl = op.lsqr(y, f["maps"], f["zero"], f["r"], f["tol"], f["maxit"], f["zero"])
    x.setflags(write=False)
    return x, it, fl


def slice_errors(x, f):
    """err[b][c] = ||x[b] - phantom c|| / ||phantom c||."""
    return [[float(np.linalg.norm(x[b] - f["x"][c]) / np.linalg.norm(f["x"][c])) for c in range(f["Z"])] for b in range(f["Z"])]
