"""GPU: the trajectory operator, its Toeplitz normal operator (section 16) and its density compensation (section 21) on
every grid side, every kernel width and every channel count the library accepts -- the instantiations the other trajectory tests never reach:
  - the w-pass twins k_nu_adj_w<R1,R2> / k_toep_adj_w<R1,R2> and the h-passes on 4B sub-grid slices at the sides 112, 128, 160, 192 and 256
    (GRIDS: each of those sides once as N and once as M; the last grid pairs the largest h plan with the smallest w plan);
  - k_nu_interp<W>, k_dcf_interp_div<W> and the spreading windows at every width 2 ... 16, the odd ones, 2 and 16 included;
  - the `c < s` guards, the packed triangle of k_toep_mul and the w-pass activity masks at every s = 1 ... 10.

Yardsticks.  The exact non-uniform DFT (nufft_ref.nudft_*) at the bounds tests/test_gpu_nufft.py and tests/test_gpu_toeplitz.py already hold
32^2 ... 224^2 to.  Per width, the numpy restatement of the same gridding NUFFT (nufft_ref.gridded_*; tests/test_nufft_host.py proves it on the
CPU): the library's bound 10^(2-w) cannot tell a wrong window from a right one at w <= 5 and is below what fp64 delivers at w >= 13, but the
library and the restatement compute the SAME approximation -- the same window, kernel values, deapodisation and transform -- so they differ by
summation order alone.  The bound on that difference is max(1e-3 eps_ref(w), 1e-11): eps_ref(w) is the restatement's own error against the exact
NUDFT on the same inputs (a window off by one point moves the result by about eps_ref(w - 1) >> 1e-3 eps_ref(w)), and 1e-11 is 100 x the
adjointness figure 1e-13 these kernels meet: fp64 rounding (1.1e-16) of a sum of w^2 terms after a deapodisation 1 / Phi that amplifies the band
edge by about e^(0.31 w) (150 at w = 16) stays two orders below it."""
import numpy as np
import pytest

import dcf_ref as D
import nufft_ref as R
from conftest import rel_err
from test_gpu_dcf import WEIGHTS_RTOL

pytestmark = pytest.mark.gpu

GRIDS = [(112, 128), (128, 160), (160, 192), (192, 256), (256, 112), (256, 32)]
WIDTH_GRIDS = [(112, 32), (32, 112)]
WIDTHS = list(range(2, 17))
CHANNELS = list(range(1, 11))
_ids = lambda grids: [f"{n}x{m}" for n, m in grids]


def _cx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _traj_case(N, M, T, per, s, seed):                                # (as tests/test_gpu_nufft.py)
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((T, s))
    fp = np.arange(T + 1, dtype=np.int32) * per
    om = rng.uniform(-np.pi, np.pi, (T * per, 2))
    om[:6] = [[np.pi, np.pi], [-np.pi, -np.pi], [0.0, 0.0], [np.pi, -np.pi], [-np.pi, 1e-9], [1e-12, np.pi]]   # the edges of [-pi, pi]
    return rng, V, fp, om


def _maps(N, M, nc):                                                  # (as tests/test_gpu_nufft.py)
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                  for a in np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def _adjointness(Ax, y, Ahy, x):
    return float(abs(np.vdot(y, Ax) - np.vdot(Ahy, x)) / (np.linalg.norm(Ax) * np.linalg.norm(y)))


def _exact_case(N, M, T=2, per=300, s=3):
    """inputs and their exact NUDFT results on one grid (the slow part, on the CPU): built once per grid, shared, never changed."""
    rng, V, fp, om = _traj_case(N, M, T, per, s, seed=N + M)
    x, z, y = _cx(rng, N, M, s), _cx(rng, N, M, s), _cx(rng, om.shape[0])
    ye = R.nudft_forward(x, om, V, fp)
    case = dict(N=N, M=M, s=s, V=V, fp=fp, om=om, x=x, z=z, y=y, ye=ye, xe=R.nudft_adjoint(y, om, V, fp, N, M),
                ne=R.nudft_adjoint(ye, om, V, fp, N, M))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@pytest.fixture(scope="module")
def exact():
    """exact(N, M): the shared read-only case of a grid (T = 2 frames of 300 samples, s = 3)."""
    cache = {}

    def get(N, M):
        if (N, M) not in cache:
            cache[(N, M)] = _exact_case(N, M)
        return cache[(N, M)]
    return get


# ---- a. the operator on every side ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M", GRIDS, ids=_ids(GRIDS))
def test_operator_on_every_side(engine_mod, exact, N, M):
    """Forward and adjoint within 1e-9 of the exact NUDFT and adjoint to 1e-13 at the default width; with 3 coils at max_batch 2 (dense passes on
    8 and then 4 sub-grid slices) adjoint to 1e-13; the adjoint of one data vector carries the same bits at max_batch 1 and 2."""
    c = exact(N, M)
    e = engine_mod.Engine(0)
    try:
        e.set_trajectory(N, M, c["V"], c["fp"], c["om"])
        Ax, Ahy = e.forward(c["x"]), e.adjoint(c["y"])
        errs = (rel_err(Ax, c["ye"]), rel_err(Ahy, c["xe"]))
        gap = _adjointness(Ax, c["y"], Ahy, c["x"])
        e.set_trajectory(N, M, c["V"], c["fp"], c["om"], max_batch=2)
        Ahy2 = e.adjoint(c["y"])
        e.set_coils(_maps(N, M, 3))
        yc = _cx(np.random.default_rng(1), c["om"].shape[0], 3)
        Axc, Ahyc = e.forward_mc(c["x"]), e.adjoint_mc(yc)
        gapc = _adjointness(Axc, yc, Ahyc, c["x"])
    finally:
        e.close()
    print(f"{N} x {M}: forward / adjoint against the exact NUDFT {errs[0]:.3e} / {errs[1]:.3e}, adjointness {gap:.3e}, 3 coils {gapc:.3e}")
    assert max(errs) <= 1e-9, errs
    assert gap <= 1e-13, gap
    assert gapc <= 1e-13, gapc
    assert np.array_equal(Ahy2, Ahy)


# ---- b. the normal operator on every side --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M", GRIDS, ids=_ids(GRIDS))
def test_normal_operator_on_every_side(engine_mod, exact, N, M):
    """normal(x) within 2e-9 of the exact A^H A x and of the device's own adjoint(forward(x)) (the bounds of
    test_gpu_toeplitz.test_apply_accuracy_against_the_exact_nudft); Hermitian to 1e-12 ||x|| ||z||."""
    c = exact(N, M)
    e = engine_mod.Engine(0)
    try:
        e.set_trajectory(N, M, c["V"], c["fp"], c["om"])
        Tx, Tz = e.normal(c["x"]), e.normal(c["z"])
        pair = e.adjoint(e.forward(c["x"]))
    finally:
        e.close()
    errs = (rel_err(Tx, c["ne"]), rel_err(Tx, pair))
    herm = float(abs(np.vdot(c["z"], Tx) - np.vdot(Tz, c["x"])) / (np.linalg.norm(c["x"]) * np.linalg.norm(c["z"])))
    print(f"{N} x {M}: normal against the exact A^H A x {errs[0]:.3e}, against the device pair {errs[1]:.3e}, Hermitian gap {herm:.3e}")
    assert max(errs) <= 2e-9, errs
    assert herm <= 1e-12, herm


def test_toeplitz_xupdate_against_the_lsqr_route(engine_mod, exact):
    """One x-update on 128 x 160 at tol 1e-10: Toeplitz CG and LSQR agree to 1e-6, or within twice the LSQR route's own gap to the LSQR on the exact
    NUDFT (the tolerance of test_gpu_toeplitz.test_loop_against_the_lsqr_route; that gap is only computed if the first bound is missed)."""
    N, M = 128, 160
    c = exact(N, M)
    r = 0.05
    e = engine_mod.Engine(0)
    try:
        e.set_trajectory(N, M, c["V"], c["fp"], c["om"])
        xl, il, fl = e.xupdate(c["y"], c["z"], r, tol=1e-10, maxit=300)
        xt, it, ft = e.xupdate(c["y"], c["z"], r, tol=1e-10, maxit=300, solver="toeplitz")
    finally:
        e.close()
    gap = rel_err(xt, xl)
    floor = 0.0
    if gap > 1e-6:
        op = R.NudftOperator(N, M, c["V"], c["fp"], c["om"])
        xo, _, _ = op.lsqr_mc(np.asarray(c["y"])[:, None], np.ones((N, M, 1), np.complex128), np.asarray(c["z"]), r, tol=1e-10, maxit=300)
        floor = rel_err(xl, xo)
    print(f"toeplitz against lsqr: {gap:.3e} (iterations {it} / {il}, flags {ft} / {fl}), lsqr against the exact route: {floor:.3e}")
    assert gap <= 1e-6 or gap <= 2 * floor, (gap, floor)


# ---- c. every kernel width ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M", WIDTH_GRIDS, ids=_ids(WIDTH_GRIDS))
@pytest.mark.parametrize("width", WIDTHS)
def test_every_width_against_the_restatement(engine_mod, exact, N, M, width):
    """Per width: adjoint to 1e-13; forward and adjoint within max(1e-3 eps_ref(w), 1e-11) of the restatement at the same width (header);
    within max(10^(2-w), 10 eps_ref(w)) of the exact NUDFT; normal(x) within twice that of the exact A^H A x."""
    c = exact(N, M)
    yr = R.gridded_forward(c["x"], c["om"], c["V"], c["fp"], width)
    xr = R.gridded_adjoint(c["y"], c["om"], c["V"], c["fp"], N, M, width)
    eps = (rel_err(yr, c["ye"]), rel_err(xr, c["xe"]))                 # eps_ref(w): the restatement's own error, forward and adjoint
    e = engine_mod.Engine(0)
    try:
        e.set_trajectory(N, M, c["V"], c["fp"], c["om"], width=width)
        Ax, Ahy = e.forward(c["x"]), e.adjoint(c["y"])
        Tx = e.normal(c["x"])
    finally:
        e.close()
    gap = _adjointness(Ax, c["y"], Ahy, c["x"])
    diff = (rel_err(Ax, yr), rel_err(Ahy, xr))
    err = (rel_err(Ax, c["ye"]), rel_err(Ahy, c["xe"]))
    nerr = rel_err(Tx, c["ne"])
    print(f"{N} x {M} width {width}: eps_ref {eps[0]:.3e} / {eps[1]:.3e}, device against the restatement {diff[0]:.3e} / {diff[1]:.3e}, "
          f"against the exact NUDFT {err[0]:.3e} / {err[1]:.3e}, normal {nerr:.3e}, adjointness {gap:.3e}")
    assert gap <= 1e-13, gap
    for k in range(2):
        assert diff[k] <= max(1e-3 * eps[k], 1e-11), (k, diff[k], eps[k])
        assert err[k] <= max(10.0 ** (2 - width), 10 * eps[k]), (k, err[k], eps[k])
    assert nerr <= 2 * max(10.0 ** (2 - width), 10 * max(eps)), (nerr, eps)


@pytest.fixture(scope="module")
def spiral32():
    N, S, T = 32, 60, 48
    fp, om = R.spiral_traj(N, S, T)
    om.setflags(write=False)
    return N, T, fp, om


@pytest.mark.parametrize("width", WIDTHS)
def test_density_weights_at_every_width(engine_mod, spiral32, width):
    N, T, fp, om = spiral32
    plan = D.Plan(N, N, om, width)
    wr, it, dev, _ = D.iterate(plan, 5)
    assert np.all(np.isfinite(wr)) and np.all(wr > 0)
    e = engine_mod.Engine(0)
    try:
        e.set_trajectory(N, N, np.full((T, 1), 1 / np.sqrt(T)), fp, om, width=width)
        w, info = e.density_weights(niter=5)
    finally:
        e.close()
    err = float(np.max(np.abs(w - D.kappa(T, width, plan.beta) * wr) / np.abs(D.kappa(T, width, plan.beta) * wr)))
    print(f"width {width}: weights against the reference, max relative difference {err:.3e}, dev {info['dev']:.6e} (reference {dev:.6e})")
    assert w.shape == (om.shape[0],) and np.all(np.isfinite(w)) and np.all(w > 0)
    assert info["iters"] == it == 5 and info["clamped"] == 0
    assert abs(info["dev"] - dev) <= 1e-10 * dev
    assert err <= WEIGHTS_RTOL, err


# ---- d. every channel count ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", CHANNELS)
def test_every_channel_count(engine_mod, s):
    """112 x 128, default width, 2 frames of 200 samples: forward and adjoint within 1e-9 of the exact NUDFT, normal within 2e-9, adjoint to
    1e-13, and adjoint(y, weighted=True) the bits of adjoint(w .* y) (the fused multiply forms (w yr, w yi): tests/test_gpu_dcf.py)."""
    N, M = 112, 128
    rng, V, fp, om = _traj_case(N, M, 2, 200, s, seed=100 + s)
    x, y = _cx(rng, N, M, s), _cx(rng, om.shape[0])
    wq = rng.uniform(0.5, 2.0, om.shape[0])
    ye, xe = R.nudft_forward(x, om, V, fp), R.nudft_adjoint(y, om, V, fp, N, M)
    ne = R.nudft_adjoint(ye, om, V, fp, N, M)
    e = engine_mod.Engine(0)
    try:
        e.set_trajectory(N, M, V, fp, om)
        Ax, Ahy, Tx = e.forward(x), e.adjoint(y), e.normal(x)
        e.set_sample_weights(wq)
        xw = e.adjoint(y, weighted=True)
        xwy = e.adjoint(wq * y.real + 1j * (wq * y.imag))
    finally:
        e.close()
    errs = (rel_err(Ax, ye), rel_err(Ahy, xe), rel_err(Tx, ne))
    gap = _adjointness(Ax, y, Ahy, x)
    print(f"s = {s}: forward / adjoint / normal against the exact NUDFT {errs[0]:.3e} / {errs[1]:.3e} / {errs[2]:.3e}, adjointness {gap:.3e}")
    assert Ahy.shape == (N, M, s)
    assert max(errs[:2]) <= 1e-9, errs
    assert errs[2] <= 2e-9, errs
    assert gap <= 1e-13, gap
    assert np.array_equal(xw, xwy)


# ---- e. density compensation on large grids and split tiles ---------------------------------------------------------------------------

def _dcf_against_the_reference(engine_mod, N, M, S, T, width, niter=5):
    fp, om = R.spiral_traj(N, S, T)                                    # (omega in radians per pixel: the same spiral on a rectangular grid)
    plan = D.Plan(N, M, om, width)
    wr, it, dev, _ = D.iterate(plan, niter)
    ref = D.kappa(T, plan.width, plan.beta) * wr
    e = engine_mod.Engine(0)
    try:
        e.set_trajectory(N, M, np.full((T, 1), 1 / np.sqrt(T)), fp, om, width=width)
        w, info = e.density_weights(niter=niter)
    finally:
        e.close()
    err = float(np.max(np.abs(w - ref) / np.abs(ref)))
    print(f"{N} x {M} S {S} T {T} width {plan.width}: max relative difference {err:.3e}, dev {info['dev']:.6e} (reference {dev:.6e}), "
          f"split tiles {info['split_tiles']}")
    assert w.shape == (S * T,) and np.all(np.isfinite(w)) and np.all(w > 0)
    assert info["iters"] == it == niter and info["clamped"] == 0
    assert abs(info["dev"] - dev) <= 1e-10 * dev
    assert err <= WEIGHTS_RTOL, err
    return info


@pytest.mark.parametrize("N,M", [(160, 192), (256, 112)], ids=["160x192", "256x112"])
def test_density_weights_on_large_grids(engine_mod, N, M):
    _dcf_against_the_reference(engine_mod, N, M, 100, 24, 0)


def test_density_weights_split_tiles_on_new_sides(engine_mod):
    """112 x 128, width 6, T = 48: at S = 300 the spreading lists of the tiles at the centre of k-space exceed one segment of 512 samples (the
    longest holds about 3 300; S = 200 is the first round figure at which the plan splits any), so the weights go through the partial tiles and
    k_dcf_reduce."""
    info = _dcf_against_the_reference(engine_mod, 112, 128, 300, 48, 6)
    assert info["split_tiles"] > 0
