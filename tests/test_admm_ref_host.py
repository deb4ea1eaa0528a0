"""CPU: tests/admm_ref.py, the numpy restatement of the PnP-ADMM loop that tests/test_gpu_admm_glue.py holds the kernels to, held to two independent
statements of the same loop -- the CPU oracle's orc_admm.c (real TSMIs) and tests/complex_admm_ref.py (complex TSMIs) -- on the same routing
weights, with the network keeping fp32 values (roundtrip = identity: the oracle's network is plain fp32); the premise that makes the reference
network exact; and the measured table ADMM_SENS the device's bounds are derived from."""
import numpy as np
import pytest

import admm_ref as A
import complex_admm_ref as CA
import conv_ref as CR
import gridded_ref as GR
from conftest import rel_err

NETS = sorted({(r["grid"], r["mode"][0], r["mode"][1]) for r in A.RUNS.values()})


@pytest.mark.parametrize("grid,cpx,multi", NETS)
def test_routing_network_premise(grid, cpx, multi):
    """Every case's weights: one weight from {1, -1, 0.5} per output channel; multi-level: some output reads the noise plane; complex: every output
    of the real half reads the imaginary half and the other way round (but the one that reads the noise plane); every input plane is read,
    multi-level all but one image plane (in_nc = out_nc + 1); most taps are off centre.  And conv_ref.conv3x3 of a tensor with these weights is the
    routed, scaled and shifted tensor bit for bit -- with the split's round trip of the values as with the values themselves."""
    run = dict(grid=grid, mode=(cpx, multi, 0))
    routes, w, in_nc, out_nc = A.net_of(run)
    c = GR.CASES[grid]
    s, N, M = c["s"], c["N"], c["M"]
    assert (in_nc, out_nc) == A.channels(s, cpx, multi) and w.shape == (out_nc, in_nc, 3, 3)
    assert all(np.count_nonzero(w[o]) == 1 and w[o][w[o] != 0][0] in (1.0, -1.0, 0.5) for o in range(out_nc))
    read = {r[0] for r in routes}
    assert len(read) == out_nc and (not multi or in_nc - 1 in read)
    if cpx:
        assert all(s <= routes[o][0] < 2 * s for o in range(s))
        assert all(routes[o][0] < s or routes[o][0] == 2 * s for o in range(s, 2 * s))
        assert multi or any(routes[o][0] < s for o in range(s, 2 * s))
    off = sum((kh, kw) != (1, 1) for _, kh, kw, _ in routes)
    assert off >= max(1, out_nc - -(-out_nc // 9))
    rng = np.random.default_rng(c["seed"])
    x = rng.random((N, M, in_nc), dtype=np.float32)
    x[0, 0, :], x[-1, -1, :], x[0, -1, :] = 0.0, 1.0, np.float32(2.0 ** -15 * 1.37)
    for rt in (None, CR.split_roundtrip):
        want = CR.conv3x3(x.astype(np.float64) if rt is None else rt(x), w)
        got = A.route(x, routes, rt)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    if grid == A.MODE_GRID:                                          # (the planes really move: a shifted plane differs from the plane itself)
        assert not np.array_equal(A.route(x, routes)[:, :, 0], routes[0][3] * x[:, :, routes[0][0]])


class _OracleNet:
    """complex_admm_ref calls net.denoise(V): the oracle's network with this run's residual_noise"""

    def __init__(self, net, residual):
        self.net, self.residual = net, residual

    def denoise(self, V):
        return self.net.denoise(V, residual_noise=self.residual)


@pytest.mark.parametrize("solver", ["lsqr", "direct"])
@pytest.mark.parametrize("mode", A.MODES, ids=A.mode_id)
def test_against_the_other_statements_of_the_loop(oracle, mode, solver):
    """admm_ref against orc_admm.c (real modes) and complex_admm_ref (complex modes) after three iterations, x and both diagnostic columns.  With the
    LSQR x-update all three call the same oracle LSQR, so only the glue differs: 1e-12.  With DIRECT the x-updates differ too (the numpy
    minimiser against the oracle's), by rounding: the run's bound."""
    key = A.run_key(A.MODE_GRID, mode, solver=solver, rt="id" if solver == "lsqr" else "f16")
    cpx, multi, res = mode
    if solver == "direct":                                           # (no 'id' run of DIRECT in the table: make it here)
        run = dict(A.RUNS[key], rt="id")
        xr, dr, lr = A._loop(A.problem(run))
    else:
        run = A.RUNS[key]
        xr, dr, lr = A.reference(key)
    p = A.problem(run)
    c = p["c"]
    op = GR.oracle_operator(A.MODE_GRID)
    net = oracle.Net(p["w"].ravel(), in_nc=p["in_nc"], out_nc=p["out_nc"], nc=(p["out_nc"], 0, 0, 0), nb=1, arch=1)
    kw = dict(gamma=A.GAMMA, iters=A.ITERS, cg_tol=A.TOL, cg_maxit=A.MAXIT, solver=solver, multi_level=bool(multi), noise_std=A.NOISE_STD, gt=p["gt"],
              want_diag=True)
    if cpx:
        xo, do, lo = CA.pnp_admm(op, _OracleNet(net, bool(res)), p["y"], tsmi_domain="complex", **kw)
    else:
        xo, do, lo = oracle.pnp_admm(op, net, p["y"], residual_noise=bool(res), **kw)
    ex, ed = rel_err(xr, xo), float(np.abs(dr / do - 1.0).max())
    tol = 1e-12 if solver == "lsqr" else A.bound(key)
    print(f"{key}: x {ex:.2e} diagnostics {ed:.2e} (bound {tol:.1e}), inner iterations {lr.tolist()} / {np.asarray(lo).tolist()}")
    assert np.array_equal(lr, np.asarray(lo).ravel()[:A.ITERS])
    assert ex < tol and ed < tol


@pytest.mark.parametrize("key", list(A.RUNS))
def test_sensitivity_table(oracle, key):
    """ADMM_SENS from above, with a factor 2 of room; no x-update of a perturbed run changes its inner iteration count (a run on a stop-rule
    boundary gets another seed, not a looser assertion); the derived bound is at or below 1e-6."""
    mx, md, same = A.loop_sensitivity(key)
    print(f"{key}: x moves by {mx:.2e}, the diagnostics by {md:.2e} (recorded {A.ADMM_SENS[key]:.1e}, device bound {A.bound(key):.1e}); inner iterations "
          f"{A.reference(key)[2].tolist()}")
    assert same
    assert max(mx, md) <= 2.0 * A.ADMM_SENS[key]
    assert A.bound(key) <= 1e-6


def test_table_covers_every_run():
    assert sorted(A.ADMM_SENS) == sorted(A.RUNS)
    assert all(np.isfinite(v) and v > 0 for v in A.ADMM_SENS.values())
