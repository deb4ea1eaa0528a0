"""GPU: the gridded operator (dc_kernels.hip), its k-space LSQR (kslsqr_kernels.hip) and the DIRECT solver on every case of tests/gridded_ref.py --
every supported side as the h axis and as the w axis, s = 1 .. 10, T s on both sides of DC_VCAP (V in LDS or in memory), and the masks that reach
every unit shape and planner branch (pinned on the CPU by tests/test_op_plan_host.py) -- against two yardsticks: the numpy restatement
gridded_ref (written from the reference's definitions) and the CPU oracle, which tests/test_gridded_ref_host.py holds to each other on the same
inputs.  One Engine for the whole file: every case plans a new operator on the live context, after operators of other sizes and shapes.

Bounds: forward / adjoint / adjointness 1e-12 (the figure tests/test_gpu_grids.py holds against the oracle; the yardsticks agree to 1e-15);
LSQR at tol 1e-4: the oracle's (iterations, flag), which the host test shows not to sit on a stop-rule boundary, and x to 1e-10 -- except on the
eight masks of gridded_ref.LSQR_SENS, where the iteration itself is ill conditioned (the ORACLE's x moves by 1e-10 .. 4e-8 under a one-ulp change
of its inputs; measured on the host) and the bound is derived from that figure (gridded_ref.lsqr_bound: 8e-9 .. 4e-6; the device was at
1.6e-10 .. 6.4e-8).  LSQR at tol 1e-13 and DIRECT at r = 0.05 against the exact minimiser: 1e-7 and 1e-10 (tests/test_gpu_operator.py's figures)
on every case; DIRECT at r = 1e-3: gridded_ref.direct_bound_small_r, from the oracle's own distance to the minimiser.

Measured on the MI355X: 143 tests in 4.8 s (6.1 s wall with the interpreter's start), the slowest case 0.4 s."""
import numpy as np
import pytest

import gridded_ref as GR
from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(engine_mod, oracle):
    e = engine_mod.Engine(0)
    yield e
    e.close()


def _plan(e, c):
    e.set_operator(c["N"], c["M"], c["V"], c["fp"], c["k"])
    assert (e.N, e.M, e.s, e.m) == (c["N"], c["M"], c["s"], c["m"])


@pytest.mark.parametrize("name", GR.ALL)
def test_operator(eng, name):
    """forward and adjoint against the restatement, adjointness, and real input = complex input with a zero imaginary part."""
    c = GR.inputs(name)
    _plan(eng, c)
    V, fp, k = c["V"], c["fp"], c["k"]
    yg, xg = eng.forward(c["x"]), eng.adjoint(c["yn"])
    ef, ea = rel_err(yg, GR.forward(c["x"], V, fp, k)), rel_err(xg, GR.adjoint(c["yn"], V, fp, k, c["N"], c["M"]))
    lhs, rhs = np.vdot(c["yn"], yg), np.vdot(xg, c["x"])
    print(f"{name}: forward {ef:.2e} adjoint {ea:.2e} adjointness {abs(lhs - rhs) / abs(lhs):.2e}")
    assert ef < 1e-12 and ea < 1e-12
    assert abs(lhs - rhs) / abs(lhs) < 1e-12
    yr = eng.forward(c["xr"])
    assert rel_err(yr, GR.forward(c["xr"], V, fp, k)) < 1e-12
    assert np.array_equal(yr, eng.forward(c["xr"] + 0j))


@pytest.mark.parametrize("name", GR.ALL)
def test_lsqr_xupdate(eng, name):
    """tol 1e-4: the oracle's count and flag, x to gridded_ref.lsqr_bound (1e-10 wherever the iteration is well conditioned) -- for s = 10 with all
    iterations in one launch (where the plan allows it) and with two launches per iteration: identical bits, and no time-out of the one-launch
    kernel.  tol 1e-13: the exact minimiser to 1e-7."""
    c = GR.inputs(name)
    _plan(eng, c)
    y, z, x0 = c["y"], c["z"], c["x0"]
    xo, io, flo = GR.oracle_lsqr(name)
    xg, ig, flg = eng.xupdate(y, z, GR.R, 1e-4, 100, x0, solver="lsqr")
    xt, _, flt = eng.xupdate(y, z, GR.R, 1e-13, 300, x0, solver="lsqr")
    et = rel_err(xt, GR.minimisers(name)[GR.R])
    print(f"{name}: gpu ({ig}, {flg}) oracle ({io}, {flo}) x {rel_err(xg, xo):.2e} (bound {GR.lsqr_bound(name):.1e}); tol 1e-13 against the minimiser {et:.2e}")
    assert (ig, flg) == (io, flo)
    assert rel_err(xg, xo) < GR.lsqr_bound(name)
    assert flt == 0 and et < 1e-7
    if c["s"] == 10:
        try:
            eng.lsqr_persist(True)
            xa, ia, fla = eng.xupdate(y, z, GR.R, 1e-4, 100, x0, solver="lsqr")
            eng.lsqr_persist(False)
            xb, ib, flb = eng.xupdate(y, z, GR.R, 1e-4, 100, x0, solver="lsqr")
        finally:
            eng.lsqr_persist(True)
        assert (ia, fla) == (ib, flb) == (io, flo) and np.array_equal(xa, xb) and np.array_equal(xa, xg), (ia, ib, rel_err(xa, xb))
    assert eng.health()["lsqr_one_launch_timeouts"] == 0


@pytest.mark.parametrize("name", GR.ALL)
def test_direct_xupdate(eng, name):
    """DIRECT against the exact minimiser.  On the r-sweep cases: r = 0.05, 1e-3 and 0.05 again on one operator (the inverse tables are cached per r),
    then another mask on the same grid with the same V (the tables belong to the operator: a stale one fails here)."""
    c = GR.inputs(name)
    _plan(eng, c)
    y, z, xm = c["y"], c["z"], GR.minimisers(name)
    e1 = rel_err(eng.xupdate(y, z, GR.R, solver="direct")[0], xm[GR.R])
    print(f"{name}: direct {e1:.2e}")
    assert e1 < 1e-10
    if not c["sweep"]:
        return
    e2 = rel_err(eng.xupdate(y, z, GR.R_SMALL, solver="direct")[0], xm[GR.R_SMALL])
    e3 = rel_err(eng.xupdate(y, z, GR.R, solver="direct")[0], xm[GR.R])
    print(f"{name}: direct at r = {GR.R_SMALL:g}: {e2:.2e} (bound {GR.direct_bound_small_r(name):.1e}), at r = {GR.R:g} again: {e3:.2e}")
    assert e2 < GR.direct_bound_small_r(name)
    assert e3 < 1e-10
    N, M, T, V = c["N"], c["M"], c["T"], c["V"]
    fp2, k2 = GR.user_mask(N, M, T, N * M // 32, c["seed"] + 991)
    rng = np.random.default_rng(c["seed"] + 992)
    y2 = rng.standard_normal(int(fp2[-1])) + 1j * rng.standard_normal(int(fp2[-1]))
    eng.set_operator(N, M, V, fp2, k2)
    e4 = rel_err(eng.xupdate(y2, z, GR.R, solver="direct")[0], GR.minimiser(y2, z, GR.R, V, fp2, k2))
    print(f"{name}: direct on another mask {e4:.2e}")
    assert e4 < 1e-10


@pytest.mark.parametrize("name", ["chan6", "chan10"])
def test_lsqr_prediction_chunking(eng, name):
    """The two-launch form launches the predicted number of iterations, then two more at a time, running the final kernels again each time
    (qmri_lsqr_run).  A solve from the exact minimiser stops at once and makes the prediction small; the next solve, at tol 1e-10 from 0, goes
    through that loop many times and must still give the oracle's count, flag and x."""
    c = GR.inputs(name)
    xm = GR.minimisers(name)[GR.R]
    xo, io, flo = GR.oracle_lsqr(name, 1e-10, 100, True)
    try:
        eng.lsqr_persist(False)
        _plan(eng, c)
        x1, i1, fl1 = eng.xupdate(c["y"], c["z"], GR.R, 1e-4, 100, xm, solver="lsqr")
        assert i1 <= 1 and fl1 == 0 and rel_err(x1, xm) < 1e-9
        x2, i2, fl2 = eng.xupdate(c["y"], c["z"], GR.R, 1e-10, 100, None, solver="lsqr")
    finally:
        eng.lsqr_persist(True)
    print(f"{name}: first solve {i1}, second gpu ({i2}, {fl2}) oracle ({io}, {flo}) x {rel_err(x2, xo):.2e}")
    assert io > 3 and (i2, fl2) == (io, flo)
    assert rel_err(x2, xo) < 1e-10
