"""CPU: the oracle's gridded operator, DIRECT and LSQR x-update against the numpy restatement tests/gridded_ref.py, on every case of the gridded
sweep (rectangular grids with every side on either axis, s = 1 .. 10, T s on both sides of DC_VCAP, the masks that reach every unit shape), and
the two conditions tests/test_gpu_gridded_sweep.py relies on: the oracle's iteration count does not sit on a stop-rule boundary, and the iteration
really runs.  Bounds: forward / adjoint 1e-13, DIRECT 1e-11, LSQR at tol 1e-13 against the exact minimiser 1e-10 -- what tests/test_oracle_operator.py
holds the oracle to at 224 x 224."""
import numpy as np
import pytest

import gridded_ref as GR
from conftest import rel_err


def test_mask_builders_equal_the_oracles(oracle):
    """The restated spiral and EPI builders give the oracle's masks on the sweep's cases and on a rectangular EPI grid."""
    for N, S, T in ((32, 57, 9), (32, 400, 24), (64, 200, 48)):
        fo, ko = oracle.spiral_mask(N, S, T)
        fr, kr = GR.spiral_mask(N, S, T)
        assert np.array_equal(fo, fr) and np.array_equal(ko, kr), (N, S, T)
    for N, M, pct, T in ((160, 160, 0.2, 9), (128, 128, 0.2, 30), (96, 32, 1 / 8, 100)):
        fo, ko = oracle.epi_mask(N, M, pct, T)
        fr, kr = GR.epi_mask(N, M, pct, T)
        assert np.array_equal(fo, fr) and np.array_equal(ko, kr), (N, M, pct, T)


def test_case_tables_hold_what_the_sweep_is_for():
    """The structural properties the cases were chosen for (read off the masks, not off the planner)."""
    assert len(GR.GRIDS) == 18 and len(GR.CHANNELS) == 10 and len(GR.VCAP_CASES) == 7 and len(GR.MASKS) == 12
    assert {GR.CASES[n]["M"] for n in GR.GRIDS} == set(GR.SIDES) == {GR.CASES[n]["N"] for n in GR.GRIDS}
    assert sorted(GR.CASES[n]["T"] * GR.CASES[n]["s"] for n in GR.VCAP_CASES) == [2040, 2048, 2048, 2049, 2050, 2056, 2100]
    for n in GR.ALL:
        c = GR.inputs(n)
        fp, k = c["fp"], c["k"]
        assert fp[0] == 0 and fp.size == c["T"] + 1 and np.all(np.diff(fp) >= 0) and k.size == fp[-1] and k.min() >= 0 and k.max() < c["N"] * c["M"]
        for t in range(c["T"]):
            assert np.all(np.diff(k[fp[t]:fp[t + 1]]) > 0), (n, t)                     # distinct and ascending inside a frame
        if c["v"] != "random":
            assert c["T"] >= c["s"]
    per_k = lambda n: np.bincount(GR.inputs(n)["k"], minlength=GR.CASES[n]["N"] * GR.CASES[n]["M"])
    assert per_k("busy32_T300")[0] == 300 and per_k("busy32_T1100")[0] == 1100 and per_k("full32_T300").min() == 300
    cnt = per_k("full32_T8")
    assert cnt.sum() / np.count_nonzero(cnt) == 8.0
    cnt = per_k("full32_T8_last1023")
    assert np.count_nonzero(cnt) == 1024 and 7.99 < cnt.sum() / 1024 < 8.0
    c = GR.inputs("empty_rows_frames32")
    assert np.any(np.diff(c["fp"]) == 0) and np.unique(c["k"] % 32).size < 32 and 0 not in c["k"] % 32
    c = GR.inputs("busy_row32_T20")
    assert np.count_nonzero(c["k"] % 32 == 5) == 640 > 512                               # DC_CH = 512: two chunks in k_adj_w
    assert GR.inputs("single_sample32")["m"] == 1
    for n in GR.VCAP_CASES:                                                              # every shape of s != 10 holds at most 1024 samples of one k
        assert per_k(n).max() <= 1024


@pytest.mark.parametrize("name", GR.ALL)
def test_oracle_agrees_with_the_restatement(oracle, name):
    c = GR.inputs(name)
    V, fp, k, N, M = c["V"], c["fp"], c["k"], c["N"], c["M"]
    op = GR.oracle_operator(name)
    assert op.m == c["m"]
    ef = rel_err(op.forward(c["x"]), GR.forward(c["x"], V, fp, k))
    ea = rel_err(op.adjoint(c["yn"]), GR.adjoint(c["yn"], V, fp, k, N, M))
    xm = GR.minimisers(name)
    ed = rel_err(op.direct(c["y"], c["z"], GR.R), xm[GR.R])
    xt, itt, flt, _ = op.lsqr(c["y"], c["z"], GR.R, 1e-13, 300, c["x0"])
    et = rel_err(xt, xm[GR.R])
    print(f"{name}: forward {ef:.2e} adjoint {ea:.2e} direct {ed:.2e} tight lsqr {et:.2e} ({itt} iterations, flag {flt})")
    assert ef < 1e-13 and ea < 1e-13
    assert ed < 1e-11
    assert et < 1e-10
    # the minimiser is one: the gradient A^H (A x - y) + r (x - z) vanishes (checks the restatement against itself, through forward / adjoint)
    g = GR.adjoint(GR.forward(xm[GR.R], V, fp, k) - c["y"], V, fp, k, N, M) + GR.R * (xm[GR.R] - c["z"])
    assert np.linalg.norm(g) < 1e-11 * (np.linalg.norm(GR.adjoint(c["y"], V, fp, k, N, M)) + GR.R * np.linalg.norm(c["z"]))
    if c["sweep"]:
        es = rel_err(op.direct(c["y"], c["z"], GR.R_SMALL), xm[GR.R_SMALL])
        print(f"{name}: direct at r = {GR.R_SMALL:g}: {es:.2e} (recorded {GR.DIRECT_SENS[name]:.1e})")
        assert es <= GR.DIRECT_SENS[name]


def _stable(name, tol, maxit, zero_start):
    c = GR.inputs(name)
    op = GR.oracle_operator(name)
    _, it, fl = GR.oracle_lsqr(name, tol, maxit, zero_start)
    x0 = None if zero_start else c["x0"]
    for f in (1.0 - 1e-3, 1.0 + 1e-3):
        _, it2, fl2, _ = op.lsqr(c["y"], c["z"], GR.R, tol * f, maxit, x0)
        assert (it2, fl2) == (it, fl), (name, tol, f, it, it2, fl, fl2)
    return it, fl


@pytest.mark.parametrize("name", GR.ALL)
def test_oracle_count_is_stable_and_the_iteration_runs(oracle, name):
    """What the GPU test compares the kernels' (iterations, flag) with does not depend on the last bits: the oracle's count at tol 1e-4 is the same at
    tol (1 +- 1e-3).  And the count is at least 5, so that the iteration kernels run (single_sample32 excepted: one equation, one step)."""
    it, fl = _stable(name, 1e-4, 100, False)
    print(f"{name}: {it} iterations, flag {fl}")
    assert fl == 0
    if GR.CASES[name]["few_iters"]:
        assert name == "single_sample32"
    else:
        assert it >= 5, (name, it)


@pytest.mark.parametrize("name", GR.ALL)
def test_oracle_lsqr_sensitivity_is_what_the_device_bound_assumes(oracle, name):
    """The oracle's x at tol 1e-4 under one-ulp perturbations of y and z: <= 1e-12 wherever the device is held to the project's 1e-10, and <= the
    recorded figure on the ill-conditioned cases of gridded_ref.LSQR_SENS; the count and the flag do not move."""
    worst, same = GR.lsqr_sensitivity(name)
    print(f"{name}: x moves by {worst:.2e} (recorded {GR.LSQR_SENS.get(name, 1e-12):.1e}, device bound {GR.lsqr_bound(name):.1e})")
    assert same
    assert worst <= GR.LSQR_SENS.get(name, 1e-12)


@pytest.mark.parametrize("name", ["chan6", "chan10"])
def test_oracle_count_of_the_long_solve_is_stable(oracle, name):
    """The prediction-chunking test solves at tol 1e-10 from x0 = 0: that count is stable too, and long enough for several chunks of two."""
    it, fl = _stable(name, 1e-10, 100, True)
    assert fl == 0 and it >= 8, (name, it, fl)
