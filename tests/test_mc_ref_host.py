"""CPU: the oracle's multi-coil operator and x-update (Operator.forward_mc / adjoint_mc / lsqr_mc) against the numpy restatement tests/mc_ref.py, on
every case of the multi-coil sweep (coil counts and chunkings, the strides of the streaming kernels, masks, kinds of maps, staggered stops), and the
conditions tests/test_gpu_mc_sweep.py relies on: the oracle's (iterations, flag) does not sit on a stop-rule boundary, its x does not move under
one-ulp perturbations, the tables of mc_ref bound what they say from above, the staggered case really staggers, the flag-3 case really stagnates.

Measured: forward_mc / adjoint_mc agree to 6.6e-16 .. 1.2e-15 (bound 1e-13; the single-coil yardsticks agree to 1e-15), mc_ref's adjointness
<= 5.9e-15, normal_mc against adjoint_mc(forward_mc) <= 3.2e-16, minimiser_mc's residual <= 4.9e-14 and 3.4e-14 from gridded_ref.minimiser with one
unit coil, the oracle's x at tol 1e-4 moves by <= 7.2e-16 under the perturbations with no count changing, tol 1e-13 against minimiser_mc 2.8e-16 ..
1.1e-13 (1.7e-12 on the staggered case's ill-conditioned slice).  The whole file takes about 45 s, 8 s of it the perturbed solves of stride128x64."""
import numpy as np
import pytest

import gridded_ref as GR
import mc_ref as MR
from conftest import rel_err


def _chunks(nc, S, mb):
    """(g0, cnt) of every chunk of max_batch = mb consecutive coil images g = b nc + j (the definition in mc_kernels.hip's header)."""
    return [(g0, min(mb, nc * S - g0)) for g0 in range(0, nc * S, mb)]


def _slices_touched(nc, g0, cnt):
    return len({g // nc for g in range(g0, g0 + cnt)})


def test_case_table_holds_what_the_sweep_is_for():
    """The structural properties the cases were chosen for, read off the table and the inputs (not off the kernels)."""
    C = MR.CASES
    assert [(C[n]["nc"], C[n]["S"], set(C[n]["max_batch"])) for n in MR.COILS] == [
        (1, 5, {1, 3, 8}), (2, 5, {8}), (3, 3, {8, 2}), (4, 3, {4, 3}), (5, 3, {2, 4, 7}), (8, 2, {3, 8, 16}), (13, 1, {4})]
    for n in MR.COILS:
        assert (C[n]["N"], C[n]["M"], C[n]["s"], C[n]["T"]) == (32, 32, 6, 24) and C[n]["maps_kind"] == "smooth"
        assert np.all(np.diff(MR.inputs(n)["fp"]) == 100)
    ch = lambda n, mb: _chunks(C[n]["nc"], C[n]["S"], mb)
    touched = lambda n, mb: [_slices_touched(C[n]["nc"], g0, cnt) for g0, cnt in ch(n, mb)]
    midstart = lambda n, mb: [g0 % C[n]["nc"] for g0, _ in ch(n, mb)]
    assert touched("coils1x5", 3) == [3, 2] and touched("coils1x5", 8) == [5]            # one coil per slice, several whole slices per chunk
    assert touched("coils2x5", 8) == [4, 1]                                              # a chunk over four slices
    assert touched("coils3x3", 8) == [3, 1] and ch("coils3x3", 8)[1] == (8, 1)           # all three slices, then one image that continues slice 2
    assert midstart("coils4x3", 3) == [0, 3, 2, 1] and midstart("coils4x3", 4) == [0, 0, 0]
    assert [cnt for _, cnt in ch("coils5x3", 2)][-1] == 1 and [cnt for _, cnt in ch("coils5x3", 4)][-1] == 3 and [cnt for _, cnt in ch("coils5x3", 7)][-1] == 1
    assert any(midstart("coils5x3", mb)[i] for mb in (2, 4, 7) for i in range(1, len(ch("coils5x3", mb))))
    assert max(C["coils8x2"]["max_batch"]) >= 8 * 2 and len(ch("coils13x1", 4)) == 4
    for n in MR.ALL:                                                                     # every max_batch of every case: the chunks tile the images
        c = MR.inputs(n)
        assert c["maps"].shape == (c["S"], c["N"], c["M"], c["nc"]) and c["y"].shape == (c["S"], c["m"], c["nc"])
        for mb in c["max_batch"]:
            assert sum(cnt for _, cnt in ch(n, mb)) == c["nc"] * c["S"]
    c = MR.inputs("stride128x64")
    assert c["m"] == 24576 > 64 * 256 and c["N"] * c["M"] * c["s"] == 81920 > 256 * 256 and np.all(np.diff(c["fp"]) == 2048)
    assert (c["s"], c["T"], c["nc"], c["S"], c["max_batch"]) == (10, 12, 3, 2, (4,))
    assert [(C[n]["N"], C[n]["M"], C[n]["s"], C[n]["nc"], C[n]["S"]) for n in MR.STRIDES[1:]] == [(32, 128, 10, 2, 2), (32, 32, 1, 4, 2), (64, 32, 3, 3, 1)]
    for n in MR.MASKS + MR.MAPCASES:
        assert (C[n]["s"], C[n]["nc"], C[n]["S"]) == (6, 3, 2)
    assert MR.inputs("single_sample")["m"] == 1
    c = MR.inputs("empty_rows_frames")
    assert np.any(np.diff(c["fp"]) == 0) and 0 not in c["k"] % 32 and np.unique(c["k"] % 32).size < 32
    c = MR.inputs("full_then_k0")
    assert c["T"] == 8 and np.bincount(c["k"], minlength=1024)[0] == 8 and np.bincount(c["k"], minlength=1024)[1:].max() < 8
    assert (C["epi64x32"]["N"], C["epi64x32"]["M"]) == (64, 32) and {(C[n]["N"], C[n]["M"]) for n in MR.MASKED} == {(32, 32), (64, 32)}
    for n in MR.ALL:                                                                     # the maps are what their names say
        c = MR.inputs(n)
        ss = np.sum(np.abs(c["maps"]) ** 2, axis=3)
        if c["kind"] == "stagger":
            assert np.allclose(ss[[0, 1, 2, 4]], 1.0, rtol=0, atol=1e-14) and ss[3].min() < 0.03 and ss[3].max() > 11.0
        elif c["maps_kind"] == "masked":
            out = ~MR.ellipse(c["N"], c["M"])
            assert 0.1 < out.mean() < 0.6 and not np.any(c["maps"][:, out, :]) and np.allclose(ss[:, ~out], 1.0, rtol=0, atol=1e-14)
        elif c["maps_kind"] == "unnormalised":
            assert 0.2 - 1e-12 <= ss.min() < 0.25 and 2.5 < ss.max() <= 3.0 + 1e-12
        else:
            assert np.allclose(ss, 1.0, rtol=0, atol=1e-14)
        if c["maps_kind"] == "constant":
            assert np.all(c["maps"] == c["maps"][:, :1, :1, :]) and not np.array_equal(c["maps"][0], c["maps"][1])
        assert np.allclose(c["V"].T @ c["V"], np.eye(c["s"]), rtol=0, atol=1e-14)
    # the tables: at most a quarter of the cases may carry an LSQR_SENS entry, none of the coil-count / chunking cases
    assert set(MR.LSQR_SENS) <= set(MR.ALL) and 4 * len(MR.LSQR_SENS) <= len(MR.ALL) and not set(MR.LSQR_SENS) & set(MR.COILS)


@pytest.mark.parametrize("name", MR.ALL)
def test_oracle_operator_agrees_with_the_restatement(oracle, name):
    """forward_mc / adjoint_mc of the oracle against mc_ref under every slice's maps: 1e-13.  mc_ref's own adjointness and its k-space route to
    A_mc^H A_mc (normal_mc, which minimiser_mc iterates with) against adjoint_mc(forward_mc): 1e-13."""
    c = MR.inputs(name)
    V, fp, k, N, M = c["V"], c["fp"], c["k"], c["N"], c["M"]
    op = MR.oracle_operator(name)
    assert op.m == c["m"]
    G = GR.gram(V, fp, k, N * M)
    for b in range(c["S"]):
        maps, x = c["maps"][b], c["xop"]
        yr, xr = MR.forward_mc(x, maps, V, fp, k), MR.adjoint_mc(c["yn"], maps, V, fp, k, N, M)
        assert yr.shape == (c["m"], c["nc"])
        ef, ea = rel_err(op.forward_mc(x, maps), yr), rel_err(op.adjoint_mc(c["yn"], maps), xr)
        lhs, rhs = np.vdot(c["yn"], yr), np.vdot(xr, x)
        en = rel_err(MR.normal_mc(x, maps, G), MR.adjoint_mc(yr, maps, V, fp, k, N, M))
        print(f"{name} slice {b}: forward {ef:.2e} adjoint {ea:.2e} adjointness of the restatement {abs(lhs - rhs) / abs(lhs):.2e} normal_mc {en:.2e}")
        assert ef < 1e-13 and ea < 1e-13
        assert abs(lhs - rhs) / abs(lhs) < 1e-13
        assert en < 1e-13


@pytest.mark.parametrize("name", MR.ALL)
def test_minimiser_solves_the_normal_equations(name):
    """The residual of (A_mc^H A_mc + r I) x = A_mc^H y + r z, computed from x through forward_mc / adjoint_mc: <= 1e-13 on every slice.  Where every
    coil's map is exactly zero A_mc has a null space and the minimiser is z: to 1e-12."""
    c = MR.inputs(name)
    xm = MR.minimisers(name)
    for b in range(c["S"]):
        res = MR.normal_residual(xm[b], c["y"][b], c["maps"][b], c["z"][b], MR.R, c["V"], c["fp"], c["k"])
        print(f"{name} slice {b}: normal-equation residual {res:.2e}")
        assert res <= 1e-13
        if c["maps_kind"] == "masked":
            out = ~MR.ellipse(c["N"], c["M"])
            e = rel_err(xm[b][out], c["z"][b][out])
            print(f"{name} slice {b}: x against z where every map is zero {e:.2e}")
            assert e < 1e-12 and rel_err(xm[b][~out], c["z"][b][~out]) > 1e-3


def test_minimiser_with_one_unit_coil_is_the_gridded_minimiser():
    """One all-ones coil: A_mc = A, and minimiser_mc equals gridded_ref.minimiser (a dense solve per k) to 1e-11."""
    c = MR.inputs("coils3x3")
    ones = np.ones((c["N"], c["M"], 1))
    y, z = c["y"][0][:, :1], c["z"][0]
    e = rel_err(MR.minimiser_mc(y, ones, z, MR.R, c["V"], c["fp"], c["k"]), GR.minimiser(y[:, 0], z, MR.R, c["V"], c["fp"], c["k"]))
    print(f"one unit coil: minimiser_mc against gridded_ref.minimiser {e:.2e}")
    assert e < 1e-11


def test_minimiser_raises_instead_of_returning_a_loose_solve():
    c = MR.inputs("coils3x3")
    with pytest.raises(RuntimeError):
        MR.minimiser_mc(c["y"][0], c["maps"][0], c["z"][0], MR.R, c["V"], c["fp"], c["k"], maxit=5)


@pytest.mark.parametrize("name", MR.ALL)
def test_oracle_lsqr_is_off_the_stop_rule_boundary_and_insensitive(oracle, name):
    """lsqr_mc per slice at tol 1e-4, maxit 100: five one-ulp perturbations of y and z leave (iterations, flag) unchanged, and x moves by <= 1e-12
    (the case takes the project's 1e-10 on the device) or by <= the case's entry in mc_ref.LSQR_SENS.  The iteration runs: at least 5 iterations on
    every generic slice (single_sample: one equation, 4)."""
    c = MR.inputs(name)
    for b in range(c["S"]):
        _, it, fl = MR.oracle_lsqr(name, b)
        worst, counts = MR.lsqr_sensitivity(name, b)
        print(f"{name} slice {b}: ({it}, {fl}), x moves by {worst:.2e} (recorded {MR.LSQR_SENS.get(name, 1e-12):.1e}, device bound {MR.lsqr_bound(name):.1e})")
        assert fl == 0 and set(counts) == {(it, fl)}, (name, b, it, fl, counts)
        assert worst <= MR.LSQR_SENS.get(name, 1e-12)
        if c["kind"] == "generic":
            assert it >= (4 if name == "single_sample" else 5), (name, b, it)


@pytest.mark.parametrize("name", MR.ALL)
def test_oracle_tight_lsqr_reaches_the_minimiser(oracle, name):
    """lsqr_mc at tol 1e-13, maxit 300 against minimiser_mc, per slice: within the case's entry in mc_ref.TIGHT_SENS (from which the device's bound
    follows) -- the oracle's iteration and the conjugate gradients of the restatement share nothing but the definition."""
    c = MR.inputs(name)
    xm = MR.minimisers(name)
    worst = 0.0
    for b in range(c["S"]):
        xt, it, fl = MR.oracle_lsqr(name, b, 1e-13, 300)
        e = rel_err(xt, xm[b])
        worst = max(worst, e)
        print(f"{name} slice {b}: tol 1e-13 ({it}, {fl}) against the minimiser {e:.2e}")
        assert it < 300
    print(f"{name}: {worst:.2e} (recorded {MR.TIGHT_SENS[name]:.1e}, device bound {MR.tight_bound(name):.1e})")
    assert worst <= MR.TIGHT_SENS[name]


def test_staggered_case_staggers(oracle):
    """The five slices of one stack stop at different iterations -- at least three distinct counts, the largest at least 5 above the smallest
    non-zero one -- so that a frozen slice is outlived by several iterations.  Slice 1 stops at 0 with x = 0, slice 2 at 0 or 1 on its start.  The
    prediction test's long solve (slice 3 at tol 1e-10) is stable under the perturbations too and more than twice as long as any of them."""
    c = MR.inputs("stagger")
    res = [MR.oracle_lsqr("stagger", b) for b in range(5)]
    counts = [it for _, it, _ in res]
    print(f"stagger: counts {counts}")
    assert all(fl == 0 for _, _, fl in res)
    assert len(set(counts)) >= 3 and max(counts) - min(i for i in counts if i > 0) >= 5
    assert counts[1] == 0 and not np.any(res[1][0])
    assert counts[2] <= 1 and rel_err(res[2][0], MR.minimisers("stagger")[2]) < 1e-12
    assert counts[0] >= 5 and counts[4] >= 5 and not np.array_equal(c["maps"][0], c["maps"][4])
    _, il, fll = MR.oracle_lsqr("stagger", 3, MR.STAGGER_LONG_TOL, 100)
    worst, cl = MR.lsqr_sensitivity("stagger", 3, MR.STAGGER_LONG_TOL, 100)
    print(f"stagger slice 3 at tol {MR.STAGGER_LONG_TOL:g}: ({il}, {fll}), x moves by {worst:.2e}")
    assert fll == 0 and set(cl) == {(il, fll)} and il >= 2 * max(counts) and worst <= 1e-12


def test_stagnation_exit_and_maxit_zero(oracle):
    """tol = 0 (qmri_xupdate_mc accepts it: only r > 0 and maxit >= 0 are checked) and maxit 300 on mc_ref.FLAG3_CASE's slice 0: the oracle ends by
    stagnation, flag 3, before maxit (measured: 42 iterations), at the minimiser; its count moves by at most mc_ref.FLAG3_SPREAD under the five
    perturbations (measured: not at all).  maxit = 0 returns x0 with flag 1."""
    name = MR.FLAG3_CASE
    c = MR.inputs(name)
    x, it, fl = MR.oracle_lsqr(name, 0, 0.0, 300)
    _, counts = MR.lsqr_sensitivity(name, 0, 0.0, 300)
    e = rel_err(x, MR.minimisers(name)[0])
    print(f"{name}: tol 0 ({it}, {fl}), perturbed {counts}, against the minimiser {e:.2e}")
    assert fl == 3 and 0 < it < 300 and all(f == 3 for _, f in counts)
    assert max(abs(i - it) for i, _ in counts) <= MR.FLAG3_SPREAD
    assert e <= MR.TIGHT_SENS[name]
    x, it, fl = MR.oracle_lsqr(name, 0, 1e-4, 0)
    assert (it, fl) == (0, 1) and np.array_equal(x, c["x0"][0])
