"""GPU: the multi-coil operator (the set_coils route of api_operator.cpp / ew_kernels.hip) and the batched image-domain LSQR (mc_kernels.hip, behind
xupdate_mc and xupdate_mc_batch) on every case of tests/mc_ref.py -- coil counts against chunkings of the coil images (chunks over several slices,
chunks that start inside a slice, ragged last chunks, max_batch above the image count), image and sample counts on both sides of the streaming
kernels' strides, masks down to one sample, masked / unnormalised / constant maps, and one stack whose slices stop at different iterations --
against two yardsticks: the numpy restatement mc_ref (written from the definition in include/qmri.h) and the CPU oracle's lsqr_mc, which
tests/test_mc_ref_host.py holds to each other on the same inputs.  One Engine for the file, re-planned per case and max_batch; the prediction test
takes fresh ones.

Bounds: forward_mc / adjoint_mc / adjointness 1e-12 (the figure the single-coil sweeps hold; the yardsticks agree to 1e-15).  LSQR at tol 1e-4: the
oracle's (iterations, flag), which the host test shows not to sit on a stop-rule boundary, and x to mc_ref.lsqr_bound = 1e-10 on every case (the
project's figure; no case needed an entry in mc_ref.LSQR_SENS).  LSQR at tol 1e-13 against the exact minimiser: mc_ref.tight_bound = 1e-7 on every
case (tests/test_gpu_operator.py's figure).  Everything the header of mc_kernels.hip promises to be batch-invariant -- a slice alone, in a stack, in
any order, under any max_batch -- is held to identical bits.

Measured on the MI355X: forward / adjoint <= 4.2e-16, adjointness <= 6.4e-15, x against the oracle <= 7.9e-16 with every count equal, tol 1e-13
against the minimiser <= 1.2e-13 (1.4e-12 on the staggered case's ill-conditioned slice); the flag-3 solve stops at the oracle's 42 iterations.
64 tests in 7.4 s with the interpreter's start and the CPU references; the slowest case 1.4 s (stride128x64 under set_coils, most of it
minimiser_mc and the oracle on the CPU), every other under 0.5 s.

Tried against wrong builds of mc_kernels.hip that the earlier multi-coil tests at 32 x 32 pass: the slice count of a chunk taken as
ceil(cnt / ncoil) (fails coils3x3 .. coils8x2, stagger), the sample loop of k_mcl_ulin or the image loop of k_mcl_vupd run once instead of with its
stride (fails stride128x64 only), the stagnation exit disabled (fails test_exits)."""
import numpy as np
import pytest

import mc_ref as MR
from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(engine_mod, oracle):
    e = engine_mod.Engine(0)
    yield e
    e.close()


def _plan(e, c, max_batch):
    e.set_operator(c["N"], c["M"], c["V"], c["fp"], c["k"], max_batch=max_batch)
    assert (e.N, e.M, e.s, e.m) == (c["N"], c["M"], c["s"], c["m"])


def _same(a, b):
    """Two (x, iterations, flags) results: identical bits and counts."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _check_against_oracle(name, b, x, it, fl, tol=1e-4, maxit=100, what=""):
    xo, io, flo = MR.oracle_lsqr(name, b, tol, maxit)
    e = rel_err(x, xo)
    print(f"{name} slice {b} {what}: gpu ({it}, {fl}) oracle ({io}, {flo}) x {e:.2e} (bound {MR.lsqr_bound(name):.1e})")
    assert (int(it), int(fl)) == (io, flo), (name, b, what, it, io, fl, flo)
    assert e < MR.lsqr_bound(name), (name, b, what, e)


def _check_against_minimiser(name, b, x, what=""):
    e = rel_err(x, MR.minimisers(name)[b])
    print(f"{name} slice {b} {what}: tol 1e-13 against the minimiser {e:.2e} (bound {MR.tight_bound(name):.1e})")
    assert e < MR.tight_bound(name), (name, b, what, e)


@pytest.mark.parametrize("name", MR.ALL)
def test_operator_set_coils_route(eng, name):
    """forward_mc and adjoint_mc under slice 0's maps against the restatement, and adjointness, under each max_batch of the case (the coils go
    through the transforms max_batch at a time, the conjugate sum continues from chunk to chunk): identical bits across the max_batch values."""
    c = MR.inputs(name)
    V, fp, k, maps = c["V"], c["fp"], c["k"], c["maps"][0]
    yr, xr = MR.forward_mc(c["xop"], maps, V, fp, k), MR.adjoint_mc(c["yn"], maps, V, fp, k, c["N"], c["M"])
    first = None
    for mb in c["max_batch"]:
        _plan(eng, c, mb)
        eng.set_coils(maps)
        yg, xg = eng.forward_mc(c["xop"]), eng.adjoint_mc(c["yn"])
        ef, ea = rel_err(yg, yr), rel_err(xg, xr)
        lhs, rhs = np.vdot(c["yn"], yg), np.vdot(xg, c["xop"])
        print(f"{name} max_batch {mb}: forward {ef:.2e} adjoint {ea:.2e} adjointness {abs(lhs - rhs) / abs(lhs):.2e}")
        assert yg.shape == (c["m"], c["nc"])
        assert ef < 1e-12 and ea < 1e-12
        assert abs(lhs - rhs) / abs(lhs) < 1e-12
        assert rel_err(eng.forward_mc(c["xr"]), MR.forward_mc(c["xr"], maps, V, fp, k)) < 1e-12
        if first is None:
            first = (yg, xg)
        assert np.array_equal(yg, first[0]) and np.array_equal(xg, first[1]), (name, mb)


@pytest.mark.parametrize("name", MR.ALL)
def test_xupdate_set_coils_route(eng, name):
    """xupdate_mc on slice 0 under set_coils: the oracle's (iterations, flag) and x within the case's bound at tol 1e-4, the exact minimiser at tol
    1e-13; the same bits under every max_batch.  The one-slice xupdate_mc_batch call with the same maps (the other coil-multiply route's caller):
    equal (iterations, flag), x to 1e-10."""
    c = MR.inputs(name)
    maps, y, z, x0 = c["maps"][0], c["y"][0], c["z"][0], c["x0"][0]
    first = None
    for mb in c["max_batch"]:
        _plan(eng, c, mb)
        eng.set_coils(maps)
        xg, ig, flg = eng.xupdate_mc(y, z, MR.R, 1e-4, 100, x0)
        _check_against_oracle(name, 0, xg, ig, flg, what=f"set_coils, max_batch {mb}")
        xt, _, _ = eng.xupdate_mc(y, z, MR.R, 1e-13, 300, x0)
        _check_against_minimiser(name, 0, xt, what=f"set_coils, max_batch {mb}")
        xb, ib, flb = eng.xupdate_mc_batch(maps[None], y[None], z[None], MR.R, 1e-4, 100, x0[None])
        assert (int(ib[0]), int(flb[0])) == (ig, flg) and rel_err(xb[0], xg) < 1e-10, (name, mb, ib, ig, rel_err(xb[0], xg))
        if first is None:
            first = (xg, ig, flg, xt)
        assert np.array_equal(xg, first[0]) and (ig, flg) == first[1:3] and np.array_equal(xt, first[3]), (name, mb)


@pytest.mark.parametrize("name", MR.ALL)
def test_xupdate_batch_route(eng, name):
    """xupdate_mc_batch on the whole stack under each max_batch: per slice the oracle's (iterations, flag) and x within the case's bound at tol
    1e-4, the exact minimiser at tol 1e-13; identical bits and counts across the max_batch values, for every slice solved alone, and (staggered
    case) for the stack in reversed order."""
    c = MR.inputs(name)
    S, maps, y, z, x0 = c["S"], c["maps"], c["y"], c["z"], c["x0"]
    first = None
    for mb in c["max_batch"]:
        _plan(eng, c, mb)
        res = eng.xupdate_mc_batch(maps, y, z, MR.R, 1e-4, 100, x0)
        tight = eng.xupdate_mc_batch(maps, y, z, MR.R, 1e-13, 300, x0)
        for b in range(S):
            _check_against_oracle(name, b, res[0][b], res[1][b], res[2][b], what=f"stack, max_batch {mb}")
            _check_against_minimiser(name, b, tight[0][b], what=f"stack, max_batch {mb}")
        if first is None:
            first = (res, tight)
        assert _same(res, first[0]) and _same(tight, first[1]), (name, mb)
        for b in range(S):                                         # alone: the same bits as in the stack
            solo = eng.xupdate_mc_batch(maps[b:b + 1], y[b:b + 1], z[b:b + 1], MR.R, 1e-4, 100, x0[b:b + 1])
            assert np.array_equal(solo[0][0], res[0][b]) and (solo[1][0], solo[2][0]) == (res[1][b], res[2][b]), (name, mb, b)
        if c["kind"] == "stagger":
            rev = eng.xupdate_mc_batch(maps[::-1], y[::-1], z[::-1], MR.R, 1e-4, 100, x0[::-1])
            assert _same((rev[0][::-1], rev[1][::-1], rev[2][::-1]), res), (name, mb)
            rev = eng.xupdate_mc_batch(maps[::-1], y[::-1], z[::-1], MR.R, 1e-13, 300, x0[::-1])
            assert _same((rev[0][::-1], rev[1][::-1], rev[2][::-1]), tight), (name, mb)


@pytest.mark.parametrize("max_batch", MR.CASES["stagger"]["max_batch"])
def test_frozen_slices_are_left_alone(eng, max_batch):
    """The staggered stack: slices that stop at iteration 0 while others run 18 and 28 more (the transforms still run on their coil images).  After
    the batch slice 1 is exactly zero, slice 2 is its minimiser (its start) within the bound, and every slice -- in the whole stack and in stacks
    that pair a stopped slice with the longest one, either way round -- holds the bits of its solo solve."""
    name = "stagger"
    c = MR.inputs(name)
    maps, y, z, x0 = c["maps"], c["y"], c["z"], c["x0"]
    _plan(eng, c, max_batch)
    run = lambda idx: eng.xupdate_mc_batch(maps[idx], y[idx], z[idx], MR.R, 1e-4, 100, x0[idx])
    solo = [run([b]) for b in range(5)]
    counts = [int(s[1][0]) for s in solo]
    print(f"stagger max_batch {max_batch}: solo counts {counts}")
    assert counts == [MR.oracle_lsqr(name, b)[1] for b in range(5)]
    for idx in ([0, 1, 2, 3, 4], [1, 3], [3, 1], [2, 3, 1], [0, 2, 4], [3, 2, 0]):
        xs, its, fls = run(idx)
        for pos, b in enumerate(idx):
            assert np.array_equal(xs[pos], solo[b][0][0]) and (its[pos], fls[pos]) == (solo[b][1][0], solo[b][2][0]), (max_batch, idx, b)
        if 1 in idx:
            assert not np.any(xs[idx.index(1)])
        if 2 in idx:
            assert rel_err(xs[idx.index(2)], MR.minimisers(name)[2]) < MR.lsqr_bound(name)


def test_prediction_in_both_directions(engine_mod, oracle):
    """w.pred queues as many iterations as the last solve needed, then a quarter of that at a time.  On ONE Engine, in this order: slice 2 (stops at
    once: the prediction falls to 1), slice 3 at tol 1e-10 (76 iterations, queued two at a time), slice 2 again, slice 0 (from a prediction of 1),
    slice 3 again, slice 0 (18 iterations under a prediction of 77: some sixty whole iterations are queued with the slice frozen).  Each result
    equals -- bits, count and flag -- the same solve on a fresh Engine, and has the oracle's count and x."""
    name = "stagger"
    c = MR.inputs(name)
    mb = c["max_batch"][0]
    maps, y, z, x0 = c["maps"], c["y"], c["z"], c["x0"]
    solve = lambda e, b, tol: e.xupdate_mc_batch(maps[b:b + 1], y[b:b + 1], z[b:b + 1], MR.R, tol, 100, x0[b:b + 1])
    fresh = {}
    for b, tol in ((2, 1e-4), (3, MR.STAGGER_LONG_TOL), (0, 1e-4)):
        e = engine_mod.Engine(0)
        _plan(e, c, mb)
        fresh[(b, tol)] = solve(e, b, tol)
        e.close()
    e = engine_mod.Engine(0)
    _plan(e, c, mb)
    for step, (b, tol) in enumerate(((2, 1e-4), (3, MR.STAGGER_LONG_TOL), (2, 1e-4), (0, 1e-4), (3, MR.STAGGER_LONG_TOL), (0, 1e-4))):
        got = solve(e, b, tol)
        xo, io, flo = MR.oracle_lsqr(name, b, tol, 100)
        print(f"step {step}: slice {b} at tol {tol:g}: gpu ({got[1][0]}, {got[2][0]}) oracle ({io}, {flo}) x {rel_err(got[0][0], xo):.2e}")
        assert _same(got, fresh[(b, tol)]), (step, b, tol, got[1], fresh[(b, tol)][1])
        assert (int(got[1][0]), int(got[2][0])) == (io, flo)
        assert rel_err(got[0][0], xo) < MR.lsqr_bound(name)
    e.close()


def test_exits(eng, oracle):
    """maxit = 3: flag 1 after 3 iterations on every running slice and the oracle's x to 1e-10 (staggered stack: the two slices that stop at 0 keep
    flag 0 in the same batch).  maxit = 0: x0 back bit for bit, flag 1.  tol = 0 (mc_ref.FLAG3_CASE, slice 0; both routes): the stagnation exit,
    flag 3 before maxit = 300, at the exact minimiser; the count within the spread the host test recorded + 2 of the oracle's."""
    for name in (MR.FLAG3_CASE, "stagger"):
        c = MR.inputs(name)
        maps, y, z, x0 = c["maps"], c["y"], c["z"], c["x0"]
        _plan(eng, c, c["max_batch"][0])
        xs, its, fls = eng.xupdate_mc_batch(maps, y, z, MR.R, 1e-4, 3, x0)
        for b in range(c["S"]):
            xo, io, flo = MR.oracle_lsqr(name, b, 1e-4, 3)
            assert (int(its[b]), int(fls[b])) == (io, flo) and rel_err(xs[b], xo) < 1e-10, (name, b, its[b], io, fls[b], flo, rel_err(xs[b], xo))
        assert [int(f) for f in fls] == ([1, 0, 0, 1, 1] if name == "stagger" else [1] * c["S"])
        xs, its, fls = eng.xupdate_mc_batch(maps, y, z, MR.R, 1e-4, 0, x0)
        stopped = [b for b in range(c["S"]) if MR.oracle_lsqr(name, b, 1e-4, 0)[2] == 0]        # (y = 0 and z = 0: flag 0 whatever maxit)
        assert np.array_equal(xs, x0) and not np.any(its) and [int(f) for f in fls] == [0 if b in stopped else 1 for b in range(c["S"])]
        assert stopped == ([1] if name == "stagger" else [])
    name = MR.FLAG3_CASE
    c = MR.inputs(name)
    maps, y, z, x0 = c["maps"], c["y"], c["z"], c["x0"]
    _, io, flo = MR.oracle_lsqr(name, 0, 0.0, 300)
    assert flo == 3
    _plan(eng, c, c["max_batch"][0])
    xb, ib, flb = eng.xupdate_mc_batch(maps[:1], y[:1], z[:1], MR.R, 0.0, 300, x0[:1])
    eng.set_coils(maps[0])
    xc, ic, flc = eng.xupdate_mc(y[0], z[0], MR.R, 0.0, 300, x0[0])
    for what, x, it, fl in (("batch", xb[0], int(ib[0]), int(flb[0])), ("set_coils", xc, ic, flc)):
        print(f"{name} at tol 0, {what} route: gpu ({it}, {fl}) oracle ({io}, {flo}), against the minimiser {rel_err(x, MR.minimisers(name)[0]):.2e}")
        assert fl == 3 and it < 300
        assert abs(it - io) <= MR.FLAG3_SPREAD + 2
        assert rel_err(x, MR.minimisers(name)[0]) < MR.tight_bound(name)
