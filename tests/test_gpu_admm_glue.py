"""GPU: the denoiser-step glue of the PnP-ADMM loop -- min / max, normalise, cast, noise plane, residual subtraction, un-normalise, dual update, z --
in all three forms the library has (k_minmax / k_normalise / k_unnormalise_dual of ew_kernels.hip; the fused k_adj_h min / max and k_dual_fwd_h of
dc_kernels.hip, instantiated per grid side; either with slice batches) against tests/admm_ref.py, an exact fp64 restatement of the loop whose
network is exact too (one routing 3x3 convolution: the f16 x 3 kernels return conv_ref.split_roundtrip of a value, the bf16 x 6 and f32 kernels the
value).  tests/test_admm_ref_host.py holds the restatement to the oracle's loop and measures the table the bounds come from.

Three ADMM iterations (iteration k's glue shows in x of iteration k + 1; by the third u is non-zero in both parts), gamma 0.05 and, on one case per
path, 5 (x close to z: glue errors pass almost unattenuated).  Paths: (a) default, fused, one-launch LSQR; (b) lsqr_persist(False), same bits as
(a); (c) QMRI_DEBUG=fuse_ew=0 / conv_scheme=3 / conv_f32=1, one child process each; (d) solver="direct"; (e) pnp_admm_mc with one coil of ones;
(f) pnp_admm_batch, three slices scaled by 1, 1e3 and 1e-3, three and two per launch.  Asserted: the reference's inner LSQR count in every
iteration of every slice, x and both diagnostic columns to admm_ref.bound (max(1e-9, 3 x the reference's own movement under 1e-10 perturbations
of its x-updates): 1e-8 .. 2e-7, against the 1e-4 the whole-loop parity tests allow), denoiser_scheme() == (2, 0) and every health counter zero
after every run -- a defect must fail, not move the work to another kernel.

Until this module no pnp_admm* call of the suite ran with residual_noise set (only Engine.denoise did): the in32 reads of k_unnormalise_dual and
k_dual_fwd_h had never run in a loop, with b > 0 or in complex mode.  Half of the mode grid below sets it, on every path.

The precondition, the network alone through Engine.denoise (the first exact test of k_pack / k_unpack), on inputs with exact 0 and 1 and values
below 2^-14 and 2^-24: see test_network_alone_is_exact for what the matrix cores keep of f16 subnormal pieces.

Measured on the MI355X: 114 tests in 10.3 s (the three child processes 0.6 .. 0.8 s each, the slowest in-process case 1.3 s: 256 x 256 with LSQR,
most of it the reference's three oracle solves on the CPU; every other case at most 0.45 s).  x and the diagnostics were within 4e-16 .. 6e-15 of
the reference on every run, every inner LSQR count equal; inputs below 2^-14 and 2^-24 came back with the bits numpy's float16 gives.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import admm_ref as A
import conv_ref as CR
from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("denoiser_fallbacks", "repeated_calls", "lsqr_one_launch_timeouts", "resident_tile_timeouts")
BIG = (1, 1, 1)                                                     # the mode that also runs at gamma = 5


@pytest.fixture(scope="module")
def eng(engine_mod, oracle):
    e = engine_mod.Engine(0)
    yield e
    e.close()


def healthy(e, scheme=(2, 0)):
    h = e.health()
    assert e.denoiser_scheme() == scheme, e.denoiser_scheme()
    assert all(h[n] == 0 for n in COUNTERS), h


def plan(e, d, max_batch=1):
    """operator and routing network of a run on the engine"""
    c = d["c"]
    e.set_operator(c["N"], c["M"], c["V"], c["fp"], c["k"], max_batch=max_batch)
    e.set_denoiser(d["w"].ravel(), c["N"], c["M"], in_nc=d["in_nc"], out_nc=d["out_nc"], nc=(d["out_nc"], 0, 0, 0), nb=1, arch=1,
                   residual_noise=bool(d["mode"][2]), max_batch=max_batch)


def loop_args(d):
    cpx, multi, _ = d["mode"]
    return dict(gamma=d["gamma"], iters=A.ITERS, cg_tol=A.TOL, cg_maxit=A.MAXIT, multi_level=bool(multi), noise_std=A.NOISE_STD,
                tsmi_domain="complex" if cpx else "real")


def check(what, key, x, li, diag=None):
    """one slice against its reference run"""
    xr, dr, lr = A.reference(key)
    b = A.bound(key)
    ex = rel_err(x, xr)
    ed = float(np.abs(diag / dr - 1.0).max()) if diag is not None else 0.0
    msg = f"{what} {key}: x {ex:.2e} diagnostics {ed:.2e} (bound {b:.1e}), inner iterations {np.asarray(li).tolist()} / {lr.tolist()}"
    if not A.RUNS[key]["mode"][0]:
        msg += f", max |x - x_ref| {np.abs(x - xr).max():.2e} of max |x| {np.abs(xr).max():.2e}"
    print(msg)
    assert np.array_equal(np.asarray(li), lr), msg
    assert ex < b and ed < b, msg


def mode_runs():
    return [(m, A.GAMMA) for m in A.MODES] + [(BIG, A.GAMMA_BIG)]


def run_id(v):
    return A.mode_id(v) if isinstance(v, tuple) else v if isinstance(v, str) else f"g{v:g}"


# ---- the precondition: the network alone ---------------------------------------------------------------------------------------------------------
def special_input(rng, H, W, C, B):
    """fp32 values in [0, 1] with full mantissas; exact 0 and 1 and values below 2^-14 (f16 subnormal) and below 2^-24 (below f16's smallest)"""
    x = rng.random((H, W, C, B), dtype=np.float32)
    x = np.maximum(x, np.float32(2.0 ** -10))
    sp = np.float32([0.0, 1.0, 2.0 ** -15 * 1.37, 2.0 ** -20 * 1.11, 2.0 ** -23 * 1.73, 2.0 ** -25 * 1.9, 2.0 ** -30 * 1.3])
    for c in range(C):
        for b in range(B):
            hs, ws = rng.permutation(H)[:sp.size], rng.permutation(W)[:sp.size]
            x[hs, ws, c, b] = sp
    x[0, 0, 0, 0], x[H - 1, W - 1, C - 1, B - 1] = 0.0, 1.0
    return x


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(17, 9), (32, 32), (40, 24)])
def test_network_alone_is_exact(eng, H, W, B, res):
    """Engine.denoise (k_pack, one 3x3 layer, k_unpack) with routing weights, 4 -> 3 channels as the real multi-level mode has them: the output bits
    are weight * split_roundtrip(input), shifted, and with the residual float32(input - that).  That includes the outputs that copy an input below
    2^-14 (a subnormal f16 high piece) or below 2^-24 (no high piece at all; the low piece, (x - hi) * 2^11, is subnormal in turn): on the MI355X
    the conversions and the matrix cores keep subnormal f16 pieces exactly as numpy's float16 does, no output differed.  The count of such outputs
    is printed, and a difference confined to them would be a finding about the f16 path rather than about k_pack / k_unpack."""
    routes = A.routing(3, 0, 1, seed=H + W)
    w = A.routing_weights(routes, 4)
    x = special_input(np.random.default_rng(1000 * H + 10 * W + B), H, W, 4, B)
    eng.set_denoiser(w.ravel(), H, W, in_nc=4, out_nc=3, nc=(3, 0, 0, 0), nb=1, arch=1, residual_noise=res, max_batch=B)
    y = eng.denoise(x.astype(np.float64))
    healthy(eng)
    want = np.stack([A.route(x[..., b], routes, CR.split_roundtrip) for b in range(B)], axis=3)
    small = np.stack([A.route(((x[..., b] > 0) & (x[..., b] < 2.0 ** -14)).astype(np.float32), routes) != 0 for b in range(B)], axis=3)
    if res:
        want = x[:, :, :3] - want
        assert want.dtype == np.float32
    assert y.shape == want.shape and np.array_equal(y.astype(np.float32).astype(np.float64), y)
    diff = y != want.astype(np.float64)
    print(f"{H} x {W} B {B} residual {res}: {int(diff.sum())} outputs differ, {int((diff & small).sum())} of them among the {int(small.sum())} that copy an "
          f"input below 2^-14; largest difference {np.abs(y - want).max():.3g}")
    assert not (diff & ~small).any()
    assert not diff.any()


# ---- the loop, in this process ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,gamma", mode_runs(), ids=run_id)
def test_modes_fused_lsqr(eng, mode, gamma):
    """(a) and (b): the default path and two launches per LSQR iteration, the same bits of x; diagnostics of every iteration"""
    key = A.run_key(A.MODE_GRID, mode, gamma=gamma)
    d = A.data(A.RUNS[key])
    plan(eng, d)
    x, diag, li = eng.pnp_admm(d["y"], gt=d["gt"], want_diag=True, **loop_args(d))
    healthy(eng)
    check("fused", key, x, li, diag)
    try:
        eng.lsqr_persist(False)
        x2, diag2, li2 = eng.pnp_admm(d["y"], gt=d["gt"], want_diag=True, **loop_args(d))
    finally:
        eng.lsqr_persist(True)
    healthy(eng)
    assert np.array_equal(li, li2) and np.array_equal(x, x2), rel_err(x2, x)
    check("two-launch", key, x2, li2, diag2)


@pytest.mark.parametrize("mode,gamma", mode_runs(), ids=run_id)
def test_modes_direct(eng, mode, gamma):
    """(d): the DIRECT solver runs the separate kernels"""
    key = A.run_key(A.MODE_GRID, mode, solver="direct", gamma=gamma)
    d = A.data(A.RUNS[key])
    plan(eng, d)
    x, diag, li = eng.pnp_admm(d["y"], solver="direct", gt=d["gt"], want_diag=True, **loop_args(d))
    healthy(eng)
    check("direct", key, x, li, diag)


@pytest.mark.parametrize("mode,gamma", mode_runs(), ids=run_id)
def test_modes_multi_coil_loop(eng, mode, gamma):
    """(e): the multi-coil loop with one coil of ones -- the separate kernels, z prepared before the loop, its own LSQR -- against the same reference"""
    key = A.run_key(A.MODE_GRID, mode, gamma=gamma)
    d = A.data(A.RUNS[key])
    plan(eng, d)
    c = d["c"]
    eng.set_coils(np.ones((c["N"], c["M"], 1), np.complex128))
    x, li = eng.pnp_admm_mc(d["y"][:, None], **loop_args(d))
    healthy(eng)
    check("multi-coil", key, x, li)


@pytest.mark.parametrize("spl", [3, 2])
@pytest.mark.parametrize("mode,gamma", mode_runs(), ids=run_id)
def test_modes_slice_batch(eng, mode, gamma, spl):
    """(f): three slices scaled by 1, 1e3, 1e-3, all in one launch and two per launch (the last group short); each against its own reference"""
    keys = [A.run_key(A.MODE_GRID, mode, gamma=gamma, scale=sc) for sc in A.SCALES]
    ds = [A.data(A.RUNS[k]) for k in keys]
    plan(eng, ds[0], max_batch=3)
    X, LI = eng.pnp_admm_batch(np.stack([d["y"] for d in ds]), slices_per_launch=spl, **loop_args(ds[0]))
    healthy(eng)
    for b, key in enumerate(keys):
        check(f"batch of 3, {spl} per launch, slice {b}", key, X[b], LI[b])


@pytest.mark.parametrize("solver", ["lsqr", "direct"])
@pytest.mark.parametrize("grid,mode", [(g, m) for g in A.SIDE_GRIDS for m in A.EXTREME] + [(g, BIG) for g in A.CHAN_GRIDS], ids=run_id)
def test_sides_and_channel_counts(eng, grid, mode, solver):
    """(a) and (d) on every supported side as N (k_dual_fwd_h and k_adj_h are instantiated per N), on the grids whose h-pass takes 8 lines per
    workgroup, and for s = 1, 2, 7 (complex multi-level residual only)"""
    key = A.run_key(grid, mode, solver=solver)
    d = A.data(A.RUNS[key])
    plan(eng, d)
    x, diag, li = eng.pnp_admm(d["y"], solver=solver, gt=d["gt"], want_diag=True, **loop_args(d))
    healthy(eng)
    check(solver, key, x, li, diag)


# ---- (c): the knobs that are read when the plan is made, one child process each -----------------------------------------------------------------
_CHILD = (
    "import sys\n"
    "sys.path[:0] = [%r, %r]\n"
    "import test_gpu_admm_glue as T\n"
    "from qmri_pnp_recon_poc_amd import engine as E\n"
    "T.child_main(E, sys.argv[1], sys.argv[2])\n" % (ROOT, os.path.join(ROOT, "tests")))


def child_main(E, what, out):
    res = {}
    e = E.Engine(0)
    for mode, gamma in (mode_runs() if what == "separate" else [(m, A.GAMMA) for m in A.MODES]):
        name = f"{A.mode_id(mode)}:g{gamma:g}"
        ds = [A.data(A.RUNS[A.run_key(A.MODE_GRID, mode, gamma=gamma, scale=sc)]) for sc in (A.SCALES if what == "separate" else A.SCALES[:1])]
        plan(e, ds[0], max_batch=len(ds))
        x, diag, li = e.pnp_admm(ds[0]["y"], gt=ds[0]["gt"], want_diag=True, **loop_args(ds[0]))
        res[name + ":x"], res[name + ":diag"], res[name + ":li"] = x, diag, li
        if what == "separate":
            for spl in (3, 2):
                res[f"{name}:X{spl}"], res[f"{name}:LI{spl}"] = e.pnp_admm_batch(np.stack([d["y"] for d in ds]), slices_per_launch=spl, **loop_args(ds[0]))
        h = e.health()
        res[name + ":state"] = np.array(e.denoiser_scheme() + tuple(h[n] for n in COUNTERS))
    e.close()
    np.savez(out, **res)


def run_child(what, knobs):
    """one fresh process, one at a time, under its own time limit; a failing one raises"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "x.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, what, out], env=dict(os.environ, QMRI_DEBUG=knobs), timeout=240, capture_output=True, text=True)
        assert r.returncode == 0, (knobs, r.returncode, r.stderr[-3000:])
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


def test_modes_separate_kernels(oracle):
    """fuse_ew=0: the mode grid through k_minmax / k_normalise / k_unnormalise_dual with the LSQR solver, single slices and the scaled batch"""
    res = run_child("separate", "fuse_ew=0")
    for mode, gamma in mode_runs():
        name = f"{A.mode_id(mode)}:g{gamma:g}"
        assert tuple(res[name + ":state"]) == (2, 0, 0, 0, 0, 0), (name, res[name + ":state"])
        keys = [A.run_key(A.MODE_GRID, mode, gamma=gamma, scale=sc) for sc in A.SCALES]
        check("fuse_ew=0", keys[0], res[name + ":x"], res[name + ":li"], res[name + ":diag"])
        for spl in (3, 2):
            for b, key in enumerate(keys):
                check(f"fuse_ew=0, batch of 3, {spl} per launch, slice {b}", key, res[f"{name}:X{spl}"][b], res[f"{name}:LI{spl}"][b])


@pytest.mark.parametrize("knobs,scheme", [("conv_scheme=3", 3), ("conv_f32=1", 2)])
def test_modes_other_network_arithmetic(oracle, knobs, scheme):
    """bf16 x 6 and the f32-MFMA kernels return the fp32 value of a routed element: the reference with the identity for the round trip"""
    res = run_child("arith", knobs)
    for mode in A.MODES:
        name = f"{A.mode_id(mode)}:g{A.GAMMA:g}"
        assert tuple(res[name + ":state"]) == (scheme, 0, 0, 0, 0, 0), (name, res[name + ":state"])
        check(knobs, A.run_key(A.MODE_GRID, mode, rt="id"), res[name + ":x"], res[name + ":li"], res[name + ":diag"])
