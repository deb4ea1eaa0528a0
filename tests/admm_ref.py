"""The PnP-ADMM loop (PnP_ADMM.m:76-148) restated in plain numpy, with the x-update and the network passed in as functions, and the case tables of
the denoiser-step ("glue") tests.  Test infrastructure only: tests/test_admm_ref_host.py holds it to the CPU oracle's loop and to
tests/complex_admm_ref.py and proves the premises stated here; tests/test_gpu_admm_glue.py holds the kernels to it.

What is restated is everything between two x-updates: t = real(x + u) (complex mode: the real and the imaginary part as two stacks of planes), the
global min and max, n32 = float32((t - lo) / (hi - lo)) with no zero-range guard, the appended plane float32(noise_std) (channel s, or 2s in complex
mode), the network, the optional fp32 subtraction n32 - I of residual_noise, v = double(I) * (hi - lo) + lo with one lo and one range for both
halves, u = u + x - v (u complex: in real mode its imaginary part accumulates imag(x)) and z = v - u.  All of it is fp64 except the two marked
fp32 steps; the kernels contract I * range + lo into one FMA, one ulp of fp64.

The network is QMRI_ARCH_SEQ_CONV with nb = 1, one bias-free 3x3 convolution, with weights that only route (`routing`): output channel o reads ONE
input channel through ONE weight from {1, -1, 0.5} at one tap, so o = weight * shift(input channel) with zeros pulled in from the halo by the
off-centre taps.  On the f16 x 3 scheme such a layer returns conv_ref.split_roundtrip(value) times the weight (conv_ref.copy_weights states this),
under conv_scheme=3 and conv_f32=1 the fp32 value itself: `roundtrip` is that function, or None for the identity.  Either way every summation
order gives the same bits, so the reference network is exact.  The input channel of output o is (o + shift) mod in_nc with shift = s in complex
mode (the real half reads the imaginary half and the other way round) and 1 in real mode; in multi-level mode the output that lands on the noise
plane reads it.  in_nc = out_nc (+ 1): single-level, every input plane is read; multi-level has one more input plane than outputs, so with one
weight per output one image plane stays unread (real: plane 0; complex: plane s - 1 of the real half) -- it is still normalised, cast and
written, and the planes beside it show a store that strays.

The bound (ADMM_SENS, bound()): x on the device differs from x here by fp64 rounding in every x-update, 1e-10 by the project's own bound
(tests/test_gpu_gridded_sweep.py).  The cast to fp32 and the 22-bit split are discontinuous: such a difference flips the rounding of a few
elements per iteration, each by 2^-23 or 2^-22 of the range.  loop_sensitivity() measures that on the reference alone: five reruns with every
x-update's output multiplied elementwise (real and imaginary part separately) by 1 + 1e-10 * gaussian; ADMM_SENS records the largest movement of
the final x and of the diagnostics per run, asserted from above by the host test with a factor 2 of room.  The device's bound is
max(1e-9, 3 x entry): it errs in every operation of every iteration, not once per x-update, and 1e-9 is the figure tests/test_gpu_lrtv.py holds
fp64 loops to."""
import functools

import numpy as np

import conv_ref as CR
import gridded_ref as GR

ITERS = 3
NOISE_STD = 0.03             # not the default 0.01, and no power of two: the plane's value is pinned through float32() and the f16 split
GAMMA, GAMMA_BIG = 0.05, 5.0
TOL, MAXIT = 1e-4, 100
PERTURB = 1e-10              # the project's bound on one x-update (gridded_ref.lsqr_bound's floor, test_gpu_gridded_sweep's DIRECT bound)

MODES = [(cpx, multi, res) for cpx in (0, 1) for multi in (0, 1) for res in (0, 1)]       # (complex, multi_level, residual_noise)
EXTREME = [(0, 0, 0), (1, 1, 1)]


def mode_id(mode):
    return ("cpx" if mode[0] else "real") + ("_multi" if mode[1] else "_single") + ("_res" if mode[2] else "")


# ---- grids: gridded_ref's cases, and the 32 x 32 x 3 grid of the mode table (same builders: orthonormal V, user_mask) -----------------------------
GR._case([], "glue32x32_s3", 32, 32, 3, 12, functools.partial(GR.user_mask, 32, 32, 12, 64, 32032), seed=903)
MODE_GRID = "glue32x32_s3"
SIDE_GRIDS = [f"grid{n}x32" for n in GR.SIDES] + ["grid32x96", "grid32x256", "grid256x256"]
CHAN_GRIDS = ["chan1", "chan2", "chan7"]
SCALES = (1.0, 1e3, 1e-3)    # the slices of the batch path: a lo or a range taken from another slice is wrong by a factor 1e3 or more


# ---- the routing network ----------------------------------------------------------------------------------------------------------------------------
def channels(s, cpx, multi):
    planes = 2 * s if cpx else s
    return planes + (1 if multi else 0), planes


def routing(s, cpx, multi, seed):
    """[(input channel, kh, kw, weight)] per output channel (module docstring).  Taps walk through all nine from a random start, so all but at
    most a ninth of the outputs shift; the weights walk through 1, -1, 0.5."""
    in_nc, out_nc = channels(s, cpx, multi)
    rng = np.random.default_rng(seed)
    t0, w0 = int(rng.integers(9)), int(rng.integers(3))
    shift = s if cpx else 1
    routes = []
    for o in range(out_nc):
        tap = (t0 + 4 * o) % 9                                      # (4 is coprime to 9: nine outputs in a row take nine different taps)
        if out_nc < 9 and tap == 4:
            tap = 5                                                  # few outputs: none of them spends itself on the centre tap
        routes.append(((o + shift) % in_nc, tap // 3, tap % 3, (1.0, -1.0, 0.5)[(w0 + o) % 3]))
    return routes


def routing_weights(routes, in_nc):
    """The OIHW 3x3 blob of a routing."""
    w = np.zeros((len(routes), in_nc, 3, 3), np.float32)
    for o, (c, kh, kw, val) in enumerate(routes):
        w[o, c, kh, kw] = val
    return w


def route(x, routes, roundtrip=None):
    """The routing network on x [H, W, in_nc] (fp32 values): out[h, w, o] = weight * rt(x)[h + kh - 1, w + kw - 1, c], zero outside; float32."""
    x = np.asarray(x, np.float32)
    H, W, _ = x.shape
    xr = (x.astype(np.float64) if roundtrip is None else roundtrip(x))
    xp = np.zeros((H + 2, W + 2, x.shape[2]))
    xp[1:-1, 1:-1] = xr
    out = np.stack([val * xp[kh:kh + H, kw:kw + W, c] for c, kh, kw, val in routes], axis=2)
    o32 = out.astype(np.float32)
    assert np.array_equal(o32.astype(np.float64), out)              # (weight * kept value is an fp32 value: nothing rounds here)
    return o32


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------------
def normalise(x, u, cpx, multi, noise_std):
    """Step 2 up to the network: (n32 [N, M, in_nc] float32, lo, range)."""
    t = x + u
    t = np.concatenate([t.real, t.imag], axis=2) if cpx else t.real
    lo, hi = t.min(), t.max()
    rng = hi - lo
    n32 = ((t - lo) / rng).astype(np.float32)
    if multi:
        n32 = np.concatenate([n32, np.full(n32.shape[:2] + (1,), np.float32(noise_std), np.float32)], axis=2)
    return n32, lo, rng


def denoiser_step(x, u, net, cpx, multi, noise_std, residual):
    """Steps 2 and 3: (v, u_new)."""
    s = x.shape[2]
    n32, lo, rng = normalise(x, u, cpx, multi, noise_std)
    I = np.asarray(net(n32), np.float32)
    if residual:
        I = n32[:, :, :I.shape[2]] - I                              # an fp32 subtraction (denoiseImage_PnP_ADMM.m:99-104)
        assert I.dtype == np.float32
    W = I.astype(np.float64) * rng + lo
    v = W[:, :, :s] + 1j * W[:, :, s:2 * s] if cpx else W[:, :, :s] + 0j
    return v, (u + x) - v


def admm(y, x0, xupdate, net, forward, iters=ITERS, gamma=GAMMA, cpx=False, multi=False, noise_std=NOISE_STD, residual=False, gt=None, after_xupdate=None):
    """PnP_ADMM.m:76-148.  xupdate(y, z, gamma, x_prev) -> (x, inner iterations); net(n32) -> fp32 [N, M, out_nc]; forward(x) -> A x (diagnostics).
    after_xupdate(x) -> x, if given, replaces every x-update's output (loop_sensitivity).  Returns (x, diag [iters, 2], inner iterations [iters])."""
    x = np.array(x0, np.complex128)
    v, u = x.copy(), np.zeros_like(x)
    diag, li = np.full((iters, 2), np.nan), np.zeros(iters, np.int32)
    ny, ngt = np.linalg.norm(y), (np.linalg.norm(gt) if gt is not None else None)
    for it in range(iters):
        x, li[it] = xupdate(y, v - u, gamma, x)
        if after_xupdate is not None:
            x = after_xupdate(x)
        diag[it, 0] = np.linalg.norm(y - forward(x)) / ny
        if gt is not None:
            diag[it, 1] = np.linalg.norm(gt - x) / ngt
        v, u = denoiser_step(x, u, net, cpx, multi, noise_std, residual)
    return x, diag, li


# ---- the runs: one reference loop each --------------------------------------------------------------------------------------------------------------
def run_key(grid, mode, solver="lsqr", gamma=GAMMA, scale=1.0, rt="f16"):
    """rt: 'f16' (the f16 x 3 scheme keeps split_roundtrip of a value) or 'id' (conv_scheme=3, conv_f32=1 and the CPU oracle keep the fp32 value)."""
    return f"{grid}/{mode_id(mode)}/{solver}/g{gamma:g}/x{scale:g}/{rt}"


RUNS = {}


def _run(grid, mode, **kw):
    key = run_key(grid, mode, **kw)
    assert key not in RUNS
    RUNS[key] = dict(dict(solver="lsqr", gamma=GAMMA, scale=1.0, rt="f16"), key=key, grid=grid, mode=mode, **kw)


for _mode in MODES:                                                                # the mode grid, on every path
    for _sc in SCALES:
        _run(MODE_GRID, _mode, scale=_sc)
    _run(MODE_GRID, _mode, rt="id")
    _run(MODE_GRID, _mode, solver="direct")
for _sc in SCALES:                                                                 # gamma = 5 on one case per path: x close to z
    _run(MODE_GRID, (1, 1, 1), gamma=GAMMA_BIG, scale=_sc)
_run(MODE_GRID, (1, 1, 1), gamma=GAMMA_BIG, solver="direct")
for _g in SIDE_GRIDS + CHAN_GRIDS:
    for _mode in (EXTREME if _g in SIDE_GRIDS else [(1, 1, 1)]):
        for _solver in ("lsqr", "direct"):
            _run(_g, _mode, solver=_solver)


@functools.lru_cache(maxsize=None)
def _gram(grid):
    c = GR.inputs(grid)
    return GR.gram(c["V"], c["fp"], c["k"], c["N"] * c["M"])


def net_of(run):
    """(routes, weights blob, in_nc, out_nc) of a run: one routing per (grid, mode)."""
    c = GR.CASES[run["grid"]]
    cpx, multi, _ = run["mode"]
    in_nc, out_nc = channels(c["s"], cpx, multi)
    routes = routing(c["s"], cpx, multi, seed=c["seed"] + 17 * cpx + 5 * multi)
    return routes, routing_weights(routes, in_nc), in_nc, out_nc


def data(run):
    """What a run is given: dict(c: the grid's gridded_ref.inputs, y and gt (the grid's, times the run's scale), routes, w, in_nc, out_nc)."""
    c = GR.inputs(run["grid"])
    routes, w, in_nc, out_nc = net_of(run)
    return dict(run, c=c, y=c["y"] * run["scale"], gt=c["x"] * run["scale"], routes=routes, w=w, in_nc=in_nc, out_nc=out_nc)


def problem(run):
    """data(run) and the reference's functions: x0 = A^H y, xupdate, forward, net."""
    d = data(run)
    c, y, gt, routes, w, in_nc, out_nc = (d[n] for n in ("c", "y", "gt", "routes", "w", "in_nc", "out_nc"))
    V, fp, k, N, M = c["V"], c["fp"], c["k"], c["N"], c["M"]
    rt = CR.split_roundtrip if run["rt"] == "f16" else None
    if run["solver"] == "direct":
        G = _gram(run["grid"])
        xupdate = lambda y_, z, g, xp: (GR.minimiser(y_, z, g, V, fp, k, G=G), 0)
    else:
        op = GR.oracle_operator(run["grid"])

        def xupdate(y_, z, g, xp):
            x, it, fl, _ = op.lsqr(y_, z, g, TOL, MAXIT, xp)
            assert fl == 0
            return x, it
    return dict(run, c=c, y=y, gt=gt, x0=GR.adjoint(y, V, fp, k, N, M), xupdate=xupdate, forward=lambda x: GR.forward(x, V, fp, k),
                net=lambda n32: route(n32, routes, rt), routes=routes, w=w, in_nc=in_nc, out_nc=out_nc)


def _loop(p, after_xupdate=None):
    cpx, multi, res = p["mode"]
    return admm(p["y"], p["x0"], p["xupdate"], p["net"], p["forward"], ITERS, p["gamma"], bool(cpx), bool(multi), NOISE_STD, bool(res), p["gt"], after_xupdate)


@functools.lru_cache(maxsize=None)
def reference(key):
    """(x, diag, inner iterations) of a run, computed once per process and read-only."""
    out = _loop(problem(RUNS[key]))
    for a in out:
        a.setflags(write=False)
    return out


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def loop_sensitivity(key, trials=5):
    """How far the reference's own result moves when every x-update's output is perturbed by the project's bound on an x-update: (largest relative
    movement of the final x, largest relative movement of a diagnostic, the inner iteration counts stayed the same in every run)."""
    p = problem(RUNS[key])
    x0, d0, l0 = reference(key)
    rng = np.random.default_rng(GR.CASES[p["grid"]]["seed"] + 777)

    def jolt(x):
        return x.real * (1.0 + PERTURB * rng.standard_normal(x.shape)) + 1j * x.imag * (1.0 + PERTURB * rng.standard_normal(x.shape))

    mx, md, same = 0.0, 0.0, True
    for _ in range(trials):
        x, d, li = _loop(p, jolt)
        mx, md = max(mx, _rel(x, x0)), max(md, float(np.abs(d / d0 - 1.0).max()))
        same = same and np.array_equal(li, l0)
    return mx, md, same


# max(movement of x, movement of the diagnostics) per run, as loop_sensitivity measured it on the CPU (tests/test_admm_ref_host.py asserts every
# entry from above with a factor 2 of room, and that every bound() stays at or below 1e-6)
ADMM_SENS = {
    "glue32x32_s3/real_single/lsqr/g0.05/x1/f16": 3.4e-08, "glue32x32_s3/real_single/lsqr/g0.05/x1000/f16": 3.4e-08,
    "glue32x32_s3/real_single/lsqr/g0.05/x0.001/f16": 3.4e-08, "glue32x32_s3/real_single/lsqr/g0.05/x1/id": 2.0e-08,
    "glue32x32_s3/real_single/direct/g0.05/x1/f16": 3.0e-08, "glue32x32_s3/real_single_res/lsqr/g0.05/x1/f16": 6.6e-08,
    "glue32x32_s3/real_single_res/lsqr/g0.05/x1000/f16": 6.6e-08, "glue32x32_s3/real_single_res/lsqr/g0.05/x0.001/f16": 6.6e-08,
    "glue32x32_s3/real_single_res/lsqr/g0.05/x1/id": 4.7e-08, "glue32x32_s3/real_single_res/direct/g0.05/x1/f16": 3.4e-08,
    "glue32x32_s3/real_multi/lsqr/g0.05/x1/f16": 1.3e-08, "glue32x32_s3/real_multi/lsqr/g0.05/x1000/f16": 1.3e-08,
    "glue32x32_s3/real_multi/lsqr/g0.05/x0.001/f16": 1.3e-08, "glue32x32_s3/real_multi/lsqr/g0.05/x1/id": 5.2e-09,
    "glue32x32_s3/real_multi/direct/g0.05/x1/f16": 6.6e-09, "glue32x32_s3/real_multi_res/lsqr/g0.05/x1/f16": 2.1e-08,
    "glue32x32_s3/real_multi_res/lsqr/g0.05/x1000/f16": 2.1e-08, "glue32x32_s3/real_multi_res/lsqr/g0.05/x0.001/f16": 2.1e-08,
    "glue32x32_s3/real_multi_res/lsqr/g0.05/x1/id": 2.1e-08, "glue32x32_s3/real_multi_res/direct/g0.05/x1/f16": 2.9e-08,
    "glue32x32_s3/cpx_single/lsqr/g0.05/x1/f16": 1.7e-08, "glue32x32_s3/cpx_single/lsqr/g0.05/x1000/f16": 1.7e-08,
    "glue32x32_s3/cpx_single/lsqr/g0.05/x0.001/f16": 1.7e-08, "glue32x32_s3/cpx_single/lsqr/g0.05/x1/id": 1.1e-08,
    "glue32x32_s3/cpx_single/direct/g0.05/x1/f16": 1.0e-08, "glue32x32_s3/cpx_single_res/lsqr/g0.05/x1/f16": 2.2e-08,
    "glue32x32_s3/cpx_single_res/lsqr/g0.05/x1000/f16": 2.2e-08, "glue32x32_s3/cpx_single_res/lsqr/g0.05/x0.001/f16": 2.2e-08,
    "glue32x32_s3/cpx_single_res/lsqr/g0.05/x1/id": 2.1e-08, "glue32x32_s3/cpx_single_res/direct/g0.05/x1/f16": 1.4e-08,
    "glue32x32_s3/cpx_multi/lsqr/g0.05/x1/f16": 1.5e-08, "glue32x32_s3/cpx_multi/lsqr/g0.05/x1000/f16": 1.5e-08,
    "glue32x32_s3/cpx_multi/lsqr/g0.05/x0.001/f16": 1.5e-08, "glue32x32_s3/cpx_multi/lsqr/g0.05/x1/id": 1.2e-08,
    "glue32x32_s3/cpx_multi/direct/g0.05/x1/f16": 1.7e-08, "glue32x32_s3/cpx_multi_res/lsqr/g0.05/x1/f16": 2.7e-08,
    "glue32x32_s3/cpx_multi_res/lsqr/g0.05/x1000/f16": 2.7e-08, "glue32x32_s3/cpx_multi_res/lsqr/g0.05/x0.001/f16": 2.7e-08,
    "glue32x32_s3/cpx_multi_res/lsqr/g0.05/x1/id": 3.0e-08, "glue32x32_s3/cpx_multi_res/direct/g0.05/x1/f16": 2.3e-08,
    "glue32x32_s3/cpx_multi_res/lsqr/g5/x1/f16": 1.1e-08, "glue32x32_s3/cpx_multi_res/lsqr/g5/x1000/f16": 1.1e-08,
    "glue32x32_s3/cpx_multi_res/lsqr/g5/x0.001/f16": 1.1e-08, "glue32x32_s3/cpx_multi_res/direct/g5/x1/f16": 1.1e-08,
    "grid32x32/real_single/lsqr/g0.05/x1/f16": 6.2e-09, "grid32x32/real_single/direct/g0.05/x1/f16": 7.9e-09,
    "grid32x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.4e-08, "grid32x32/cpx_multi_res/direct/g0.05/x1/f16": 1.7e-08,
    "grid64x32/real_single/lsqr/g0.05/x1/f16": 6.5e-09, "grid64x32/real_single/direct/g0.05/x1/f16": 7.7e-09,
    "grid64x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.1e-08, "grid64x32/cpx_multi_res/direct/g0.05/x1/f16": 1.7e-08,
    "grid96x32/real_single/lsqr/g0.05/x1/f16": 4.0e-09, "grid96x32/real_single/direct/g0.05/x1/f16": 4.8e-09,
    "grid96x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.8e-08, "grid96x32/cpx_multi_res/direct/g0.05/x1/f16": 1.6e-08,
    "grid112x32/real_single/lsqr/g0.05/x1/f16": 7.0e-09, "grid112x32/real_single/direct/g0.05/x1/f16": 5.1e-09,
    "grid112x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.8e-08, "grid112x32/cpx_multi_res/direct/g0.05/x1/f16": 2.4e-08,
    "grid128x32/real_single/lsqr/g0.05/x1/f16": 6.6e-09, "grid128x32/real_single/direct/g0.05/x1/f16": 7.6e-09,
    "grid128x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.4e-08, "grid128x32/cpx_multi_res/direct/g0.05/x1/f16": 1.5e-08,
    "grid160x32/real_single/lsqr/g0.05/x1/f16": 4.1e-09, "grid160x32/real_single/direct/g0.05/x1/f16": 5.1e-09,
    "grid160x32/cpx_multi_res/lsqr/g0.05/x1/f16": 2.0e-08, "grid160x32/cpx_multi_res/direct/g0.05/x1/f16": 1.8e-08,
    "grid192x32/real_single/lsqr/g0.05/x1/f16": 5.7e-09, "grid192x32/real_single/direct/g0.05/x1/f16": 5.5e-09,
    "grid192x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.8e-08, "grid192x32/cpx_multi_res/direct/g0.05/x1/f16": 1.5e-08,
    "grid224x32/real_single/lsqr/g0.05/x1/f16": 6.7e-09, "grid224x32/real_single/direct/g0.05/x1/f16": 5.1e-09,
    "grid224x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.9e-08, "grid224x32/cpx_multi_res/direct/g0.05/x1/f16": 1.7e-08,
    "grid256x32/real_single/lsqr/g0.05/x1/f16": 4.9e-09, "grid256x32/real_single/direct/g0.05/x1/f16": 4.6e-09,
    "grid256x32/cpx_multi_res/lsqr/g0.05/x1/f16": 1.3e-08, "grid256x32/cpx_multi_res/direct/g0.05/x1/f16": 1.5e-08,
    "grid32x96/real_single/lsqr/g0.05/x1/f16": 5.5e-09, "grid32x96/real_single/direct/g0.05/x1/f16": 4.8e-09,
    "grid32x96/cpx_multi_res/lsqr/g0.05/x1/f16": 1.3e-08, "grid32x96/cpx_multi_res/direct/g0.05/x1/f16": 1.3e-08,
    "grid32x256/real_single/lsqr/g0.05/x1/f16": 4.7e-09, "grid32x256/real_single/direct/g0.05/x1/f16": 5.1e-09,
    "grid32x256/cpx_multi_res/lsqr/g0.05/x1/f16": 1.5e-08, "grid32x256/cpx_multi_res/direct/g0.05/x1/f16": 1.6e-08,
    "grid256x256/real_single/lsqr/g0.05/x1/f16": 4.6e-09, "grid256x256/real_single/direct/g0.05/x1/f16": 4.7e-09,
    "grid256x256/cpx_multi_res/lsqr/g0.05/x1/f16": 1.4e-08, "grid256x256/cpx_multi_res/direct/g0.05/x1/f16": 1.2e-08,
    "chan1/cpx_multi_res/lsqr/g0.05/x1/f16": 1.7e-08, "chan1/cpx_multi_res/direct/g0.05/x1/f16": 9.7e-09,
    "chan2/cpx_multi_res/lsqr/g0.05/x1/f16": 2.3e-08, "chan2/cpx_multi_res/direct/g0.05/x1/f16": 2.0e-08,
    "chan7/cpx_multi_res/lsqr/g0.05/x1/f16": 1.5e-08, "chan7/cpx_multi_res/direct/g0.05/x1/f16": 1.5e-08,
}


def bound(key):
    return max(1e-9, 3.0 * ADMM_SENS[key])
