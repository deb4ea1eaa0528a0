"""GPU: density compensation of a trajectory operator (qmri_nufft_dcf and the weighted adjoints) against the numpy
restatement of tests/dcf_ref.py and the exact non-uniform DFT of tests/nufft_ref.py.  This file runs 32 x 32 and 64 x 96 at widths 6 and 12 with
s = 1 and 3; every width 2 ... 16, the grids 160 x 192, 256 x 112 and 112 x 128 (split tiles) and the weighted adjoint at every s = 1 ... 10 are in
tests/test_gpu_traj_grids.py, held to this file's WEIGHTS_RTOL."""
import ctypes as C

import numpy as np
import pytest

import dcf_ref as D
import nufft_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

# weights against the restatement, relative, both sides fp64: ten times the largest value measured on an MI355X over every comparison of this
# file, 7.96e-14 (the split-tile spiral of test_split_tiles; the weights-against-the-reference shapes reach 3.74e-14)
WEIGHTS_RTOL = 8e-13


def _cx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _max_rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.fixture(scope="module")
def spiral32():
    N, S, T = 32, 60, 48
    fp, om = R.spiral_traj(N, S, T)
    return N, T, fp, om


@pytest.fixture(scope="module")
def ref_w6(spiral32):
    """the reference's weights on the 32 x 32 spiral at width 6, 20 iterations: computed once, shared, never changed."""
    N, T, fp, om = spiral32
    w, info = D.weights(N, N, T, om, 6, 20)
    w.setflags(write=False)
    return w, info


@pytest.mark.parametrize("N,M,S,T,width", [(32, 32, 60, 48, 6), (32, 32, 60, 48, 12), (64, 96, 100, 24, 0)])
def test_weights_against_the_reference(engine_mod, N, M, S, T, width):
    fp, om = R.spiral_traj(N, S, T)                                    # (omega in radians per pixel: the same spiral on a rectangular grid)
    V = np.full((T, 1), 1 / np.sqrt(T))
    e = engine_mod.Engine(0)
    e.set_trajectory(N, M, V, fp, om, width=width)
    plan = D.Plan(N, M, om, width)
    kap = D.kappa(T, plan.width, plan.beta)
    worst = 0.0
    for niter in (1, 5, 20):
        w, info = e.density_weights(niter=niter)
        wr, it, dev, _ = D.iterate(plan, niter)
        err = _max_rel(w, kap * wr)
        worst = max(worst, err)
        print(f"{N} x {M} width {plan.width} niter {niter}: max relative difference {err:.3e}, dev {info['dev']:.6e} (reference {dev:.6e})")
        assert w.shape == (S * T,) and np.all(np.isfinite(w)) and np.all(w > 0)
        assert info["iters"] == it == niter and info["clamped"] == 0
        assert abs(info["dev"] - dev) <= 1e-10 * dev
        assert err <= WEIGHTS_RTOL, (niter, err)
    w0, info0 = e.density_weights()                                    # niter = 0: the default, 20
    assert info0["iters"] == 20 and np.array_equal(w0, w)
    e.close()
    print("largest:", worst)


def test_early_stop_and_repeatability(engine_mod, spiral32):
    N, T, fp, om = spiral32
    plan = D.Plan(N, N, om, 6)
    _, _, _, devs = D.iterate(plan, 20)
    tol = 0.5 * (devs[5] + devs[6])                                    # the reference crosses it at iteration 7
    wr, it, dev, _ = D.iterate(plan, 20, tol)
    assert it == 7
    e = engine_mod.Engine(0)
    e.set_trajectory(N, N, np.full((T, 1), 1 / np.sqrt(T)), fp, om, width=6)
    w, info = e.density_weights(niter=20, tol=tol)
    assert info["iters"] == 7 and abs(info["dev"] - dev) <= 1e-10 * dev
    err = _max_rel(w, D.kappa(T, 6, plan.beta) * wr)
    print(f"early stop at iteration 7: max relative difference {err:.3e}")
    assert err <= WEIGHTS_RTOL
    w7, _ = e.density_weights(niter=7)
    assert np.array_equal(w, w7)                                       # the iterations after the stop changed nothing
    wa, ia = e.density_weights(niter=20)
    wb, ib = e.density_weights(niter=20)
    assert np.array_equal(wa, wb) and ia == ib and ia["iters"] == 20
    e.close()


def test_split_tiles(engine_mod):
    """S = 100, T = 48 at 32 x 32: the tiles at the centre of k-space hold more samples than one spreading segment, so the weights go through
    the partial tiles and k_dcf_reduce.  The plan's own count of split tiles (nred) comes back in info["split_tiles"]."""
    N, S, T = 32, 100, 48
    fp, om = R.spiral_traj(N, S, T)
    plan = D.Plan(N, N, om, 6)
    e = engine_mod.Engine(0)
    e.set_trajectory(N, N, np.full((T, 1), 1 / np.sqrt(T)), fp, om, width=6)
    w, info = e.density_weights(niter=5)
    wr, _, dev, _ = D.iterate(plan, 5)
    e.close()
    err = _max_rel(w, D.kappa(T, 6, plan.beta) * wr)
    print(f"split tiles in the plan: {info['split_tiles']}; max relative difference {err:.3e}")
    assert info["split_tiles"] > 0
    assert info["iters"] == 5 and abs(info["dev"] - dev) <= 1e-10 * dev
    assert err <= WEIGHTS_RTOL


def test_wrap_around_and_duplicates(engine_mod):
    N, M, T = 32, 32, 6
    rng = np.random.default_rng(3)
    per = 40
    om = rng.uniform(-np.pi, np.pi, (T * per, 2))
    om[:8] = [[np.pi, np.pi], [-np.pi, -np.pi], [np.pi, -np.pi], [-np.pi, np.pi], [np.pi, 0.3], [-0.2, -np.pi], [-np.pi, 1e-9], [1e-12, np.pi]]
    fp = np.arange(T + 1, dtype=np.int32) * per
    V = np.full((T, 1), 1 / np.sqrt(T))
    e = engine_mod.Engine(0)
    for width in (6, 0):
        e.set_trajectory(N, M, V, fp, om, width=width)
        w, info = e.density_weights(niter=5)
        wr, inf = D.weights(N, M, T, om, width, 5)
        err = _max_rel(w, wr)
        print(f"wrap-around, width {width}: max relative difference {err:.3e}")
        assert err <= WEIGHTS_RTOL and abs(info["dev"] - inf["dev"]) <= 1e-10 * inf["dev"], width
        assert _max_rel(w[:4], np.full(4, w[0])) <= 1e-12              # the four corners of [-pi, pi]^2 are one point of the periodic grid
    # the same point in every frame: 1 / T of the weight of the single point
    p = np.array([[0.7, -1.1]])
    e.set_trajectory(N, M, V[:1] * np.sqrt(T), np.array([0, 1], np.int32), p, width=6)
    w1, _ = e.density_weights(niter=3)
    e.set_trajectory(N, M, V, np.arange(T + 1, dtype=np.int32), np.repeat(p, T, axis=0), width=6)
    wT, _ = e.density_weights(niter=3)
    e.close()
    k1, kT = D.kappa(1, 6, D.plan_beta(6)), D.kappa(T, 6, D.plan_beta(6))       # (kappa carries the factor T: compare the unscaled weights)
    assert _max_rel(wT / kT, np.full(T, (w1[0] / k1) / T)) <= 1e-12, (wT, w1)


def test_weighted_adjoint(engine_mod, spiral32, ref_w6):
    N, T, fp, om = spiral32
    s = 3
    rng = np.random.default_rng(5)
    V = rng.standard_normal((T, s))
    y = _cx(rng, om.shape[0])
    w = ref_w6[0]
    e = engine_mod.Engine(0)
    e.set_trajectory(N, N, V, fp, om, width=6, max_batch=3)
    e.set_sample_weights(w)
    xw = e.adjoint(y, weighted=True)
    # the NUFFT tolerance of the existing adjoint test at this width (tests/test_gpu_nufft.py: 10^(2 - w))
    assert rel_err(xw, R.nudft_adjoint(w * y, om, V, fp, N, N)) <= 10.0 ** (2 - 6)
    # the multiply is fused where y is staged, BEFORE the phase: (w yr, w yi) is what numpy forms, so the bits are those of adjoint(w .* y)
    wy = w * y.real + 1j * (w * y.imag)
    assert np.array_equal(xw, e.adjoint(wy))
    # device arrays, batch 3 at max_batch 3: each slice the bits it has alone
    hip = engine_mod._hip_runtime()
    m, n = om.shape[0], N * N * s
    ys = [y, y[::-1].copy(), 1j * y]
    yb = np.concatenate(ys)
    d_y, d_x = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_y), 3 * m * 16) == 0 and hip.hipMalloc(C.byref(d_x), 3 * n * 16) == 0
    try:
        assert hip.hipMemcpy(d_y, yb.ctypes.data, yb.nbytes, 1) == 0
        e._check(e.L.qmri_adjoint_w_dev(e.h, d_y, d_x, 3))
        e.synchronize()
        xd = np.empty(3 * n, np.complex128)
        assert hip.hipMemcpy(xd.ctypes.data, d_x, xd.nbytes, 2) == 0
    finally:
        hip.hipFree(d_y); hip.hipFree(d_x)
    for b in range(3):
        assert np.array_equal(xd[b * n:(b + 1) * n].reshape((N, N, s), order="F"), e.adjoint(ys[b], weighted=True)), b
    # three coils against the sum formed in numpy
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, N), indexing="ij")
    maps = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww)) for a in (0.0, 2.1, 4.2)], axis=2)
    e.set_coils(maps)
    ymc = np.stack(ys, axis=1)
    want = sum(np.conj(maps[:, :, j])[:, :, None] * e.adjoint(ys[j], weighted=True) for j in range(3))
    assert rel_err(e.adjoint_mc(ymc, weighted=True), want) <= 1e-14
    # clearing the weights: the _w calls are refused again (QMRI_ERR_STATE), the plain adjoint is untouched
    e.set_sample_weights(None)
    with pytest.raises(engine_mod.QmriError) as err:
        e.adjoint(y, weighted=True)
    assert err.value.code == -2 and "no sample weights attached" in str(err.value)
    # replacing the operator drops the weights
    e.set_sample_weights(w)
    e.set_trajectory(N, N, V, fp, om, width=6)
    with pytest.raises(engine_mod.QmriError) as err:
        e.adjoint(y, weighted=True)
    assert err.value.code == -2
    e.set_operator(N, N, V, *engine_mod.build_spiral(N, 60, T))
    for call in (lambda: e.density_weights(), lambda: e.set_sample_weights(np.ones(e.m)), lambda: e.adjoint(np.zeros(e.m, np.complex128), weighted=True)):
        with pytest.raises(engine_mod.QmriError) as err:
            call()
        assert err.value.code == -4
    e.close()


def test_nothing_else_moved(engine_mod, synth, spiral32, ref_w6):
    """adjoint, xupdate (lsqr and toeplitz), adjoint_mc and pnp_admm for 2 iterations: the same bits with and without weights attached."""
    N, T, fp, om = spiral32
    s = 3
    rng = np.random.default_rng(6)
    V = np.linalg.qr(rng.standard_normal((T, s)))[0]
    y, z = _cx(rng, om.shape[0]), _cx(rng, N, N, s)
    nc = (8, 16, 16, 32)
    wn = synth.structured_weights(in_nc=s, out_nc=s, nc=nc, nb=2, seed=3, eps=0.05)
    maps = np.stack([np.ones((N, N)), 1j * np.ones((N, N))], axis=2) / np.sqrt(2)
    ymc = np.stack([y, y[::-1]], axis=1)

    def run(attach):
        e = engine_mod.Engine(0)
        e.set_trajectory(N, N, V, fp, om, width=6)
        e.set_denoiser(wn, N, N, in_nc=s, out_nc=s, nc=nc, nb=2)
        e.set_coils(maps)
        if attach:
            e.set_sample_weights(ref_w6[0])
        out = [e.adjoint(y), e.xupdate(y, z, 0.05)[0], e.xupdate(y, z, 0.05, solver="toeplitz")[0], e.adjoint_mc(ymc), e.pnp_admm(y, iters=2)[0]]
        e.close()
        return out

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


def test_the_weighted_adjoint_is_a_gridding_reconstruction(engine_mod, spiral32):
    """The reason for the feature.  The 32 x 32 phantom, s = 3 with a random orthonormal V, y = forward(x), width 6, the default 20 iterations:
    the weighted adjoint WITHOUT any rescale is at most half as far from x as the bare adjoint after the best possible scalar rescale, and its scale
    c = <x, A^H W y> / <x, x> (the least-squares fit of A^H W y by c x) is within 0.02 of 1.  "The best-fit scalar of adjoint_w(y) onto x" is
    read here as this c, the transfer scale that kappa sets; the other regression, alpha = argmin ||alpha A^H W y - x||, has the aliasing energy
    of the s = 3 channels in its denominator and is 0.949 on the CPU: it measures noise, not scale (DESIGN.md section 21 says so too).
    The same conditions on the CPU with the restatement's weights and the exact NUDFT, forward and adjoint, at the plan's beta (width 6):
    0.231 against 0.651, c = 1.0002 (s = 1: 0.031 against 0.651, c = 1.0006).  MI355X: 0.2311 against 0.6506, c = 1.00024.  At the default width 12 the iteration converges more slowly and 20 iterations leave c = 1.024
    (100 iterations: 1.006) -- DESIGN.md section 21; the width here is the issue's."""
    N, T, fp, om = spiral32
    s = 3
    V = np.linalg.qr(np.random.default_rng(0).standard_normal((T, s)))[0]
    x = np.stack([D.phantom(N) * (1 + 0.3 * c) for c in range(s)], axis=2).astype(np.complex128)
    e = engine_mod.Engine(0)
    e.set_trajectory(N, N, V, fp, om, width=6)
    y = e.forward(x)
    e.density_weights()
    aw, a = e.adjoint(y, weighted=True), e.adjoint(y)
    e.close()
    err_w, err_bare = rel_err(aw, x), D.best_fit(a, x)[1]
    c = (np.vdot(x, aw) / np.vdot(x, x)).real
    print(f"weighted adjoint, no rescale: {err_w:.4f}; bare adjoint, best rescale: {err_bare:.4f}; scale of the weighted adjoint: {c:.5f}")
    assert err_w <= 0.5 * err_bare, (err_w, err_bare)
    assert abs(c - 1.0) <= 0.02, c


def test_pnp_admm_starts_from_the_weighted_adjoint(engine_mod, synth, spiral32):
    N, T, fp, om = spiral32
    s = 3
    V = np.linalg.qr(np.random.default_rng(1).standard_normal((T, s)))[0]
    nc = (8, 16, 16, 32)
    wn = synth.structured_weights(in_nc=s, out_nc=s, nc=nc, nb=2, seed=3, eps=0.05)
    y = _cx(np.random.default_rng(2), om.shape[0])
    e = engine_mod.Engine(0)
    e.set_trajectory(N, N, V, fp, om, width=6)
    e.set_denoiser(wn, N, N, in_nc=s, out_nc=s, nc=nc, nb=2)
    e.density_weights()
    x1, _, l1 = e.pnp_admm(y, iters=2, x0="dcf")
    x2, _, l2 = e.pnp_admm(y, iters=2, x0=e.adjoint(y, weighted=True))
    assert np.array_equal(x1, x2) and np.array_equal(l1, l2)
    e.set_coils(np.ones((N, N, 1)))
    x3, l3 = e.pnp_admm_mc(y[:, None], iters=2, x0="dcf")
    x4, l4 = e.pnp_admm_mc(y[:, None], iters=2, x0=e.adjoint_mc(y[:, None], weighted=True))
    assert np.array_equal(x3, x4) and np.array_equal(l3, l4)
    e.close()


def test_harness_density_compensation(engine_mod, synth):
    """recon_tsmis(..., "SpiralExact", recon_method="SVD_MRF", density_compensation=True) at 32 x 32 beats the same call with False on the masked
    TSMI error; False gives the bits of the path without the option.  The same two reconstructions with the restatement's weights and the exact
    NUDFT on the CPU (default width 12, 20 iterations): masked error 3.62 bare against 0.45 density-compensated."""
    from qmri_pnp_recon_poc_amd import harness as H, reference_api as RA
    N, T, s, S = 32, 48, 3, 60
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    q = synth.make_phantom_qmaps(N, seed=4)
    X0 = synth.synthesize_tsmi(q, dic)
    kw = dict(recon_method="SVD_MRF", subsampling_pattern="SpiralExact", spiral_sampling_curve=S, seed=7)
    try:
        r0 = H.recon_tsmis(dic, X0, np.asarray(q), **kw)
        rf = H.recon_tsmis(dic, X0, np.asarray(q), density_compensation=False, **kw)
        r1 = H.recon_tsmis(dic, X0, np.asarray(q), density_compensation=True, **kw)
        fp, om = engine_mod.build_spiral_traj(N, S, T)
        e = engine_mod.Engine(0)
        e.set_trajectory(N, N, dic["V"], fp, om)
        xa = e.adjoint(r0["Y"])
        e.close()
    finally:
        RA.release()
    assert np.array_equal(r0["X"], xa) and np.array_equal(rf["X"], r0["X"]) and np.array_equal(r1["Y"], r0["Y"])
    mask = r0["foreground_mask"] > 0
    errs = [float(np.linalg.norm((r["X"] - X0)[mask]) / np.linalg.norm(X0[mask])) for r in (r0, r1)]
    print("masked TSMI error, bare / density-compensated adjoint:", errs)
    assert errs[1] < errs[0], errs


def test_reference_api_and_harness_start_pnp_admm_from_the_weighted_adjoint(engine_mod, synth):
    """param["x0"] = "dcf" of reference_api.PnP_ADMM and recon_tsmis(..., recon_method="PnP_ADMM", density_compensation=True): the bits of the
    engine's own pnp_admm started from adjoint(y, weighted=True).  Weights the caller attached are used as they are; an operator without any
    gets density_weights()."""
    from qmri_pnp_recon_poc_amd import harness as H, reference_api as RA
    N, T, s, S = 32, 48, 3, 60
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    q = synth.make_phantom_qmaps(N, seed=4)
    X0 = synth.synthesize_tsmi(q, dic)
    netc = (8, 16, 16, 32)
    wn = synth.structured_weights(in_nc=s, out_nc=s, nc=netc, nb=2, seed=3, eps=0.05)
    fp, om = engine_mod.build_spiral_traj(N, S, T)
    try:
        r = H.recon_tsmis(dic, X0, np.asarray(q), weights=wn, recon_method="PnP_ADMM", subsampling_pattern="SpiralExact", spiral_sampling_curve=S,
                          iters=2, seed=7, net_arch={"nc": netc, "nb": 2}, density_compensation=True)
        y = r["Y"]
        F = RA.make_F(RA.setup_subsampling_spiral_exact(N, N, S, np.asarray(dic["V"], dtype=np.float64)))
        net = RA.make_net(wn, "single_level", False, H=N, W=N, out_nc=s, nc=netc, nb=2)
        param = {"gamma": 1 / 20, "iter": 2, "cg_tol": 1e-4, "F": F, "net": net, "denoiser_type": "single_level", "noise_map": None, "x0": "dcf"}
        xa = RA.PnP_ADMM(y, param)                                     # nothing attached: the Pipe-Menon weights
        own = np.linspace(0.5, 2.0, y.size)
        F._engine.set_sample_weights(own)
        xo = RA.PnP_ADMM(y, param)                                     # the caller's own weights are not overwritten
    finally:
        RA.release()
    e = engine_mod.Engine(0)
    e.set_trajectory(N, N, dic["V"], fp, om)
    e.set_denoiser(wn, N, N, in_nc=s, out_nc=s, nc=netc, nb=2)
    e.density_weights()
    xe, _, _ = e.pnp_admm(y, iters=2, gamma=1 / 20, x0=e.adjoint(y, weighted=True))
    e.set_sample_weights(own)
    xeo, _, _ = e.pnp_admm(y, iters=2, gamma=1 / 20, x0="dcf")
    e.close()
    assert np.array_equal(r["X"], xe) and np.array_equal(xa, xe)
    assert np.array_equal(xo, xeo) and not np.array_equal(xo, xa)
