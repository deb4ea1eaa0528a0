"""GPU parity on the grids beyond the four square sizes: N, M in {32, 64, 96, 112, 128, 160, 192, 224, 256}, chosen independently
(N: h axis, contiguous; M: w axis).  Every FFT kernel runs on the plan of its own axis.  Operator, LSQR x-update, denoiser, PnP-ADMM,
batches, LRTV and the multi-coil extension against the CPU oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECT = [(256, 256), (96, 160), (160, 96), (112, 224), (192, 256), (256, 32)]
QMRI_ERR_UNSUPPORTED = -4
NC = (64, 64, 64, 64)                  # (nc[0] = 64: the resident-tile form applies at the full-resolution level)


def _V(T, s=10, seed=0):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((T, s)))[0]


def _user_mask(N, M, T, per_frame, seed):
    """A caller-supplied (frame_ptr, kidx): random distinct k locations per frame, 0-based column-major."""
    rng = np.random.default_rng(seed)
    ks = [np.sort(rng.choice(N * M, per_frame, replace=False)) for _ in range(T)]
    fp = np.concatenate([[0], np.cumsum([len(k) for k in ks])]).astype(np.int32)
    return fp, np.concatenate(ks).astype(np.int32)


def _phantom(synth, dic, N, M, seed=0):
    """A brain-like N x M TSMI: the centre crop of the square phantom of side max(N, M)."""
    L = max(N, M)
    X = synth.synthesize_tsmi(synth.make_phantom_qmaps(L, seed=seed), dic)
    h0, w0 = (L - N) // 2, (L - M) // 2
    return np.ascontiguousarray(X[h0:h0 + N, w0:w0 + M])


def _check_operator(e, op, N, M, s, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, M, s)) + 1j * rng.standard_normal((N, M, s))
    y = rng.standard_normal(e.m) + 1j * rng.standard_normal(e.m)
    yg, xg = e.forward(x), e.adjoint(y)
    assert rel_err(yg, op.forward(x)) < 1e-12, (N, M)
    assert rel_err(xg, op.adjoint(y)) < 1e-12, (N, M)
    lhs, rhs = np.vdot(y, yg), np.vdot(xg, x)
    assert abs(lhs - rhs) / abs(lhs) < 1e-12, (N, M)
    xr = rng.standard_normal((N, M, s))                             # real input (F.forward(double(X0)))
    assert rel_err(e.forward(xr), op.forward(xr)) < 1e-12
    # single-precision entry points: fp64 inside, rounded to single once on the way out
    x32 = x.astype(np.complex64)
    y32 = e.forward(x32)
    assert y32.dtype == np.complex64 and rel_err(y32, op.forward(x32.astype(np.complex128))) < 1e-6
    return x, y


@pytest.mark.parametrize("N,M", RECT, ids=[f"{n}x{m}" for n, m in RECT])
@pytest.mark.parametrize("mask", ["epi", "user"])
def test_operator_and_lsqr_on_new_grids(engine_mod, oracle, N, M, mask):
    """Forward / adjoint to 1e-12, adjointness to 1e-12, the _f32 entry points, and the LSQR x-update with the oracle's iteration count and
    flag, x to 1e-10 (EPI masks as the builder makes them and a random caller-supplied mask).  Fails with QMRI_ERR_UNSUPPORTED before the
    per-axis plans."""
    s, T = 10, 100
    V = _V(T, s, seed=N + M)
    if mask == "epi":
        fp, k = oracle.epi_mask(N, M, 1 / 8, T)
        fg, kg = engine_mod.build_epi(N, M, 1 / 8, T)
        assert np.array_equal(fp, fg) and np.array_equal(k, kg)
    else:
        fp, k = _user_mask(N, M, T, N * M // 40, seed=N * 1000 + M)
    op = oracle.Operator(N, M, V, fp, k)
    e = engine_mod.Engine(0)
    e.set_operator(N, M, V, fp, k)
    assert (e.N, e.M, e.m) == (N, M, op.m)
    x, y = _check_operator(e, op, N, M, s, seed=N + 7 * M)
    yy = op.forward(x) + 0.01 * y
    x0 = op.adjoint(yy)
    z = 0.9 * x0
    xg, ig, flg = e.xupdate(yy, z, 0.05, 1e-4, 100, x0=x0)
    xo, io, flo, _ = op.lsqr(yy, z, 0.05, tol=1e-4, maxit=100, x0=x0)
    assert (ig, flg) == (io, flo), (N, M, ig, io)
    assert rel_err(xg, xo) < 1e-10
    e.close()


@pytest.mark.parametrize("N", [96, 256])
def test_spiral_operator_on_new_sides(engine_mod, oracle, N):
    """The square spiral at the new sides: the builder equals the oracle's; operator to 1e-12."""
    T, S = 100, 771
    fp, k = oracle.spiral_mask(N, S, T)
    fg, kg = engine_mod.build_spiral(N, S, T)
    assert np.array_equal(fp, fg) and np.array_equal(k, kg)
    V = _V(T)
    op = oracle.Operator(N, N, V, fp, k)
    e = engine_mod.Engine(0)
    e.set_operator(N, N, V, fp, k)
    _check_operator(e, op, N, N, 10, seed=N)
    e.close()


@pytest.mark.parametrize("case", ["spiral256_T200", "spiral256_T1000", "epi192x256"])
def test_lsqr_one_launch_equals_two_launch_on_new_grids(engine_mod, oracle, case):
    """At 256 x 256 (spiral cut3 and T = 1000) and at a rectangular EPI grid the planner still cuts work units; the one-launch LSQR
    iteration (where it is planned) and the two-launch iteration give the same bits, count and flag, both equal to the oracle's count,
    and the health record says which form is armed."""
    rng = np.random.default_rng(3)
    if case.startswith("spiral"):
        N = M = 256
        T = 1000 if case.endswith("T1000") else 200
        fp, k = oracle.spiral_mask(N, 771, T)
    else:
        N, M, T = 192, 256, 200
        fp, k = oracle.epi_mask(N, M, 1 / 65, T)
    V = _V(T, seed=T)
    op = oracle.Operator(N, M, V, fp, k)
    y = op.forward(rng.standard_normal((N, M, 10))) + 0.01 * (rng.standard_normal(op.m) + 1j * rng.standard_normal(op.m))
    e = engine_mod.Engine(0)
    e.set_operator(N, M, V, fp, k)
    x0 = op.adjoint(y)
    z = x0 + 0.1 * (rng.standard_normal(x0.shape) + 1j * rng.standard_normal(x0.shape))
    e.lsqr_persist(True)
    xa, ita, fla = e.xupdate(y, z, 0.05, 1e-4, 100, x0, solver="lsqr")
    assert e.health()["lsqr_one_launch"] == "armed"
    e.lsqr_persist(False)
    xb, itb, flb = e.xupdate(y, z, 0.05, 1e-4, 100, x0, solver="lsqr")
    assert e.health()["lsqr_one_launch"] == "off"
    assert (ita, fla) == (itb, flb) and np.array_equal(xa, xb), (case, ita, itb, rel_err(xa, xb))
    xo, ito, flo, _ = op.lsqr(y, z, 0.05, 1e-4, 100, x0)
    assert (ita, fla) == (ito, flo) and rel_err(xa, xo) < 1e-10
    e.close()


@pytest.mark.parametrize("hw", [(256, 256), (96, 160)], ids=["256x256", "96x160"])
def test_denoiser_forms_on_new_grids(engine_mod, oracle, synth, hw):
    """The denoiser at the new levels (256: 256/128/64/32; 96 x 160: H != W at every level) against oracle.Net to 2e-5: one launch per
    layer, the resident-tile form (same bits as one launch per layer), and a batch of three through the persistent form."""
    H, W = hw
    w = synth.structured_weights(in_nc=10, out_nc=10, nc=NC, nb=1, seed=5, eps=0.05)
    net = oracle.Net(w, in_nc=10, out_nc=10, nc=NC, nb=1)
    xs = synth.uniform01(H + W, H * W * 10 * 3).reshape(H, W, 10, 3)
    yo = [net.denoise(xs[..., b]) for b in range(3)]
    e = engine_mod.Engine(0)
    e.set_denoiser(w, H, W, in_nc=10, out_nc=10, nc=NC, nb=1, max_batch=3)
    e.conv_resident(0)
    y1 = e.denoise(xs[..., 0])
    assert rel_err(y1, yo[0]) < 2e-5
    e.conv_resident(1)
    y2 = e.denoise(xs[..., 0])
    assert np.array_equal(y1, y2)
    yb = e.denoise(xs)
    for b in range(3):
        assert rel_err(yb[..., b], yo[b]) < 2e-5, (hw, b)
    assert e.denoiser_scheme() == (2, 0)
    e.close()


@pytest.mark.parametrize("knobs", ["conv_splitk=0", "conv_scheme=3"], ids=["no_splitK", "bf16x6"])
def test_denoiser_other_forms_on_a_rectangular_grid(oracle, synth, knobs):
    """Split-K off and the bf16 x 6 scheme (QMRI_DEBUG knobs, read when the plan is made: own process) at 96 x 160, against the oracle."""
    H, W = 96, 160
    w = synth.structured_weights(in_nc=10, out_nc=10, nc=NC, nb=1, seed=5, eps=0.05)
    x = synth.uniform01(7, H * W * 10).reshape(H, W, 10)
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from qmri_pnp_recon_poc_amd import engine as E\n"
        "w, x = np.load(sys.argv[1]), np.load(sys.argv[2])\n"
        "e = E.Engine(0)\n"
        "e.set_denoiser(w, %d, %d, in_nc=10, out_nc=10, nc=%r, nb=1)\n"
        "np.save(sys.argv[3], e.denoise(x))\n"
    ) % (ROOT, H, W, NC)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        pw, px, py = (os.path.join(d, f) for f in ("w.npy", "x.npy", "y.npy"))
        np.save(pw, w)
        np.save(px, x)
        r = subprocess.run([sys.executable, "-c", code, pw, px, py], capture_output=True, text=True,
                           env=dict(os.environ, QMRI_DEBUG=knobs), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        y = np.load(py)
    assert rel_err(y, oracle.Net(w, in_nc=10, out_nc=10, nc=NC, nb=1).denoise(x)) < 2e-5


@pytest.mark.parametrize("case", ["spiral256", "epi192x256"])
def test_pnp_admm_on_new_grids(engine_mod, oracle, synth, case):
    """10 PnP-ADMM iterations against oracle.pnp_admm: LSQR counts identical, x to 1e-5; the dictionary match on the result is bit-equal
    to oracle.dict_match.  The fused step k_dual_fwd_h reads the denoiser's padded output with H != W at 192 x 256."""
    if case == "spiral256":
        N = M = 256
    else:
        N, M = 192, 256
    T, s = 200, 10
    dic = synth.make_dictionary(T=T, n_t1=32, n_t2=16, s=s)
    fp, k = oracle.spiral_mask(N, 771, T) if N == M else oracle.epi_mask(N, M, 1 / 65, T)
    op = oracle.Operator(N, M, dic["V"], fp, k)
    y = synth.awgn_measured(op.forward(_phantom(synth, dic, N, M)), 30.0, seed=1)
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=NC, nb=1, seed=2, eps=0.05)
    e = engine_mod.Engine(0)
    e.set_operator(N, M, dic["V"], fp, k)
    e.set_denoiser(w, N, M, in_nc=s, out_nc=s, nc=NC, nb=1)
    e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
    xg, _, lg = e.pnp_admm(y, iters=10)
    xo, _, lo = oracle.pnp_admm(op, oracle.Net(w, in_nc=s, out_nc=s, nc=NC, nb=1), y, iters=10)
    err = rel_err(xg, xo)
    print(f"{case}: lsqr gpu {lg.tolist()} oracle {lo.tolist()}, rel_err {err:.2e}")
    assert np.array_equal(lg, lo) and err < 1e-5
    mg = e.dict_match(xg)
    mx = oracle.dict_match(xg, dic["D"], dic["normD"], dic["lut"])
    assert np.array_equal(mg["qmap"], mx["qmap"]) and np.array_equal(mg["pd"], mx["pd"])
    e.close()


def test_batches_on_a_rectangular_grid(engine_mod, oracle, synth):
    """192 x 256 EPI: pnp_admm_batch over 3 slices is bit-equal to one slice at a time, and qmri_recon_batch with two workers on one
    device gives the same bits and dictionary maps bit-equal to oracle.dict_match."""
    from qmri_pnp_recon_poc_amd import batch
    N, M, T, s, iters = 192, 256, 200, 10, 3
    dic = synth.make_dictionary(T=T, n_t1=32, n_t2=16, s=s)
    fp, k = oracle.epi_mask(N, M, 1 / 65, T)
    op = oracle.Operator(N, M, dic["V"], fp, k)
    ys = np.stack([synth.awgn_measured(op.forward(_phantom(synth, dic, N, M, seed=sl)), 30.0, seed=sl) for sl in range(3)])
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=NC, nb=1, seed=2, eps=0.05)
    e = engine_mod.Engine(0)
    e.set_operator(N, M, dic["V"], fp, k, max_batch=3)
    e.set_denoiser(w, N, M, in_nc=s, out_nc=s, nc=NC, nb=1, max_batch=3)
    Xb, lb = e.pnp_admm_batch(ys, slices_per_launch=3, iters=iters)
    for sl in range(3):
        x1, _, l1 = e.pnp_admm(ys[sl], iters=iters)
        assert np.array_equal(Xb[sl], x1) and np.array_equal(lb[sl], l1), sl
    e.close()
    res = batch.recon_batch([0, 0], ys, N=N, M=M, V=dic["V"], frame_ptr=fp, kidx=k, weights=w, in_nc=s, out_nc=s, nc=NC, nb=1,
                            dictionary=dic, iters=iters, slices_per_launch=1)
    for sl in range(3):
        assert np.array_equal(res["X"][sl], Xb[sl]), sl
        o = oracle.dict_match(res["X"][sl], dic["D"], dic["normD"], dic["lut"])
        assert np.array_equal(res["qmap"][sl], o["qmap"])


def test_lrtv_and_multi_coil_on_a_rectangular_grid(engine_mod, oracle, synth):
    """5 LRTV iterations at 96 x 160 (TV on 2N x M*s) with identical counts, x to 1e-9; one multi-coil forward / adjoint at 160 x 96."""
    N, M, T, s = 96, 160, 100, 10
    V = _V(T, s, seed=9)
    fp, k = oracle.epi_mask(N, M, 1 / 8, T)
    op = oracle.Operator(N, M, V, fp, k)
    rng = np.random.default_rng(4)
    y = op.forward(rng.standard_normal((N, M, s))) + 0.01 * (rng.standard_normal(op.m) + 1j * rng.standard_normal(op.m))
    e = engine_mod.Engine(0)
    e.set_operator(N, M, V, fp, k)
    xl, il = e.lrtv(y, K=1e-3, iters=5)
    xlo, ilo = oracle.fista_lrtv(op, y, K=1e-3, iters=5)
    assert il["iters"] == ilo["iters"] and il["prox_iters_total"] == int(ilo["prox_iters"].sum()) and il["halvings"] == ilo["halvings"]
    assert rel_err(xl, xlo) < 1e-9
    e.close()

    N, M, nc = 160, 96, 4
    fp, k = oracle.epi_mask(N, M, 1 / 8, T)
    op = oracle.Operator(N, M, V, fp, k)
    e = engine_mod.Engine(0)
    e.set_operator(N, M, V, fp, k, max_batch=2)
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    maps = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                     for a in np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    e.set_coils(maps)
    x = rng.standard_normal((N, M, s)) + 1j * rng.standard_normal((N, M, s))
    yg = e.forward_mc(x)
    assert yg.shape == (e.m, nc) and rel_err(yg, op.forward_mc(x, maps)) < 1e-12
    wv = rng.standard_normal(yg.shape) + 1j * rng.standard_normal(yg.shape)
    assert rel_err(e.adjoint_mc(wv), op.adjoint_mc(wv, maps)) < 1e-12
    e.close()


@pytest.mark.parametrize("N,M", [(230, 230), (512, 512), (200, 224)])
def test_unsupported_grids_are_refused(engine_mod, oracle, N, M):
    """Sides outside the set still give QMRI_ERR_UNSUPPORTED, naming the supported sides, before anything is launched."""
    T = 4
    fp, k = _user_mask(N, M, T, 64, seed=N + M)
    e = engine_mod.Engine(0)
    with pytest.raises(engine_mod.QmriError) as ei:
        e.set_operator(N, M, _V(T), fp, k)
    assert ei.value.code == QMRI_ERR_UNSUPPORTED
    assert "32, 64, 96, 112, 128, 160, 192, 224, 256" in str(ei.value)
    e.close()
