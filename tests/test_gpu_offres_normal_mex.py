"""GPU: the MATLAB gateway's 'prepare_normal_fm' command and param.field_normal under the mock runtime (tests/mexmock.py), bit for bit against the
Engine on the same C ABI, and the argument checks that need a planned operator."""
import numpy as np
import pytest

import offres_ref as F

pytestmark = pytest.mark.gpu
NETC = (8, 16, 16, 32)


def _num(info):
    return {k: float(np.asarray(v).ravel()[0]) for k, v in info.items()}


def test_prepare_normal_fm_and_field_normal_match_python_bit_for_bit(engine_mod, synth):
    import mexmock as mex
    fp, om, V, f, tau = F.spiral_case(s=3)
    N, s, m = f.shape[0], V.shape[1], om.shape[0]
    x, y = F.vectors(N, N, s, m)
    dims = np.array([N, N, s], np.float64)
    nb = 2
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=NETC, nb=nb, seed=3, eps=0.05)
    none = np.zeros((0, 0))
    try:
        mex.mex_exit()                                                 # (the gateway is one per process: start without an operator)
        with pytest.raises(mex.MexError) as err:
            mex.qmri_mex("prepare_normal_fm", nargout=1)
        assert err.value.id == "qmri:state"
        mex.qmri_mex("set_trajectory", float(N), float(N), V, fp.astype(np.int32), om, 1.0, 6.0)
        mex.qmri_mex("set_denoiser", w.astype(np.float32), float(s), float(s), np.array([NETC], np.float64), float(nb), 0.0, float(N), float(N))
        e = engine_mod.Engine(0)
        e.set_trajectory(N, N, V, fp, om, width=6)
        e.set_denoiser(w, N, N, in_nc=s, out_nc=s, nc=NETC, nb=nb)
        plain = e.normal(x)
        with pytest.raises(mex.MexError) as err:                       # no map yet: the library's QMRI_ERR_STATE, naming both calls
            mex.qmri_mex("prepare_normal_fm", nargout=1)
        assert err.value.id == "qmri:err2" and "qmri_set_field_map" in err.value.msg and "qmri_nufft_prepare_normal" in err.value.msg
        mex.qmri_mex("set_field_map", f, tau, 4.0, nargout=1)
        e.set_field_map(f, tau, nseg=4)
        with pytest.raises(mex.MexError) as err:                       # opt-in: refused until the command has run for this map
            mex.qmri_mex("normal", x, nargout=1)
        assert err.value.id == "qmri:err4" and "LSQR" in err.value.msg and "field map" in err.value.msg
        # ---- the command against Engine.prepare_normal_field: the info and the operator, bit for bit
        for args, kw in (((), {}), ((6.0,), dict(nseg=6)), ((0.0, 1e-3), dict(nseg=0, tol=1e-3))):
            info = mex.qmri_mex("prepare_normal_fm", *args, nargout=1)
            ie = e.prepare_normal_field(**kw)
            assert set(info) == {"nseg", "tol_reached", "fit_max", "fit_rms", "khat_bytes"}
            assert _num(info) == {k: float(v) for k, v in ie.items()}, (info, ie)
            z = mex.qmri_mex("normal", x, nargout=1)
            assert z.shape == (N, N, s) and np.array_equal(z, e.normal(x))
        assert _num(info)["nseg"] == 8.0                               # (tol = 1e-3: the L' of tests/test_gpu_offres_normal.py's auto-mode test)
        # ---- the checks that need the operator, every one with an identifier
        for args, ident in (((1.0,), "qmri:prepare_normal_fm:nseg"), ((33.0,), "qmri:prepare_normal_fm:nseg"), ((2.5,), "qmri:prepare_normal_fm:nseg"),
                            ((-1.0,), "qmri:prepare_normal_fm:nseg"), ((np.ones(2),), "qmri:prepare_normal_fm:nseg"),
                            ((0.0, -1.0), "qmri:prepare_normal_fm:tol"), ((0.0, float("nan")), "qmri:prepare_normal_fm:tol"),
                            ((0.0, 1j), "qmri:prepare_normal_fm:tol")):
            with pytest.raises(mex.MexError) as err:
                mex.qmri_mex("prepare_normal_fm", *args, nargout=1)
            assert err.value.id == ident, (ident, err.value.id)
        assert np.array_equal(mex.qmri_mex("normal", x, nargout=1), e.normal(x))          # (a refused call leaves the transform in place)
        # ---- a new map drops the transform; param.field_normal builds it before the loop
        mex.qmri_mex("set_field_map", f, tau, 4.0, nargout=1)
        e.set_field_map(f, tau, nseg=4)
        yv = e.forward(x)
        prm = {"gamma": 0.05, "iter": 2, "cg_tol": 1e-4, "multi_level": 0, "noise_std": 0.01, "solver": 2.0}
        with pytest.raises(mex.MexError) as err:
            mex.qmri_mex("pnp_admm", yv.astype(np.complex128), prm, none, none, dims, nargout=3)
        assert err.value.id == "qmri:err4"
        for extra, kw in (({"field_normal": 1.0}, {}), ({"field_normal": 1.0, "field_normal_nseg": 6.0}, dict(nseg=6)),
                          ({"field_normal": 1.0, "field_normal_tol": 1e-3}, dict(tol=1e-3))):
            mex.qmri_mex("set_field_map", f, tau, 4.0, nargout=1)      # (every round starts without the transform)
            e.set_field_map(f, tau, nseg=4)
            xm, _, li = mex.qmri_mex("pnp_admm", yv.astype(np.complex128), {**prm, **extra}, none, none, dims, nargout=3)
            e.prepare_normal_field(**kw)
            xe, _, le = e.pnp_admm(yv, iters=2, solver="toeplitz")
            assert np.array_equal(xm, xe) and np.array_equal(li.ravel(), le), extra
        xl, _, _ = e.pnp_admm(yv, iters=2)
        assert not np.array_equal(xe, xl)                              # (and it is not the LSQR route's result)
        for extra in ({"field_normal": 1.0, "field_normal_nseg": 1.0}, {"field_normal": 1.0, "field_normal_nseg": 40.0},
                      {"field_normal": 1.0, "field_normal_tol": -1.0}):
            with pytest.raises(mex.MexError) as err:
                mex.qmri_mex("pnp_admm", yv.astype(np.complex128), {**prm, **extra}, none, none, dims, nargout=3)
            assert err.value.id == "qmri:pnp_admm:field_normal", (extra, err.value.id)
        # field_normal = 0 is absent: the LSQR route with the map, as Python's
        xm, _, _ = mex.qmri_mex("pnp_admm", yv.astype(np.complex128), {**prm, "solver": 0.0, "field_normal": 0.0}, none, none, dims, nargout=3)
        assert np.array_equal(xm, xl)
        # ---- clearing the map returns the plain normal operator; a gridded mask refuses the command by its identifier
        mex.qmri_mex("set_field_map", none)
        assert np.array_equal(mex.qmri_mex("normal", x, nargout=1), plain)
        e.close()
        fg, kg = engine_mod.build_spiral(N, 60, 48)
        mex.qmri_mex("set_operator", float(N), float(N), V, fg, kg)
        with pytest.raises(mex.MexError) as err:
            mex.qmri_mex("prepare_normal_fm", nargout=1)
        assert err.value.id == "qmri:prepare_normal_fm:trajectory"
        with pytest.raises(mex.MexError) as err:
            mex.qmri_mex("pnp_admm", np.zeros(int(fg[-1]), np.complex128), {**prm, "field_normal": 1.0}, none, none, dims, nargout=3)
        assert err.value.id == "qmri:pnp_admm:field_normal"
    finally:
        mex.mex_exit()
