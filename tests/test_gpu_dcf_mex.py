"""GPU: the MATLAB gateway's 'dcf', 'set_sample_weights' and 'adjoint_w' commands under the mock runtime (tests/mexmock.py), bit for bit against the
Engine on the same C ABI, and the argument checks that need a planned operator."""
import numpy as np
import pytest

import nufft_ref as R

pytestmark = pytest.mark.gpu


def test_dcf_commands_match_python_bit_for_bit(engine_mod):
    import mexmock as mex
    N, S, T, s = 32, 60, 48, 3
    rng = np.random.default_rng(0)
    V = np.linalg.qr(rng.standard_normal((T, s)))[0]
    fp, om = R.spiral_traj(N, S, T)
    y = rng.standard_normal(S * T) + 1j * rng.standard_normal(S * T)
    try:
        mex.qmri_mex("set_trajectory", float(N), float(N), V, fp.astype(np.int32), om, 1.0, 6.0)
        with pytest.raises(mex.MexError) as err:                       # no weights yet: the library's refusal
            mex.qmri_mex("adjoint_w", y, nargout=1)
        assert err.value.id == "qmri:err2"
        e = engine_mod.Engine(0)
        e.set_trajectory(N, N, V, fp, om, width=6)
        for args, kw in (((), {}), ((5.0,), dict(niter=5)), ((20.0, 0.05), dict(niter=20, tol=0.05))):
            w, info = mex.qmri_mex("dcf", *args, nargout=2)
            we, ie = e.density_weights(**kw)
            assert w.shape == (S * T, 1) and w.dtype == np.float64 and np.array_equal(w.ravel(), we)
            assert {k: float(np.asarray(v).ravel()[0]) for k, v in info.items()} == {k: float(v) for k, v in ie.items()}
            x = mex.qmri_mex("adjoint_w", y, nargout=1)
            assert x.shape == (N, N, s) and np.array_equal(x, e.adjoint(y, weighted=True))
        w2 = np.abs(rng.standard_normal(S * T))
        mex.qmri_mex("set_sample_weights", w2)
        e.set_sample_weights(w2)
        assert np.array_equal(mex.qmri_mex("adjoint_w", y, nargout=1), e.adjoint(y, weighted=True))
        assert np.array_equal(mex.qmri_mex("adjoint", y, np.array([N, N, s], np.float64), nargout=1), e.adjoint(y))
        for cmd, args, ident in (("set_sample_weights", (w2[:-1],), "qmri:set_sample_weights:size"), ("adjoint_w", (y[:-1],), "qmri:adjoint_w:size"),
                                 ("set_sample_weights", (-w2,), "qmri:err1")):
            with pytest.raises(mex.MexError) as err:
                mex.qmri_mex(cmd, *args, nargout=1)
            assert err.value.id == ident, (cmd, err.value.id)
        mex.qmri_mex("set_sample_weights", np.zeros((0, 0)))           # [] clears
        with pytest.raises(mex.MexError) as err:
            mex.qmri_mex("adjoint_w", y, nargout=1)
        assert err.value.id == "qmri:err2"
        fg, kg = engine_mod.build_spiral(N, S, T)                      # a gridded mask: nothing to compensate
        mex.qmri_mex("set_operator", float(N), float(N), V, fg, kg)
        for cmd, args, ident in (("dcf", (), "qmri:dcf:trajectory"), ("set_sample_weights", (w2,), "qmri:set_sample_weights:trajectory"),
                                 ("adjoint_w", (y,), "qmri:adjoint_w:trajectory")):
            with pytest.raises(mex.MexError) as err:
                mex.qmri_mex(cmd, *args, nargout=1)
            assert err.value.id == ident, (cmd, err.value.id)
        e.close()
    finally:
        mex.mex_exit()
