"""GPU: the MATLAB gateway's 'set_field_map' command under the mock runtime (tests/mexmock.py), bit for bit against the Engine on the same C ABI,
and the argument checks that need a planned operator."""
import numpy as np
import pytest

import offres_ref as F

pytestmark = pytest.mark.gpu


def test_set_field_map_matches_python_bit_for_bit(engine_mod):
    import mexmock as mex
    fp, om, V, f, tau = F.spiral_case(s=3)
    N, s, m = f.shape[0], V.shape[1], om.shape[0]
    x, y = F.vectors(N, N, s, m)
    dims = np.array([N, N, s], np.float64)
    try:
        mex.qmri_mex("set_trajectory", float(N), float(N), V, fp.astype(np.int32), om, 1.0, 6.0)
        e = engine_mod.Engine(0)
        e.set_trajectory(N, N, V, fp, om, width=6)
        plain = e.adjoint(y)
        for args, kw in (((), {}), ((4.0,), dict(nseg=4)), ((0.0, 64.0, 1e-3), dict(nseg=0, nbins=64, tol=1e-3))):
            info = mex.qmri_mex("set_field_map", f, tau, *args, nargout=1)
            ie = e.set_field_map(f, tau, **kw)
            assert {k: float(np.asarray(v).ravel()[0]) for k, v in info.items()} == {k: float(v) for k, v in ie.items()}
            assert np.array_equal(mex.qmri_mex("adjoint", y, dims, nargout=1), e.adjoint(y))
            assert np.array_equal(mex.qmri_mex("forward", x, nargout=1).ravel(), e.forward(x))
        for args, ident in (((f[:-1], tau), "qmri:set_field_map:size"), ((f.T[:, :-1], tau), "qmri:set_field_map:size"), ((f, tau[:-1]), "qmri:set_field_map:size"),
                            ((f + 0j, tau), "qmri:set_field_map:type"), ((f, tau + 0j), "qmri:set_field_map:type"), ((f,), "qmri:usage"),
                            ((f, tau, 17.0), "qmri:set_field_map:nseg"), ((f, tau, 4.0, 8.0), "qmri:set_field_map:nbins"),
                            ((f, tau, 4.0, 0.0, -1.0), "qmri:set_field_map:tol"), ((f, tau, 1.0), "qmri:err1")):
            with pytest.raises(mex.MexError) as err:
                mex.qmri_mex("set_field_map", *args, nargout=1)
            assert err.value.id == ident, (ident, err.value.id)
        with pytest.raises(mex.MexError) as err:                       # the Toeplitz form is refused while a map is attached
            mex.qmri_mex("normal", x, nargout=1)
        assert err.value.id == "qmri:err4"
        mex.qmri_mex("set_field_map", np.zeros((0, 0)))                # [] clears
        assert np.array_equal(mex.qmri_mex("adjoint", y, dims, nargout=1), plain)
        mex.qmri_mex("set_field_map", f, tau, 3.0, nargout=1)
        mex.qmri_mex("set_trajectory", float(N), float(N), V, fp.astype(np.int32), om, 1.0, 6.0)     # a new operator drops the map
        assert np.array_equal(mex.qmri_mex("adjoint", y, dims, nargout=1), plain)
        fg, kg = engine_mod.build_spiral(N, 60, 48)                    # a gridded mask has no readout times
        mex.qmri_mex("set_operator", float(N), float(N), V, fg, kg)
        with pytest.raises(mex.MexError) as err:
            mex.qmri_mex("set_field_map", f, tau, nargout=1)
        assert err.value.id == "qmri:set_field_map:trajectory"
        e.close()
    finally:
        mex.mex_exit()
