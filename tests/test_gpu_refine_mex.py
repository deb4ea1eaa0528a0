"""GPU: the sub-grid refinement through the MATLAB gateway under the mock runtime (tests/mexmock.py): 'set_refine' and 'dict_refine' give
Engine.dict_refine's bits."""
import numpy as np
import pytest

import refine_ref as RR

pytestmark = pytest.mark.gpu


def test_mex_refine_equals_the_engine(engine_mod):
    from mexmock import MexError, qmri_mex
    fxa = RR.FIXTURES[1]
    fx = RR.fixture(*fxa, snr_db=40)
    dic, n = fx["dic"], 301
    X, dm = fx["X"][:n].copy(), fx["dm"][:n].copy()
    X[7, 3] = np.nan
    dm[11] = 0
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
        info = e.set_refine((0, 1))
        want = e.dict_refine(X, dm)
        e.set_refine((1,))
        want_t2 = e.dict_refine(X, dm)
    finally:
        e.close()
    qmri_mex("set_dictionary", dic["D"], dic["normD"], dic["lut"])
    with pytest.raises(MexError) as err:                        # no refinement yet
        qmri_mex("dict_refine", X, dm, nargout=1)
    assert err.value.id == "qmri:state"
    got = qmri_mex("set_refine", np.array([0.0, 1.0]), nargout=1)
    assert got["P"].item() == 2 and got["K"].item() == info["K"] and got["s"].item() == info["s"] and np.array_equal(got["count"], info["count"])
    qmap, pd, res, t, centre, flags = qmri_mex("dict_refine", X, dm, nargout=6)
    assert np.array_equal(qmap, want["qmap"]) and np.array_equal(pd.ravel(), want["pd"]) and np.array_equal(res.ravel(), want["res"])
    assert np.array_equal(t, want["t"]) and np.array_equal(centre.ravel(), want["centre"]) and np.array_equal(flags.ravel(), want["flags"])
    assert flags.dtype == np.int32 and centre.dtype == np.int32 and pd.dtype == np.complex128
    assert flags.ravel()[7] == RR.FLAG_DEGENERATE and flags.ravel()[11] == RR.FLAG_SKIPPED
    assert np.array_equal(qmri_mex("dict_refine", X, dm, nargout=1), want["qmap"])
    for args, ident in ((("dict_refine", X[:, :4], dm), "qmri:dict_refine:size"), (("set_refine", np.array([1.0, 1.0])), "qmri:err1"),
                        (("set_refine", np.array([0.0, 2.0])), "qmri:err1"), (("set_refine", np.array([-1.0])), "qmri:set_refine:value")):
        with pytest.raises(MexError) as err:
            qmri_mex(*args, nargout=1)
        assert err.value.id == ident, (args[0], ident, err.value.id)
    assert np.array_equal(qmri_mex("dict_refine", X, dm, nargout=1), want["qmap"])       # a refused call left the state in place
    qmri_mex("set_refine", np.array([1.0]))
    q1, _, _, t1 = qmri_mex("dict_refine", X, dm, nargout=4)
    assert np.array_equal(q1, want_t2["qmap"]) and t1.shape == (n, 1) and np.array_equal(t1, want_t2["t"])
    qmri_mex("set_refine", np.zeros((0, 0)))                                              # clears
    with pytest.raises(MexError) as err:
        qmri_mex("dict_refine", X, dm, nargout=1)
    assert err.value.id == "qmri:state"
    qmri_mex("set_refine", np.array([0.0, 1.0]))
    qmri_mex("set_dictionary", dic["D"], dic["normD"], dic["lut"])                        # drops it
    with pytest.raises(MexError) as err:
        qmri_mex("dict_refine", X, dm, nargout=1)
    assert err.value.id == "qmri:state"
