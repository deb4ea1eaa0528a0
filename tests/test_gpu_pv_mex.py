"""GPU: the tissue-fraction unmixing through the MATLAB gateway under the mock runtime (tests/mexmock.py): 'set_components' and 'dict_unmix' give
Engine.tissue_fractions' bits."""
import numpy as np
import pytest

import pv_ref as PV

pytestmark = pytest.mark.gpu


def test_mex_unmix_equals_the_engine(engine_mod):
    from mexmock import MexError, qmri_mex
    C_, s, n = 5, 10, 301
    dic = PV.dictionary(s)
    atoms, _, G = PV.fixture_components(C_, s)
    X = PV.fixture_pixels(C_, s, PV.PHASE)[0][:n].copy()
    X[7, 3] = np.nan
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
        info = e.set_components(atoms)
        want = {m: e.tissue_fractions(X, mode=m) for m in ("real", "phase")}
    finally:
        e.close()
    qmri_mex("set_dictionary", dic["D"], dic["normD"], dic["lut"])
    with pytest.raises(MexError) as err:                        # no components yet
        qmri_mex("dict_unmix", X, 0.0, nargout=1)
    assert err.value.id == "qmri:state"
    got = qmri_mex("set_components", atoms.astype(np.float64), nargout=1)
    assert got["min_pivot"].item() == info["min_pivot"] and got["C"].item() == C_ and got["s"].item() == s
    for m, code in (("real", 0.0), ("phase", 1.0)):
        w, frac, pd, res, flags = qmri_mex("dict_unmix", X, code, nargout=5)
        assert np.array_equal(w, want[m]["w"]) and np.array_equal(frac, want[m]["frac"]) and np.array_equal(pd.ravel(), want[m]["pd"])
        assert np.array_equal(res.ravel(), want[m]["res"]) and np.array_equal(flags.ravel(), want[m]["flags"])
        assert flags.dtype == np.int32 and pd.dtype == np.complex128 and flags.ravel()[7] == PV.FLAG_NONFINITE
        assert np.array_equal(qmri_mex("dict_unmix", X, code, nargout=1), want[m]["w"])
    for args, ident in ((("dict_unmix", X[:, :9], 0.0), "qmri:dict_unmix:size"), (("set_components", np.array([1.0, 1.0])), "qmri:err1"),
                        (("set_components", np.array([0.0, 2.0])), "qmri:set_components:size"), (("set_components", np.array([1.0, 513.0])), "qmri:set_components:size"),
                        (("set_components", np.array([1.5, 2.0])), "qmri:set_components:size")):
        with pytest.raises(MexError) as err:
            qmri_mex(*args, nargout=1)
        assert err.value.id == ident, (args[0], ident, err.value.id)
    assert np.array_equal(qmri_mex("dict_unmix", X, 1.0, nargout=1), want["phase"]["w"])       # a refused call left the components in place
    qmri_mex("set_components", np.zeros((0, 0)))                                                  # clears
    with pytest.raises(MexError) as err:
        qmri_mex("dict_unmix", X, 0.0, nargout=1)
    assert err.value.id == "qmri:state"
    qmri_mex("set_components", atoms.astype(np.float64))
    qmri_mex("set_dictionary", dic["D"], dic["normD"], dic["lut"])                                # drops them
    with pytest.raises(MexError) as err:
        qmri_mex("dict_unmix", X, 0.0, nargout=1)
    assert err.value.id == "qmri:state"
