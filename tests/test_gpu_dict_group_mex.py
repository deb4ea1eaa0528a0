"""GPU: the grouped dictionary match through the MATLAB gateway under the mock runtime (tests/mexmock.py): 'set_dictionary_groups' and
'dict_match_grouped' give Engine.dict_match(X, sel)'s bits."""
import numpy as np
import pytest

import dict_group_ref as GR

pytestmark = pytest.mark.gpu


def test_mex_grouped_match_equals_the_engine(engine_mod):
    from mexmock import MexError, qmri_mex
    rng = np.random.default_rng(31)
    D, nd, lut = GR.random_dictionary(207, 10, seed=32)
    gp, gv = np.array([0, 37, 42, 106, 107, 207]), np.array([0.8, 0.9, 1.0, 1.1, 1.2])
    X = rng.standard_normal((301, 10)) + 1j * rng.standard_normal((301, 10))
    sel = rng.uniform(0.7, 1.3, 301)
    sel[::13] = np.nan
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(D, nd, lut)
        e.set_dictionary_groups(gp, gv)
        want = e.dict_match(X, sel=sel, want_xfit=True)
    finally:
        e.close()
    qmri_mex("set_dictionary", D, nd, lut)
    with pytest.raises(MexError) as err:                        # no groups yet: the library's QMRI_ERR_STATE
        qmri_mex("dict_match_grouped", X, 2.0, sel, nargout=5)
    assert err.value.id == "qmri:err2"
    qmri_mex("set_dictionary_groups", gp.astype(np.float64), gv)
    qmap, pd, mt, dm, grp, xfit = qmri_mex("dict_match_grouped", X, 2.0, sel, nargout=6)
    assert np.array_equal(qmap, want["qmap"]) and np.array_equal(pd.ravel(), want["pd"]) and np.array_equal(mt.ravel(), want["mt"])
    assert np.array_equal(dm.ravel(), want["dm"]) and np.array_equal(grp.ravel(), want["grp"]) and np.array_equal(xfit, want["Xfit"])
    assert dm.dtype == np.int32 and grp.dtype == np.int32 and (grp.ravel()[::13] == 0).all()
    for args, ident in ((("dict_match_grouped", X[:, :9], 2.0, sel), "qmri:dict_match_grouped:size"), (("dict_match_grouped", X, 3.0, sel), "qmri:dict_match_grouped:size")):
        with pytest.raises(MexError) as err:
            qmri_mex(*args, nargout=1)
        assert err.value.id == ident
    qmri_mex("set_dictionary_groups", np.zeros((0, 0)), np.zeros((0, 0)))                      # clears
    with pytest.raises(MexError) as err:
        qmri_mex("dict_match_grouped", X, 2.0, sel, nargout=1)
    assert err.value.id == "qmri:err2"
