"""GPU: the B1 estimate through the MATLAB gateway under the mock runtime (tests/mexmock.py): 'group_scores' and 'b1_estimate' give the bits of
Engine.group_scores and Engine.estimate_b1."""
import numpy as np
import pytest

import b1_ref as BR

pytestmark = pytest.mark.gpu


def test_mex_b1_commands_equal_the_engine(engine_mod):
    from mexmock import MexError, qmri_mex
    s = 10
    D, nd, lut, gp, gv = BR.ragged_dictionary(s)
    X, _ = BR.pooling_fixture(s, nslices=2)
    mask = np.ones(X.shape[:-1], bool)
    mask[::4, 2] = False
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(D, nd, lut)
        e.set_dictionary_groups(gp, gv)
        score = e.group_scores(X)
        want = e.estimate_b1(X, mask=mask, window=3)
        free = e.estimate_b1(X, window=4)
    finally:
        e.close()
    n = 43 * 7 * 2
    Xm = X.reshape((n, s), order="F")
    dims = np.array([43.0, 7.0, 2.0])
    qmri_mex("set_dictionary", D, nd, lut)
    for args in (("group_scores", Xm), ("b1_estimate", Xm, dims, np.zeros(0), 4.0)):              # no groups yet
        with pytest.raises(MexError) as err:
            qmri_mex(*args, nargout=1)
        assert err.value.id == "qmri:state"
    qmri_mex("set_dictionary_groups", gp.astype(np.float64), gv)
    sc = qmri_mex("group_scores", Xm, nargout=1)
    assert sc.dtype == np.float32 and sc.shape == (n, 5)
    assert np.array_equal(sc.view(np.int32), score.reshape((5, n), order="F").T.view(np.int32))
    b1, grp, conf, info = qmri_mex("b1_estimate", Xm, dims, mask.ravel(order="F").astype(np.float64), 3.0, nargout=4)
    assert grp.dtype == np.int32 and b1.shape == (n, 1)
    got = {"b1": b1.reshape((43, 7, 2), order="F"), "grp": grp.reshape((43, 7, 2), order="F"), "conf": conf.reshape((43, 7, 2), order="F")}
    assert not BR.same(got, want)
    assert {k: float(np.asarray(v).ravel()[0]) for k, v in info.items()} == {k: float(v) for k, v in want["info"].items()}
    b1 = qmri_mex("b1_estimate", Xm, dims, np.zeros(0), 4.0, nargout=1)                           # [] mask: every pixel
    assert np.array_equal(b1.reshape((43, 7, 2), order="F"), free["b1"], equal_nan=True)
    for args, ident in ((("group_scores", Xm[:, :9]), "qmri:group_scores:size"), (("b1_estimate", Xm[:, :9], dims, np.zeros(0), 4.0), "qmri:b1_estimate:size")):
        with pytest.raises(MexError) as err:
            qmri_mex(*args, nargout=1)
        assert err.value.id == ident
    qmri_mex("set_dictionary", D, nd, lut)                                                        # drops the groups
    with pytest.raises(MexError) as err:
        qmri_mex("group_scores", Xm, nargout=1)
    assert err.value.id == "qmri:state"
