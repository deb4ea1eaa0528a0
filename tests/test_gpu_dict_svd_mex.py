"""GPU: the MATLAB gateway's 'dict_compress' command under the mock runtime (tests/mexmock.py), bit for bit against Engine.compress_dictionary,
and its argument checks by identifier."""
import numpy as np
import pytest

import dict_svd_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    T, n1, n2, _ = R.FIXTURES["t48"]
    return R.simulate(T, n1, n2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dict_compress_is_the_engine_call_bit_for_bit(F, dtype):
    from mexmock import qmri_mex
    from qmri_pnp_recon_poc_amd import engine
    Fd = F.astype(dtype)
    eng = engine.Engine(0)
    for params, kw in (({"s": 6.0}, dict(s=6)), ({"energy": 0.9999, "s_max": 8.0}, dict(energy=0.9999, s_max=8)), ({"s": 3.0, "tol": 1e-10, "maxit": 50.0}, dict(s=3, tol=1e-10, maxit=50))):
        V, D, nd, eig, info = qmri_mex("dict_compress", Fd, params, nargout=5)
        want = eng.compress_dictionary(Fd, **kw)
        s = want["info"]["s"]
        assert V.shape == (48, s) and V.dtype == np.float64 and D.shape == (264, s) and D.dtype == np.float32 and nd.shape == (264, 1) and nd.dtype == np.float32
        assert np.array_equal(V, want["V"]) and np.array_equal(D, want["D"]) and np.array_equal(nd.ravel(), want["normD"])
        assert np.array_equal(eig.ravel(), want["eig"])
        assert {k: float(np.asarray(v).ravel()[0]) for k, v in info.items()} == {k: float(v) for k, v in want["info"].items()}
    eng.close()
    assert qmri_mex("dict_compress", Fd, {"s": 2.0}, nargout=1).shape == (48, 2)         # fewer outputs asked for


def test_argument_checks_by_identifier(F):
    from mexmock import MexError, qmri_mex
    for args, ident in (((F,), "qmri:usage"), ((F, 1.0), "qmri:dict_compress:params"), ((F + 0j, {"s": 2.0}), "qmri:dict_compress:F"),
                        ((F.astype(np.int32), {"s": 2.0}), "qmri:dict_compress:F"), ((np.zeros((4, 1025)), {"s": 2.0}), "qmri:dict_compress:F"),
                        ((np.zeros((4, 3, 2)), {"s": 2.0}), "qmri:dict_compress:F"),
                        ((F, {"s": 0.0}), "qmri:dict_compress:params"), ((F, {"s": 17.0}), "qmri:dict_compress:params"), ((F[:4], {"s": 5.0}), "qmri:dict_compress:params"),
                        ((F, {"s": 2.5}), "qmri:dict_compress:params"), ((F, {"s": 2.0, "energy": 0.9}), "qmri:dict_compress:params"), ((F, {"tol": 0.0}), "qmri:dict_compress:params"),
                        ((F, {"energy": 0.0}), "qmri:dict_compress:params"), ((F, {"energy": 0.9, "s_max": 17.0}), "qmri:dict_compress:params"),
                        ((F, {"s": 2.0, "tol": -1.0}), "qmri:dict_compress:params"), ((F, {"s": 2.0, "maxit": 0.5}), "qmri:dict_compress:params")):
        with pytest.raises(MexError) as e:
            qmri_mex("dict_compress", *args, nargout=1)
        assert e.value.id == ident, (args[1:], e.value.id)
