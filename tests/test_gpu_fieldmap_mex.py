"""GPU: the MATLAB gateway's 'field_map_estimate' command under the mock runtime (tests/mexmock.py), bit for bit against Engine.estimate_field_map,
and the library's own refusal by identifier."""
import numpy as np
import pytest

import fieldmap_ref as R
import offres_ref as O

pytestmark = pytest.mark.gpu

T3 = np.array([0.0, 2e-3, 5e-3])


def matlab_layout(Y):
    """[S, L, C, N, M] (or fewer leading axes) -> MATLAB's N x M x C x L x S."""
    n = Y.ndim
    return np.transpose(Y, (n - 2, n - 1) + tuple(range(n - 3, -1, -1)))


def test_field_map_estimate_is_the_engine_call_bit_for_bit():
    from mexmock import qmri_mex
    from qmri_pnp_recon_poc_amd import engine
    N, M = 33, 47
    x = 1.0 / (1.0 + ((np.arange(N)[:, None] - 16) / 9.0) ** 2 + ((np.arange(M)[None, :] - 20) / 14.0) ** 2)
    Y = np.stack([R.echoes(x, O.field(N, M), T3, C=2, sigma_rel=0.02, seed=s) for s in (0, 1)])          # [S, L, C, N, M]
    eng = engine.Engine(0)
    want, info, trust = eng.estimate_field_map(Y, T3, iters=19, beta=0.02, return_info=True, return_trust=True)
    f, fi, tr = qmri_mex("field_map_estimate", matlab_layout(Y), T3, 19.0, 0.02, -1.0, nargout=3)
    assert f.shape == (N, M, 2) and f.dtype == np.float64
    assert np.array_equal(np.moveaxis(f, 2, 0), want) and np.array_equal(np.moveaxis(tr, 2, 0), trust)
    assert fi["iters"].tolist() == [[19.0, 19.0]] and fi["cost"].tolist() == [[info[0]["cost"], info[1]["cost"]]]
    assert fi["cost0"].tolist() == [[info[0]["cost0"], info[1]["cost0"]]] and fi["unwrap_limit_hz"].tolist() == [[250.0, 250.0]]
    f1 = qmri_mex("field_map_estimate", matlab_layout(Y[0]), T3, 19.0, 0.02, nargout=1)                   # N x M x C x L, the default sign
    assert f1.shape == (N, M) and np.array_equal(f1, want[0])
    f2 = qmri_mex("field_map_estimate", matlab_layout(Y[1, :, 0]), T3, nargout=1)                         # N x M x L: one coil, the defaults
    assert np.array_equal(f2, eng.estimate_field_map(Y[1, :, 0], T3))
    f3 = qmri_mex("field_map_estimate", matlab_layout(Y[0]), T3, 5.0, 0.0, 1.0, nargout=1)
    assert np.array_equal(f3, eng.estimate_field_map(Y[0], T3, iters=5, phase_sign=1))
    eng.close()


def test_the_librarys_refusal_comes_through_by_identifier():
    from mexmock import MexError, qmri_mex
    Y = np.ones((4, 5, 2, 3), complex)
    Y[1, 2, 0, 1] = complex(0.0, np.inf)
    with pytest.raises(MexError) as e:
        qmri_mex("field_map_estimate", Y, T3, nargout=1)
    assert e.value.id == "qmri:err1" and "Y must be finite" in e.value.msg
