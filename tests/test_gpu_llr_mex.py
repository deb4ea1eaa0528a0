"""GPU: the MATLAB gateway's 'llr_prox', 'set_llr' and 'clear_llr' commands under the mock runtime (tests/mexmock.py) and the call sequence of
PnP_ADMM_hip.m with a qmri_make_llr struct as param.net, bit for bit against the Python engine."""
import numpy as np
import pytest

import llr_ref as R

pytestmark = pytest.mark.gpu


def test_llr_prox_is_the_engine_call_bit_for_bit():
    from mexmock import qmri_mex
    from qmri_pnp_recon_poc_amd import engine
    eng = engine.Engine(0)
    Xs = np.stack([R.tsmi_like(32, 64, 5, seed=k) for k in range(2)])                                     # [S, N, M, s]
    want, sm = eng.llr_prox(Xs, 0.04, block=4, offset=(3, 1))
    out, smax = qmri_mex("llr_prox", np.moveaxis(Xs, 0, 3), 0.04, 4.0, 3.0, 1.0, nargout=2)               # MATLAB's N x M x s x S
    assert out.shape == (32, 64, 5, 2) and np.array_equal(np.moveaxis(out, 3, 0), want) and np.array_equal(smax.ravel(), sm)
    o1 = qmri_mex("llr_prox", Xs[0], 0.04, nargout=1)                                                     # the defaults: block 8, offsets (0, 0)
    assert np.array_equal(o1, eng.llr_prox(Xs[0], 0.04)[0])
    o2, s2 = qmri_mex("llr_prox", np.ascontiguousarray(Xs[1].real), 0.1, 16.0, nargout=2)                 # a real array: real mode
    w2, m2 = eng.llr_prox(Xs[1], 0.1, block=16, real=True)
    assert np.array_equal(o2, w2) and s2.ravel()[0] == m2 and np.array_equal(o2.imag, np.zeros_like(o2.imag))
    eng.close()


def test_pnp_admm_hip_with_a_make_llr_struct_equals_python(oracle, synth):
    """What PnP_ADMM_hip.m does with param.net = qmri_make_llr(F): sigma_max of the start image through 'llr_prox' with tau = 0, 'set_llr',
    'pnp_admm', 'clear_llr' -- and after 'clear_llr' the loop asks for a denoiser again."""
    from mexmock import MexError, mex_exit, qmri_mex
    from qmri_pnp_recon_poc_amd import engine
    mex_exit()                                                                 # a fresh gateway: no denoiser from an earlier test
    N, s, iters, block = 32, 4, 4, 8
    dic, q, X0 = synth.make_case(N=N, T=24, s=s, K=(24, 16), slice_seed=0)
    fp, k = oracle.spiral_mask(N, 120, 24)
    eng = engine.Engine(0)
    eng.set_operator(N, N, dic["V"], fp, k)
    y = synth.awgn_measured(eng.forward(X0), 30.0, seed=0)
    start = eng.adjoint(y)
    _, smax = eng.llr_prox(start, 0.0, block=block, real=True)
    eng.set_llr(0.02 * smax, block=block, shift=True)
    want, _, li = eng.pnp_admm(y, gamma=0.05, iters=iters)
    eng.close()
    qmri_mex("set_operator", float(N), float(N), np.asarray(dic["V"], np.float64), fp.astype(np.int32), k.astype(np.int32), 1.0)
    a = qmri_mex("adjoint", y.reshape(-1, 1), np.array([N, N, s], np.float64), nargout=1)
    assert np.array_equal(a, start)
    _, sm = qmri_mex("llr_prox", np.ascontiguousarray(a.real), 0.0, float(block), nargout=2)
    assert sm.ravel()[0] == smax
    p = {"gamma": 0.05, "iter": float(iters), "cg_tol": 1e-4, "multi_level": 0.0, "noise_std": 0.01, "complex_tsmi": 0.0}
    empty = np.zeros((0, 0))
    qmri_mex("set_llr", 0.02 * sm.ravel()[0], float(block), 1.0)
    x, _, l2 = qmri_mex("pnp_admm", y.reshape(-1, 1), p, empty, empty, np.array([N, N, s], np.float64), nargout=3)
    assert np.array_equal(x, want) and np.array_equal(l2.ravel(), li)
    qmri_mex("clear_llr")
    with pytest.raises(MexError) as e:
        qmri_mex("pnp_admm", y.reshape(-1, 1), p, empty, empty, np.array([N, N, s], np.float64), nargout=1)
    assert e.value.id == "qmri:state"
    mex_exit()


def test_the_librarys_refusal_comes_through_by_identifier():
    from mexmock import MexError, qmri_mex
    with pytest.raises(MexError) as e:
        qmri_mex("llr_prox", np.ones((32, 32, 17), complex), 0.1, nargout=1)
    assert e.value.id == "qmri:llr_prox:size"
