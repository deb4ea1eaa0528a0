"""GPU: the MATLAB gateway's 'set_sms', 'forward_sms', 'adjoint_sms', 'xupdate_sms' and 'pnp_admm_sms' commands under the mock runtime
(tests/mexmock.py), bit for bit against the Python engine on sms_ref's case z2c4, and the phases' lifetime in the gateway: kept across its own
re-plans of the operator, dropped by a new operator."""
import numpy as np
import pytest

import sms_ref as SR

pytestmark = pytest.mark.gpu


def test_the_five_commands_are_the_engine_calls_bit_for_bit(engine_mod):
    from mexmock import MexError, mex_exit, qmri_mex
    mex_exit()                                                                 # a fresh gateway
    c = SR.inputs("z2c4")
    N, M, s, Z = c["N"], c["M"], c["s"], c["Z"]
    maps2 = np.concatenate([c["maps"], c["maps"][:, :, :, ::-1]])             # two groups
    y2 = np.concatenate([c["y"], 0.5 * c["y"][:, ::-1]])
    z2, x02 = np.concatenate([c["z"], c["z"][:, ::-1]]), np.concatenate([c["x0"], 0.5 * c["x0"]])
    e = engine_mod.Engine(0)
    e.set_operator(N, M, c["V"], c["fp"], c["k"], max_batch=4)
    e.set_sms(c["E"])
    wy, wx = e.forward_sms(maps2, z2), e.adjoint_sms(maps2, y2)
    wyr = e.forward_sms(maps2, z2.real)
    wu = e.xupdate_sms(maps2, y2, z2, SR.R, 1e-4, 100, x02)
    wu0 = e.xupdate_sms(maps2, y2, z2, SR.R, 1e-6, 7)
    e.set_llr(0.05, block=8, shift=True)
    wp, wl = e.pnp_admm_sms(maps2, y2, groups_per_launch=2, gamma=0.05, iters=3, tsmi_domain="complex")
    wp1, wl1 = e.pnp_admm_sms(maps2[:1], y2[:1], gamma=0.05, iters=3, x0=x02[:1])
    e.close()
    # MATLAB shapes: maps N x M x ncoil x Z x G, y m x ncoil x G, images N x M x s x Z x G
    mm = lambda a: np.ascontiguousarray(np.transpose(a, (2, 3, 4, 1, 0)))
    my = lambda a: np.ascontiguousarray(np.transpose(a, (1, 2, 0)))
    back = lambda a, G: np.transpose(a.reshape((N, M, s, Z, G), order="F"), (4, 3, 0, 1, 2))
    qmri_mex("set_operator", float(N), float(M), np.asarray(c["V"], np.float64), c["fp"].astype(np.int32), c["k"].astype(np.int32), 1.0)
    with pytest.raises(MexError) as err:                                       # no phases yet
        qmri_mex("forward_sms", mm(maps2), mm(z2), nargout=1)
    assert err.value.id == "qmri:state"
    with pytest.raises(MexError) as err:                                       # T x Z with the wrong T
        qmri_mex("set_sms", np.ones((c["T"] + 1, Z), complex))
    assert err.value.id == "qmri:set_sms:size"
    qmri_mex("set_sms", np.asarray(c["E"], complex))
    yg = qmri_mex("forward_sms", mm(maps2), mm(z2), nargout=1)
    assert yg.shape == (c["m"], c["nc"], 2) and np.array_equal(np.transpose(yg, (2, 0, 1)), wy)
    assert np.array_equal(np.transpose(qmri_mex("forward_sms", mm(maps2), np.ascontiguousarray(mm(z2).real), nargout=1), (2, 0, 1)), wyr)
    assert np.array_equal(back(qmri_mex("adjoint_sms", mm(maps2), my(y2), nargout=1), 2), wx)
    x, it, fl = qmri_mex("xupdate_sms", mm(maps2), my(y2), mm(z2), SR.R, 1e-4, 100.0, mm(x02), nargout=3)
    assert np.array_equal(back(x, 2), wu[0]) and np.array_equal(it.ravel(), wu[1]) and np.array_equal(fl.ravel(), wu[2])
    x, it, fl = qmri_mex("xupdate_sms", mm(maps2), my(y2), mm(z2), SR.R, 1e-6, 7.0, nargout=3)
    assert np.array_equal(back(x, 2), wu0[0]) and np.array_equal(it.ravel(), wu0[1]) and np.array_equal(fl.ravel(), wu0[2]) and np.all(fl.ravel() == 1)
    p = {"gamma": 0.05, "iter": 3.0, "cg_tol": 1e-4, "multi_level": 0.0, "noise_std": 0.01, "complex_tsmi": 1.0}
    with pytest.raises(MexError) as err:                                       # no Step 2 configured
        qmri_mex("pnp_admm_sms", mm(maps2), my(y2), p, nargout=1)
    assert err.value.id == "qmri:state"
    qmri_mex("set_llr", 0.05, 8.0, 1.0)
    # two groups per launch: the gateway grows the operator's plan to 2 x Z images and re-attaches the phases
    x, li = qmri_mex("pnp_admm_sms", mm(maps2), my(y2), p, np.zeros((0, 0)), 2.0, nargout=2)
    assert np.array_equal(back(x, 2), wp) and np.array_equal(li.T, wl)
    p["complex_tsmi"] = 0.0
    x, li = qmri_mex("pnp_admm_sms", mm(maps2[:1]), my(y2[:1]), p, mm(x02[:1]), nargout=2)
    assert np.array_equal(back(x, 1), wp1) and np.array_equal(li.T, wl1)
    p["solver"] = 2.0
    with pytest.raises(MexError) as err:                                       # the library's own refusal comes through by its code
        qmri_mex("pnp_admm_sms", mm(maps2[:1]), my(y2[:1]), p, nargout=1)
    assert err.value.id == "qmri:err4" and "TOEPLITZ" in err.value.msg
    qmri_mex("set_sms", np.zeros((0, 0)))                                      # cleared
    with pytest.raises(MexError) as err:
        qmri_mex("adjoint_sms", mm(maps2), my(y2), nargout=1)
    assert err.value.id == "qmri:state"
    qmri_mex("set_sms", np.asarray(c["E"], complex))
    qmri_mex("set_operator", float(N), float(M), np.asarray(c["V"], np.float64), c["fp"].astype(np.int32), c["k"].astype(np.int32), 1.0)
    with pytest.raises(MexError) as err:                                       # a new operator drops the phases
        qmri_mex("adjoint_sms", mm(maps2), my(y2), nargout=1)
    assert err.value.id == "qmri:state"
    qmri_mex("clear_llr")
    mex_exit()
