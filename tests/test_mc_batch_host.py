"""CPU: the multi-coil slice-stack entry points (include/qmri.h) are exported and refuse a NULL context or bad arguments without a device."""
import ctypes as C

import numpy as np
import pytest

NEW = ("qmri_xupdate_mc_batch", "qmri_pnp_admm_mc_batch", "qmri_pnp_admm_mc_dev")


def test_new_symbols_exported_and_declared():
    from qmri_pnp_recon_poc_amd import _lib
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(L, s)


def test_null_context_refused():
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import AdmmParams
    L = _lib.lib()
    buf = np.zeros(64, np.complex128)
    vp = buf.ctypes.data_as(C.c_void_p)
    p = AdmmParams(0.05, 2, 1e-4, 10, 0, 0, 0.01, 0)
    assert L.qmri_xupdate_mc_batch(None, 1, 1, vp, vp, vp, 0.05, 1e-4, 10, None, vp, None, None) == -1
    assert L.qmri_pnp_admm_mc_batch(None, 1, 1, 1, vp, vp, C.byref(p), None, vp, None) == -1
    assert L.qmri_pnp_admm_mc_dev(None, 1, 1, vp, vp, C.byref(p), None, vp, None) == -1


def test_engine_checks_stack_shapes_before_the_library():
    """Engine.xupdate_mc_batch / pnp_admm_mc_batch refuse mismatched stacks in Python (no context or device needed)."""
    from qmri_pnp_recon_poc_amd import engine
    e = engine.Engine.__new__(engine.Engine)
    e.N, e.M, e.s, e.m = 8, 8, 2, 10
    with pytest.raises(ValueError):
        e.xupdate_mc_batch(np.zeros((2, 8, 8, 3)), np.zeros((2, 10, 4)), np.zeros((2, 8, 8, 2)), 0.05)     # 3 coils in maps, 4 in y
    with pytest.raises(ValueError):
        e.xupdate_mc_batch(np.zeros((8, 8, 3)), np.zeros((10, 3)), np.zeros((8, 8, 2)), 0.05)                # not a stack
    with pytest.raises(ValueError):
        e.pnp_admm_mc_batch(np.zeros((2, 8, 8, 3)), np.zeros((3, 10, 3)))                                    # 2 slices of maps, 3 of y
    with pytest.raises(ValueError):
        e.xupdate_mc_batch(np.zeros((2, 8, 8, 3)), np.zeros((2, 10, 3)), np.zeros((2, 8, 8, 5)), 0.05)     # z has s = 5


def test_recon_batch_mc_refuses_bad_arguments_without_a_device():
    """qmri_recon_batch_mc checks its arguments before any worker starts: ncoil < 1, NULL maps, NULL Y, no devices."""
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import NetDesc, Problem
    L = _lib.lib()
    V = np.zeros(8)
    fp = np.array([0, 4], np.int32)
    k = np.arange(4, dtype=np.int32)
    w = np.zeros(4, np.float32)
    desc = NetDesc(0, 2, 2, (C.c_int32 * 4)(8, 16, 16, 32), 2, 0)
    pb = Problem()
    pb.N, pb.M, pb.s, pb.T = 8, 8, 2, 1
    pb.V, pb.frame_ptr, pb.kidx = V.ctypes.data_as(C.POINTER(C.c_double)), fp.ctypes.data_as(C.POINTER(C.c_int32)), k.ctypes.data_as(C.POINTER(C.c_int32))
    pb.net, pb.weights, pb.weights_nbytes = C.pointer(desc), w.ctypes.data_as(C.POINTER(C.c_float)), w.nbytes
    buf = np.zeros(1024, np.complex128)
    vp = buf.ctypes.data_as(C.c_void_p)
    devs = (C.c_int * 1)(0)
    err = C.create_string_buffer(256)
    for args in ((1, devs, 1, C.byref(pb), 0, vp, vp), (1, devs, 1, C.byref(pb), 2, None, vp), (1, devs, 1, C.byref(pb), 2, vp, None),
                 (0, devs, 1, C.byref(pb), 2, vp, vp)):
        err.value = b""
        assert L.qmri_recon_batch_mc(*args, vp, None, None, err, len(err)) == -1
        assert b"qmri_recon_batch_mc" in err.value


def test_mex_recon_batch_mc_checks_its_arguments_under_the_mock_gateway():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from mexmock import MexError, qmri_mex
    with pytest.raises(MexError) as e:
        qmri_mex("recon_batch_mc", np.zeros((4, 2, 1), np.complex128), {"iter": 1}, nargout=1)        # too few arguments
    assert e.value.id == "qmri:usage"
    with pytest.raises(MexError) as e:
        qmri_mex("recon_batch_mc", np.zeros((4, 2, 1), np.complex128), np.zeros((2, 2, 2, 1), np.complex128), {"iter": 1}, np.array([0.0]), 1.0,
                 np.array([2.0, 2.0, 1.0]), nargout=1)
    assert e.value.id == "qmri:recon_batch:state"                                                   # nothing planned yet
