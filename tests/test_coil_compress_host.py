"""CPU: the coil compression's host parts (include/qmri.h) without a device -- the Jacobi eigensolver against numpy.linalg.eigh, the exported and
declared symbols, a NULL context, the Python shape and argument checks and the MEX command's argument checks under the mock gateway."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coil_cc_ref import eig_desc  # noqa: E402

NEW = ("qmri_coil_compress", "qmri_coil_compress_dev", "qmri_coil_eig", "qmri_recon_batch_mc_cc")


def _eig(L, A):
    n = A.shape[0]
    Ab = np.ascontiguousarray(A.ravel(order="F"))
    ev, V = np.empty(n), np.empty(n * n, np.complex128)
    st = L.qmri_coil_eig(n, Ab.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.POINTER(C.c_double)), V.ctypes.data_as(C.c_void_p))
    return st, ev, V.reshape((n, n), order="F")


def test_coil_eig_matches_numpy_eigh():
    """Random Hermitian matrices, n = 1..128: eigenvalues within 1e-12 of max |lambda|; eigenvectors within 1e-10 after the phase rule on
    matrices whose eigenvalue gaps exceed 1e-6 (relative)."""
    from qmri_pnp_recon_poc_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    checked = 0
    for n in list(range(1, 33)) + [40, 48, 63, 64, 65, 96, 127, 128]:
        A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        A = A + A.conj().T
        st, ev, V = _eig(L, A)
        assert st == 0
        lo, Uo = eig_desc(A)
        scale = max(np.max(np.abs(lo)), 1e-300)
        assert np.max(np.abs(ev - lo)) <= 1e-12 * scale, n
        assert np.all(np.diff(ev) <= 0)
        gaps = np.abs(np.diff(lo)) / scale
        if n == 1 or gaps.min() > 1e-6:
            assert np.max(np.abs(V - Uo)) < 1e-10, n
            checked += 1
        assert np.max(np.abs(V.conj().T @ V - np.eye(n))) < 1e-12
    assert checked >= 30


def test_coil_eig_low_rank_and_phase_rule():
    """A covariance of rank 3 among 16 coils (the shape compression meets): the 13 null eigenvalues vanish to 1e-12 of the largest, and every
    column's entry of largest magnitude is real and positive."""
    from qmri_pnp_recon_poc_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(9)
    B = rng.standard_normal((16, 3)) + 1j * rng.standard_normal((16, 3))
    A = B @ np.diag([9.0, 4.0, 1.0]) @ B.conj().T
    st, ev, V = _eig(L, A)
    assert st == 0
    lo, Uo = eig_desc(A)
    assert np.max(np.abs(ev - lo)) < 1e-12 * lo[0] and np.all(np.abs(ev[3:]) < 1e-12 * ev[0])
    assert np.max(np.abs(V[:, :3] - Uo[:, :3])) < 1e-10
    for l in range(16):
        k = int(np.argmax(np.abs(V[:, l])))
        assert V[k, l].imag == 0.0 and V[k, l].real > 0


def test_coil_eig_refuses_bad_sizes():
    from qmri_pnp_recon_poc_amd import _lib
    L = _lib.lib()
    buf = np.zeros(129 * 129, np.complex128)
    ev = np.zeros(129)
    vp, dp = buf.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.POINTER(C.c_double))
    assert L.qmri_coil_eig(0, vp, dp, vp) == -1
    assert L.qmri_coil_eig(129, vp, dp, vp) == -1
    assert b"128" in L.qmri_last_error(None)
    assert L.qmri_coil_eig(4, None, dp, vp) == -1


def test_new_symbols_exported_and_declared():
    from qmri_pnp_recon_poc_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qmri.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(L, s) and f"{s}(" in header
    assert "qmri_cc_params" in header


def test_null_context_refused():
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import CcParams
    L = _lib.lib()
    buf = np.zeros(64, np.complex128)
    vp = buf.ctypes.data_as(C.c_void_p)
    p = CcParams(2, 0.99, 0)
    nv = C.c_int(0)
    assert L.qmri_coil_compress(None, 1, 4, vp, None, None, C.byref(p), C.byref(nv), vp, None, None, None) == -1
    assert L.qmri_coil_compress_dev(None, 1, 4, vp, None, None, C.byref(p), C.byref(nv), vp, None, None, None) == -1


def test_engine_coil_compress_checks_shapes_before_the_library():
    from qmri_pnp_recon_poc_amd import engine
    e = engine.Engine.__new__(engine.Engine)
    e.N, e.M, e.s, e.m = 8, 8, 2, 10
    with pytest.raises(ValueError):
        e.coil_compress(np.zeros((10, 4)))                                              # not a stack
    with pytest.raises(ValueError):
        e.coil_compress(np.zeros((2, 11, 4)))                                           # m = 11, the operator's is 10
    with pytest.raises(ValueError):
        e.coil_compress(np.zeros((2, 10, 4)), maps=np.zeros((2, 8, 8, 3)))             # 3 coils in maps, 4 in y
    with pytest.raises(ValueError):
        e.coil_compress(np.zeros((2, 10, 4)), maps=np.zeros((1, 8, 8, 4)))             # 1 slice of maps, 2 of y
    with pytest.raises(ValueError):
        e.coil_compress(np.zeros((2, 10, 4)), noise_cov=np.eye(3))                     # Psi 3 x 3 for 4 coils
    with pytest.raises(ValueError):
        e.coil_compress(np.zeros((2, 10, 4)), nv=5)                                     # nv > ncoil


def test_recon_batch_coil_compress_argument_checks():
    """batch.recon_batch refuses coil_compress / noise_cov without coil_maps, noise_cov without coil_compress, unknown fields and a Psi of the
    wrong size, in Python; and qmri_recon_batch_mc_cc refuses energy, shared, nv > ncoil, nv < 0, ncoil > 128 and a NULL cc before any worker
    starts, with a message naming itself."""
    from qmri_pnp_recon_poc_amd import _lib, batch
    from qmri_pnp_recon_poc_amd._lib import CcParams, NetDesc, Problem
    kw = dict(N=8, M=8, V=np.zeros((1, 2)), frame_ptr=np.array([0, 4]), kidx=np.arange(4), weights=np.zeros(4, np.float32), in_nc=2, out_nc=2,
              nc=(8, 16, 16, 32), nb=2)
    Y = np.zeros((1, 4, 3), np.complex128)
    maps = np.zeros((1, 8, 8, 3), np.complex128)
    with pytest.raises(ValueError):
        batch.recon_batch([0], Y, coil_compress=2, **kw)
    with pytest.raises(ValueError):
        batch.recon_batch([0], Y, coil_maps=maps, noise_cov=np.eye(3), **kw)
    with pytest.raises(ValueError):
        batch.recon_batch([0], Y, coil_maps=maps, coil_compress={"nv": 2, "rank": 1}, **kw)
    with pytest.raises(ValueError):
        batch.recon_batch([0], Y, coil_maps=maps, coil_compress=2, noise_cov=np.eye(2), **kw)
    L = _lib.lib()
    V = np.zeros(2)
    fp = np.array([0, 4], np.int32)
    k = np.arange(4, dtype=np.int32)
    w = np.zeros(4, np.float32)
    desc = NetDesc(0, 2, 2, (C.c_int32 * 4)(8, 16, 16, 32), 2, 0)
    pb = Problem()
    pb.N, pb.M, pb.s, pb.T = 8, 8, 2, 1
    pb.V, pb.frame_ptr, pb.kidx = V.ctypes.data_as(C.POINTER(C.c_double)), fp.ctypes.data_as(C.POINTER(C.c_int32)), k.ctypes.data_as(C.POINTER(C.c_int32))
    pb.net, pb.weights, pb.weights_nbytes = C.pointer(desc), w.ctypes.data_as(C.POINTER(C.c_float)), w.nbytes
    buf = np.zeros(200 * 200, np.complex128)
    vp = buf.ctypes.data_as(C.c_void_p)
    devs = (C.c_int * 1)(0)
    err = C.create_string_buffer(512)
    cases = [(3, CcParams(0, 0.99, 0), -1, b"energy"), (3, CcParams(2, 0.99, 1), -1, b"shared"), (3, CcParams(4, 0.99, 0), -1, b"nv"),
             (3, CcParams(-1, 0.99, 0), -1, b"nv"), (129, CcParams(4, 0.99, 0), -4, b"128"), (3, None, -1, b"NULL")]
    for ncoil, cc, code, word in cases:
        err.value = b""
        st = L.qmri_recon_batch_mc_cc(1, devs, 1, C.byref(pb), ncoil, vp, vp, vp, None, None, err, len(err), None, C.byref(cc) if cc else None)
        assert st == code and b"qmri_recon_batch_mc_cc" in err.value and word in err.value, (ncoil, err.value)


def test_mex_coil_compress_checks_its_arguments_under_the_mock_gateway():
    from mexmock import MexError, qmri_mex
    with pytest.raises(MexError) as e:
        qmri_mex("coil_compress", np.zeros((4, 2, 1), np.complex128), nargout=1)                                 # too few arguments
    assert e.value.id == "qmri:usage"
    with pytest.raises(MexError) as e:
        qmri_mex("coil_compress", np.zeros((4, 2, 1), np.complex128), np.zeros((0, 0)), np.zeros((0, 0)), 1.0, nargout=1)
    assert e.value.id == "qmri:state"                                                                          # no operator yet
    with pytest.raises(MexError) as e:
        qmri_mex("recon_batch_mc", np.zeros((4, 2, 1), np.complex128), np.zeros((2, 2, 2, 1), np.complex128), {"iter": 1}, np.array([0.0]), 1.0,
                 np.array([2.0, 2.0, 1.0]), 1.0, nargout=1)
    assert e.value.id == "qmri:recon_batch:state"                                                              # nothing planned yet
