"""CPU: the numpy restatement of the density compensation (tests/dcf_ref.py) on its own, and the host side of the new entry points
(DESIGN.md section 21): declared, exported, every refusal, the Python and MEX argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dcf_ref as D
import nufft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qmri_nufft_dcf", "qmri_set_sample_weights", "qmri_adjoint_w", "qmri_adjoint_w_dev", "qmri_adjoint_w_mc")


def test_reference_converges_on_the_spiral():
    """32 x 32, S = 60, T = 48, w = 6: the deviation after 20 iterations is below that after 10, the weights are finite and positive and span
    the orders of magnitude the spiral's density does."""
    N, S, T = 32, 60, 48
    fp, om = R.spiral_traj(N, S, T)
    plan = D.Plan(N, N, om, 6)
    w, it, dev, devs = D.iterate(plan, 20)
    print("dev after 10 / 20 iterations:", devs[9], devs[19], " max / min weight:", w.max() / w.min())
    assert it == 20 and dev == devs[19] and devs[19] < devs[9]
    assert np.all(np.isfinite(w)) and np.all(w > 0)
    assert w.max() / w.min() > 100
    ws, info = D.weights(N, N, T, om, 6, 20)
    assert info == {"iters": 20, "dev": dev} and np.array_equal(ws, D.kappa(T, 6, plan.beta) * w)
    _, it7, _, _ = D.iterate(plan, 20, tol=0.5 * (devs[6] + devs[5]))
    assert it7 == 7


def test_reference_reads_the_plans_kernel_parameters():
    assert D.plan_width(0) == 12 and D.plan_width(6) == 6
    assert D.plan_beta(6) > 0 and abs(D.plan_beta(12) - 2 * D.plan_beta(6)) < 1e-12
    # the window at zero offset is the w points around 0 and the kernel is 1 at its centre
    assert D.phi(0.0, 3.0, D.plan_beta(6)) == 1.0 and D.kernel_sum(6, D.plan_beta(6)) > 1.0


def test_scale_of_the_reference_on_one_channel():
    """kappa: with V = 1 / sqrt(T) the weighted adjoint of forward(x) is x in scale and shape, the bare adjoint is neither (exact transforms)."""
    N, S, T = 32, 60, 48
    fp, om = R.spiral_traj(N, S, T)
    V = np.full((T, 1), 1 / np.sqrt(T))
    x = D.phantom(N)[..., None].astype(np.complex128)
    y = R.nudft_forward(x, om, V, fp)
    w, _ = D.weights(N, N, T, om, 6, 20)
    aw, a = R.nudft_adjoint(w * y, om, V, fp, N, N), R.nudft_adjoint(y, om, V, fp, N, N)
    err_w, err_bare = np.linalg.norm(aw - x) / np.linalg.norm(x), D.best_fit(a, x)[1]
    c = (np.vdot(x, aw) / np.vdot(x, x)).real
    print("weighted:", err_w, " bare, best rescale:", err_bare, " scale:", c)
    assert err_w <= 0.06 and err_bare >= 0.6 and abs(c - 1) <= 0.02


def test_symbols_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert re.search(r"typedef struct \{ int32_t niter; double tol; int32_t reserved\[6\]; \} qmri_dcf_params;", header)
    assert re.search(r"typedef struct \{ int32_t iters; double dev; int32_t clamped; int32_t split_tiles; int32_t reserved\[4\]; \} qmri_dcf_info;", header)
    assert re.search(r"#define QMRI_ABI_VERSION 1\b", header)
    assert C.sizeof(_lib.DcfParams) == 40 and C.sizeof(_lib.DcfInfo) == 40          # (the C layout: int32, pad, double, int32 x 6)


def test_null_context_is_refused():
    from qmri_pnp_recon_poc_amd import _lib
    L = _lib.lib()
    buf = np.zeros(4, np.complex128)
    p = buf.ctypes.data_as(C.c_void_p)
    dp = buf.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))
    prm, info = _lib.DcfParams(), _lib.DcfInfo()
    assert L.qmri_nufft_dcf(None, C.byref(prm), dp, C.byref(info)) == -1
    assert L.qmri_set_sample_weights(None, dp) == -1
    assert L.qmri_adjoint_w(None, p, p) == -1
    assert L.qmri_adjoint_w_dev(None, p, p, 1) == -1
    assert L.qmri_adjoint_w_mc(None, p, p) == -1


def test_python_argument_checks():
    """Checked before the library is called: no context is needed (an Engine without __init__)."""
    from qmri_pnp_recon_poc_amd import engine as E
    e = E.Engine.__new__(E.Engine)
    e.N, e.M, e.s, e.T, e.m, e.h = 32, 32, 1, 2, 8, None
    for bad in (-1, 201, 2.5):
        with pytest.raises(ValueError):
            e.density_weights(niter=bad)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            e.density_weights(tol=bad)
    with pytest.raises(ValueError):
        e.set_sample_weights(np.ones(7))
    with pytest.raises(ValueError):
        e.set_sample_weights(np.ones(8) + 0j)
    with pytest.raises(ValueError):
        e.adjoint(np.zeros(7, np.complex128), weighted=True)
    with pytest.raises(ValueError) as err:
        e.pnp_admm(np.zeros(8, np.complex128), iters=1, x0="adjoint")
    assert '"dcf"' in str(err.value)
    from qmri_pnp_recon_poc_amd import harness as H
    with pytest.raises(ValueError) as err:
        H.recon_tsmis({"V": np.ones((2, 1))}, np.zeros((32, 32, 1)), np.zeros((32, 32, 3)), recon_method="SVD_MRF", subsampling_pattern="Spiral",
                      spiral_sampling_curve=20, density_compensation=True)
    assert "SpiralExact" in str(err.value)


def test_mex_argument_checks_under_the_mock_gateway():
    """What the three commands check before they need an operator; the checks that need one are in tests/test_gpu_dcf_mex.py."""
    from mexmock import MexError, qmri_mex
    y = np.zeros(4, np.complex128)
    cases = [("dcf", (-1.0,), "qmri:dcf:niter"), ("dcf", (201.0,), "qmri:dcf:niter"), ("dcf", (2.5,), "qmri:dcf:niter"), ("dcf", (float("nan"),), "qmri:dcf:niter"),
             ("dcf", (5.0, -1.0), "qmri:dcf:tol"), ("dcf", (5.0, float("nan")), "qmri:dcf:tol"), ("dcf", (5.0, np.ones(2)), "qmri:dcf:tol"),
             ("dcf", (5.0, 1e-3), "qmri:state"), ("dcf", (), "qmri:state"),
             ("set_sample_weights", (), "qmri:usage"), ("set_sample_weights", (y,), "qmri:set_sample_weights:type"),
             ("set_sample_weights", (np.ones(4, np.float32),), "qmri:set_sample_weights:type"), ("set_sample_weights", (np.ones(4),), "qmri:state"),
             ("adjoint_w", (), "qmri:usage"), ("adjoint_w", (np.ones(4),), "qmri:adjoint_w:type"), ("adjoint_w", (y,), "qmri:state")]
    for cmd, args, ident in cases:
        with pytest.raises(MexError) as e:
            qmri_mex(cmd, *args, nargout=1)
        assert e.value.id == ident, (cmd, args, e.value.id, e.value.msg)


def test_refusals_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_dcf.cpp against the host-only sanitised library: null context, no operator, a gridded operator,
    null arrays, bad niter / tol / reserved / weights / batch, and the _w calls without weights."""
    csrc = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    if not rt_dirs:
        pytest.skip("clang sanitizer runtime not found")
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "_build_asan", "host_asan_dcf")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_DCF_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
