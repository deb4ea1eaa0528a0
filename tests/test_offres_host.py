"""CPU: the numpy restatement of the time-segmented off-resonance correction (tests/offres_ref.py) against the exact operator with the field term,
and the host side of qmri_set_field_map: declared, exported, every refusal, the Python argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nufft_ref as R
import offres_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmented_operator_against_the_exact_one():
    """eps_ref(L) on the 32 x 32 spiral (s = 3) and on the 32 x 64 random case: the recorded table is what the restatement gives, and the error
    falls at least 5x per added segment over L = 3 ... 6."""
    for name, case in (("spiral32", F.spiral_case(s=3)), ("rect32x64", F.rect_case())):
        got = {}
        for L in (3, 4, 5, 6):
            ef, ea = F.eps_ref(case, L)
            got[L] = max(ef, ea)
            print(f"{name} L = {L}: forward {ef:.3e} adjoint {ea:.3e} recorded {F.EPS_REF[name][L]:.3e}")
            assert abs(got[L] - F.EPS_REF[name][L]) <= 0.02 * F.EPS_REF[name][L]
        for L in (4, 5, 6):
            assert got[L] <= got[L - 1] / 5, (name, L, got)


def test_the_approximation_itself():
    """max over pixels x samples of the segmentation error on the 32 x 32 field, 5 ms readout: about 10x per segment; fit_max (bins) tracks it."""
    _, _, _, f, tau = F.spiral_case()
    prev = None
    for L, bound in ((3, 1.5e-1), (4, 1.7e-2), (5, 1.9e-3), (6, 1.7e-4), (8, 5.7e-6)):
        sg = F.Segmentation(f, tau, L)
        err = sg.approximation_error()
        print(f"L = {L}: max error {err:.3e}, fit_max {sg.fit_max:.3e}, fit_rms {sg.fit_rms:.3e}")
        assert err <= bound and sg.fit_max <= err * 1.0000001 and sg.fit_rms <= sg.fit_max
        assert prev is None or err <= prev / 5
        prev = err


def test_restatement_is_adjoint():
    case = F.spiral_case(s=3)
    fp, om, V, f, tau = case
    N = f.shape[0]
    x, y = F.vectors(N, N, 3, om.shape[0])
    sg = F.Segmentation(f, tau, 6)
    Ax, Ahy = F.segmented_forward(x, om, V, fp, sg), F.segmented_adjoint(y, om, V, fp, N, N, sg)
    gap = abs(np.vdot(y, Ax) - np.vdot(Ahy, x)) / (np.linalg.norm(Ax) * np.linalg.norm(y))
    Ex, Ehy = F.exact_forward(x, om, V, fp, f, tau), F.exact_adjoint(y, om, V, fp, N, N, f, tau)
    gap_e = abs(np.vdot(y, Ex) - np.vdot(Ehy, x)) / (np.linalg.norm(Ex) * np.linalg.norm(y))
    print("segmented:", gap, " exact:", gap_e)
    assert gap <= 1e-12 and gap_e <= 1e-12


def test_constant_map_is_exact_at_one_segment():
    fp, om, V, _, tau = F.spiral_case(s=3)
    N = 32
    f = np.full((N, N), 80.0)
    x, _ = F.vectors(N, N, 3, om.shape[0])
    sg = F.Segmentation(f, tau, 1)
    ys = F.segmented_forward(x, om, V, fp, sg)
    ye = F.exact_forward(x, om, V, fp, f, tau)
    assert sg.fit_max == 0.0 and np.linalg.norm(ys - ye) <= 1e-13 * np.linalg.norm(ye)
    assert np.linalg.norm(ys - np.exp(-2j * np.pi * 80.0 * tau) * R.nudft_forward(x, om, V, fp)) <= 1e-13 * np.linalg.norm(ye)


def test_symbol_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    assert re.search(r"\bint\s+qmri_set_field_map\s*\(", header)
    assert "qmri_set_field_map" in _lib.SYMBOLS and hasattr(_lib.lib(), "qmri_set_field_map")
    assert re.search(r"#define QMRI_ABI_VERSION 1\b", header)
    assert C.sizeof(_lib.OffresParams) == 32 and C.sizeof(_lib.OffresInfo) == 72       # (the C layout)
    assert _lib.lib().qmri_set_field_map(None, None, None, None, None) == -1


def test_python_argument_checks_and_readout_times():
    """Checked before the library is called: no context is needed (an Engine without __init__)."""
    from qmri_pnp_recon_poc_amd import engine as E
    t = E.spiral_readout_times(60, 48, 5e-3)
    assert t.shape == (2880,) and t.dtype == np.float64 and np.array_equal(t, F.readout_times(60, 48, 5e-3))
    assert t[0] == 0 and t[60] == 0 and t[59] == 59 * (5e-3 / 60)
    for bad in ((0, 4, 1e-3), (4, 0, 1e-3), (4, 4, -1.0), (4, 4, float("nan")), (2.5, 4, 1e-3)):
        with pytest.raises(ValueError):
            E.spiral_readout_times(*bad)
    e = E.Engine.__new__(E.Engine)
    e.N, e.M, e.s, e.T, e.m, e.h = 32, 64, 1, 2, 8, None
    f, tau = np.zeros((32, 64)), np.zeros(8)
    for args, kw in (((f.T, tau), {}), ((f + 0j, tau), {}), ((f, None), {}), ((f, tau[:-1]), {}), ((f, tau + 0j), {}), ((f, tau), dict(nseg=17)),
                     ((f, tau), dict(nseg=-1)), ((f, tau), dict(nseg=2.5)), ((f, tau), dict(nbins=15)), ((f, tau), dict(nbins=1025)),
                     ((f, tau), dict(tol=-1.0)), ((f, tau), dict(tol=float("nan")))):
        with pytest.raises(ValueError):
            e.set_field_map(*args, **kw)


def test_refusals_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_offres.cpp against the host-only sanitised library: null context, no operator, a gridded operator,
    a null t_s, non-finite f / t, nseg / nbins / tol / reserved out of range, nseg = 1 on a varying map, and the Toeplitz calls with a map attached."""
    csrc = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    if not rt_dirs:
        pytest.skip("clang sanitizer runtime not found")
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "_build_asan", "host_asan_offres")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_OFFRES_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
