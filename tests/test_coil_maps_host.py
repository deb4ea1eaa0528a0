"""CPU: the numpy restatement of the coil-map estimate (tests/coil_maps_ref.py) on the shared fixture -- its conventions, its gauges, the conditions
the GPU comparison rests on and its accuracy against the true maps -- and the host side of the new entry points without a device: exports, every
refusal, the Engine's shape checks, the MEX command's argument checks under the mock gateway, and the refusals under the sanitised host build."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coil_maps_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qmri_coil_maps", "qmri_coil_maps_dev")
THRESH = 0.1
ACCURACY_RMS = 0.0663         # measured on the fixture below (object gauge, 7 x 7 patch, Hann taper): see test_accuracy_against_the_true_maps


def true_maps(N, M, nc):
    """The _coil_maps formula of tests/test_gpu_operator.py (copied), on an N x M grid: smooth phases, sum_j |C_j|^2 = 1."""
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww)) for a in np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def phantom(N, M):
    """Piecewise-constant magnitude with a smooth non-trivial phase; support S: an ellipse covering about half the grid."""
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    S = (hh / 0.85) ** 2 + (ww / 0.75) ** 2 <= 1.0
    mag = np.where(S, 1.0, 0.0)
    mag[(hh + 0.2) ** 2 + (ww - 0.1) ** 2 <= 0.1] = 0.6
    mag[(np.abs(hh - 0.4) <= 0.15) & (np.abs(ww + 0.25) <= 0.2)] = 1.4
    return mag * np.exp(1j * (0.8 * hh + 0.5 * ww ** 2 - 0.3 * hh * ww)), S


_CACHE = {}


def fixture(N=32, M=32, nc=8, cN=16, cM=16, seed=0, noise=0.01):
    """dict(x, S, C, block, N, M): the calibration block cN x cM x nc is cut from fft2(C_j x) / sqrt(NM), plus 1 % complex noise (seeded)."""
    key = (N, M, nc, cN, cM, seed, noise)
    if key not in _CACHE:
        x, S = phantom(N, M)
        Ct = true_maps(N, M, nc)
        block = R.centre_block(Ct * x[..., None], cN, cM)
        rng = np.random.default_rng(seed)
        block = block + noise * np.abs(block).mean() * (rng.standard_normal(block.shape) + 1j * rng.standard_normal(block.shape))
        for a in (x, S, Ct, block):
            a.setflags(write=False)
        _CACHE[key] = dict(x=x, S=S, C=Ct, block=block, N=N, M=M)
    return _CACHE[key]


def test_untapered_full_size_block_inverts_fft2():
    """Sign, origin and scale: the block of a whole grid, untapered, gives the images back exactly; and the k = 0 entry sits at (cN/2, cM/2)."""
    rng = np.random.default_rng(1)
    for N, M in ((32, 32), (16, 24)):
        img = rng.standard_normal((N, M, 3)) + 1j * rng.standard_normal((N, M, 3))
        full = R.centre_block(img, N, M)
        assert np.allclose(full[N // 2, M // 2], img.sum(axis=(0, 1)) / np.sqrt(N * M), rtol=1e-12)
        back = R.calib_images(full, N, M, window=False)
        assert np.max(np.abs(back - img)) <= 1e-13 * np.max(np.abs(img))
    small = R.centre_block(img, 8, 12)
    assert np.array_equal(small, full[N // 2 - 4:N // 2 + 4, M // 2 - 6:M // 2 + 6])
    w = R.hann(16)
    assert w[8] == 1.0 and abs(w[0]) < 1e-16 and np.allclose(w[1:], w[1:][::-1])


def test_restatement_norm_and_gauges():
    f = fixture()
    for ref in ("object", "coil"):
        C_, img, l1, l2, kept, I, rc = R.coil_maps_ref(f["block"], 32, 32, phase_ref=ref, thresh=THRESH, full=True)
        nrm = np.sqrt(np.sum(np.abs(C_) ** 2, axis=2))
        assert np.max(np.abs(nrm[kept] - 1.0)) < 1e-13 and np.all(nrm[~kept] == 0.0)
        assert np.all(l1 >= 0) and np.all(l2 <= l1)
        if ref == "object":
            assert np.all(img.real[kept] >= 0) and np.max(np.abs(img.imag)) <= 1e-13 * np.max(np.abs(img))
        else:
            c = C_[..., rc]
            assert np.all(c.real[kept] >= 0) and np.max(np.abs(c.imag)) <= 1e-13
    # patch = 0: the closed form u = I / |I|
    C0, _, l10 = R.coil_maps_ref(f["block"], 32, 32, patch=0, phase_ref="coil")
    I = R.calib_images(f["block"], 32, 32)
    rc = int(np.argmax(np.sum(np.abs(I) ** 2, axis=(0, 1))))
    want = I / np.linalg.norm(I, axis=2, keepdims=True) * np.exp(-1j * np.angle(I[..., rc]))[..., None]
    assert np.max(np.abs(C0 - want)) < 1e-12 and np.max(np.abs(l10 - np.sum(np.abs(I) ** 2, axis=2))) < 1e-12 * l10.max()


@pytest.mark.parametrize("N,M,cN,cM", [(32, 32, 16, 16), (64, 96, 24, 16)])
def test_conditions_the_gpu_comparison_rests_on(N, M, cN, cM):
    """With thresh = 0.1 the kept set covers >= 90 % of the support, and on every kept pixel lambda_2 / lambda_1 <= 0.1."""
    f = fixture(N, M, 8, cN, cM)
    for window in (True, False):
        for p in (1, 3):
            _, _, l1, l2, kept, _, _ = R.coil_maps_ref(f["block"], N, M, patch=p, window=window, thresh=THRESH, full=True)
            cover = np.mean(kept[f["S"]])
            ratio = np.max(l2[kept] / l1[kept])
            print(f"{N}x{M} window {window} p {p}: kept covers {cover:.3f} of S, max lambda2/lambda1 on kept {ratio:.4f}")
            assert cover >= 0.9 and ratio <= 0.1


def test_accuracy_against_the_true_maps():
    """The true maps in the object gauge, C_true e^{i arg x}: RMS of |C_hat(r) - C_true(r)|_2 over kept and S.  The limit is the estimator's own
    smoothing bias (patch and taper); the assertion is twice the value measured when the fixture was written (0.0663: DESIGN.md section 17), a
    regression fence on the restatement only."""
    f = fixture()
    C_, _, _, _, kept, _, _ = R.coil_maps_ref(f["block"], 32, 32, thresh=THRESH, full=True)
    Ct = f["C"] * np.exp(1j * np.angle(f["x"]))[..., None]
    sel = kept & f["S"]
    rms = np.sqrt(np.mean(np.sum(np.abs(C_ - Ct) ** 2, axis=2)[sel]))
    print("RMS error of the estimated maps over kept and S:", rms)
    assert rms <= 2 * ACCURACY_RMS


def test_symbols_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert "qmri_csm_params" in header and "qmri_csm_info" in header and "QMRI_CSM_PARAMS_DEFAULT" in header
    assert re.search(r"#define\s+QMRI_ABI_VERSION\s+1\b", header) and _lib.lib().qmri_abi_version() == 1
    assert C.sizeof(_lib.CsmParams) == 32 and C.sizeof(_lib.CsmInfo) == 8


def test_every_refusal_of_both_entry_points_without_a_device():
    """The argument rules run before the context is looked at: with ctx == NULL each call returns the code of its first failing check and leaves
    the message in qmri_last_error(NULL); a call whose arguments are all fine is refused for the missing context."""
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import CsmInfo, CsmParams
    L = _lib.lib()
    buf, out = np.zeros(64, np.complex128), np.zeros(64, np.complex128)
    a, b = buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    info = CsmInfo()

    def P(kind=0, cN=16, cM=16, patch=3, window=1, phase=0, thresh=0.0):
        return CsmParams(kind, cN, cM, patch, window, phase, thresh)

    cases = [  # (nslices, ncoil, N, M, calib, params, maps_out, code, word)
        (1, 8, 32, 32, a, None, b, -1, b"params"), (1, 8, 32, 32, None, P(), b, -1, b"calib"), (1, 8, 32, 32, a, P(), None, -1, b"maps_out"),
        (0, 8, 32, 32, a, P(), b, -1, b"nslices"), (1, 0, 32, 32, a, P(), b, -1, b"ncoil"), (1, 129, 32, 32, a, P(), b, -4, b"128"),
        (1, 8, 30, 32, a, P(), b, -1, b"supported sizes"), (1, 8, 32, 100, a, P(), b, -1, b"supported sizes"),
        (1, 8, 32, 32, a, P(kind=2), b, -1, b"kind"), (1, 8, 32, 32, a, P(cN=15), b, -1, b"cN"), (1, 8, 32, 32, a, P(cN=6), b, -1, b"cN"),
        (1, 8, 32, 32, a, P(cN=34), b, -1, b"cN"), (1, 8, 32, 64, a, P(cM=17), b, -1, b"cM"), (1, 8, 32, 64, a, P(cM=66), b, -1, b"cM"),
        (1, 8, 32, 32, a, P(window=2), b, -1, b"window"), (1, 8, 32, 32, a, P(patch=-1), b, -1, b"patch"), (1, 8, 32, 32, a, P(patch=5), b, -1, b"patch"),
        (1, 8, 32, 32, a, P(phase=2), b, -1, b"phase_ref"), (1, 8, 32, 32, a, P(thresh=-1.0), b, -1, b"thresh"),
        (1, 8, 32, 32, a, P(thresh=float("nan")), b, -1, b"thresh"), (1, 8, 32, 32, a, P(), b, -1, b"ctx"), (1, 128, 256, 32, a, P(kind=1, cN=0, cM=0), b, -1, b"ctx"),
    ]
    for fn in (L.qmri_coil_maps, L.qmri_coil_maps_dev):
        for S, nc, N, M, cal, p, mo, code, word in cases:
            st = fn(None, S, nc, N, M, cal, C.byref(p) if p is not None else None, mo, None, None, C.byref(info))
            assert st == code and word in L.qmri_last_error(None), (S, nc, N, M, st, L.qmri_last_error(None))
    assert L.qmri_coil_maps_dev(None, 1, 8, 32, 32, a, C.byref(P()), a, None, None, None) == -1 and b"alias" in L.qmri_last_error(None)


def test_engine_coil_maps_checks_shapes_before_the_library():
    from qmri_pnp_recon_poc_amd import engine
    e = engine.Engine.__new__(engine.Engine)
    e.N, e.M, e.s, e.m = 32, 64, 2, 10
    z = np.zeros
    bad = [dict(calib=z((16, 16))), dict(calib=z((2, 2, 16, 16, 4))), dict(calib=z((15, 16, 4))), dict(calib=z((16, 6, 4))), dict(calib=z((34, 16, 4))),
           dict(calib=z((16, 66, 4))), dict(calib=z((16, 16, 129))), dict(calib=z((0, 16, 16, 4))), dict(calib=z((64, 32, 4)), kind="images"),
           dict(calib=z((16, 16, 4)), kind="acs"), dict(calib=z((16, 16, 4)), phase_ref="first"), dict(calib=z((16, 16, 4)), patch=5),
           dict(calib=z((16, 16, 4)), patch=1.5), dict(calib=z((16, 16, 4)), thresh=-0.1)]
    for kw in bad:
        with pytest.raises(ValueError):
            e.coil_maps(**kw)


def test_mex_coil_maps_checks_its_arguments_under_the_mock_gateway():
    from mexmock import MexError, qmri_mex
    with pytest.raises(MexError) as e:
        qmri_mex("coil_maps", np.zeros((16, 16, 4), np.complex128), nargout=1)                      # too few arguments
    assert e.value.id == "qmri:usage"
    with pytest.raises(MexError) as e:
        qmri_mex("coil_maps", np.zeros((16, 16, 4), np.complex128), 3.0, nargout=1)                 # opts is not a struct
    assert e.value.id == "qmri:coil_maps:opts"
    with pytest.raises(MexError) as e:
        qmri_mex("coil_maps", np.zeros((16, 16, 4), np.complex128), {"patch": 3.0}, nargout=1)      # no operator yet
    assert e.value.id == "qmri:state"


def test_refusals_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_coilmaps.cpp against the host-only sanitised library: every refusal of qmri_coil_maps and
    qmri_coil_maps_dev without a context, with an operator of another grid and without an operator, and the eigen kernel's LDS plan for every
    (ncoil, patch)."""
    csrc = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    if not rt_dirs:
        pytest.skip("clang sanitizer runtime not found")
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "_build_asan", "host_asan_coilmaps")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_COILMAPS_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
