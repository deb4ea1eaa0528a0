"""CPU: joint wavelet soft-thresholding (include/qmri.h qmri_wavelet_prox / qmri_set_wavelet) without a device -- the numpy
restatement tests/wavelet_ref.py against closed forms and the properties of a proximal step, the offset rule, the measured gap between the filter
bank and the dense-matrix route (the table wavelet_ref.SENS), every refusal of the new entry points, the symbol list, the header text, the geometry
sweep of csrc/wav_plan.h and the stand-alone sanitizer program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import wavelet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
NEW = ["qmri_wavelet_prox", "qmri_wavelet_prox_dev", "qmri_set_wavelet"]
BOTH = (R.HAAR, R.DB2)


@pytest.mark.parametrize("n", [2, 4, 6, 8, 14, 32, 112])
def test_periodised_filters_are_orthogonal(n):
    """W W^T = I for the n x n matrix of one level, residual <= 4e-16 (n = 2: Haar only, DB2 needs n >= 4; at n = 4 every DB2 tap wraps)."""
    for filt in BOTH:
        if n < len(R.LOWPASS[filt]):
            continue
        W = R.analysis_matrix(n, filt)
        assert np.abs(W @ W.T - np.eye(n)).max() <= 4e-16 and np.abs(W.T @ W - np.eye(n)).max() <= 4e-16, (n, filt)
        x = np.random.default_rng(n).standard_normal((n, 3))
        h, g = R.filters(filt)
        assert np.abs(R._analysis(x, h, g) - W @ x).max() <= 4e-16 * np.abs(x).max() * len(h)
        assert np.abs(R._synthesis(W @ x, h, g) - x).max() <= 1e-15 * np.abs(x).max() * len(h)


def test_filter_constants_of_the_kernel_header_are_numpys():
    """csrc/wav_kernels.hip states the taps as the doubles numpy computes from the closed forms, printed to 17 digits."""
    src = open(os.path.join(CSRC, "wav_kernels.hip")).read()
    for filt in BOTH:
        h, g = R.filters(filt)
        for v in np.concatenate([h, g]):
            assert ("%.17g" % abs(v)) in src, (filt, v)
        assert np.array_equal(g, [(-1.0) ** j * h[len(h) - 1 - j] for j in range(len(h))])
    # the low-pass taps sum to sqrt 2 and their squares to 1: four terms, so three roundings of the sum at the most
    assert abs(R.LOWPASS[R.DB2].sum() - np.sqrt(2.0)) <= 3 * np.spacing(np.sqrt(2.0)) and abs((R.LOWPASS[R.DB2] ** 2).sum() - 1.0) <= 3 * np.spacing(1.0)


def test_tau_zero_is_the_identity_haar_gives_block_means_and_zero_stays_zero():
    X = R.tsmi_like(48, 80, 3)
    for filt in BOTH:
        for L in (1, 3, 4):
            for off in R.fixture_offsets(L):
                for joint in (False, True):
                    out, cm = R.wavelet_prox(X, 0.0, L, filt, joint, off)
                    assert np.abs(out - X).max() <= 6e-15 * np.abs(X).max(), (filt, L, off)
                    assert np.abs(R.idwt2(R.dwt2(X, L, filt), L, filt) - X).max() <= 6e-15 * np.abs(X).max()
                    if filt == R.HAAR:
                        for real in (False, True):
                            z, _ = R.wavelet_prox(X, 2.0 * cm, L, filt, joint, off, real)
                            assert np.abs(z - R.haar_block_means(X, L, off, real)).max() <= 6e-15 * np.abs(X).max(), (L, off, joint, real)
                zero, c0 = R.wavelet_prox(np.zeros((32, 32, 2)), 0.3, L, filt, True, off)
                assert not zero.any() and c0 == 0.0 and np.all(np.isfinite(zero.view(np.float64)))


def test_real_mode_and_mallat_layout():
    X = R.tsmi_like(32, 64, 3)
    for filt in BOTH:
        out, cm = R.wavelet_prox(X, 0.05, 3, filt, True, (3, 5), real=True)
        ref, cr = R.wavelet_prox(X.real, 0.05, 3, filt, True, (3, 5))
        assert np.array_equal(out.imag, np.zeros_like(out.imag)) and np.array_equal(out, ref) and cm == cr
    # a constant image: only the final approximation corner is non-zero, and it holds 2^L times the constant
    for filt in BOTH:
        C3 = R.dwt2(np.full((32, 64, 1), 1.5), 3, filt)
        assert np.abs(C3[:4, :8] - 1.5 * 8).max() <= 1e-13 and np.abs(C3[R.detail_mask(32, 64, 3)]).max() <= 1e-14
    assert R.detail_mask(32, 64, 3).sum() == 32 * 64 - 4 * 8


def _objective(v, x, tau, L, filt, joint):
    C = R.dwt2(v, L, filt)
    m = np.sqrt((np.abs(C) ** 2).sum(axis=2)) if joint else np.abs(C).sum(axis=2)
    return 0.5 * np.linalg.norm(v - x) ** 2 + tau * m[R.detail_mask(*x.shape[:2], L)].sum()


@pytest.mark.parametrize("filt,L,joint", [(R.HAAR, 2, True), (R.DB2, 3, True), (R.DB2, 2, False), (R.HAAR, 4, False)])
def test_prox_optimality(filt, L, joint):
    """v = prox minimises 1/2 |v - x|^2 + tau sum m over the detail positions: 200 seeded perturbations of v do not lower it."""
    rng = np.random.default_rng(17 + L)
    X = R.tsmi_like(16, 32, 3, seed=L)
    _, cm = R.wavelet_prox(X, 0.0, L, filt, joint)
    tau = 0.1 * cm
    v, _ = R.wavelet_prox(X, tau, L, filt, joint)
    best = _objective(v, X, tau, L, filt, joint)
    for trial in range(200):
        d = (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)) * 10.0 ** -(trial % 4)
        if trial % 3 == 0:                      # a sparse perturbation in the coefficient domain
            Cd = np.zeros(X.shape, complex)
            Cd[rng.integers(16), rng.integers(32), rng.integers(3)] = d[0, 0, 0]
            d = R.idwt2(Cd, L, filt)
        assert _objective(v + d, X, tau, L, filt, joint) >= best * (1 - 1e-13), trial


def test_non_expansive_on_random_pairs():
    rng = np.random.default_rng(5)
    for trial in range(12):
        filt, L = BOTH[trial % 2], (1, 2, 3)[trial % 3]
        s = (1, 2, 5, 16)[trial % 4]
        X = rng.standard_normal((32, 32, s)) + 1j * rng.standard_normal((32, 32, s))
        Y = X + (10.0 ** -(trial % 3)) * (rng.standard_normal((32, 32, s)) + 1j * rng.standard_normal((32, 32, s)))
        tau = (0.5, 2.0, 8.0)[trial % 3]
        off = (trial % (1 << L), (3 * trial) % (1 << L))
        px, _ = R.wavelet_prox(X, tau, L, filt, trial % 2 == 0, off)
        py, _ = R.wavelet_prox(Y, tau, L, filt, trial % 2 == 0, off)
        assert np.linalg.norm(px - py) <= np.linalg.norm(X - Y) * (1 + 1e-12), trial


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_offset_rule_visits_every_offset_once_per_cycle(L):
    import llr_ref
    P = 1 << L
    seen = [R.offsets(it, P) for it in range(P * P)]
    assert len(set(seen)) == P * P and all(0 <= o1 < P and 0 <= o2 < P for o1, o2 in seen)
    assert [R.offsets(it, P) for it in range(P * P, 2 * P * P)] == seen and R.offsets(0, P) == (0, 0)
    assert all(R.offsets(it, P, shift=False) == (0, 0) for it in range(3 * P))
    for it in (0, 1, P, P * P - 1, P * P + 3):
        q = it % (P * P)
        assert R.offsets(it, P) == (q % P, (q // P + q) % P) == llr_ref.offsets(it, P)


@pytest.mark.parametrize("filt", BOTH)
@pytest.mark.parametrize("L", R.FIXTURE_LEVELS)
def test_gap_between_the_filter_bank_and_the_dense_route(filt, L):
    """max |filter bank - dense matrices| / max |X| per fixture family (filter, L, joint, real) over the grids, channel counts, offsets and thresholds
    the GPU test uses.  wavelet_ref.SENS holds these figures with a factor 2 of room: asserted from above, and from below at a quarter (the table
    is the measurement, not a wish).  The shrink is 1-Lipschitz and has no ill-conditioned step, so the gap is a few rounding errors per pass."""
    for joint in (False, True):
        for real in (False, True):
            gap, entry = R.measure_sens(filt, L, joint, real), R.SENS[(filt, L, joint, real)]
            print(f"filter {filt} L {L} joint {joint} real {real}: measured {gap:.3e}, table {entry:.1e}, GPU tolerance {R.atol(filt, L, joint, real):.1e}")
            assert entry / 4 <= gap <= entry, (filt, L, joint, real, gap, entry)
            assert R.atol(filt, L, joint, real) == 16 * entry <= 1e-13


def test_symbols_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert "qmri_wavelet_params" in header and re.search(r"#define\s+QMRI_WAVELET_HAAR\s+0\b", header) and re.search(r"#define\s+QMRI_WAVELET_DB2\s+1\b", header)
    section = header[header.index("joint wavelet soft-thresholding (extension"):]
    head = section[:section.index("*/")]
    assert "extension" in head and "no reference counterpart" in head and "parity unpinned" in head
    assert "o2 = (q div P + q) mod P" in section and "exactly 0" in section and "qmri_set_llr(ctx, NULL)" in section
    assert re.search(r"#define\s+QMRI_ABI_VERSION\s+1\b", header) and _lib.lib().qmri_abi_version() == 1
    assert C.sizeof(_lib.WaveletParams) == 40 and C.sizeof(_lib.LlrParams) == 40


def test_every_refusal_of_the_new_entry_points_without_a_device():
    """The argument rules run before the context is looked at: with ctx == NULL each call returns the code of its first failing check and leaves the
    message in qmri_last_error(NULL); a call whose arguments are all fine is refused for the missing context."""
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import WaveletParams
    L = _lib.lib()
    x, out = np.zeros(2 * 16 * 32 * 3 * 2), np.zeros(2 * 16 * 32 * 3 * 2)

    def P(tau=0.1, levels=3, filt=1, joint=1, shift=0, reserved=(0, 0, 0, 0)):
        return WaveletParams(tau, levels, filt, joint, shift, (C.c_int32 * 4)(*reserved))

    def call(fn, N=16, M=32, s=3, S=2, x=x, cpx=1, p=P(), o1=0, o2=0, out=out):
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        st = fn(None, N, M, s, S, vp(x), cpx, C.byref(p) if p is not None else None, o1, o2, vp(out), None)
        return st, L.qmri_last_error(None)

    nan, inf = float("nan"), float("inf")
    cases = [(dict(x=None), b"x / p / out"), (dict(p=None), b"x / p / out"), (dict(out=None), b"x / p / out"), (dict(S=0), b"nslices"),
             (dict(s=0), b"1 <= s <= 16"), (dict(s=17), b"1 <= s <= 16"), (dict(p=P(tau=-1e-9)), b"tau"), (dict(p=P(tau=nan)), b"tau"),
             (dict(p=P(tau=inf)), b"tau"), (dict(p=P(levels=-1)), b"levels must be"), (dict(p=P(levels=5)), b"levels must be"),
             (dict(p=P(filt=2)), b"filter must be"), (dict(p=P(filt=-1)), b"filter must be"), (dict(p=P(joint=2)), b"joint"), (dict(p=P(joint=-1)), b"joint"),
             (dict(p=P(reserved=(0, 0, 0, 1))), b"reserved"), (dict(p=P(reserved=(-1, 0, 0, 0))), b"reserved"),
             (dict(N=12), b"multiples of 2^levels with N / 2^(levels-1) and M / 2^(levels-1) at least the filter length (N = 12, M = 32, levels = 3, 4 taps)"),
             (dict(M=36), b"multiples of 2^levels"), (dict(N=0), b"multiples of 2^levels"), (dict(M=-8), b"multiples of 2^levels"),
             (dict(p=P(levels=4)), b"levels = 4, 4 taps"), (dict(p=P(levels=4, filt=0), M=40), b"levels = 4, 2 taps"), (dict(p=P(levels=0), N=12), b"levels = 3"),
             (dict(o1=-1), b"offsets"), (dict(o1=8), b"offsets"), (dict(o2=8), b"offsets"), (dict(p=P(levels=2), o2=4), b"offsets"),
             (dict(), b"ctx"), (dict(cpx=0), b"ctx"), (dict(p=P(levels=0)), b"ctx"), (dict(p=P(levels=2, shift=7), o1=3, o2=3), b"ctx"),
             (dict(p=P(levels=4, filt=0), o1=15, o2=15), b"ctx"), (dict(p=P(tau=0.0, joint=0)), b"ctx")]
    for fn in (L.qmri_wavelet_prox, L.qmri_wavelet_prox_dev):
        for kw, word in cases:
            st, msg = call(fn, **kw)
            assert st == -1 and word in msg, (kw, st, msg)
    for p, word in ((P(tau=-1.0), b"tau"), (P(tau=nan), b"tau"), (P(levels=5), b"levels must be"), (P(filt=3), b"filter must be"), (P(joint=2), b"joint"),
                    (P(shift=2), b"shift"), (P(shift=-1), b"shift"), (P(reserved=(0, 1, 0, 0)), b"reserved"), (P(), b"ctx"), (P(levels=0, shift=1), b"ctx")):
        st = L.qmri_set_wavelet(None, C.byref(p))
        assert st == -1 and word in L.qmri_last_error(None), (word, L.qmri_last_error(None))
    assert L.qmri_set_wavelet(None, None) == -1 and b"ctx" in L.qmri_last_error(None)


def test_make_wavelet_and_the_harness_check_their_arguments_before_any_device_call():
    from qmri_pnp_recon_poc_amd import harness, reference_api as RA
    F = RA.SimpleNamespace(_engine=object())
    net = RA.make_wavelet(F, tau_rel=0.01, levels=2, filter="haar", joint=False, shift=False)
    assert net._wavelet and net._engine is F._engine
    assert (net.tau, net.tau_rel, net.levels, net.filter, net.joint, net.shift) == (None, 0.01, 2, "haar", False, False)
    d = RA.make_wavelet(F)
    assert (d.tau_rel, d.levels, d.filter, d.joint, d.shift) == (RA.WAVELET_TAU_REL, 3, "db2", True, True) and RA.WAVELET_TAU_REL == 0.05
    assert RA.make_wavelet(F, tau=0.5).tau == 0.5
    for kw in (dict(levels=0), dict(levels=5), dict(filter="db4"), dict(tau=-1.0), dict(tau=np.nan), dict(tau_rel=-0.1), dict(tau_rel=np.inf)):
        with pytest.raises(ValueError):
            RA.make_wavelet(F, **kw)
    with pytest.raises(TypeError):
        RA.make_wavelet(object())
    dic, X0, q0 = {"V": np.ones((4, 1))}, np.zeros((8, 8, 1)), np.zeros((8, 8, 3))
    with pytest.raises(ValueError, match='"net", "llr" or "wavelet"'):
        harness.recon_tsmis(dic, X0, q0, regulariser="tv")
    with pytest.raises(ValueError, match="PnP_ADMM"):
        harness.recon_tsmis(dic, X0, q0, regulariser="wavelet", recon_method="SVD_MRF")


def test_mex_wavelet_commands_check_their_arguments_under_the_mock_gateway():
    from mexmock import MexError, qmri_mex
    X = np.ones((16, 32, 3), complex)
    wp = "wavelet_prox"
    cases = [(wp, (X,), "qmri:usage"), (wp, (X, 0.1, 3.0, 1.0, 1.0, 1.0), "qmri:usage"), (wp, (X.astype(np.complex64), 0.1), "qmri:wavelet_prox:type"),
             (wp, (X, -0.1), "qmri:wavelet_prox:tau"), (wp, (X, np.nan), "qmri:wavelet_prox:tau"), (wp, (X, np.ones(2)), "qmri:wavelet_prox:tau"),
             (wp, (X, 0.1, 5.0), "qmri:wavelet_prox:levels"), (wp, (X, 0.1, 0.0), "qmri:wavelet_prox:levels"), (wp, (X, 0.1, 2.5), "qmri:wavelet_prox:levels"),
             (wp, (X, 0.1, 3.0, 2.0), "qmri:wavelet_prox:filter"), (wp, (X, 0.1, 3.0, 1.0, 2.0), "qmri:wavelet_prox:joint"),
             (wp, (X, 0.1, 3.0, 1.0, 1.0, 8.0, 0.0), "qmri:wavelet_prox:offset"), (wp, (X, 0.1, 2.0, 0.0, 1.0, 0.0, 4.0), "qmri:wavelet_prox:offset"),
             (wp, (X, 0.1, 3.0, 1.0, 1.0, -1.0, 0.0), "qmri:wavelet_prox:offset"), (wp, (np.ones((12, 32, 3), complex), 0.1), "qmri:wavelet_prox:size"),
             (wp, (X, 0.1, 4.0, 1.0), "qmri:wavelet_prox:size"), (wp, (np.ones((16, 40, 3), complex), 0.1, 4.0, 0.0), "qmri:wavelet_prox:size"),
             (wp, (np.ones((16, 32, 17), complex), 0.1), "qmri:wavelet_prox:size"), (wp, (np.ones((16, 32, 2, 2, 2), complex), 0.1), "qmri:wavelet_prox:size"),
             ("set_wavelet", (), "qmri:usage"), ("set_wavelet", (-1.0,), "qmri:set_wavelet:tau"), ("set_wavelet", (np.inf,), "qmri:set_wavelet:tau"),
             ("set_wavelet", (1j,), "qmri:set_wavelet:tau"), ("set_wavelet", (0.1, 6.0), "qmri:set_wavelet:levels"), ("set_wavelet", (0.1, 0.0), "qmri:set_wavelet:levels"),
             ("set_wavelet", (0.1, 3.0, 2.0), "qmri:set_wavelet:filter"), ("set_wavelet", (0.1, 3.0, 1.0, 2.0), "qmri:set_wavelet:joint"),
             ("set_wavelet", (0.1, 3.0, 1.0, 1.0, 2.0), "qmri:set_wavelet:shift"), ("set_wavelet", (0.1, 3.0, 1.0, 1.0, 0.5), "qmri:set_wavelet:shift")]
    for cmd, args, ident in cases:
        with pytest.raises(MexError) as err:
            qmri_mex(cmd, *args, nargout=1)
        assert err.value.id == ident, (cmd, args[1:], ident, err.value.id, err.value.msg)
    src = open(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "matlab", "PnP_ADMM_hip.m")).read()
    assert "qmri_mex('set_wavelet'" in src and "qmri_mex('clear_wavelet')" in src and "qmri_mex('wavelet_prox'" in src and "'qmri_wavelet'" in src
    make = open(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "matlab", "qmri_make_wavelet.m")).read()
    assert "'qmri_wavelet', true" in make and "'tau_rel', 0.05" in make


def test_design_section_and_documents_exist():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 29\. .*wavelet", design, re.M | re.I)
    assert m, "DESIGN.md section 29"
    sec = design[m.start():]
    for word in ("wav_plan.h", "k_wav_fwd", "k_wav_shrink", "k_wav_inv", "LDS", "VGPR", "tau_rel", "Not built", "wav_times"):
        assert word in sec, word
    assert "wavelet" in open(os.path.join(ROOT, "README.md")).read() and "qmri_make_wavelet" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_wav_plan_header_stands_alone():
    """wav_plan.h is plain C++17: it compiles on its own, without HIP and without the library's other headers."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "wav_plan.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_wav_plan_sweep_under_address_and_ub_sanitizer(tmp_path):
    """tests/cpp/wav_plan_test.cpp: every coefficient position written by exactly one tile, every halo index in range after wrapping, no launch reading
    the buffer it writes, the scratch sizes covering every index -- over N, M in {16, 32, 48, 80, 112, 256}, L = 1..4, both filters, s in {1, 16}, B in {1, 3}."""
    exe = tmp_path / "wav_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "wav_plan_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WAV_PLAN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    swept, refused = (int(v) for v in re.search(r"swept (\d+) refused (\d+)", r.stdout).groups())
    # 36 grids x 4 levels x 2 filters = 288 cases; refused: a side of 16 with DB2 at L = 4 (16 / 8 = 2 < 4 taps) on either axis: 11 grids
    assert refused == 11 and swept == (288 - 11) * 4


def test_refusals_and_mutual_exclusion_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_wav.cpp against the host-only sanitised library: every refusal of qmri_wavelet_prox,
    qmri_wavelet_prox_dev and qmri_set_wavelet without a context and with one, the mutual exclusion with qmri_set_llr and the offset rule of the ADMM
    loop, as a stand-alone program."""
    subprocess.run(["make", "-C", CSRC, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    if not rt_dirs:
        pytest.skip("clang sanitizer runtime not found")
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_build_asan", "host_asan_wav")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_WAV_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
