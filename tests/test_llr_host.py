"""CPU: the locally low-rank proximal step (include/qmri.h qmri_llr_prox / qmri_set_llr) without a device -- the numpy
restatement tests/llr_ref.py against closed forms, the offset rule, the measured gap between the SVD definition and the Gram / eigenpair route the
kernel takes (the table llr_ref.SENS), every refusal of the new entry points, the symbol list, the header text and the stand-alone sanitizer program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import llr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qmri_llr_prox", "qmri_llr_prox_dev", "qmri_set_llr"]


@pytest.mark.parametrize("b", R.BLOCKS)
@pytest.mark.parametrize("s", [1, 3, 16])
def test_rank_one_block_is_scaled(b, s):
    """A = u v^H has the one singular value sigma = |u| |v|: the prox is max(0, 1 - tau / sigma) A."""
    rng = np.random.default_rng(b * 100 + s)
    u = rng.standard_normal(b * b) + 1j * rng.standard_normal(b * b)
    v = rng.standard_normal(s) + 1j * rng.standard_normal(s)
    X = np.outer(u, v.conj()).reshape(b, b, s)
    sigma = np.linalg.norm(u) * np.linalg.norm(v)
    for frac in (0.0, 0.25, 0.9, 1.5):
        for fn in (R.llr_prox, R.llr_prox_gram):
            out, sm = fn(X, frac * sigma, b)
            assert abs(sm - sigma) <= 1e-13 * sigma
            assert np.abs(out - max(0.0, 1.0 - frac) * X).max() <= 1e-13 * np.abs(X).max(), (fn.__name__, frac)


def test_tau_zero_is_the_identity_and_a_large_tau_gives_exact_zeros():
    X = R.tsmi_like(32, 64, 10)
    for b in R.BLOCKS:
        for off in R.fixture_offsets(b):
            out, sm = R.llr_prox(X, 0.0, b, off)
            assert np.abs(out - X).max() <= 1e-14 * np.abs(X).max()
            for fn in (R.llr_prox, R.llr_prox_gram):
                z, _ = fn(X, 1.0001 * sm, b, off)
                assert not z.any(), (fn.__name__, b, off)


def test_real_mode_and_zero_blocks():
    X = R.tsmi_like(32, 32, 3)
    X[8:16, 16:24, :] = 0.0
    for fn in (R.llr_prox, R.llr_prox_gram):
        out, _ = fn(X, 0.05, 8, (0, 0), real=True)
        ref, _ = fn(X.real, 0.05, 8, (0, 0))
        assert np.array_equal(out.imag, np.zeros_like(out.imag)) and np.abs(out - ref).max() <= 1e-13 * np.abs(X).max()   # (a real and a complex SVD)
        out, _ = fn(X, 0.05, 8)
        assert np.all(np.isfinite(out.view(np.float64))) and not out[8:16, 16:24, :].any()


def test_non_expansive_on_random_pairs():
    rng = np.random.default_rng(5)
    for trial in range(12):
        b = R.BLOCKS[trial % 3]
        s = (1, 2, 5, 16)[trial % 4]
        X = rng.standard_normal((32, 32, s)) + 1j * rng.standard_normal((32, 32, s))
        Y = X + (10.0 ** -(trial % 3)) * (rng.standard_normal((32, 32, s)) + 1j * rng.standard_normal((32, 32, s)))
        tau = (0.5, 4.0, 20.0)[trial % 3]
        off = (trial % b, (3 * trial) % b)
        px, _ = R.llr_prox(X, tau, b, off)
        py, _ = R.llr_prox(Y, tau, b, off)
        assert np.linalg.norm(px - py) <= np.linalg.norm(X - Y) * (1 + 1e-12), trial


@pytest.mark.parametrize("b", R.BLOCKS)
def test_offset_rule_visits_every_offset_once_per_cycle(b):
    seen = [R.offsets(it, b) for it in range(b * b)]
    assert len(set(seen)) == b * b and all(0 <= o1 < b and 0 <= o2 < b for o1, o2 in seen)
    assert all(seen[i][0] != seen[i + 1][0] and seen[i][1] != seen[i + 1][1] for i in range(b * b - 1))   # both coordinates move
    assert [R.offsets(it, b) for it in range(b * b, 2 * b * b)] == seen and R.offsets(0, b) == (0, 0)
    assert all(R.offsets(it, b, shift=False) == (0, 0) for it in range(3 * b))
    for it in (0, 1, b, b * b - 1, b * b + 3):
        q = it % (b * b)
        assert R.offsets(it, b) == (q % b, (q // b + q) % b)


def measured_gap(s, b, real):
    worst = 0.0
    for N, M in R.FIXTURE_GRIDS:
        X = R.tsmi_like(N, M, s)
        _, sm = R.llr_prox(X, 0.0, b, (0, 0), real)
        for off in R.fixture_offsets(b):
            for tr in R.FIXTURE_TAUS:
                a, sa = R.llr_prox(X, tr * sm, b, off, real)
                g, sg = R.llr_prox_gram(X, tr * sm, b, off, real)
                assert abs(sa - sg) <= 1e-13 * sa
                worst = max(worst, float(np.abs(a - g).max() / np.abs(X).max()))
    return worst


@pytest.mark.parametrize("s", R.FIXTURE_S)
def test_gap_between_the_svd_definition_and_the_gram_route(s):
    """max |SVD - Gram / eigh| / max |X| per fixture family (s, block, real) over the grids, offsets and thresholds the GPU test uses.  llr_ref.SENS holds
    these figures with a factor 2 of room: asserted from above, and from below at a quarter (the table is the measurement, not a wish).  The gap is
    larger than the 2e-15 a well-separated spectrum gives: sigma = sqrt(lambda) loses accuracy for the singular values near the noise floor, and
    those decide f = 1 - tau / sigma at the small thresholds."""
    for b in R.BLOCKS:
        for real in (False, True):
            gap, entry = measured_gap(s, b, real), R.SENS[(s, b, real)]
            print(f"s {s} block {b} real {real}: measured {gap:.3e}, table {entry:.1e}, GPU tolerance {R.atol(s, b, real):.1e}")
            assert entry / 4 <= gap <= entry, (s, b, real, gap, entry)
            assert R.atol(s, b, real) == 16 * entry <= 2e-12


def test_symbols_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert "qmri_llr_params" in header
    section = header[header.index("locally low-rank regulariser"):]
    head = section[:section.index("*/")]
    assert "extension" in head and "no reference counterpart" in head and "parity unpinned" in head
    assert "o2 = (q div b + q) mod b" in section and "exactly 0" in section
    assert re.search(r"#define\s+QMRI_ABI_VERSION\s+1\b", header) and _lib.lib().qmri_abi_version() == 1
    assert C.sizeof(_lib.LlrParams) == 40


def test_every_refusal_of_the_new_entry_points_without_a_device():
    """The argument rules run before the context is looked at: with ctx == NULL each call returns the code of its first failing check and leaves the
    message in qmri_last_error(NULL); a call whose arguments are all fine is refused for the missing context."""
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import LlrParams
    L = _lib.lib()
    x, out = np.zeros(2 * 16 * 32 * 3 * 2), np.zeros(2 * 16 * 32 * 3 * 2)

    def P(tau=0.1, block=8, shift=0, reserved=(0, 0, 0, 0, 0)):
        return LlrParams(tau, block, shift, (C.c_int32 * 5)(*reserved))

    def call(fn, N=16, M=32, s=3, S=2, x=x, cpx=1, p=P(), o1=0, o2=0, out=out):
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        st = fn(None, N, M, s, S, vp(x), cpx, C.byref(p) if p is not None else None, o1, o2, vp(out), None)
        return st, L.qmri_last_error(None)

    nan, inf = float("nan"), float("inf")
    cases = [(dict(x=None), b"x / p / out"), (dict(p=None), b"x / p / out"), (dict(out=None), b"x / p / out"), (dict(S=0), b"nslices"),
             (dict(s=0), b"1 <= s <= 16"), (dict(s=17), b"1 <= s <= 16"), (dict(p=P(tau=-1e-9)), b"tau"), (dict(p=P(tau=nan)), b"tau"),
             (dict(p=P(tau=inf)), b"tau"), (dict(p=P(block=2)), b"block"), (dict(p=P(block=12)), b"block"), (dict(p=P(block=32)), b"block"),
             (dict(p=P(block=-8)), b"block"), (dict(p=P(reserved=(0, 0, 0, 0, 1))), b"reserved"), (dict(p=P(reserved=(-1, 0, 0, 0, 0))), b"reserved"),
             (dict(N=12), b"multiples of the block side (N = 12, M = 32, block = 8)"), (dict(M=36), b"multiples of the block side"),
             (dict(N=0), b"multiples of the block side"), (dict(M=-8), b"multiples of the block side"),
             (dict(p=P(block=16), M=40), b"block = 16"), (dict(p=P(block=0), N=12), b"block = 8"),
             (dict(o1=-1), b"offsets"), (dict(o1=8), b"offsets"), (dict(o2=8), b"offsets"), (dict(p=P(block=4), o2=4), b"offsets"),
             (dict(), b"ctx"), (dict(cpx=0), b"ctx"), (dict(p=P(block=0)), b"ctx"), (dict(p=P(block=4, shift=7), o1=3, o2=3), b"ctx"),
             (dict(p=P(block=16), o1=15, o2=15), b"ctx"), (dict(p=P(tau=0.0)), b"ctx")]
    for fn in (L.qmri_llr_prox, L.qmri_llr_prox_dev):
        for kw, word in cases:
            st, msg = call(fn, **kw)
            assert st == -1 and word in msg, (kw, st, msg)
    for p, word in ((P(tau=-1.0), b"tau"), (P(tau=nan), b"tau"), (P(block=5), b"block"), (P(shift=2), b"shift"), (P(shift=-1), b"shift"),
                    (P(reserved=(0, 1, 0, 0, 0)), b"reserved"), (P(), b"ctx"), (P(block=0, shift=1), b"ctx")):
        st = L.qmri_set_llr(None, C.byref(p))
        assert st == -1 and word in L.qmri_last_error(None), (word, L.qmri_last_error(None))
    assert L.qmri_set_llr(None, None) == -1 and b"ctx" in L.qmri_last_error(None)


def test_make_llr_and_the_harness_check_their_arguments_before_any_device_call():
    from qmri_pnp_recon_poc_amd import harness, reference_api as RA
    F = RA.SimpleNamespace(_engine=object())
    net = RA.make_llr(F, tau_rel=0.05, block=4, shift=False)
    assert net._llr and net._engine is F._engine and (net.tau, net.tau_rel, net.block, net.shift) == (None, 0.05, 4, False)
    assert RA.make_llr(F, tau=0.5).tau == 0.5
    for kw in (dict(block=5), dict(tau=-1.0), dict(tau=np.nan), dict(tau_rel=-0.1), dict(tau_rel=np.inf)):
        with pytest.raises(ValueError):
            RA.make_llr(F, **kw)
    with pytest.raises(TypeError):
        RA.make_llr(object())
    dic, X0, q0 = {"V": np.ones((4, 1))}, np.zeros((8, 8, 1)), np.zeros((8, 8, 3))
    with pytest.raises(ValueError, match="regulariser"):
        harness.recon_tsmis(dic, X0, q0, regulariser="tv")
    with pytest.raises(ValueError, match="PnP_ADMM"):
        harness.recon_tsmis(dic, X0, q0, regulariser="llr", recon_method="SVD_MRF")


def test_mex_llr_commands_check_their_arguments_under_the_mock_gateway():
    from mexmock import MexError, qmri_mex
    X = np.ones((16, 32, 3), complex)
    cases = [("llr_prox", (X,), "qmri:usage"), ("llr_prox", (X, 0.1, 8.0, 1.0), "qmri:usage"), ("llr_prox", (X.astype(np.complex64), 0.1), "qmri:llr_prox:type"),
             ("llr_prox", (X, -0.1), "qmri:llr_prox:tau"), ("llr_prox", (X, np.nan), "qmri:llr_prox:tau"), ("llr_prox", (X, np.ones(2)), "qmri:llr_prox:tau"),
             ("llr_prox", (X, 0.1, 5.0), "qmri:llr_prox:block"), ("llr_prox", (X, 0.1, 12.0), "qmri:llr_prox:block"), ("llr_prox", (X, 0.1, 2.5), "qmri:llr_prox:block"),
             ("llr_prox", (X, 0.1, 8.0, 8.0, 0.0), "qmri:llr_prox:offset"), ("llr_prox", (X, 0.1, 4.0, 0.0, 4.0), "qmri:llr_prox:offset"),
             ("llr_prox", (X, 0.1, 8.0, -1.0, 0.0), "qmri:llr_prox:offset"), ("llr_prox", (np.ones((12, 32, 3), complex), 0.1), "qmri:llr_prox:size"),
             ("llr_prox", (np.ones((16, 40, 3), complex), 0.1, 16.0), "qmri:llr_prox:size"),
             ("llr_prox", (np.ones((16, 32, 17), complex), 0.1), "qmri:llr_prox:size"), ("llr_prox", (np.ones((16, 32, 2, 2, 2), complex), 0.1), "qmri:llr_prox:size"),
             ("set_llr", (), "qmri:usage"), ("set_llr", (-1.0,), "qmri:set_llr:tau"), ("set_llr", (np.inf,), "qmri:set_llr:tau"), ("set_llr", (1j,), "qmri:set_llr:tau"),
             ("set_llr", (0.1, 6.0), "qmri:set_llr:block"), ("set_llr", (0.1, 32.0), "qmri:set_llr:block"), ("set_llr", (0.1, 8.0, 2.0), "qmri:set_llr:shift"),
             ("set_llr", (0.1, 8.0, 0.5), "qmri:set_llr:shift")]
    for cmd, args, ident in cases:
        with pytest.raises(MexError) as err:
            qmri_mex(cmd, *args, nargout=1)
        assert err.value.id == ident, (cmd, ident, err.value.id, err.value.msg)
    src = open(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "matlab", "PnP_ADMM_hip.m")).read()
    assert "qmri_mex('set_llr'" in src and "qmri_mex('clear_llr')" in src and "qmri_mex('llr_prox'" in src
    assert os.path.exists(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "matlab", "qmri_make_llr.m"))


def test_refusals_and_offset_rule_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_llr.cpp against the host-only sanitised library: every refusal of qmri_llr_prox, qmri_llr_prox_dev and
    qmri_set_llr without a context and with one, and the offset rule of the ADMM loop, as a stand-alone program."""
    csrc = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    if not rt_dirs:
        pytest.skip("clang sanitizer runtime not found")
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "_build_asan", "host_asan_llr")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_LLR_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
