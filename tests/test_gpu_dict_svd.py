"""GPU: the dictionary compression (include/qmri.h qmri_dict_compress) against tests/dict_svd_ref.py -- numpy's eigh of numpy's
F^T F, never the device's own output.  Tolerances (tol = the default 1e-13 of the stop rule, gaps relative to lambda_1 from the reference spectrum):
  eigenvalues  |lambda_c - ref| <= 1e-13 lambda_1 T     (a symmetric matrix's eigenvalues move by at most the perturbation of G: fp64 sums of K terms)
  basis        |V^T V - I|_max <= 1e-13
  residual     |G_ref v_c - lambda_c v_c|_2 <= 2 tol lambda_1, and info.converged == 1
  per column   max |v_c - v_c^ref| <= 2 tol / min(gap_{c-1}, gap_c)    (Davis-Kahan bound of the stop rule; a wrong basis is off by O(1))
  D            atol 2^-23 (both sides round values that agree far below an fp32 ulp: one ulp of 1 at a rounding boundary);  normD rtol 2^-23
The fixture facts behind them (gaps, sign margin) are asserted in tests/test_dict_svd_host.py."""
import ctypes as C
import os

import numpy as np
import pytest

import dict_svd_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-13
# name: (T, n_t1, n_t2, s, input dtype).  k5000: 5000 atoms = the Gram kernel's chunks of 2048 + 2048 + a ragged 904; t1024: the largest T
SHAPES = {"t48": (48, 24, 11, 6, np.float64), "t48_f32": (48, 24, 11, 6, np.float32), "t100": (100, 32, 16, 10, np.float64), "t40": (40, 10, 7, 3, np.float64),
          "t1024": (1024, 32, 16, 10, np.float64), "k5000": (32, 100, 50, 4, np.float64)}


def _hip():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


@pytest.fixture(scope="module")
def eng(engine_mod):
    e = engine_mod.Engine(0)
    yield e
    e.close()


_cases = {}


def case(name):
    """(F as it goes to the device, the reference of exactly that F), computed once per shape and left unchanged"""
    if name not in _cases:
        T, n1, n2, s, dt = SHAPES[name]
        F = R.simulate(T, n1, n2).astype(dt)
        ref = R.dict_compress_ref(F.astype(np.float64), s=s)
        F.setflags(write=False)
        _cases[name] = (F, ref)
    return _cases[name]


def gram_of(eng, F):
    K, T = F.shape
    Fb = np.ascontiguousarray(F.ravel(order="F"))
    G = np.empty(T * T)
    eng._check(eng.L.qmri_debug_dsvd_gram(eng.h, K, T, Fb.ctypes.data_as(C.c_void_p), int(F.dtype == np.float64), 0, G.ctypes.data_as(C.c_void_p)))
    return G.reshape((T, T), order="F")


@pytest.mark.parametrize("K,T,dtype", [(70, 48, np.float64), (70, 40, np.float64), (71, 40, np.float64), (70, 40, np.float32), (71, 48, np.float32),
                                        (70, 100, np.float64), (5000, 130, np.float64), (1, 1, np.float64)])
def test_mfma_map_with_exact_integers(eng, K, T, dtype):
    """Small integers (|F| <= 8): every product and every partial sum is an integer far below 2^53, so G must equal F^T F exactly whatever the
    order -- a wrong C/D row map, a dropped tail of the ragged last 16-frame tile (T = 40) or of the ragged K stage (K = 70; 71: the odd-K path
    without 16-byte loads), a wrong mirror of an off-diagonal block (T = 100, 130) or a lost split-K chunk (K = 5000) all show as wrong integers."""
    rng = np.random.RandomState(K * 1000 + T)
    F = rng.randint(-8, 9, size=(K, T)).astype(dtype)
    G = gram_of(eng, F)
    want = F.astype(np.float64).T @ F.astype(np.float64)
    assert np.array_equal(G, want), np.argwhere(G != want)[:8]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_compression_against_the_numpy_restatement(eng, name):
    F, ref = case(name)
    K, T = F.shape
    s = SHAPES[name][3]
    out = eng.compress_dictionary(F, s=s)
    info, V, lam = out["info"], out["V"], out["eig"]
    lam1 = ref["eig"][0]
    print(name, info)
    assert info["s"] == s and V.shape == (T, s) and out["D"].shape == (K, s) and out["normD"].shape == (K,)
    assert info["converged"] == 1 and info["energy_reached"] == 1 and 1 <= info["iters"] <= 200 and info["max_resid"] <= TOL
    d_eig = np.max(np.abs(lam - ref["eig"][:s]))
    ortho = np.max(np.abs(V.T @ V - np.eye(s)))
    resid = np.linalg.norm(ref["G"] @ V - V * lam[None, :], axis=0)
    gaps = ref["gaps"]
    bound = 2 * TOL / np.minimum(np.append(np.inf, gaps[:-1]), gaps)
    d_V = np.max(np.abs(V - ref["V"]), axis=0)
    d_D = np.max(np.abs(out["D"].astype(np.float64) - ref["D"].astype(np.float64)))
    print(name, "eig", d_eig / lam1, "ortho", ortho, "resid", resid.max() / lam1, "dV", d_V, "bound", bound, "dD", d_D)
    assert d_eig <= 1e-13 * lam1 * T
    assert ortho <= 1e-13
    assert resid.max() <= 2 * TOL * lam1
    assert np.all(d_V <= bound), (d_V, bound)
    assert d_D <= 2.0 ** -23
    np.testing.assert_allclose(out["normD"], ref["normD"], rtol=2.0 ** -23)
    assert abs(info["energy_kept"] - ref["energy_kept"]) <= 1e-12


def test_determinism_and_device_entry_point_bits(eng):
    """Two calls give identical bits; qmri_dict_compress_dev on device arrays gives the bits of the host-array call."""
    from qmri_pnp_recon_poc_amd._lib import DsvdInfo, DsvdParams
    F, _ = case("k5000")
    K, T = F.shape
    s = 4
    a, b = eng.compress_dictionary(F, s=s), eng.compress_dictionary(F, s=s)
    for key in ("V", "D", "normD", "eig"):
        assert np.array_equal(a[key], b[key]), key
    assert a["info"] == b["info"]
    hip = _hip()
    Fb = np.ascontiguousarray(F.ravel(order="F"))
    V, D, nd, eig = np.empty(T * s), np.empty(K * s, np.float32), np.empty(K, np.float32), np.empty(16)
    d_F, d_V, d_D, d_n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    for d, nb in ((d_F, Fb.nbytes), (d_V, T * 16 * 8), (d_D, K * 16 * 4), (d_n, nd.nbytes)):
        assert hip.hipMalloc(C.byref(d), nb) == 0
    try:
        assert hip.hipMemcpy(d_F, Fb.ctypes.data, Fb.nbytes, 1) == 0
        p, info, got = DsvdParams(s, 16, 0.0, 0.0, 0), DsvdInfo(), C.c_int(0)
        eng._check(eng.L.qmri_dict_compress_dev(eng.h, K, T, d_F, 1, C.byref(p), C.byref(got), d_V, d_D, d_n, eig.ctypes.data_as(C.c_void_p), C.byref(info)))
        for host, d in ((V, d_V), (D, d_D), (nd, d_n)):
            assert hip.hipMemcpy(host.ctypes.data, d, host.nbytes, 2) == 0
    finally:
        for d in (d_F, d_V, d_D, d_n):
            hip.hipFree(d)
    assert got.value == s and info.iters == a["info"]["iters"] and info.converged == 1
    assert np.array_equal(V.reshape((T, s), order="F"), a["V"]) and np.array_equal(D.reshape((K, s), order="F"), a["D"])
    assert np.array_equal(nd, a["normD"]) and np.array_equal(eig[:s], a["eig"])


@pytest.mark.parametrize("name", ["t48", "t100"])
def test_energy_mode(eng, name):
    F, ref = case(name)
    for energy, want in ((0.99, 3), (0.999, 4), (0.9999, 5), (0.99999, 7)):
        out = eng.compress_dictionary(F, energy=energy)
        r = R.dict_compress_ref(F, energy=energy)
        assert r["s"] == want
        assert out["info"]["s"] == want and out["V"].shape[1] == want and out["D"].shape[1] == want and out["eig"].shape == (want,)
        assert out["info"]["energy_reached"] == 1 and abs(out["info"]["energy_kept"] - r["energy_kept"]) <= 1e-12
        assert np.max(np.abs(out["D"].astype(np.float64) - r["D"])) <= 2.0 ** -23
    out = eng.compress_dictionary(F, energy=0.99999, s_max=4)
    assert out["info"]["s"] == 4 and out["info"]["energy_reached"] == 0 and out["V"].shape[1] == 4
    assert out["info"]["energy_kept"] < 0.99999


def test_zero_atoms_and_refused_input(eng, engine_mod):
    F = case("t48")[0].copy()
    F[[0, 17, 263]] = 0.0
    out = eng.compress_dictionary(F, s=6)
    ref = R.dict_compress_ref(F, s=6)
    for k in (0, 17, 263):
        assert np.all(out["D"][k] == 0.0) and out["normD"][k] == 0.0
    assert np.max(np.abs(out["D"].astype(np.float64) - ref["D"])) <= 2.0 ** -23
    np.testing.assert_allclose(out["normD"], ref["normD"], rtol=2.0 ** -23)
    zero = eng.compress_dictionary(np.zeros((9, 5)), s=2)                         # nothing to compress: an orthonormal V, zero atoms
    assert np.all(zero["D"] == 0) and np.all(zero["normD"] == 0) and np.max(np.abs(zero["V"].T @ zero["V"] - np.eye(2))) <= 1e-13
    bad = F.copy()
    bad[5, 7] = np.nan
    with pytest.raises(engine_mod.QmriError) as e:
        eng.compress_dictionary(bad, s=6)
    assert e.value.code == -1 and "trace" in str(e.value)
    bad[5, 7] = np.inf
    with pytest.raises(engine_mod.QmriError):
        eng.compress_dictionary(bad, s=6)
    assert eng.compress_dictionary(case("t48")[0], s=6)["info"]["converged"] == 1   # the context is fine afterwards
    few = eng.compress_dictionary(case("t100")[0], s=10, maxit=1)                   # the cap is reported, not hidden
    assert few["info"]["iters"] == 1 and few["info"]["converged"] == 0 and few["info"]["max_resid"] > TOL


def test_the_device_dictionary_in_use(eng, engine_mod, synth):
    """set_operator takes the device's V, set_dictionary its D and normD; the match of 500 compressed atoms under the device's dictionary against the
    match under the numpy-compressed one: identical on >= 99 % of the pixels, the rest one grid step of lut away (the reference alone meets this on
    the fixture: tests/test_dict_svd_host.py)."""
    T, n1, n2, s, _ = SHAPES["t100"]
    F, ref = case("t100")
    lut = synth.make_dictionary(T=T, n_t1=n1, n_t2=n2, uncompressed=True)["lut"]
    out = eng.compress_dictionary(F, s=s)
    K = F.shape[0]
    idx = np.arange(500) * K // 500
    X = (ref["D64"][idx] * ref["normD"][idx, None].astype(np.float64)).reshape(25, 20, s)
    e = engine_mod.Engine(0)
    fp, k = engine_mod.build_spiral(32, 60, T)
    e.set_operator(32, 32, out["V"], fp, k)
    y = e.forward(np.ones((32, 32, s), np.complex128))
    assert np.all(np.isfinite(y)) and np.linalg.norm(y) > 0
    e.set_dictionary(out["D"], out["normD"], lut)
    dev = e.dict_match(X)
    e.set_dictionary(ref["D"], ref["normD"], lut)
    host = e.dict_match(X)
    e.close()
    steps = R.grid_steps(dev["dm"], host["dm"], n2)
    print("identical on", np.mean(steps == 0), "largest step", steps.max(), "on their own atom", np.mean(host["dm"].ravel() - 1 == idx))
    assert np.mean(steps == 0) >= 0.99 and steps.max() <= 1


def test_harness_compress_then_reconstruct(synth):
    """harness.compress_dictionary on an uncompressed dictionary, then recon_tsmis(recon_method="SVD_MRF") at 32 x 32 on the result, unchanged."""
    from qmri_pnp_recon_poc_amd import harness
    unc = synth.make_dictionary(T=48, n_t1=24, n_t2=11, uncompressed=True)
    dic = harness.compress_dictionary(unc, s=6)
    assert set(("V", "D", "normD", "lut")) <= set(dic) and dic["V"].shape == (48, 6) and dic["D"].shape == (264, 6)
    ref = R.dict_compress_ref(R.fingerprints(unc), s=6)
    assert np.max(np.abs(dic["D"].astype(np.float64) - ref["D"])) <= 2.0 ** -23
    q = synth.make_phantom_qmaps(32, seed=0)
    X0 = synth.synthesize_tsmi(q, dict(dic, t1_grid=unc["t1_grid"], t2_grid=unc["t2_grid"]))
    out = harness.recon_tsmis(dic, X0, q, recon_method="SVD_MRF", spiral_sampling_curve=120, measurements_type="clean")
    assert out["qmap"].shape == (32, 32, 3) and np.all(np.isfinite(out["qmap"])) and np.all(np.isfinite(out["X"]))
    byenergy = harness.compress_dictionary(unc, energy=0.9999)
    assert byenergy["info"]["s"] == 5 and byenergy["V"].shape == (48, 5)
