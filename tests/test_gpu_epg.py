"""GPU: the FISP dictionary simulation by extended phase graphs (include/qmri.h qmri_dict_simulate) against
tests/epg_ref.py -- the numpy restatement of the definition, never the device's own output.  The tolerance is absolute on F (|F| <= 1): per
fixture 16 x the larger of the two sensitivity figures tests/test_epg_host.py asserts for it (fp64 against longdouble; every exponential one ulp
away), read from the one table epg_ref.SENS: 1.4e-15 (one atom, one frame) .. 4e-13 (T = 1024).  A wrong coefficient, a shift in the wrong direction or a dropped state shows at
1e-3 or more."""
import ctypes as C
import os

import numpy as np
import pytest

import dict_svd_ref as DR
import epg_ref as R

pytestmark = pytest.mark.gpu


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


def simulate_dev(eng, inp, dtype=np.float64):
    """qmri_dict_simulate_dev on device copies of t1, t2, b1: F [K, T]"""
    from qmri_pnp_recon_poc_amd import engine
    a, tr, te, t1, t2, b1, p = engine.simulation_arguments(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], inp["b1"], inp["nstates"], inp["inversion"],
                                                           inp["ti"], inp["inv_eff"], dtype)
    K, T = t1.size, a.size
    hip = _hip()
    F = np.empty(K * T, dtype)
    ptrs = [C.c_void_p() for _ in range(4)]
    d_t1, d_t2, d_b1, d_F = ptrs
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    try:
        for d, nb in ((d_t1, K * 8), (d_t2, K * 8), (d_b1, K * 8), (d_F, F.nbytes)):
            assert hip.hipMalloc(C.byref(d), nb) == 0
        for d, h in ((d_t1, t1), (d_t2, t2)) + (((d_b1, b1),) if b1 is not None else ()):
            assert hip.hipMemcpy(d, h.ctypes.data, h.nbytes, 1) == 0
        eng._check(eng.L.qmri_dict_simulate_dev(eng.h, K, T, vp(a), vp(tr), vp(te), d_t1, d_t2, d_b1 if b1 is not None else None, C.byref(p), d_F))
        assert hip.hipMemcpy(F.ctypes.data, d_F, F.nbytes, 2) == 0
    finally:
        for d in ptrs:
            hip.hipFree(d)
    return F.reshape((K, T), order="F")


@pytest.mark.parametrize("name", [n for n in sorted(R.CASES) if n != "chain"])
def test_simulation_against_the_numpy_restatement(eng, name):
    """Every (G, R) instantiation (s1 .. s256: 16, 32, 64 lanes x 1, 2, 4 states; 17, 33, 65, 129 are the first S of the next one, with padding
    states that must stay zero; 45 atoms leave a ragged last group in every workgroup size), one atom of one frame, the longest train, many
    workgroups with a ragged tail of the staged stores (k5000), per-frame TR and TE, no inversion, an imperfect inversion with TI, per-atom b1."""
    inp, ref = R.case_inputs(name), R.case_ref(name)
    F = eng.simulate_dictionary(**inp)
    err = np.max(np.abs(F - ref))
    print(name, "max |F - ref| =", err, "atol =", R.atol(name), "peak |F| =", np.abs(ref).max())
    assert F.shape == ref.shape and F.dtype == np.float64
    assert err <= R.atol(name)


def test_varying_timing_differs_from_constant_timing(eng):
    """The per-frame TR / TE fixture is not the constant one in disguise: its result is away from the constant-timing result by far more than
    the tolerance, and each is within tolerance of its own reference."""
    a, b = R.case_inputs("timing"), R.case_inputs("s32")
    Fa, Fb = eng.simulate_dictionary(**a), eng.simulate_dictionary(**b)
    assert np.max(np.abs(R.case_ref("timing") - R.case_ref("s32"))) > 1e-3
    assert np.max(np.abs(Fa - R.case_ref("timing"))) <= R.atol("timing") and np.max(np.abs(Fb - R.case_ref("s32"))) <= R.atol("s32")
    # constant timing given per frame is the same computation: same bits as the scalar form
    Fc = eng.simulate_dictionary(**dict(b, tr=R.TR0, te=R.TE0))
    assert np.array_equal(Fb, Fc)


def test_b1_null_is_b1_one_bit_for_bit(eng):
    inp = R.case_inputs("s32")
    assert np.array_equal(eng.simulate_dictionary(**inp), eng.simulate_dictionary(**dict(inp, b1=np.ones(inp["t1"].size))))
    assert np.all(eng.simulate_dictionary(**dict(inp, b1=np.zeros(inp["t1"].size))) == 0.0)      # b1 = 0 is allowed: no signal


@pytest.mark.parametrize("name", ["s32", "s129", "k5000"])
def test_fp32_output_is_the_fp64_output_rounded_once(eng, name):
    inp = R.case_inputs(name)
    F64, F32 = eng.simulate_dictionary(**inp), eng.simulate_dictionary(**inp, dtype=np.float32)
    assert F32.dtype == np.float32 and np.array_equal(F32, F64.astype(np.float32))


@pytest.mark.parametrize("name", ["s16", "b1", "timing", "k5000"])
def test_entry_points_and_repeated_calls_give_equal_bits(eng, name):
    inp = R.case_inputs(name)
    a, b = eng.simulate_dictionary(**inp), eng.simulate_dictionary(**inp)
    assert np.array_equal(a, b)
    assert np.array_equal(simulate_dev(eng, inp), a)
    assert np.array_equal(simulate_dev(eng, inp, np.float32), a.astype(np.float32))


def test_device_route_marks_a_bad_atom_with_nan_in_its_row_only(eng, engine_mod):
    """The device route cannot refuse a T1 <= 0 on the host: that atom's fingerprint is NaN in every frame, every other atom is untouched; the
    host-array route refuses the same input."""
    inp = R.case_inputs("s32")
    good = simulate_dev(eng, inp)
    for key, k, v in (("t1", 7, 0.0), ("t1", 44, -1.0), ("t2", 0, np.nan), ("t2", 20, np.inf)):
        x = inp[key].copy()
        x[k] = v
        F = simulate_dev(eng, dict(inp, **{key: x}))
        assert np.all(np.isnan(F[k]))
        rest = np.arange(F.shape[0]) != k
        assert np.array_equal(F[rest], good[rest])
        with pytest.raises(engine_mod.QmriError) as e:
            eng.simulate_dictionary(**dict(inp, **{key: x}))
        assert e.value.code == -1 and key in str(e.value)
    b = np.ones(45)
    b[3] = -0.5
    F = simulate_dev(eng, dict(inp, b1=b))
    assert np.all(np.isnan(F[3])) and np.array_equal(np.delete(F, 3, axis=0), np.delete(good, 3, axis=0))


@pytest.mark.parametrize("S", [2, 16, 17, 64, 65, 256])
@pytest.mark.parametrize("nshift", [1, 3])
def test_spoiler_moves_exact_integers(eng, S, nshift):
    """qmri_debug_epg_shift runs step 5 alone on a state of distinct integers: the result equals numpy's shift exactly.  A move that crosses a
    16-lane row (S = 17 .. 64), a 64-lane wave's end or a register boundary inside a lane (S = 65: two states per lane, 256: four) the wrong way
    shows as a wrong integer."""
    st = np.concatenate([1000.0 + np.arange(S), 2000.0 + np.arange(S), 3000.0 + np.arange(S)])
    out = np.full(3 * S, -1.0)
    eng._check(eng.L.qmri_debug_epg_shift(eng.h, S, nshift, st.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    fp, fm = st[:S], st[S:2 * S]
    for _ in range(nshift):
        fp, fm = R.shift(fp, fm)
    assert np.array_equal(out[:S], fp), (out[:S], fp)
    assert np.array_equal(out[S:2 * S], fm), (out[S:2 * S], fm)
    assert np.array_equal(out[2 * S:], st[2 * S:])


def test_one_pulse_then_free_precession_with_exact_data(eng):
    """alpha = pi/2 in frame 0 and 0 afterwards, TR and TE so long against T1 and T2 that every exponential underflows to 0: frame 0 reads
    F+_0 = sin(pi/2) * 0 = 0 after the decay and every later frame is exactly 0; with TE = 0 frame 0 reads sin(pi / 2) = 1 to one ulp."""
    al = np.zeros(12)
    al[0] = np.pi / 2
    t1, t2 = np.full(5, 1e-3), np.full(5, 1e-4)
    F = eng.simulate_dictionary(al, 10.0, 5.0, t1, t2, nstates=16, inversion=False)
    assert np.all(F == 0.0)
    F = eng.simulate_dictionary(al, 10.0, 0.0, t1, t2, nstates=16, inversion=False)
    assert np.all(np.abs(F[:, 0] - 1.0) <= 2.0 ** -52) and np.all(F[:, 1:] == 0.0)


def test_the_chain_simulate_compress_match(engine_mod):
    """harness.simulate_dictionary (simulate -> compress on one device buffer) on T = 48, 24 x 11 atoms, S = 32, s = 6 against epg_ref ->
    dict_svd_ref.dict_compress_ref with the bounds of tests/test_gpu_dict_svd.py; then the match under the device's dictionary against the match
    under the reference's on TSMIs made of the reference's own atoms: identical on >= 99 % of 32 x 32 pixels, the rest one grid step away."""
    from qmri_pnp_recon_poc_amd import harness
    TOL, s, n1, n2 = 1e-13, 6, 24, 11
    inp = R.case_inputs("chain")
    t1g, t2g = np.exp(np.linspace(np.log(0.1), np.log(4.0), n1)), np.exp(np.linspace(np.log(0.01), np.log(0.6), n2))
    out = harness.simulate_dictionary(inp["alpha"], R.TR0, R.TE0, t1g, t2g, s=s, nstates=32)
    ref = DR.dict_compress_ref(R.case_ref("chain"), s=s)
    V, lam, lam1, T = out["V"], out["eig"], ref["eig"][0], 48
    assert out["info"]["s"] == s and out["info"]["converged"] == 1 and V.shape == (T, s) and out["D"].shape == (n1 * n2, s) and out["lut"].shape == (n1 * n2, 2)
    assert np.array_equal(out["lut"], np.stack([inp["t1"], inp["t2"]], axis=1).astype(np.float32))
    d_eig = np.max(np.abs(lam - ref["eig"][:s]))
    ortho = np.max(np.abs(V.T @ V - np.eye(s)))
    gaps = ref["gaps"]
    bound = 2 * TOL / np.minimum(np.append(np.inf, gaps[:-1]), gaps)
    d_V = np.max(np.abs(V - ref["V"]), axis=0)
    print("eig", d_eig / lam1, "ortho", ortho, "dV", d_V, "bound", bound)
    assert d_eig <= 1e-13 * lam1 * T
    assert ortho <= 1e-13
    assert np.all(d_V <= bound), (d_V, bound)
    X = R.chain_match_input(ref)
    e = engine_mod.Engine(0)
    e.set_dictionary(out["D"], out["normD"], out["lut"])
    dev = e.dict_match(X)
    e.set_dictionary(ref["D"], ref["normD"], out["lut"])
    host = e.dict_match(X)
    e.close()
    steps = DR.grid_steps(dev["dm"], host["dm"], n2)
    print("identical on", np.mean(steps == 0), "largest step", steps.max())
    assert np.mean(steps == 0) >= 0.99 and steps.max() <= 1
