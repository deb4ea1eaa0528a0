"""GPU: the slice-profile-aware FISP dictionary simulation (include/qmri.h qmri_dict_simulate_sp) against tests/epgsp_ref.py
-- the numpy restatement of the definition, never the device's own output.  The tolerance is absolute on F: per fixture 16 x the largest of the
three sensitivity figures tests/test_epgsp_host.py asserts for it (fp64 against longdouble; every exponential one ulp away; every RF argument one
ulp away), read from the one table epgsp_ref.SENS: 6.7e-16 (one atom, one frame) .. 2.1e-13.  A kernel that ignores the profile is 6.7e-2 away
(tests/test_epgsp_host.py::test_the_profile_matters); a sub-slice summed twice, dropped or taken with its neighbour's weight shows at 1e-3 or more."""
import ctypes as C
import os

import numpy as np
import pytest

import dict_svd_ref as DR
import epg_ref as R
import epgsp_ref as SP

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


def simulate(eng, inp, **more):
    return eng.simulate_dictionary(**SP.engine_kwargs(inp, **more))


def simulate_dev(eng, inp, dtype=np.float64, profile=True):
    """qmri_dict_simulate_sp_dev (profile = False: qmri_dict_simulate_dev, ignoring prof and w) on device copies of t1, t2, b1: F [K, T]"""
    from qmri_pnp_recon_poc_amd import engine
    a, tr, te, t1, t2, b1, p = engine.simulation_arguments(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], inp["b1"], inp["nstates"], inp["inversion"],
                                                           inp["ti"], inp["inv_eff"], dtype)
    K, T = t1.size, a.size
    sp = engine.slice_profile_arguments(inp["prof"], inp["w"], T) if profile else None
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
        head = (eng.h, K, T, vp(a), vp(tr), vp(te), d_t1, d_t2, d_b1 if b1 is not None else None, C.byref(p))
        if profile:
            eng._check(eng.L.qmri_dict_simulate_sp_dev(*head, C.byref(sp[2]), d_F))
        else:
            eng._check(eng.L.qmri_dict_simulate_dev(*head, d_F))
        assert hip.hipMemcpy(F.ctypes.data, d_F, F.nbytes, 2) == 0
    finally:
        for d in ptrs:
            hip.hipFree(d)
    return F.reshape((K, T), order="F")


@pytest.mark.parametrize("name", sorted(SP.CASES))
def test_simulation_against_the_numpy_restatement(eng, name):
    """Every (G, R) instantiation at Q = 5 with a per-frame profile (s1 .. s256; 45 atoms leave ragged workgroups at every atoms-per-workgroup
    count); Q one short of, exactly, and one past the groups of a workgroup at every G, at S = 32 (q1 .. q64: one pass shared by 8, 4 and 1 atoms,
    then 2, 3, 5 and 8 passes through the LDS accumulator); one atom of one frame and one sub-slice; a frame past a block; 64 sub-slices of 256
    states (16 passes); per-frame TR and TE; no inversion; an imperfect inversion with TI; per-atom b1; a zero weight in the middle; a
    frame-constant profile with and without per-atom b1; the trivial profile."""
    inp, ref = SP.case_inputs(name), SP.case_ref(name)
    F = simulate(eng, inp)
    err = np.max(np.abs(F - ref))
    print(name, "max |F - ref| =", err, "atol =", SP.atol(name), "peak |F| =", np.abs(ref).max())
    assert F.shape == ref.shape and F.dtype == np.float64
    assert err <= SP.atol(name)


@pytest.mark.parametrize("name", ["q5", "q17", "s129"])
def test_fp32_output_is_the_fp64_output_rounded_once(eng, name):
    inp = SP.case_inputs(name)
    F64, F32 = simulate(eng, inp), simulate(eng, inp, dtype=np.float32)
    assert F32.dtype == np.float32 and np.array_equal(F32, F64.astype(np.float32))
    assert np.max(np.abs(F64 - SP.case_ref(name))) <= SP.atol(name)


def test_the_trivial_profile_gives_the_plain_calls_bits(eng):
    """Q = 1, w = 1, prof = 1: the bits of qmri_dict_simulate_dev and of qmri_dict_simulate, with constant and with per-frame timing."""
    for name in ("one", "timing"):
        inp = dict(SP.case_inputs(name), prof=np.ones(1), w=np.ones(1))
        plain = simulate_dev(eng, inp, profile=False)
        assert np.array_equal(simulate_dev(eng, inp), plain) and np.array_equal(simulate(eng, inp), plain)
        assert np.array_equal(eng.simulate_dictionary(**{k: v for k, v in inp.items() if k not in ("prof", "w")}), plain)
        per_frame = dict(inp, prof=np.ones((48, 1)))
        assert np.array_equal(simulate(eng, per_frame), plain)


@pytest.mark.parametrize("name", ["q2", "q5", "q17", "s16", "b1", "timing", "p4b1"])
def test_entry_points_and_repeated_calls_give_equal_bits(eng, name):
    inp = SP.case_inputs(name)
    a, b = simulate(eng, inp), simulate(eng, inp)
    assert np.array_equal(a, b)
    assert np.array_equal(simulate_dev(eng, inp), a)
    assert np.array_equal(simulate_dev(eng, inp, np.float32), a.astype(np.float32))


@pytest.mark.parametrize("name", ["q5", "q17", "q2"])
def test_an_atom_alone_has_the_bits_of_its_row(eng, name):
    """Each atom simulated alone (K = 1) equals its row of the K = 45 call: one atom per workgroup (Q = 5 at S = 32), three passes (Q = 17), and
    four atoms sharing a workgroup (Q = 2), where the atom alone sits in another group than in the full call."""
    inp = SP.case_inputs(name)
    F = simulate(eng, inp)
    for k in range(45):
        one = simulate(eng, dict(inp, t1=inp["t1"][k:k + 1], t2=inp["t2"][k:k + 1]))
        assert np.array_equal(one[0], F[k]), k


def test_a_frame_constant_profile_is_the_weighted_sum_of_plain_calls(eng):
    """per_frame = 0 on the b1 ramp against sum_q w_q x (the plain device simulation with b1 p_q), summed here in ascending q from 0: within the
    fixture's tolerance, whose third figure covers the product order (alpha b1) p against alpha (b1 p)."""
    inp = SP.case_inputs("p4b1")
    F = simulate_dev(eng, inp)
    want = np.zeros_like(F)
    for q in range(4):
        want = want + inp["w"][q] * simulate_dev(eng, dict(inp, b1=inp["b1"] * inp["prof"][q]), profile=False)
    err = np.max(np.abs(F - want))
    print("profiled call against the sum of plain calls:", err, "atol:", SP.atol("p4b1"))
    assert err <= SP.atol("p4b1")
    assert np.max(np.abs(F - SP.case_ref("p4b1"))) <= SP.atol("p4b1")


@pytest.mark.parametrize("name,k", [("q2", 5), ("s16", 4), ("q5", 20), ("q17", 7)])
def test_device_route_marks_a_bad_atom_with_nan_in_its_row_only(eng, engine_mod, name, k):
    """The device route cannot refuse a bad atom on the host: its fingerprint is NaN in every frame, every other atom keeps its bits -- with the
    bad atom between two good ones of the same workgroup (q2: atoms 4 .. 7 share one, s16: atoms 3 .. 5), alone in its workgroup (q5), and carried
    through the pass accumulator (q17); a zero weight does not hide it.  The host-array route refuses the same input."""
    inp = SP.case_inputs(name)
    good = simulate_dev(eng, inp)
    rest = np.arange(45) != k
    for key, v in (("t1", 0.0), ("t1", -1.0), ("t2", np.nan), ("t2", np.inf), ("b1", -0.5), ("b1", np.nan)):
        x = (np.ones(45) if key == "b1" else inp[key]).copy()
        x[k] = v
        bad = dict(inp, **{key: x})
        if key == "b1":
            good_b = simulate_dev(eng, dict(inp, b1=np.ones(45)))
            assert np.array_equal(good_b, good)
        F = simulate_dev(eng, bad)
        assert np.all(np.isnan(F[k])) and np.array_equal(F[rest], good[rest]), (key, v)
        with pytest.raises(engine_mod.QmriError) as e:
            simulate(eng, bad)
        assert e.value.code == -1 and key in str(e.value)
    w = inp["w"].copy()
    w[0] = 0.0
    x = inp["t1"].copy()
    x[k] = -1.0
    F = simulate_dev(eng, dict(inp, t1=x, w=w))
    assert np.all(np.isnan(F[k])) and not np.any(np.isnan(F[rest]))


def test_the_chain_simulate_compress_match(engine_mod):
    """harness.simulate_dictionary(..., slice_profile=, b1_grid=) (simulate -> compress on one device buffer) on T = 48, 24 x 11 atoms x 3 transmit
    scales, S = 32, Q = 5, s = 6 against epgsp_ref -> dict_svd_ref.dict_compress_ref with the bounds of tests/test_gpu_dict_svd.py; then the match
    under the device's dictionary against the match under the reference's on 32 x 32 pixels made of the reference's own atoms: identical on
    >= 99 %, the rest one grid step away (tests/test_epgsp_host.py shows the reference alone meets this)."""
    from qmri_pnp_recon_poc_amd import harness
    TOL, s, n1, n2 = 1e-13, SP.CHAIN["s"], 24, 11
    inp = SP.case_inputs("chain")
    F_ref = SP.case_ref("chain")
    ref = DR.dict_compress_ref(F_ref, s=s)
    gaps = ref["gaps"]
    assert gaps.min() > 1e-6                                  # the precondition of the per-column bound, on the CPU
    t1g, t2g = np.exp(np.linspace(np.log(0.1), np.log(4.0), n1)), np.exp(np.linspace(np.log(0.01), np.log(0.6), n2))
    out = harness.simulate_dictionary(inp["alpha"], R.TR0, R.TE0, t1g, t2g, s=s, nstates=32, b1_grid=SP.CHAIN["b1_grid"], slice_profile=inp["prof"],
                                      slice_weights=inp["w"])
    K = 3 * n1 * n2
    V, lam, lam1, T = out["V"], out["eig"], ref["eig"][0], 48
    assert out["info"]["s"] == s and out["info"]["converged"] == 1 and V.shape == (T, s) and out["D"].shape == (K, s) and out["lut"].shape == (K, 3)
    assert np.array_equal(out["lut"], np.stack([inp["t1"], inp["t2"], inp["b1"]], axis=1).astype(np.float32))
    assert out["group_ptr"].tolist() == [0, n1 * n2, 2 * n1 * n2, K] and out["group_val"].tolist() == list(SP.CHAIN["b1_grid"])
    d_eig = np.max(np.abs(lam - ref["eig"][:s]))
    ortho = np.max(np.abs(V.T @ V - np.eye(s)))
    bound = 2 * TOL / np.minimum(np.append(np.inf, gaps[:-1]), gaps)
    d_V = np.max(np.abs(V - ref["V"]), axis=0)
    print("eig", d_eig / lam1, "ortho", ortho, "dV", d_V, "bound", bound)
    assert d_eig <= 1e-13 * lam1 * T
    assert ortho <= 1e-13
    assert np.all(d_V <= bound), (d_V, bound)
    X = R.chain_match_input(ref)
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(out["D"], out["normD"], out["lut"])
        dev = e.dict_match(X)
        e.set_dictionary(ref["D"], ref["normD"], out["lut"])
        host = e.dict_match(X)
    finally:
        e.close()
    steps = DR.grid_steps(dev["dm"], host["dm"], n2)
    print("identical on", np.mean(steps == 0), "largest step", steps.max())
    assert np.mean(steps == 0) >= 0.99 and steps.max() <= 1
