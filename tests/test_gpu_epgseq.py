"""GPU: the EPG simulation of prepared, repeated FISP trains (include/qmri.h qmri_dict_simulate_seq) against
tests/epgseq_ref.py -- the numpy restatement of the definition, never the device's own output -- within 16 x the larger of the two sensitivity
figures tests/test_epgseq_host.py asserts per fixture (epgseq_ref.SENS: 2.2e-17 for one atom of one frame .. 7.5e-14 at T = 1024), absolute on F
(|F| <= 1); and bit for bit against qmri_dict_simulate (one block), against itself (cycles equal tiling; entry points; an atom's position).  A
wrong event, an event on the wrong segment, a cycle too few or a store from the wrong cycle shows at 1e-3 or more."""
import ctypes as C
import os

import numpy as np
import pytest

import dict_svd_ref as DR
import epg_ref as R
import epgseq_ref as Q

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
    """qmri_dict_simulate_seq_dev on device copies of t1, t2, b1: F [K, T]"""
    from qmri_pnp_recon_poc_amd import engine
    a, tr, te, t1, t2, b1, p = engine.simulation_arguments(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], inp["b1"], inp["nstates"], False, 0.0, 1.0, dtype)
    K, T = t1.size, a.size
    arr, seq = engine.sequence_arguments(inp["blocks"], inp["ncycles"], T)
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
        eng._check(eng.L.qmri_dict_simulate_seq_dev(eng.h, K, T, vp(a), vp(tr), vp(te), d_t1, d_t2, d_b1 if b1 is not None else None, C.byref(p), C.byref(seq), d_F))
        assert hip.hipMemcpy(F.ctypes.data, d_F, F.nbytes, 2) == 0
    finally:
        for d in ptrs:
            hip.hipFree(d)
    return F.reshape((K, T), order="F")


@pytest.mark.parametrize("name", [n for n in sorted(Q.CASES) if n != "chain"])
def test_simulation_against_the_numpy_restatement(eng, name):
    """Every (G, R) instantiation on the four-block list in two cycles (s1 .. s256; block boundaries at 5, 21, 38 inside the kernel's 16-frame
    blocks, one block exactly 16 long; 45 atoms leave a ragged last group in every workgroup size), boundaries on multiples of 16 (b16), 48
    one-frame blocks with alternating preparations (ones), one atom of one frame in one block (k1), T = 1024 in 64 blocks played 16 times (t1024),
    many workgroups with a ragged tail of the staged stores (k5000), per-frame TR and TE (timing), per-atom b1 (b1)."""
    inp, ref = Q.case_inputs(name), Q.case_ref(name)
    F = eng.simulate_dictionary_seq(**inp)
    err = np.max(np.abs(F - ref))
    print(name, "max |F - ref| =", err, "atol =", Q.atol(name), "peak |F| =", np.abs(ref).max())
    assert F.shape == ref.shape and F.dtype == np.float64
    assert err <= Q.atol(name)


@pytest.mark.parametrize("name", ["s16", "s33", "s256", "timing", "inveff", "noinv", "b1", "k5000", "t1024"])
def test_one_block_gives_the_numbers_of_the_plain_simulation(eng, name):
    """One block {T, inversion, wait 0, ti, inv_eff} (or {T, none, 0, 0, 1}) in one cycle against Engine.simulate_dictionary on the fixtures of
    tests/epg_ref.py: equal as numbers (np.array_equal; the sign of a zero is not pinned)."""
    inp = R.case_inputs(name)
    want = eng.simulate_dictionary(**inp)
    F = eng.simulate_dictionary_seq(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], Q.degenerate_blocks(inp), 1, b1=inp["b1"], nstates=inp["nstates"])
    assert np.array_equal(F, want)


@pytest.mark.parametrize("name", ["s32", "timing", "s129"])
def test_cycles_equal_tiling_on_the_device(eng, name):
    """C = 3 cycles are the last T frames of one cycle on the 3-fold tiled train and block list (T = 144), bit for bit."""
    inp = Q.case_inputs(name)
    al, tr, te, bl = Q.tiled(inp["alpha"], inp["tr"], inp["te"], inp["blocks"], 3)
    big = eng.simulate_dictionary_seq(**dict(inp, alpha=al, tr=tr, te=te, blocks=bl, ncycles=1))
    F = eng.simulate_dictionary_seq(**dict(inp, ncycles=3))
    assert big.shape == (45, 144) and np.array_equal(F, big[:, 96:])
    assert not np.array_equal(F, big[:, :48])


def test_the_prepared_result_differs_from_the_plain_one(eng):
    """The schedule is not the plain train in disguise: the four-block, two-cycle result is away from qmri_dict_simulate's on the same train, and
    from its own first cycle, by far more than the tolerance, while each is within tolerance of its own reference."""
    a, b = Q.case_inputs("s32"), R.case_inputs("s32")
    Fa, Fb = eng.simulate_dictionary_seq(**a), eng.simulate_dictionary(**b)
    F1 = eng.simulate_dictionary_seq(**dict(a, ncycles=1))
    assert np.max(np.abs(Fa - Fb)) > 1e-3 and np.max(np.abs(Fa - F1)) > 1e-3
    assert np.max(np.abs(Fa - Q.case_ref("s32"))) <= Q.atol("s32") and np.max(np.abs(Fb - R.case_ref("s32"))) <= R.atol("s32")


@pytest.mark.parametrize("name", ["s32", "s129", "k5000"])
def test_fp32_output_is_the_fp64_output_rounded_once(eng, name):
    inp = Q.case_inputs(name)
    F64, F32 = eng.simulate_dictionary_seq(**inp), eng.simulate_dictionary_seq(**inp, dtype=np.float32)
    assert F32.dtype == np.float32 and np.array_equal(F32, F64.astype(np.float32))


@pytest.mark.parametrize("name", ["s16", "b1", "timing", "k5000"])
def test_entry_points_and_repeated_calls_give_equal_bits(eng, name):
    inp = Q.case_inputs(name)
    a, b = eng.simulate_dictionary_seq(**inp), eng.simulate_dictionary_seq(**inp)
    assert np.array_equal(a, b)
    assert np.array_equal(simulate_dev(eng, inp), a)
    assert np.array_equal(simulate_dev(eng, inp, np.float32), a.astype(np.float32))


def test_device_route_marks_a_bad_atom_with_nan_in_its_row_only(eng, engine_mod):
    """The device route cannot refuse a T1 <= 0 on the host: that atom's fingerprint is NaN in every frame, every other atom is untouched; the
    host-array route refuses the same input."""
    inp = Q.case_inputs("s32")
    good = simulate_dev(eng, inp)
    for key, k, v in (("t1", 7, 0.0), ("t1", 44, -1.0), ("t2", 0, np.nan), ("t2", 20, np.inf)):
        x = inp[key].copy()
        x[k] = v
        F = simulate_dev(eng, dict(inp, **{key: x}))
        assert np.all(np.isnan(F[k]))
        rest = np.arange(F.shape[0]) != k
        assert np.array_equal(F[rest], good[rest])
        with pytest.raises(engine_mod.QmriError) as e:
            eng.simulate_dictionary_seq(**dict(inp, **{key: x}))
        assert e.value.code == -1 and key in str(e.value)
    b = np.ones(45)
    b[3] = -0.5
    F = simulate_dev(eng, dict(inp, b1=b))
    assert np.all(np.isnan(F[3])) and np.array_equal(np.delete(F, 3, axis=0), np.delete(good, 3, axis=0))


def test_an_atoms_bits_do_not_depend_on_its_position(eng):
    """One atom simulated alone, first, last and inside K = 5000 (S = 16, T = 32, two blocks, two cycles): the same row every time."""
    inp = Q.case_inputs("k5000")
    full = eng.simulate_dictionary_seq(**inp)
    k = 2718
    t1, t2 = inp["t1"], inp["t2"]
    alone = eng.simulate_dictionary_seq(**dict(inp, t1=t1[k:k + 1], t2=t2[k:k + 1]))
    first = eng.simulate_dictionary_seq(**dict(inp, t1=t1[k:k + 70], t2=t2[k:k + 70]))
    last = eng.simulate_dictionary_seq(**dict(inp, t1=t1[k - 36:k + 1], t2=t2[k - 36:k + 1]))
    assert alone.shape == (1, 32) and np.array_equal(alone[0], full[k]) and np.array_equal(first[0], full[k]) and np.array_equal(last[-1], full[k])


def test_the_chain_simulate_compress_match(engine_mod):
    """harness.simulate_dictionary(blocks=synth.cmrf_blocks(...)) (simulate -> compress on one device buffer) on T = 48, 24 x 11 atoms, S = 32,
    s = 6 against epgseq_ref -> dict_svd_ref.dict_compress_ref with the bounds of tests/test_gpu_dict_svd.py; then set_dictionary and the match of
    the 32 x 32 pixels epg_ref.chain_match_input makes of the reference's own atoms: every pixel returns its own atom."""
    from qmri_pnp_recon_poc_amd import harness, synth
    TOL, s, n1, n2 = 1e-13, 6, 24, 11
    inp = Q.case_inputs("chain")
    t1g, t2g = np.exp(np.linspace(np.log(0.1), np.log(4.0), n1)), np.exp(np.linspace(np.log(0.01), np.log(0.6), n2))
    out = harness.simulate_dictionary(inp["alpha"], R.TR0, R.TE0, t1g, t2g, s=s, nstates=32, blocks=synth.cmrf_blocks(Q.CHAIN_RR, 8, R.TR0), ncycles=1)
    ref = DR.dict_compress_ref(Q.case_ref("chain"), s=s)
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
    e.close()
    idx = np.arange(1024) * (n1 * n2) // 1024
    assert np.array_equal(np.asarray(dev["dm"]), (idx + 1).reshape(32, 32))
