"""CPU: the slice-profile-aware FISP dictionary simulation (include/qmri.h qmri_dict_simulate_sp) without a device -- the
identities of the numpy restatement tests/epgsp_ref.py, that the profile matters, synth.rf_slice_profile against its closed forms, the matching
bias a profile-blind dictionary causes, the fixture facts the GPU tolerances of tests/test_gpu_epgsp.py rest on, every refusal of both entry points,
the shape rules of the Python arguments, the MEX command's argument checks, the symbol list and the header text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import epg_ref as R
import epgsp_ref as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qmri_dict_simulate_sp", "qmri_dict_simulate_sp_dev"]


def _unit(F):
    return F / np.linalg.norm(F, axis=1, keepdims=True)


def test_identities_of_the_restatement():
    """Q = 1, w = 1, p = 1 is epg_fisp exactly; a frame-constant profile is sum_q w_q epg_fisp(b1 p_q) (exactly at b1 = 1, where both product orders
    give alpha_t p_q; on the b1 ramp within the RF-argument sensitivity of the fixture, the one-ulp difference between (alpha b1) p and
    alpha (b1 p)); a per-frame profile is sum_q w_q epg_fisp(alpha prof[:, q])."""
    inp = SP.case_inputs("one")
    plain = R.epg_fisp(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], nstates=32)
    assert np.array_equal(SP.case_ref("one"), plain) and np.array_equal(plain, R.case_ref("s32"))
    inp = SP.case_inputs("p4")
    want = np.zeros_like(plain)
    for q in range(4):
        want = want + inp["w"][q] * R.epg_fisp(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], b1=np.full(45, SP.P4[q]), nstates=32)
    assert np.array_equal(SP.case_ref("p4"), want)
    inp = SP.case_inputs("p4b1")
    want = np.zeros_like(plain)
    for q in range(4):
        want = want + inp["w"][q] * R.epg_fisp(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], b1=inp["b1"] * SP.P4[q], nstates=32)
    d = np.max(np.abs(SP.case_ref("p4b1") - want))
    print("product order on the b1 ramp:", d, "RF-argument sensitivity:", SP.SENS["p4b1"][2])
    assert 0.0 < d <= SP.SENS["p4b1"][2]
    inp = SP.case_inputs("q5")
    want = np.zeros_like(plain)
    for q in range(5):
        want = want + inp["w"][q] * R.epg_fisp(inp["alpha"] * inp["prof"][:, q], inp["tr"], inp["te"], inp["t1"], inp["t2"], nstates=32)
    assert np.array_equal(SP.case_ref("q5"), want)
    # a zero weight contributes nothing; the weights are not normalised
    z = SP.case_inputs("wzero")
    keep = [0, 1, 3, 4]
    assert np.array_equal(SP.case_ref("wzero"), SP.epg_fisp_sp(**dict(z, prof=z["prof"][:, keep], w=z["w"][keep])))
    assert np.array_equal(SP.epg_fisp_sp(**dict(inp, w=2.0 * inp["w"])), 2.0 * SP.case_ref("q5"))


def test_the_profile_matters():
    """Section 19's 9 x 5 grid, T = 48, S = 32 under the 4-point profile (1, 0.9, 0.6, 0.25) with equal weights: after each result is divided by its
    own norm the fingerprints are 6.7e-2 away from the unprofiled ones (measured: 0.0668; the floor is half of that).  A kernel that ignores prof is
    wrong by eleven orders more than the GPU tolerance."""
    d = np.max(np.abs(_unit(SP.case_ref("p4")) - _unit(R.case_ref("s32"))))
    print("normalised difference from the unprofiled simulation:", d)
    assert d > 0.033
    assert d > 1e9 * SP.atol("p4")


def test_rf_slice_profile_against_its_closed_forms():
    """One sub-pulse is a hard pulse: prof = 1 to 1e-14.  At z = 0 nothing precesses: 1.  At alpha = 1e-3 the profile is the small-tip one,
    |sum_p b_p exp(i phi_p(z))| / sum_p b_p: to 1e-6 of the profile's peak everywhere, and to 1e-6 of each entry wherever the profile is above 1 % of
    its peak (measured 2.9e-8 and 3.9e-7; the exact Bloch solution leaves the small-tip one by O(alpha^2) of the PEAK, which is 1.8e-6 of the two
    stop-band entries near 3e-3).  alpha = 0 returns that limit itself.  For the Hamming-windowed sinc of tbw = 4 the 10 degree and 70 degree
    profiles differ by 4.3e-2 (measured 0.0434; asserted at half): a profile depends on the nominal flip angle, which is why per_frame exists."""
    from qmri_pnp_recon_poc_amd import synth
    env, a = SP.sinc_envelope(), np.deg2rad([10.0, 70.0])
    p1, w = synth.rf_slice_profile(a, [2.5], 4.0, 8)
    assert p1.shape == (2, 8) and np.max(np.abs(p1 - 1.0)) <= 1e-14 and np.array_equal(w, np.full(8, 0.125))
    pz, _ = synth.rf_slice_profile(a, env, 4.0, 1, zmax=1e-13)
    assert np.max(np.abs(pz - 1.0)) <= 1e-12
    ps, _ = synth.rf_slice_profile([1e-3, 0.0], env, 4.0, 16)
    P = env.size
    z = (np.arange(16) + 0.5) / 16
    want = np.abs(np.exp(1j * np.outer(2 * np.pi * 4.0 * z / P, np.arange(P))) @ env) / env.sum()
    big = want > 0.01 * want.max()
    print("small tip: of the peak", np.max(np.abs(ps[0] - want)) / want.max(), "per entry above 1 %", np.max(np.abs(ps[0] / want - 1)[big]),
          "per entry everywhere", np.max(np.abs(ps[0] / want - 1)))
    assert np.max(np.abs(ps[0] - want)) <= 1e-6 * want.max() and np.max(np.abs(ps[0] / want - 1)[big]) <= 1e-6 and big.sum() >= 12
    assert np.max(np.abs(ps[1] - want)) <= 1e-14
    prof, _ = synth.rf_slice_profile(a, env, 4.0, 16)
    gap = np.max(np.abs(prof[0] - prof[1]))
    print("10 degrees against 70 degrees:", gap)
    assert gap > 0.0216 and np.all(prof >= 0) and np.all(np.isfinite(prof)) and prof[0, 0] > 0.99 and prof[0, -1] < 0.05
    for bad in (dict(envelope=[]), dict(envelope=[1.0, -1.0]), dict(nq=0), dict(zmax=0.0), dict(alpha=[-0.1])):
        kw = dict(alpha=a, envelope=env, tbw=4.0, nq=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            synth.rf_slice_profile(**kw)


def test_a_profile_blind_dictionary_biases_t2():
    """numpy only.  24 x 11 atoms, T = 200, S = 32, the tbw = 4 sinc on 8 sub-slices: pixels made of the profiled atoms, matched (largest normalised
    inner product) against the unprofiled dictionary, land off their true T2 for 73 % of the atoms (measured 0.727, median T2 ratio 1.5; asserted
    >= 50 %) and off their true T1 for some; matched against the profiled dictionary every one lands on its own atom."""
    from qmri_pnp_recon_poc_amd import synth
    t1, t2 = R.grid(24, 11)
    alpha = synth.flip_angle_train(200)
    prof, w = synth.rf_slice_profile(alpha, SP.sinc_envelope(), SP.TBW, 8)
    Dp = _unit(SP.epg_fisp_sp(alpha, R.TR0, R.TE0, t1, t2, prof=prof, w=w))
    D0 = _unit(R.epg_fisp(alpha, R.TR0, R.TE0, t1, t2))
    blind, aware = np.argmax(Dp @ D0.T, axis=1), np.argmax(Dp @ Dp.T, axis=1)
    off_t2, off_t1 = np.mean(t2[blind] != t2), np.mean(t1[blind] != t1)
    print("off T2:", off_t2, "off T1:", off_t1, "median T2 ratio:", np.median(t2[blind] / t2))
    assert off_t2 >= 0.5 and off_t1 > 0.0 and np.median(t2[blind] / t2) > 1.2
    assert np.array_equal(aware, np.arange(t1.size))


@pytest.mark.parametrize("name", sorted(SP.CASES) + ["chain"])
def test_fixture_facts_the_gpu_tolerance_rests_on(name):
    """Per GPU fixture, by section 19's method, on the restatement alone: how far the fp64 run is from its np.longdouble run, from its two runs with
    every exponential moved one fp64 ulp, and from its two runs with every RF argument (alpha_t b1) prof[t, q] moved one ulp (which covers the
    product-order difference between the profiled call and a sum of plain calls with b1 p_q).  SP.SENS holds the figures with a factor 2 of room:
    asserted from above, and from below at a quarter; the GPU tolerance SP.atol is 16 x the largest of the three."""
    ld, ex, ar = SP.measure(name)
    F = SP.case_ref(name)
    print(name, "fp64 - longdouble:", ld, "exponentials one ulp away:", ex, "RF arguments one ulp away:", ar, "table:", SP.SENS[name], "GPU atol:", SP.atol(name),
          "peak |F|:", np.abs(F).max())
    assert np.all(np.isfinite(F)) and np.abs(F).max() <= 1.0
    for got, tab in zip((ld, ex, ar), SP.SENS[name]):
        assert tab / 4 <= got <= tab
    assert SP.atol(name) == 16 * max(SP.SENS[name]) <= 1e-11


def test_the_chain_fixture_has_separated_eigenvalues_and_keeps_its_match():
    """T = 48, 24 x 11 atoms x b1 in (0.8, 1, 1.2), S = 32, Q = 5, s = 6: the kept eigenvalues of the profiled fingerprints have a smallest relative
    gap above 1e-6 (the precondition of the chain test's per-column bound), and the restatement alone keeps the match when the Gram matrix is
    summed in the reverse order: identical on >= 99 % of 32 x 32 pixels, the rest one grid step away."""
    import dict_svd_ref as DR
    from oracle import oracle as O
    F = SP.case_ref("chain")
    inp = SP.case_inputs("chain")
    r = DR.dict_compress_ref(F, s=SP.CHAIN["s"])
    print("gaps", r["gaps"], "energy kept", r["energy_kept"])
    assert r["gaps"].min() > 1e-6
    r2 = DR.dict_compress_ref(F, s=SP.CHAIN["s"], order=np.arange(F.shape[0])[::-1])
    lut = np.stack([inp["t1"], inp["t2"], inp["b1"]], axis=1).astype(np.float32)
    X = R.chain_match_input(r)
    a, b = O.dict_match(X, r["D"], r["normD"], lut), O.dict_match(X, r2["D"], r2["normD"], lut)
    steps = DR.grid_steps(a["dm"], b["dm"], 11)
    print("identical on", np.mean(steps == 0), "largest step", steps.max())
    assert np.mean(steps == 0) >= 0.99 and steps.max() <= 1


def test_symbols_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert re.search(r"\}\s*qmri_epg_profile\s*;", header)
    section = header[header.index("slice-profile-aware FISP dictionary simulation"):]
    head = section[:section.index("*/")]
    assert "extension" in head and "no reference counterpart" in head and "parity unpinned" in head
    body = section[:section.index("qmri_dict_simulate_sp_dev(")]
    for phrase in ("(alpha_t b1_k) prof[t, q]", "ascending q", "NOT normalised", "no atomics", "NaN in every frame"):
        assert phrase in body, phrase
    plain = header[header.index("FISP dictionary simulation by extended phase graphs"):header.index("slice-profile-aware FISP")]
    assert "qmri_dict_simulate_sp" in plain                   # the plain entry points' comment points to the new calls
    assert re.search(r"#define\s+QMRI_ABI_VERSION\s+1\b", header) and _lib.lib().qmri_abi_version() == 1
    assert C.sizeof(_lib.EpgProfile) == 24 and _lib.EpgProfile.prof.offset == 8 and _lib.EpgProfile.weight.offset == 16


def test_every_refusal_of_both_entry_points_without_a_device():
    """With ctx == NULL each call returns QMRI_ERR_INVALID_ARG for its first failing check and leaves the message in qmri_last_error(NULL): the
    refusals of qmri_dict_simulate first, then the profile's own; a call whose arguments are all fine is refused for the missing context."""
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import EpgParams, EpgProfile
    L = _lib.lib()
    K, T, Q = 3, 4, 3
    base = dict(al=[0.1, 0.2, 0.0, 0.4], tr=[0.012, 0.012, 0.013, 0.012], te=[0.002, 0.0, 0.013, 0.002], t1=[1.0, 0.5, 2.0], t2=[0.1, 0.05, 0.2], b1=[1.0, 0.0, 1.2])
    Fb = np.zeros(K * T)
    keep = []

    def P(nstates=32, inversion=1, ti=0.0, inv_eff=1.0, f64=1):
        return EpgParams(nstates, inversion, ti, inv_eff, f64)

    def S(nq=Q, per_frame=0, prof=(1.0, 0.7, 0.0), w=(0.5, 0.0, 0.5)):
        arrs = [None if x is None else np.array(x, dtype=np.float64) for x in (prof, w)]
        keep.extend(arrs)
        return EpgProfile(nq, per_frame, *[None if a is None else a.ctypes.data for a in arrs])

    pf = 1.0 - 0.05 * np.arange(T * Q)

    def call(fn, K=K, T=T, p=P(), sp=S(), F=Fb, **kw):
        arrs = {k: (None if k in kw and kw[k] is None else np.array(kw.get(k, v), dtype=np.float64)) for k, v in base.items()}
        ptr = {k: (a.ctypes.data_as(C.c_void_p) if a is not None else None) for k, a in arrs.items()}
        st = fn(None, K, T, ptr["al"], ptr["tr"], ptr["te"], ptr["t1"], ptr["t2"], ptr["b1"], C.byref(p) if p is not None else None,
                C.byref(sp) if sp is not None else None, F.ctypes.data_as(C.c_void_p) if F is not None else None)
        return st, L.qmri_last_error(None)

    def with_(key, i, v):
        x = list(base[key])
        x[i] = v
        return {key: x}

    def entry(x, i, v):
        x = list(x)
        x[i] = v
        return x

    nan, inf = float("nan"), float("inf")
    common = [(dict(p=None), b"params"), (dict(al=None), b"alpha /"), (dict(tr=None), b"alpha /"), (dict(te=None), b"alpha /"), (dict(t1=None), b"alpha /"),
              (dict(t2=None), b"alpha /"), (dict(F=None), b"F_out"), (dict(K=0), b"K must"), (dict(K=-1), b"K must"), (dict(T=0), b"T must"), (dict(T=1025), b"T must"),
              (dict(p=P(nstates=0)), b"nstates"), (dict(p=P(nstates=257)), b"nstates"), (dict(p=P(inversion=2)), b"inversion"), (dict(p=P(f64=2)), b"out_is_f64"),
              (dict(p=P(ti=-1.0)), b"ti must"), (dict(p=P(ti=nan)), b"ti must"), (dict(p=P(inv_eff=0.0)), b"inv_eff"), (dict(p=P(inv_eff=1.5)), b"inv_eff"),
              (dict(p=P(inv_eff=nan)), b"inv_eff"), (dict(p=None, sp=None), b"params"), (dict(T=0, sp=S(nq=0)), b"T must")]
    for bad in (-0.1, nan, inf):
        common += [(with_("al", 2, bad), b"alpha must"), (with_("tr", 3, bad), b"tr must"), (with_("te", 1, bad), b"te must")]
        common += [(dict(sp=S(prof=entry((1.0, 0.7, 0.0), 2, bad))), b"prof must"), (dict(sp=S(per_frame=1, prof=entry(pf, T * Q - 1, bad))), b"prof must"),
                   (dict(sp=S(w=entry((0.5, 0.0, 0.5), 1, bad))), b"weight must")]
    common += [(with_("tr", 1, 0.0), b"tr must"), (with_("te", 0, 0.0125), b"te must not exceed tr"),
               (dict(sp=None), b"slice profile"), (dict(sp=S(nq=0)), b"nq must"), (dict(sp=S(nq=-1)), b"nq must"), (dict(sp=S(nq=65)), b"nq must"),
               (dict(sp=S(per_frame=2)), b"per_frame"), (dict(sp=S(per_frame=-1)), b"per_frame"), (dict(sp=S(prof=None)), b"prof / weight"),
               (dict(sp=S(w=None)), b"prof / weight"), (dict(sp=S(w=(0.0, 0.0, 0.0))), b"sum to more than 0"),
               (dict(), b"ctx"), (dict(b1=None), b"ctx"), (dict(sp=S(per_frame=1, prof=pf)), b"ctx"), (dict(sp=S(nq=1, prof=(0.0,), w=(1e-300,))), b"ctx"),
               (dict(p=P(inversion=0, ti=-1.0, inv_eff=9.0)), b"ctx"), (with_("b1", 0, 0.0), b"ctx")]
    atoms = []
    for bad in (0.0, -1.0, nan, inf):
        atoms += [(with_("t1", 2, bad), b"t1 must"), (with_("t2", 0, bad), b"t2 must")]
        if bad != 0.0:
            atoms.append((with_("b1", 1, bad), b"b1 must"))
    for fn, host in ((L.qmri_dict_simulate_sp, True), (L.qmri_dict_simulate_sp_dev, False)):
        for kw, word in common + [(kw, word if host else b"ctx") for kw, word in atoms]:
            st, msg = call(fn, **kw)
            assert st == -1 and word in msg, (host, kw, st, msg)


def test_python_argument_rules():
    """slice_profile is [Q] or [T, Q], slice_weights [Q] with the default 1 / Q; the arrays are handed over as contiguous float64 with per_frame
    saying which layout; None leaves the old calls in place."""
    from qmri_pnp_recon_poc_amd import engine, harness
    assert engine.slice_profile_arguments(None, None, 7) is None
    prof, w, sp = engine.slice_profile_arguments([1.0, 0.5, 0.25, 0.0], None, 7)
    assert (sp.nq, sp.per_frame) == (4, 0) and w.tolist() == [0.25] * 4 and prof.dtype == w.dtype == np.float64 and sp.prof == prof.ctypes.data
    pf = np.arange(21, dtype=np.float32).reshape(7, 3)[:, ::-1]           # not contiguous, not float64
    prof, w, sp = engine.slice_profile_arguments(pf, [1, 2, 3], 7)
    assert (sp.nq, sp.per_frame) == (3, 1) and prof.flags["C_CONTIGUOUS"] and np.array_equal(prof, pf) and w.tolist() == [1.0, 2.0, 3.0]
    assert sp.weight == w.ctypes.data
    prof, w, sp = engine.slice_profile_arguments(np.ones((1, 5)), None, 1)  # T = 1: [1, Q] is per frame
    assert (sp.nq, sp.per_frame) == (5, 1)
    for bad in (dict(slice_profile=np.ones((6, 3))), dict(slice_profile=np.ones((7, 3, 1))), dict(slice_profile=np.ones(65)), dict(slice_profile=np.ones(0)),
                dict(slice_profile=1.0), dict(slice_weights=[0.5, 0.5]), dict(slice_weights=np.ones((3, 1))), dict(slice_profile=[1.0, -0.1, 0.5]),
                dict(slice_profile=[1.0, np.nan, 0.5]), dict(slice_weights=[0.0, 0.0, 0.0]), dict(slice_weights=[1.0, np.inf, 0.0]),
                dict(slice_weights=[1.0, -1.0, 1.0]), dict(slice_profile=[1.0, 1j, 0.5]), dict(slice_profile=None, slice_weights=[1.0])):
        kw = dict(slice_profile=[1.0, 0.5, 0.25], slice_weights=None, T=7)
        kw.update(bad)
        with pytest.raises(ValueError):
            engine.slice_profile_arguments(**kw)
    e = engine.Engine.__new__(engine.Engine)
    al = np.linspace(0.1, 0.5, 7)
    with pytest.raises(ValueError):
        e.simulate_dictionary(al, 0.012, 0.002, [1.0], [0.1], slice_profile=np.ones((6, 3)))
    with pytest.raises(ValueError):
        e.simulate_compress_dictionary(al, 0.012, 0.002, [1.0, 2.0], [0.1], s=1, slice_profile=np.ones(3), slice_weights=np.ones(2))
    # the harness hands the profile through and composes it with b1_grid: atoms, lut and groups as without one
    seen = {}

    class Stub:
        def __init__(self, device):
            pass

        def simulate_compress_dictionary(self, alpha, tr, te, t1, t2, **kw):
            seen.update(kw=kw, K=len(t1))
            return {"V": np.zeros((len(alpha), 2)), "D": np.zeros((len(t1), 2), np.float32), "normD": np.zeros(len(t1), np.float32), "eig": np.zeros(2), "info": {"s": 2}}

        def close(self):
            pass

    real = engine.Engine
    engine.Engine = Stub
    try:
        pr = np.ones((7, 3))
        out = harness.simulate_dictionary(al, 0.012, 0.002, [1.0, 2.0], [0.1, 0.2, 0.3], s=2, b1_grid=[0.9, 1.1], slice_profile=pr, slice_weights=[0.2, 0.3, 0.5])
        assert seen["kw"]["slice_profile"] is pr and seen["kw"]["slice_weights"] == [0.2, 0.3, 0.5] and seen["K"] == 12
        assert out["lut"].shape == (12, 3) and out["group_ptr"].tolist() == [0, 6, 12] and seen["kw"]["b1"].tolist() == [0.9] * 6 + [1.1] * 6
        harness.simulate_dictionary(al, 0.012, 0.002, [1.0, 2.0], [0.1, 0.2, 0.3], s=2)
        assert "slice_profile" not in seen["kw"] and "slice_weights" not in seen["kw"]
    finally:
        engine.Engine = real


def test_mex_dict_simulate_sp_checks_its_arguments_under_the_mock_gateway():
    from mexmock import MexError, qmri_mex
    al, t1, t2, e = np.full(4, 0.2), np.array([1.0, 2.0]), np.array([0.1, 0.2]), np.zeros((0, 0))
    w, pc, pf = np.full(3, 1 / 3), np.ones(3), np.ones((3, 4))
    ok = (al, np.array([0.012]), np.array([0.002]), t1, t2, e, {}, pc, w)

    def swap(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    sp = "qmri:dict_simulate_sp:"
    for args, ident in ((ok[:8], "qmri:usage"), (swap(6, 1.0), sp + "params"), (swap(0, al + 0j), sp + "alpha"), (swap(0, np.zeros(1025)), sp + "alpha"),
                        (swap(0, al.astype(np.float32)), sp + "alpha"), (swap(1, np.full(3, 0.012)), sp + "tr"), (swap(2, np.full(5, 0.002)), sp + "te"),
                        (swap(3, t1 + 0j), sp + "atoms"), (swap(4, np.array([0.1])), sp + "atoms"), (swap(5, np.ones(3)), sp + "atoms"),
                        (swap(5, np.ones(2) + 0j), sp + "atoms"), (swap(6, {"nstates": 0.0}), sp + "params"), (swap(6, {"nstates": 257.0}), sp + "params"),
                        (swap(6, {"nstates": 2.5}), sp + "params"), (swap(6, {"inversion": 2.0}), sp + "params"), (swap(6, {"ti": -1.0}), sp + "params"),
                        (swap(6, {"inv_eff": 0.0}), sp + "params"), (swap(6, {"single": 3.0}), sp + "params"),
                        (swap(8, w + 0j), sp + "profile"), (swap(8, w.astype(np.float32)), sp + "profile"), (swap(8, np.zeros(0)), sp + "profile"),
                        (swap(8, np.full(65, 1 / 65)), sp + "profile"), (swap(7, pc + 0j), sp + "profile"), (swap(7, np.ones(4)), sp + "profile"),
                        (swap(7, np.ones((3, 3))), sp + "profile"), (swap(7, pf.T.copy()), sp + "profile"), (swap(7, pf.astype(np.float32)), sp + "profile")):
        with pytest.raises(MexError) as err:
            qmri_mex("dict_simulate_sp", *args, nargout=1)
        assert err.value.id == ident, (ident, err.value.id, err.value.msg)
    m = open(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "matlab", "qmri_dict_simulate_sp.m")).read()
    assert "qmri_mex('dict_simulate_sp'" in m and "qmri:dict_simulate_sp:profile" in m


def test_refusals_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_epgsp.cpp against the host-only sanitised library: every refusal of qmri_dict_simulate_sp and
    qmri_dict_simulate_sp_dev without a context and with one (a per-frame profile of exactly T Q entries is read to its last entry and no
    further), and the launch plan's atoms per workgroup."""
    csrc = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    if not rt_dirs:
        pytest.skip("clang sanitizer runtime not found")
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "_build_asan", "host_asan_epgsp")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_EPGSP_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
