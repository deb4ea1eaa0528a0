"""GPU: the grouped dictionary match (include/qmri.h qmri_dict_match_grouped) against the ungrouped CPU oracle run once per
group (tests/dict_group_ref.py).  The contract is bits: every comparison is np.array_equal on dm, grp, mt, pd and qmap (and Xfit where named)."""
import ctypes as C

import numpy as np
import pytest

import dict_group_ref as GR

pytestmark = pytest.mark.gpu


def _check(g, o, keys=GR.KEYS, what=""):
    diff = GR.same(g, o, keys)
    if diff:
        bad = np.nonzero(np.asarray(g["dm"]).ravel() != np.asarray(o["dm"]).ravel())[0]
        print(what, "differing outputs:", diff, "pixels with another dm:", bad.size, bad[:10], np.asarray(g["dm"]).ravel()[bad[:10]], np.asarray(o["dm"]).ravel()[bad[:10]])
    assert not diff, (what, diff)


def _pixels_of_groups(rng, D, gp, grp, noise=0.02):
    """noisy scaled atoms of each pixel's own group (grp 1-based, 0: any atom)"""
    n, s = grp.size, D.shape[1]
    lo, hi = gp[np.maximum(grp, 1) - 1], gp[np.maximum(grp, 1)]
    atom = lo + (rng.random(n) * (hi - lo)).astype(np.int64)
    amp = (0.5 + rng.random(n)) * np.exp(2j * np.pi * rng.random(n))
    return D[atom].astype(np.complex128) * amp[:, None] + noise * (rng.standard_normal((n, s)) + 1j * rng.standard_normal((n, s))), atom


@pytest.fixture(scope="module")
def eng(engine_mod):
    e = engine_mod.Engine(0)
    yield e
    e.dict_filter(True, 1.0)
    e.close()


@pytest.mark.parametrize("s", [10, 3, 16])
def test_ragged_everything(eng, oracle, s):
    """K = 207 in groups of 37, 5, 64, 1 and 100 atoms (none but the first starts on a 32-atom tile), 301 pixels assigned at random and interleaved
    in memory; group 4 receives no pixel, the others counts that are no multiple of 32.  Filter on and off; Xfit too."""
    rng = np.random.default_rng(100 + s)
    sizes = [37, 5, 64, 1, 100]
    gp = np.concatenate([[0], np.cumsum(sizes)])
    gv = np.array([0.8, 0.9, 1.0, 1.1, 1.2])
    D, nd, lut = GR.random_dictionary(207, s, seed=s)
    grp = rng.choice([1, 2, 3, 5], size=301, p=[0.3, 0.2, 0.1, 0.4])
    counts = np.bincount(grp, minlength=6)
    assert counts[4] == 0 and any(c % 32 for c in counts[1:] if c)
    sel = gv[grp - 1] + rng.uniform(-0.04, 0.04, 301)
    X, _ = _pixels_of_groups(rng, D, gp, grp)
    o = GR.match_grouped(oracle, X, sel, D, nd, lut, gp, gv, want_xfit=True)
    assert np.array_equal(o["grp"], grp)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    for filt in (True, False):
        eng.dict_filter(filt, 1.0)
        g = eng.dict_match(X, sel=sel, want_xfit=True)
        _check(g, o, GR.KEYS + ("Xfit",), f"s={s} filter={filt}")
    assert np.all((o["dm"] > gp[grp - 1]) & (o["dm"] <= gp[grp]))


def test_the_group_wall(eng, oracle):
    """The same fingerprint in group 0 and in group 1: a pixel equal to it and assigned to group 1 gets the group-1 copy; and pixels whose best atom
    over ALL atoms lies in another group still get their own group's best -- the test an unrestricted match fails."""
    rng = np.random.default_rng(7)
    D, nd, lut = GR.random_dictionary(150, 10, seed=70)
    gp, gv = np.array([0, 50, 90, 150]), np.array([0.8, 1.0, 1.2])
    D[60] = D[10]                                                # the copy in group 1
    X = np.zeros((64, 10), np.complex128)
    sel = np.full(64, 1.0)
    X[0] = D[10] * (1.5 - 0.5j)
    X[1:] = D[rng.integers(0, 50, 63)] * 2.0 + 0.05 * rng.standard_normal((63, 10))          # atoms of group 0, matched in group 1 / 2
    sel[32:] = 1.2
    eng.set_dictionary(D, nd, lut)
    eng.dict_filter(True, 1.0)
    free = eng.dict_match(X)
    eng.set_dictionary_groups(gp, gv)
    g = eng.dict_match(X, sel=sel)
    o = GR.match_grouped(oracle, X, sel, D, nd, lut, gp, gv)
    _check(g, o)
    assert g["dm"][0] == 61 and free["dm"][0] == 11
    assert np.all(free["dm"][1:] <= 50) and np.all(g["dm"][1:32] > 50) and np.all(g["dm"][1:32] <= 90) and np.all(g["dm"][32:] > 90)


def test_zero_and_degenerate_pixels(eng, oracle):
    """An all-zero pixel of group g > 0 gives the group's first atom; a group of one atom; NaN in that group's lut -> 0; duplicate atoms inside a
    group tie in magnitude and the lowest index of the group wins."""
    D, nd, lut = GR.random_dictionary(120, 10, seed=3)
    gp, gv = np.array([0, 45, 46, 120]), np.array([0.8, 1.0, 1.2])
    lut[45, 1] = np.nan
    D[100] = D[70]
    D[50] = D[70]                                                # three copies in group 2: 50, 70, 100
    D[20] = D[70]                                                # and one in group 0, which must not win
    X = np.zeros((40, 10), np.complex128)
    sel = np.repeat(gv, [10, 10, 20])
    X[3], X[13], X[23] = 0, 0, 0                                 # all-zero pixels of each group
    X[14] = D[45] * 3.0
    X[15] = D[0] * 1.0                                           # any pixel of the one-atom group gets that atom
    X[25] = D[70] * (0.7 + 0.2j)
    X[26] = -D[100] * 2.0
    rng = np.random.default_rng(4)
    rest = [i for i in range(40) if i not in (3, 13, 23, 14, 15, 25, 26)]
    X[rest] = rng.standard_normal((len(rest), 10)) + 1j * rng.standard_normal((len(rest), 10))
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    o = GR.match_grouped(oracle, X, sel, D, nd, lut, gp, gv)
    for filt in (True, False):
        eng.dict_filter(filt, 1.0)
        g = eng.dict_match(X, sel=sel)
        _check(g, o, what=f"filter={filt}")
        assert g["dm"][3] == 1 and g["dm"][13] == 46 and g["dm"][23] == 47
        assert np.all(g["dm"][10:20] == 46) and np.all(g["qmap"][10:20, 1] == 0.0)
        assert g["dm"][25] == 51 and g["dm"][26] == 51


def test_unmatched_pixels(eng, oracle):
    rng = np.random.default_rng(11)
    D, nd, lut = GR.random_dictionary(207, 10, seed=5)
    gp, gv = np.array([0, 37, 42, 106, 107, 207]), np.array([0.8, 0.9, 1.0, 1.1, 1.2])
    grp = rng.integers(1, 6, 301)
    X, _ = _pixels_of_groups(rng, D, gp, grp)
    sel = gv[grp - 1].copy()
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    eng.dict_filter(True, 1.0)
    full = eng.dict_match(X, sel=sel, want_xfit=True)
    bad = rng.choice(301, 60, replace=False)
    sel2 = sel.copy()
    sel2[bad[:20]], sel2[bad[20:40]], sel2[bad[40:]] = np.nan, np.inf, -np.inf
    g = eng.dict_match(X, sel=sel2, want_xfit=True)
    o = GR.match_grouped(oracle, X, sel2, D, nd, lut, gp, gv, want_xfit=True)
    _check(g, o, GR.KEYS + ("Xfit",))
    keep = np.setdiff1d(np.arange(301), bad)
    for k in GR.KEYS + ("Xfit",):
        assert not np.any(g[k][bad]) and np.array_equal(g[k][keep], full[k][keep]), k
    z = eng.dict_match(X, sel=np.full(301, np.nan), want_xfit=True)                            # returns QMRI_OK
    for k in GR.KEYS + ("Xfit",):
        assert z[k].shape == full[k].shape and not np.any(z[k]), k


def test_atom_parts_inside_a_group(eng, oracle):
    """Three groups of 13 000, 20 000 and 7 000 atoms and 40 x 40 pixels: the launch splits every group's atoms over workgroups (and seeds the
    filter); thousands of atoms of the middle group tie within a few ulps ACROSS its part boundaries, as in
    test_dict_match_atoms_split_over_workgroups."""
    rng = np.random.default_rng(21)
    s, sizes = 10, [13000, 20000, 7000]
    gp, gv = np.concatenate([[0], np.cumsum(sizes)]), np.array([0.8, 1.0, 1.2])
    K = int(gp[-1])
    D, nd, lut = GR.random_dictionary(K, s, seed=8)
    base = rng.standard_normal(s).astype(np.float32)
    base /= np.linalg.norm(base)
    mid = np.repeat(base[None, :], sizes[1], axis=0)
    D[gp[1]:gp[2]] = (mid.view(np.int32) + rng.integers(-3, 4, size=mid.shape, dtype=np.int32)).view(np.float32)
    grp = rng.integers(1, 4, 1600)
    X, _ = _pixels_of_groups(rng, D, gp, grp, noise=0.01)
    m = grp == 2
    X[m] = base[None, :] * ((1.0 + rng.random((m.sum(), 1))) * np.exp(1j * rng.random((m.sum(), 1)) * 6.28)) + 1e-7 * rng.standard_normal((m.sum(), s))
    X, sel = X.reshape(40, 40, s), gv[grp - 1].reshape(40, 40)
    o = GR.match_grouped(oracle, X, sel, D, nd, lut, gp, gv)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    for filt in (True, False):
        eng.dict_filter(filt, 1.0)
        g = eng.dict_match(X, sel=sel)
        _check(g, o, what=f"filter={filt}")
    print("distinct winners in the tied group:", len(np.unique(o["dm"][sel == 1.0])))
    assert len(np.unique(o["dm"][sel == 1.0])) > 20


def test_one_full_slice(eng, oracle):
    """224 x 224 pixels, 5 groups of 64 x 32 atoms, a smooth B1 map from 0.8 to 1.2 with a NaN background: the reference's bits, the same bits
    on a second call, and the same bits for a random permutation of the pixels."""
    rng = np.random.default_rng(6)
    G, n, s = 5, 64 * 32, 10
    gp, gv = np.arange(G + 1) * n, np.linspace(0.8, 1.2, G)
    D, nd, lut = GR.random_dictionary(G * n, s, seed=9, Q=3)
    yy, xx = np.mgrid[0:224, 0:224] / 223.0
    b1 = 0.8 + 0.4 * xx + 0.03 * np.sin(5.0 * yy)
    b1[(xx - 0.5) ** 2 + (yy - 0.5) ** 2 > 0.23] = np.nan
    grp = GR.assign(gv, b1).ravel()
    assert set(np.unique(grp)) == set(range(G + 1))
    X, _ = _pixels_of_groups(rng, D, gp, grp)
    X = X.reshape(224, 224, s)
    o = GR.match_grouped(oracle, X, b1, D, nd, lut, gp, gv)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    eng.dict_filter(True, 1.0)
    g = eng.dict_match(X, sel=b1)
    _check(g, o)
    _check(eng.dict_match(X, sel=b1), g, what="second call")
    perm = rng.permutation(224 * 224)
    gpm = eng.dict_match(X.reshape(-1, s)[perm], sel=b1.ravel()[perm])
    for k in GR.KEYS:
        assert np.array_equal(gpm[k], g[k].reshape((224 * 224,) + g[k].shape[2:])[perm]), k


def test_coexistence_with_the_plain_match(eng, engine_mod, oracle):
    rng = np.random.default_rng(12)
    D, nd, lut = GR.random_dictionary(207, 10, seed=13)
    gp, gv = np.array([0, 37, 42, 106, 107, 207]), np.array([0.8, 0.9, 1.0, 1.1, 1.2])
    X = rng.standard_normal((301, 10)) + 1j * rng.standard_normal((301, 10))
    sel = rng.uniform(0.7, 1.3, 301)
    eng.set_dictionary(D, nd, lut)
    eng.dict_filter(True, 1.0)
    with pytest.raises(engine_mod.QmriError) as err:            # no groups yet
        eng.dict_match(X, sel=sel)
    assert err.value.code == -2
    before = eng.dict_match(X, want_xfit=True)
    eng.set_dictionary_groups(gp, gv)
    eng.dict_match(X, sel=sel)
    after = eng.dict_match(X, want_xfit=True)
    _check(after, before, ("dm", "mt", "pd", "qmap", "Xfit"))
    _check(after, oracle.dict_match(X, D, nd, lut), ("dm", "mt", "pd", "qmap"))
    with pytest.raises(engine_mod.QmriError) as err:            # group_ptr[G] != K
        eng.set_dictionary_groups([0, 37, 200], [0.8, 1.0])
    assert err.value.code == -1
    eng.dict_match(X, sel=sel)                                  # (a refused call leaves the groups as they were)
    eng.set_dictionary_groups(None, None)                       # G = 0 clears
    with pytest.raises(engine_mod.QmriError) as err:
        eng.dict_match(X, sel=sel)
    assert err.value.code == -2
    eng.set_dictionary_groups(gp, gv)
    eng.set_dictionary(D, nd, lut)                              # drops the groups
    with pytest.raises(engine_mod.QmriError) as err:
        eng.dict_match(X, sel=sel)
    assert err.value.code == -2
    Dw, ndw, lutw = GR.random_dictionary(64, 64, seed=14)       # a wide dictionary
    eng.set_dictionary(Dw, ndw, lutw)
    with pytest.raises(engine_mod.QmriError) as err:
        eng.set_dictionary_groups([0, 30, 64], [0.9, 1.1])
    assert err.value.code == -4                                 # QMRI_ERR_UNSUPPORTED


def test_device_route_and_device_assignment(eng, engine_mod, oracle):
    rng = np.random.default_rng(15)
    D, nd, lut = GR.random_dictionary(207, 10, seed=16)
    gp, gv = np.array([0, 37, 42, 106, 107, 207]), np.array([0.8, 0.9, 1.0, 1.1, 1.2])
    grp = rng.integers(1, 6, 301)
    X, _ = _pixels_of_groups(rng, D, gp, grp)
    sel = gv[grp - 1] + rng.uniform(-0.04, 0.04, 301)
    sel[::17] = np.nan
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    eng.dict_filter(True, 1.0)
    h = eng.dict_match(X, sel=sel, want_xfit=True)
    hip = engine_mod._hip_runtime()                             # (buffers from the HIP runtime libqmri itself uses)
    xb, sb = np.ascontiguousarray(X.ravel(order="F")), np.ascontiguousarray(sel)
    outs = {"qmap": np.empty(2 * 301, np.float32), "pd": np.empty(2 * 301, np.float32), "mt": np.empty(301, np.float32), "dm": np.empty(301, np.int32),
            "grp": np.empty(301, np.int32), "Xfit": np.empty(2 * 301 * 10, np.float32)}
    d = {k: C.c_void_p() for k in ("X", "sel") + tuple(outs)}
    try:
        for k, a in (("X", xb), ("sel", sb)) + tuple(outs.items()):
            assert hip.hipMalloc(C.byref(d[k]), a.nbytes) == 0
        assert hip.hipMemcpy(d["X"], xb.ctypes.data_as(C.c_void_p), xb.nbytes, 1) == 0 and hip.hipMemcpy(d["sel"], sb.ctypes.data_as(C.c_void_p), sb.nbytes, 1) == 0
        eng.dict_match_dev(d["X"].value, 301, d["qmap"].value, d["pd"].value, d["mt"].value, d["dm"].value, d["Xfit"].value, d_sel=d["sel"].value, d_grp=d["grp"].value)
        eng.synchronize()
        for k, a in outs.items():
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), d[k], a.nbytes, 2) == 0
    finally:
        for v in d.values():
            if v.value:
                hip.hipFree(v)
    assert np.array_equal(outs["dm"], h["dm"]) and np.array_equal(outs["grp"], h["grp"]) and np.array_equal(outs["mt"], h["mt"])
    assert np.array_equal(outs["pd"].view(np.complex64), h["pd"]) and np.array_equal(outs["qmap"].reshape((301, 2), order="F"), h["qmap"])
    assert np.array_equal(outs["Xfit"].view(np.complex64).reshape((301, 10), order="F"), h["Xfit"])
    # the device assignment on the host test's vector
    gv3, v = [0.75, 1.0, 1.25], np.array([0.875, 1.125, 0.1, 9.0, 1.0, np.nan, np.inf, -0.0])
    eng.set_dictionary_groups([0, 37, 106, 207], gv3)
    r = eng.dict_match(X[:8], sel=v)
    assert r["grp"].tolist() == [1, 2, 1, 3, 2, 0, 0, 1] == engine_mod.dict_group_assign(gv3, v).tolist()
    big = rng.uniform(0.3, 1.7, 301)
    assert np.array_equal(eng.dict_match(X, sel=big)["grp"], engine_mod.dict_group_assign(gv3, big))


def test_chain_simulate_compress_group_match(synth):
    """harness.simulate_dictionary with a b1 grid on a 12 x 8 (T1, T2) grid, T = 48, S = 16; pixels synthesised from known (atom, b1) and matched
    with the true B1 map: every pixel returns its own atom, and lut column 3 is its b1."""
    from qmri_pnp_recon_poc_amd import engine, harness
    t1g, t2g = np.exp(np.linspace(np.log(0.3), np.log(3.0), 12)), np.exp(np.linspace(np.log(0.03), np.log(0.3), 8))
    b1g = [0.8, 1.0, 1.2]
    dic = harness.simulate_dictionary(synth.flip_angle_train(48), 0.012, 0.002, t1g, t2g, s=8, nstates=16, b1_grid=b1g)
    assert dic["D"].shape == (288, 8) and dic["lut"].shape == (288, 3) and dic["group_ptr"].tolist() == [0, 96, 192, 288]
    rng = np.random.default_rng(17)
    atom = rng.integers(0, 288, 500)
    amp = (0.5 + rng.random(500)) * np.exp(2j * np.pi * rng.random(500))
    X = dic["D"][atom].astype(np.complex128) * (dic["normD"][atom] * amp)[:, None]
    b1 = np.asarray(b1g)[atom // 96] + rng.uniform(-0.05, 0.05, 500)
    e = engine.Engine(0)
    try:
        e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
        e.set_dictionary_groups(dic["group_ptr"], dic["group_val"])
        r = e.dict_match(X, sel=b1)
    finally:
        e.close()
    assert np.array_equal(r["dm"], atom + 1) and np.array_equal(r["grp"], atom // 96 + 1)
    assert np.array_equal(r["qmap"][:, 2], np.float32(b1g)[atom // 96]) and np.array_equal(r["qmap"], dic["lut"][atom])


def test_recon_tsmis_with_a_b1_map(oracle, synth):
    """harness.recon_tsmis(..., b1_map=...) on a B1-resolved dictionary: the maps are the grouped reference's on the reconstructed X, bit for bit
    (T1, T2 from lut columns 1-2, PD from pd), grp is passed through, and NaN pixels of the map come back as zeros."""
    from qmri_pnp_recon_poc_amd import harness as H, reference_api as R
    N, T, s = 32, 24, 6
    base = synth.make_dictionary(T=T, n_t1=12, n_t2=8, s=s)
    n, b1g = base["D"].shape[0], np.array([0.8, 1.0, 1.2])
    rng = np.random.default_rng(23)
    D = np.concatenate([base["D"] * (1.0 + 0.1 * rng.standard_normal(s))[None, :] for _ in b1g]).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True).astype(np.float32)
    dic = {"V": base["V"], "D": D, "normD": np.tile(base["normD"], 3), "lut": np.concatenate([np.tile(base["lut"], (3, 1)), np.repeat(b1g, n)[:, None]], axis=1).astype(np.float32),
           "group_ptr": np.arange(4, dtype=np.int32) * n, "group_val": b1g}
    q = np.asarray(synth.make_phantom_qmaps(N, seed=4))
    X0 = synth.synthesize_tsmi(q, base)
    b1 = 0.75 + 0.5 * np.linspace(0, 1, N)[None, :] * np.ones((N, 1))
    b1[:3, :] = np.nan
    try:
        r = H.recon_tsmis(dic, X0, q, recon_method="SVD_MRF", spiral_sampling_curve=120, seed=7, b1_map=b1)
    finally:
        R.release()
    o = GR.match_grouped(oracle, r["X"], b1, dic["D"], dic["normD"], dic["lut"], dic["group_ptr"], b1g)
    assert np.array_equal(r["grp"], o["grp"]) and set(np.unique(r["grp"])) == {0, 1, 2, 3}
    assert r["qmap"].shape == (N, N, 3)
    assert np.array_equal(np.real(r["qmap"][:, :, :2]).astype(np.float32), o["qmap"][:, :, :2]) and np.array_equal(r["qmap"][:, :, 2].astype(np.complex64), o["pd"])
    assert not np.any(r["qmap"][:3]) and not np.any(r["grp"][:3])
