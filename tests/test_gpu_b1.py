"""GPU: the B1 estimate from the fingerprints (include/qmri.h qmri_dict_group_scores / qmri_b1_pool / qmri_b1_estimate) against
its restatement on the CPU oracle (tests/b1_ref.py).  The contract is bits: every comparison is np.array_equal.  What the fixtures themselves must
satisfy is asserted on the restatement alone in tests/test_b1_host.py."""
import ctypes as C

import numpy as np
import pytest

import b1_ref as BR
import dict_group_ref as GR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(engine_mod):
    e = engine_mod.Engine(0)
    yield e
    e.L.qmri_debug_knob(b"b1_scratch_mb", 256)
    e.dict_filter(True, 1.0)
    e.close()


def _same(g, o, what=""):
    diff = BR.same(g, o)
    if diff:
        bad = np.nonzero(np.asarray(g["grp"]).ravel() != np.asarray(o["grp"]).ravel())[0]
        print(what, "differing outputs:", diff, "pixels with another grp:", bad.size, bad[:10])
    assert not diff, (what, diff)


# ---- stage 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [3, 10, 16])
def test_scores_on_ragged_groups(eng, oracle, s):
    """Groups of 37 / 5 / 64 / 1 / 100 atoms, 301 pixels as a 43 x 7 image with one all-zero and one NaN pixel: the restatement's bits, and the mt
    of G grouped matches with a constant selector on the device."""
    D, nd, lut, gp, gv = BR.ragged_dictionary(s)
    X, zero, nan = BR.ragged_scores_image(s)
    want = BR.scores(oracle, X, D, nd, lut, gp)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    got = eng.group_scores(X)
    assert got.shape == (5, 43, 7) and got.dtype == np.float32
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))
    assert bad[0].size == 0, (bad[0].size, [b[:5] for b in bad], got[bad][:5], want[bad][:5])
    for filt in (True, False):
        eng.dict_filter(filt, 1.0)
        for g in range(5):
            mt = eng.dict_match(X, sel=np.full((43, 7), gv[g]))["mt"]
            assert np.array_equal(mt.view(np.int32), got[g].view(np.int32)), (s, filt, g)
    eng.dict_filter(True, 1.0)
    assert np.array_equal(eng.group_scores(X).view(np.int32), got.view(np.int32))                 # a repeated call


def test_scores_with_a_group_of_13000_atoms(eng, oracle):
    """Groups of 13 000, 5 and 3 000 atoms and 301 pixels: few enough units that the launch splits a group's atoms into parts (the small group
    then has empty parts); the same fingerprint is planted on both sides of every boundary a split of the 407 tiles into 2 .. 6 equal parts has,
    and 40 pixels are multiples of it."""
    rng = np.random.default_rng(31)
    s, sizes = 10, [13000, 5, 3000]
    gp, gv = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), np.array([0.8, 1.0, 1.2])
    D, nd, lut = GR.random_dictionary(int(gp[-1]), s, seed=32)
    twin = D[7].copy()
    for parts in range(2, 7):
        per = -(-407 // parts)
        for z in range(1, parts):                                                                 # the last row of a part and the first of the next
            D[32 * z * per - 1] = twin
            D[32 * z * per] = twin
    D[12999] = twin
    atom = rng.integers(0, int(gp[-1]), 301)
    amp = (0.5 + rng.random(301)) * np.exp(2j * np.pi * rng.random(301))
    X = D[atom].astype(np.complex128) * amp[:, None] + 0.02 * (rng.standard_normal((301, s)) + 1j * rng.standard_normal((301, s)))
    X[:40] = twin[None, :].astype(np.complex128) * amp[:40, None]
    X = X.reshape((43, 7, s), order="F")
    want = BR.scores(oracle, X, D, nd, lut, gp)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    got = eng.group_scores(X)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(eng.group_scores(X[:3, :2]).view(np.int32), want[:, :3, :2].view(np.int32))   # six pixels


def test_scores_device_route(eng, engine_mod, oracle):
    s = 10
    D, nd, lut, gp, gv = BR.ragged_dictionary(s)
    X, _, _ = BR.ragged_scores_image(s)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    host = eng.group_scores(X)
    hip = engine_mod._hip_runtime()
    xb = np.ascontiguousarray(X.reshape((301, s), order="F").ravel(order="F"))
    out = np.empty((5, 301), np.float32)
    dX, dS = C.c_void_p(), C.c_void_p()
    try:
        assert hip.hipMalloc(C.byref(dX), xb.nbytes) == 0 and hip.hipMalloc(C.byref(dS), out.nbytes) == 0
        assert hip.hipMemcpy(dX, xb.ctypes.data_as(C.c_void_p), xb.nbytes, 1) == 0
        for _ in range(2):
            eng.group_scores_dev(dX.value, 301, dS.value)
            eng.synchronize()
            assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), dS, out.nbytes, 2) == 0
            assert np.array_equal(out.reshape((5, 43, 7), order="F").view(np.int32), host.view(np.int32))
        eng.set_dictionary_groups(None, None)
        with pytest.raises(engine_mod.QmriError) as err:                                          # the library's own refusal: no groups
            eng.group_scores_dev(dX.value, 301, dS.value)
        assert err.value.code == -2
        with pytest.raises(ValueError):
            eng.group_scores(X)
    finally:
        for v in (dX, dS):
            if v.value:
                hip.hipFree(v)


# ---- stage 2 -------------------------------------------------------------------------------------------------------------------------------------
def _hand_scores(rng, G, lead):
    """float32 scores with everything a score can be: NaN, +Inf, negative (the oracle's -1 among them) and zero entries"""
    S = (rng.random((G,) + lead) ** 2).astype(np.float32)
    k = rng.random(S.shape)
    S[k < 0.03] = np.nan
    S[(k >= 0.03) & (k < 0.05)] = np.inf
    S[(k >= 0.05) & (k < 0.08)] = -1.0
    S[(k >= 0.08) & (k < 0.12)] = 0.0
    S[(k >= 0.12) & (k < 0.13)] = -np.inf
    return S


POOL_CASES = [(3, (5, 4), h) for h in (0, 1, 2, 32)] + [(5, (43, 7), h) for h in (0, 1, 3, 8)] + [(256, (8, 8), 1), (1, (9, 6), 2)]


@pytest.mark.parametrize("G,lead,h", POOL_CASES)
def test_pool_on_hand_made_scores(eng, G, lead, h):
    rng = np.random.default_rng(1000 * G + 10 * lead[0] + h)
    S = _hand_scores(rng, G, lead)
    gv = np.sort(rng.uniform(0.5, 1.5, G))
    mask = rng.random(lead) > 0.2                                                                 # holes
    mask[0, 0] = False
    for m in (None, mask):
        want = BR.pool(S, gv, m, h)
        _same(eng.b1_pool(S, gv, mask=m, window=h), want, f"G={G} {lead} h={h} mask={m is not None}")
    want = BR.pool(S, gv, mask, h)
    assert want["grp"][0, 0] == 0 and np.isnan(want["b1"][0, 0]) and want["conf"][0, 0] == 0.0 and (want["grp"] > 0).any()
    if G == 1:
        assert np.all(want["conf"][want["grp"] > 0] == 1.0)
    for leave in BR.KEYS:                                                                         # every nullable output left out in turn
        r = eng.b1_pool(S, gv, mask=mask, window=h, **{"want_" + leave: False})
        assert leave not in r and not BR.same(r, want, [k for k in BR.KEYS if k != leave]), leave


def test_pool_identical_planes_go_to_the_lower_group(eng):
    rng = np.random.default_rng(5)
    S = _hand_scores(rng, 4, (11, 9))
    S[1] = (1.0 + rng.random((11, 9))).astype(np.float32)                                         # finite, and above every other finite score
    S[2] = S[1]
    S[np.isinf(S)] = np.float32(0.5)
    gv = np.array([0.7, 0.9, 1.1, 1.3])
    for h in (0, 2):
        want = BR.pool(S, gv, None, h)
        got = eng.b1_pool(S, gv, window=h)
        _same(got, want)
        assert np.all(got["grp"] == 2) and np.all(got["b1"] == 0.9)                               # never group 3, its equal
        assert np.all(got["conf"] == 0.0)                                                         # best == second: no confidence


def test_pool_slices_do_not_see_each_other(eng):
    """(2, 16 x 16, 3, h = 4): the stack equals the three slices run alone; one slice is all background; the same with one slice per launch."""
    rng = np.random.default_rng(6)
    S = _hand_scores(rng, 2, (16, 16, 3))
    gv = np.array([0.9, 1.1])
    mask = rng.random((16, 16, 3)) > 0.1
    mask[:, :, 1] = False
    want = BR.pool(S, gv, mask, 4)
    got = eng.b1_pool(S, gv, mask=mask, window=4)
    _same(got, want)
    assert not np.any(got["grp"][:, :, 1]) and np.all(np.isnan(got["b1"][:, :, 1])) and not np.any(got["conf"][:, :, 1])
    for k in range(3):
        alone = eng.b1_pool(S[:, :, :, k], gv, mask=mask[:, :, k], window=4)
        assert not BR.same(alone, {key: got[key][:, :, k] for key in BR.KEYS}), k
    eng.L.qmri_debug_knob(b"b1_scratch_mb", 0)
    try:
        _same(eng.b1_pool(S, gv, mask=mask, window=4), want, "one slice per launch")
    finally:
        eng.L.qmri_debug_knob(b"b1_scratch_mb", 256)


def test_pool_refusals_with_a_context(eng, engine_mod):
    S = np.ones((3, 5, 4), np.float32)
    for gv in ([1.0, 0.8, 1.2], [0.8, 0.8, 1.2], [0.8, np.nan, 1.2]):
        with pytest.raises(engine_mod.QmriError) as err:
            eng.b1_pool(S, gv)
        assert err.value.code == -1
    with pytest.raises(engine_mod.QmriError) as err:
        eng.b1_pool(np.ones((257, 2, 2), np.float32), np.arange(257.0))
    assert err.value.code == -1


# ---- composed call -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [10, 16])
def test_estimate_is_scores_then_pool(eng, oracle, s):
    D, nd, lut, gp, gv = BR.ragged_dictionary(s)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    rng = np.random.default_rng(40 + s)
    for nsl in (1, 2):
        X, _ = BR.pooling_fixture(s, nslices=nsl)
        mask = rng.random(X.shape[:-1]) > 0.15
        S = eng.group_scores(X)
        assert np.array_equal(S.view(np.int32), BR.scores(oracle, X, D, nd, lut, gp).view(np.int32))
        for h in (0, 1, 3, 8):
            for m in (None, mask):
                got = eng.estimate_b1(X, mask=m, window=h)
                _same(got, eng.b1_pool(S, gv, mask=m, window=h), f"s={s} nsl={nsl} h={h} composed against the two stages")
                _same(got, BR.pool(S, gv, m, h), f"s={s} nsl={nsl} h={h} against the restatement")
                n_est = int(np.sum(got["grp"] > 0))
                assert got["info"]["n_estimated"] == n_est and got["info"]["n_unmatched"] == got["grp"].size - n_est
                assert abs(got["info"]["mean_conf"] - got["conf"][got["grp"] > 0].mean()) < 1e-12     # (summed in another order)
    # a slice at a time (the scratch bound forced down): the same bits, and through the device route
    X, _ = BR.pooling_fixture(s, nslices=2)
    want = eng.estimate_b1(X, window=3)
    eng.L.qmri_debug_knob(b"b1_scratch_mb", 0)
    try:
        _same(eng.estimate_b1(X, window=3), want, "one slice per run")
    finally:
        eng.L.qmri_debug_knob(b"b1_scratch_mb", 256)


def test_estimate_device_route(eng, engine_mod):
    s = 10
    D, nd, lut, gp, gv = BR.ragged_dictionary(s)
    X, _ = BR.pooling_fixture(s, nslices=2)
    eng.set_dictionary(D, nd, lut)
    eng.set_dictionary_groups(gp, gv)
    mask = np.ones(X.shape[:-1], bool)
    mask[::5, 1] = False
    host = eng.estimate_b1(X, mask=mask, window=2)
    hip = engine_mod._hip_runtime()
    n = 43 * 7 * 2
    xb = np.ascontiguousarray(X.reshape((n, s), order="F").ravel(order="F"))
    mb = np.ascontiguousarray(mask.ravel(order="F").astype(np.uint8))
    outs = {"b1": np.empty(n, np.float64), "grp": np.empty(n, np.int32), "conf": np.empty(n, np.float64)}
    two = {k: np.empty_like(v) for k, v in outs.items()}
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    d = {k: C.c_void_p() for k in ("X", "mask", "score") + tuple(outs)}
    try:
        for k, a in (("X", xb), ("mask", mb), ("score", np.empty(5 * n, np.float32))) + tuple(outs.items()):
            assert hip.hipMalloc(C.byref(d[k]), a.nbytes) == 0
        assert hip.hipMemcpy(d["X"], xb.ctypes.data_as(C.c_void_p), xb.nbytes, 1) == 0 and hip.hipMemcpy(d["mask"], mb.ctypes.data_as(C.c_void_p), mb.nbytes, 1) == 0
        eng.estimate_b1_dev(d["X"].value, 43, 7, 2, d["mask"].value, 2, d["b1"].value, d["grp"].value, d["conf"].value)
        eng.synchronize()
        for k, a in outs.items():
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), d[k], a.nbytes, 2) == 0
            assert hip.hipMemset(d[k], 0xFF, a.nbytes) == 0
        eng.group_scores_dev(d["X"].value, n, d["score"].value)                                   # the two stages on device arrays
        eng.b1_pool_dev(gv, 43, 7, 2, d["score"].value, d["mask"].value, 2, d["b1"].value, d["grp"].value, d["conf"].value)
        eng.synchronize()
        for k, a in two.items():
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), d[k], a.nbytes, 2) == 0
    finally:
        for v in d.values():
            if v.value:
                hip.hipFree(v)
    _same({k: v.reshape((43, 7, 2), order="F") for k, v in outs.items()}, host)
    _same({k: v.reshape((43, 7, 2), order="F") for k, v in two.items()}, host)


def test_recon_tsmis_with_an_estimated_b1_map(synth):
    """harness.recon_tsmis(b1_map="estimate") on a 32 x 32 case equals estimate_b1 on its X inside its foreground mask followed by
    recon_tsmis(b1_map=that), bit for bit, on grp and the maps."""
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
    kw = dict(recon_method="SVD_MRF", spiral_sampling_curve=120, seed=7)
    try:
        r = H.recon_tsmis(dic, X0, q, b1_map="estimate", b1_window=3, **kw)
        est = H.estimate_b1(dic, r["X"], mask=r["foreground_mask"], window=3)
        two = H.recon_tsmis(dic, X0, q, b1_map=est["b1"], **kw)
    finally:
        R.release()
    assert np.array_equal(r["X"], two["X"])
    assert np.array_equal(r["b1_est"], est["b1"], equal_nan=True) and np.array_equal(r["b1_conf"], est["conf"]) and np.array_equal(r["grp"], est["grp"])
    assert np.array_equal(r["grp"], two["grp"]) and np.array_equal(r["qmap"], two["qmap"])
    fg = np.asarray(r["foreground_mask"]) != 0
    assert fg.any() and not np.any(r["grp"][~fg]) and np.all(np.isnan(r["b1_est"][~fg])) and not np.any(r["qmap"][~fg])


# ---- it estimates --------------------------------------------------------------------------------------------------------------------------------
def test_the_phantom(eng, oracle):
    """The 32 x 32 EPG phantom at 30 dB (tests/b1_ref.py): the device gives the restatement's bits at h = 0 and h = 4, hence its errors -- and
    tests/test_b1_host.py holds the restatement's mean |b1 - truth| at h = 4 to 0.8 times its value at h = 0."""
    ph = BR.epg_phantom()
    eng.set_dictionary(ph["D"], ph["normD"], ph["lut"])
    eng.set_dictionary_groups(ph["group_ptr"], ph["group_val"])
    err = {}
    for h in (0, 4):
        want = BR.estimate(oracle, ph["X"], ph["D"], ph["normD"], ph["lut"], ph["group_ptr"], ph["group_val"], ph["mask"], h)
        got = eng.estimate_b1(ph["X"], mask=ph["mask"], window=h)
        _same(got, want, f"h={h}")
        err[h] = BR.b1_error(got["b1"], ph)
    print(f"mean |b1 - truth|: h = 0 {err[0]:.4f}, h = 4 {err[4]:.4f}, ratio {err[4] / err[0]:.3f}")
    assert err[4] <= 0.8 * err[0]
