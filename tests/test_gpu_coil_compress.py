"""GPU: coil compression of multi-coil stacks (cc_kernels.hip, api_cc.cpp) -- an EXTENSION with no reference counterpart.  The checker is the
numpy restatement of the definition (tests/coil_cc_ref.py); the exact identities of the SENSE model (a unitary or lossless map leaves the
reconstruction unchanged) pin the composition with the multi-coil LSQR and PnP-ADMM."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coil_cc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _maps(N, M, nc, phase):
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                  for a in phase + np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def _noisy(y, rng, level=0.01):
    return y + level * np.abs(y).mean() * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))


def _stack(oracle, synth, N, M, nc, S, epi=False, T=24, s=6, seed=0, noise=0.01, maps=None):
    rng = np.random.default_rng(seed)
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    fp, k = oracle.epi_mask(N, M, 1 / 8, T) if epi else oracle.spiral_mask(N, 120 if N <= 32 else 240, T)
    op = oracle.Operator(N, M, dic["V"], fp, k)
    if maps is None:
        maps = np.stack([_maps(N, M, nc, 0.4 * b + 0.1 * seed) for b in range(S)])
    X0 = [synth.synthesize_tsmi(synth.make_phantom_qmaps(max(N, M), seed=b)[:N, :M], dic) for b in range(S)]
    ys = np.stack([op.forward_mc(X0[b], maps[b]) for b in range(S)])
    if noise:
        ys = np.stack([_noisy(ys[b], rng, noise) for b in range(S)])
    return dic, fp, k, op, maps, ys, X0


def _random_psi(nc, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nc, nc)) + 1j * rng.standard_normal((nc, nc))
    return A @ A.conj().T / nc + 0.5 * np.eye(nc)


def _check_parity(got, want, what):
    assert got["nv"] == want["nv"], (what, got["nv"], want["nv"])
    lam = want["eig"]
    assert np.max(np.abs(got["eig"] - lam)) <= 1e-10 * np.max(np.abs(lam)), what
    for key in ("W", "y", "maps"):
        if want[key] is None:
            assert got[key] is None
            continue
        for b in range(want[key].shape[0]):
            e = rel_err(got[key][b], want[key][b])
            assert e < 1e-10, (what, key, b, e)


@pytest.mark.parametrize("N,M,nc,epi,nv,psi,energy,shared", [
    (64, 64, 8, False, 3, False, None, False),              # (nv at a clear gap: evenly spaced coils give eigenvalue pairs)
    (64, 64, 16, False, 5, False, None, False),
    (64, 64, 32, False, 7, False, None, False),
    (64, 96, 8, True, 3, False, None, False),              # rectangular EPI grid
    (64, 64, 8, False, 4, True, None, False),              # whitening with a random Psi
    (64, 64, 16, False, 0, False, 0.95, False),            # nv chosen by energy
    (64, 64, 8, False, 4, False, None, True),              # shared: one W for the stack
    (64, 64, 12, False, 0, True, 0.9, True),               # all three together
])
def test_parity_with_the_restatement(engine_mod, oracle, synth, N, M, nc, epi, nv, psi, energy, shared):
    """W, y', maps' and lambda against tests/coil_cc_ref.py to 1e-10 (3 slices, each with its own maps)."""
    dic, fp, k, op, maps, ys, _ = _stack(oracle, synth, N, M, nc, 3, epi=epi, seed=nc)
    P = _random_psi(nc, 3) if psi else None
    kw = dict(noise_cov=P, nv=nv, energy=energy if energy else 0.99, shared=shared)
    e = engine_mod.Engine(0)
    e.set_operator(N, M, dic["V"], fp, k)
    got = e.coil_compress(ys, maps, **kw)
    want = ref.coil_compress(ys, maps, **kw)
    print(f"{N}x{M} {nc} coils -> nv {got['nv']}, psi {psi}, shared {shared}")
    _check_parity(got, want, (N, M, nc, nv, psi, shared))
    if energy:
        assert 1 <= got["nv"] < nc
    no_maps = e.coil_compress(ys, None, **kw)                # maps are optional and change nothing else
    assert no_maps["maps"] is None and np.array_equal(no_maps["y"], got["y"]) and np.array_equal(no_maps["W"], got["W"])
    e.close()


def test_batch_invariance_bits(engine_mod, oracle, synth):
    """A slice compressed alone, at each position of a 3-slice stack, and with max_batch 1, 2 and 8: the same bits of y', maps', W, lambda."""
    N, nc = 64, 16
    dic, fp, k, op, maps, ys, _ = _stack(oracle, synth, N, N, nc, 3, seed=4)
    P = _random_psi(nc, 8)
    for kw in (dict(nv=5), dict(nv=5, noise_cov=P)):
        refb = None
        for maxb in (1, 2, 8):
            e = engine_mod.Engine(0)
            e.set_operator(N, N, dic["V"], fp, k, max_batch=maxb)
            a = e.coil_compress(ys[:1], maps[:1], **kw)
            if refb is None:
                refb = a
            for key in ("y", "maps", "W", "eig"):
                assert np.array_equal(a[key][0], refb[key][0]), (maxb, key)
            for pos in range(3):
                order = [1, 2]
                order.insert(pos, 0)
                b = e.coil_compress(ys[order], maps[order], **kw)
                for key in ("y", "maps", "W", "eig"):
                    assert np.array_equal(b[key][pos], refb[key][0]), (maxb, pos, key)
            e.close()


def test_unitary_compression_leaves_the_reconstruction_unchanged(engine_mod, oracle, synth):
    """nv = ncoil, no Psi: W is unitary, so xupdate_mc_batch on the compressed stack matches the uncompressed call to 1e-9 with equal LSQR counts and
    flags, and pnp_admm_mc_batch over 5 iterations to 1e-8."""
    N, nc, s = 32, 6, 6
    dic, fp, k, op, maps, ys, X0 = _stack(oracle, synth, N, N, nc, 2, seed=6)
    netc = (8, 16, 16, 32)
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=netc, nb=2, seed=3, eps=0.05)
    e = engine_mod.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=2)
    e.set_denoiser(w, N, N, in_nc=s, out_nc=s, nc=netc, nb=2, max_batch=2)
    cc = e.coil_compress(ys, maps, nv=nc)
    assert cc["nv"] == nc and np.max(np.abs(cc["W"][0].conj().T @ cc["W"][0] - np.eye(nc))) < 1e-13
    rng = np.random.default_rng(2)
    zs = np.stack([x + 0.05 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) for x in X0])
    xu, iu, fu = e.xupdate_mc_batch(maps, ys, zs, 0.05)
    xc, ic, fcc = e.xupdate_mc_batch(cc["maps"], cc["y"], zs, 0.05)
    err = max(rel_err(xc[b], xu[b]) for b in range(2))
    print(f"unitary: xupdate rel err {err:.2e}, iters {iu.tolist()} / {ic.tolist()}")
    assert np.array_equal(iu, ic) and np.array_equal(fu, fcc) and err < 1e-9
    Xu, lu = e.pnp_admm_mc_batch(maps, ys, slices_per_launch=2, iters=5)
    Xc, lc = e.pnp_admm_mc_batch(cc["maps"], cc["y"], slices_per_launch=2, iters=5)
    err = max(rel_err(Xc[b], Xu[b]) for b in range(2))
    print(f"unitary: 5 ADMM iterations rel err {err:.2e}")
    assert np.array_equal(lu, lc) and err < 1e-8
    e.close()


def test_lossless_low_rank_compression(engine_mod, oracle, synth):
    """16 maps that are 4 base maps mixed by a random 16 x 4 matrix, no noise: every sample's coil vector lies in a 4-dimensional space, so 16 -> 4
    virtual coils loses nothing -- the x-update and 3 ADMM iterations on the compressed stack reproduce the 16-coil ones to 1e-8."""
    N, nc, nv, s = 32, 16, 4, 6
    rng = np.random.default_rng(12)
    base = np.stack([_maps(N, N, nv, 0.3 * b) for b in range(2)])
    mix = rng.standard_normal((2, nc, nv)) + 1j * rng.standard_normal((2, nc, nv))
    maps = np.einsum("bhwk,bjk->bhwj", base, mix)
    dic, fp, k, op, maps, ys, X0 = _stack(oracle, synth, N, N, nc, 2, seed=12, noise=0.0, maps=maps)
    netc = (8, 16, 16, 32)
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=netc, nb=2, seed=3, eps=0.05)
    e = engine_mod.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=2)
    e.set_denoiser(w, N, N, in_nc=s, out_nc=s, nc=netc, nb=2, max_batch=2)
    cc = e.coil_compress(ys, maps, nv=nv)
    assert np.all(cc["eig"][:, nv:] < 1e-12 * cc["eig"][:, :1])
    zs = np.stack([0.9 * x for x in X0])
    # (r = 1: a well-conditioned x-update; at r = 0.05 without noise both solves run ~100 iterations and their rounding drifts to ~2e-7 apart)
    xu, iu, _ = e.xupdate_mc_batch(maps, ys, zs, 1.0)
    xc, ic, _ = e.xupdate_mc_batch(cc["maps"], cc["y"], zs, 1.0)
    err = max(rel_err(xc[b], xu[b]) for b in range(2))
    Xu, lu = e.pnp_admm_mc_batch(maps, ys, slices_per_launch=2, iters=3)
    Xc, lc = e.pnp_admm_mc_batch(cc["maps"], cc["y"], slices_per_launch=2, iters=3)
    err2 = max(rel_err(Xc[b], Xu[b]) for b in range(2))
    print(f"lossless 16 -> 4: xupdate rel err {err:.2e} iters {iu.tolist()} / {ic.tolist()}; 3 ADMM iterations {err2:.2e}")
    assert err < 1e-8 and err2 < 1e-8
    e.close()


def test_realistic_compression_keeps_the_dictionary_match(engine_mod, oracle, synth):
    """16 smooth coils, 1 % noise, compressed to 6 virtual coils: the dictionary match of the compressed reconstruction (5 ADMM iterations) picks
    the atom of the uncompressed one on >= 95 % of the object's pixels (measured with oracle.pnp_admm_mc on both stacks: 99.1 %, 98.6 %, 98.9 % of
    552-580 object pixels for these three phantoms)."""
    N, nc, nv, s = 32, 16, 6, 6
    netc = (8, 16, 16, 32)
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=netc, nb=2, seed=3, eps=0.05)
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)
        dic = synth.make_dictionary(T=24, n_t1=24, n_t2=16, s=s)
        fp, k = oracle.spiral_mask(N, 120, 24)
        op = oracle.Operator(N, N, dic["V"], fp, k)
        X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=seed), dic)
        maps = _maps(N, N, nc, 0.3 * seed)
        y = _noisy(op.forward_mc(X0, maps), rng)
        e = engine_mod.Engine(0)
        e.set_operator(N, N, dic["V"], fp, k)
        e.set_denoiser(w, N, N, in_nc=s, out_nc=s, nc=netc, nb=2)
        e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
        cc = e.coil_compress(y[None], maps[None], nv=nv)
        Xu, _ = e.pnp_admm_mc_batch(maps[None], y[None], iters=5)
        Xc, _ = e.pnp_admm_mc_batch(cc["maps"], cc["y"], iters=5)
        mu, mc = e.dict_match(Xu[0]), e.dict_match(Xc[0])
        obj = np.abs(X0[..., 0]).ravel(order="F") > 0.1 * np.abs(X0[..., 0]).max()
        frac = float(np.mean(np.asarray(mu["dm"]).ravel()[obj] == np.asarray(mc["dm"]).ravel()[obj]))
        print(f"phantom {seed}: same atom on {frac:.4f} of {obj.sum()} object pixels, energy kept {cc['eig'][0][:nv].sum() / cc['eig'][0].sum():.5f}")
        assert frac >= THRESHOLD, (seed, frac)
        e.close()


THRESHOLD = 0.95


def _problem(oracle, synth, nslices, nc, seed):
    dic, fp, k, op, maps, ys, _ = _stack(oracle, synth, 32, 32, nc, nslices, seed=seed)
    netc = (8, 16, 16, 32)
    w = synth.structured_weights(in_nc=6, out_nc=6, nc=netc, nb=2, seed=3, eps=0.05)
    kw = dict(N=32, M=32, V=dic["V"], frame_ptr=fp, kidx=k, weights=w, in_nc=6, out_nc=6, nc=netc, nb=2, dictionary=dic, iters=3, slices_per_launch=2)
    return dic, fp, k, maps, ys, kw


def test_recon_batch_mc_cc_equals_compress_then_recon(engine_mod, oracle, synth):
    """qmri_recon_batch_mc_cc (batch.recon_batch with coil_compress) equals Engine.coil_compress followed by qmri_recon_batch_mc on its outputs, bit
    for bit (X, qmap, pd), with and without Psi; workers [0, 0] equal workers [0]."""
    from qmri_pnp_recon_poc_amd import batch
    nc, nv = 8, 3
    dic, fp, k, maps, ys, kw = _problem(oracle, synth, 5, nc, 21)
    P = _random_psi(nc, 5)
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, dic["V"], fp, k)
    for psi in (None, P):
        cc = e.coil_compress(ys, maps, noise_cov=psi, nv=nv)
        two = batch.recon_batch([0, 0], ys, coil_maps=maps, coil_compress=nv, noise_cov=psi, **kw)
        one = batch.recon_batch([0], ys, coil_maps=maps, coil_compress={"nv": nv}, noise_cov=psi, **kw)
        via = batch.recon_batch([0], cc["y"], coil_maps=cc["maps"], **kw)
        for key in ("X", "qmap", "pd"):
            assert np.array_equal(one[key], via[key]) and np.array_equal(two[key], one[key]), (psi is not None, key)
    e.close()


def test_coil_compress_dev_equals_host_arrays(engine_mod, oracle, synth):
    """qmri_coil_compress_dev on device arrays gives the host-array call's bits."""
    from qmri_pnp_recon_poc_amd._lib import CcParams
    from qmri_pnp_recon_poc_amd.engine import _cbuf
    N, nc, nv, S = 32, 8, 3, 2
    dic, fp, k, op, maps, ys, _ = _stack(oracle, synth, N, N, nc, S, seed=31)
    P = _random_psi(nc, 1)
    e = engine_mod.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k)
    host = e.coil_compress(ys, maps, noise_cov=P, nv=nv)
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hy = np.concatenate([_cbuf(ys[b]) for b in range(S)])
    hm = np.concatenate([_cbuf(maps[b]) for b in range(S)])
    hp = _cbuf(P)
    bufs = {}
    for name, nbytes in (("y", hy.nbytes), ("m", hm.nbytes), ("p", hp.nbytes), ("yo", hy.nbytes), ("mo", hm.nbytes), ("w", S * nc * nc * 16)):
        bufs[name] = C.c_void_p()
        assert hip.hipMalloc(C.byref(bufs[name]), nbytes) == 0
    for name, a in (("y", hy), ("m", hm), ("p", hp)):
        assert hip.hipMemcpy(bufs[name], a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
    p = CcParams(nv, 0.99, 0)
    got = C.c_int(0)
    eig = np.empty(S * nc)
    e._check(e.L.qmri_coil_compress_dev(e.h, S, nc, bufs["y"], bufs["m"], bufs["p"], C.byref(p), C.byref(got), bufs["yo"], bufs["mo"], bufs["w"],
                                        eig.ctypes.data_as(C.POINTER(C.c_double))))
    assert got.value == nv
    yo = np.empty(S * nv * e.m, np.complex128)
    mo = np.empty(S * nv * N * N, np.complex128)
    wo = np.empty(S * nc * nv, np.complex128)
    for a, name in ((yo, "yo"), (mo, "mo"), (wo, "w")):
        assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), bufs[name], a.nbytes, 2) == 0
    assert np.array_equal(eig.reshape(S, nc), host["eig"])
    for b in range(S):
        assert np.array_equal(yo[b * nv * e.m:(b + 1) * nv * e.m].reshape((e.m, nv), order="F"), host["y"][b])
        assert np.array_equal(mo[b * nv * N * N:(b + 1) * nv * N * N].reshape((N, N, nv), order="F"), host["maps"][b])
        assert np.array_equal(wo[b * nc * nv:(b + 1) * nc * nv].reshape((nc, nv), order="F"), host["W"][b])
    e.close()
    for v in bufs.values():
        hip.hipFree(v)


def test_mex_coil_compress_and_recon_option_equal_python(engine_mod, oracle, synth):
    """Under the mock MEX runtime: qmri_mex('coil_compress', ...) equals Engine.coil_compress, and recon_batch_mc with the cc / noise_cov arguments
    equals batch.recon_batch(coil_compress=...), bit for bit; wrong arguments are MATLAB errors with identifiers."""
    import mexmock
    from mexmock import MexError
    from qmri_pnp_recon_poc_amd import batch
    nc, nv = 6, 3
    dic, fp, k, maps, ys, kw = _problem(oracle, synth, 3, nc, 41)
    P = _random_psi(nc, 7)
    N, s = 32, 6
    q = mexmock.qmri_mex
    q("set_operator", float(N), float(N), np.asarray(dic["V"], np.float64), fp.astype(np.int32), k.astype(np.int32))
    q("set_denoiser", kw["weights"].astype(np.float32), float(s), float(s), np.array([kw["nc"]], np.float64), 2.0, 0.0, float(N), float(N))
    q("set_dictionary", np.asarray(dic["D"], np.float32), np.asarray(dic["normD"], np.float32), np.asarray(dic["lut"], np.float32))
    Ym = np.ascontiguousarray(ys.transpose(1, 2, 0))
    Mm = np.ascontiguousarray(maps.transpose(1, 2, 3, 0))
    yc, mc, W, eig = q("coil_compress", Ym, Mm, P.astype(np.complex128), {"nv": float(nv)}, nargout=4)
    e = engine_mod.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k)
    py = e.coil_compress(ys, maps, noise_cov=P, nv=nv)
    e.close()
    assert np.array_equal(np.moveaxis(yc, 2, 0), py["y"]) and np.array_equal(np.moveaxis(mc, 3, 0), py["maps"])
    assert np.array_equal(np.moveaxis(W, 2, 0), py["W"]) and np.array_equal(eig.T, py["eig"])
    _, _, _, eig_e = q("coil_compress", Ym, np.zeros((0, 0)), np.zeros((0, 0)), {"nv": 0.0, "energy": 0.9, "shared": 1.0}, nargout=4)
    assert eig_e.shape == (nc, 1)
    prm = {"gamma": 0.05, "iter": 3, "cg_tol": 1e-4, "multi_level": 0, "noise_std": 0.01}
    dims = np.array([N, N, s], np.float64)
    X, qmap, pd = q("recon_batch_mc", Ym, Mm, prm, np.array([0.0]), 2.0, dims, float(nv), P.astype(np.complex128), nargout=3)
    res = batch.recon_batch([0], ys, coil_maps=maps, coil_compress=nv, noise_cov=P, **kw)
    assert np.array_equal(np.moveaxis(X, 3, 0), res["X"])
    assert np.array_equal(np.moveaxis(qmap, 3, 0), res["qmap"]) and np.array_equal(np.moveaxis(pd, 2, 0), res["pd"])
    cases = [
        ("qmri:coil_compress:size", lambda: q("coil_compress", Ym[:-1], Mm, np.zeros((0, 0)), 2.0, nargout=1)),
        ("qmri:coil_compress:maps", lambda: q("coil_compress", Ym, Mm[:, :, :2], np.zeros((0, 0)), 2.0, nargout=1)),
        ("qmri:coil_compress:noise_cov", lambda: q("coil_compress", Ym, Mm, np.eye(nc + 1, dtype=np.complex128), 2.0, nargout=1)),
        ("qmri:coil_compress:cc", lambda: q("coil_compress", Ym, Mm, np.zeros((0, 0)), 2.5, nargout=1)),
        ("qmri:err1", lambda: q("coil_compress", Ym, Mm, np.zeros((0, 0)), float(nc + 1), nargout=1)),
        ("qmri:err1", lambda: q("recon_batch_mc", Ym, Mm, prm, np.array([0.0]), 1.0, dims, {"nv": 0.0, "energy": 0.9}, nargout=1)),
    ]
    for want_id, call in cases:
        with pytest.raises(MexError) as ei:
            call()
        assert ei.value.id == want_id, (want_id, ei.value.id)
    mexmock.mex_exit()


def test_refusals(engine_mod, oracle, synth):
    """Every refusal returns its code and message, no fault: no operator, nv > ncoil, nv < 0, energy outside (0, 1], Psi not positive definite,
    ncoil > 128, maps_out without maps; energy and shared to qmri_recon_batch_mc_cc (through batch.recon_batch)."""
    from qmri_pnp_recon_poc_amd import batch
    from qmri_pnp_recon_poc_amd._lib import CcParams
    N, nc = 32, 4
    dic, fp, k, op, maps, ys, _ = _stack(oracle, synth, N, N, nc, 1, seed=51)
    e = engine_mod.Engine(0)
    L, h = e.L, e.h
    big = np.zeros(200 * 200 * 64, np.complex128)
    vp = big.ctypes.data_as(C.c_void_p)
    nv = C.c_int(0)

    def call(ncoil, p, maps_in=None, maps_out=None, psi=None):
        return L.qmri_coil_compress(h, 1, ncoil, vp, maps_in, psi, C.byref(p), C.byref(nv), big[1:].ctypes.data_as(C.c_void_p), maps_out, None, None)

    assert call(nc, CcParams(2, 0.99, 0)) == -2 and b"operator" in L.qmri_last_error(h)
    e.set_operator(N, N, dic["V"], fp, k)
    for p, code, word in ((CcParams(5, 0.99, 0), -1, b"nv"), (CcParams(-1, 0.99, 0), -1, b"nv"), (CcParams(0, 0.0, 0), -1, b"energy"),
                          (CcParams(0, 1.5, 0), -1, b"energy"), (CcParams(2, 0.99, 2), -1, b"shared")):
        assert call(nc, p) == code and word in L.qmri_last_error(h), p
    assert call(129, CcParams(2, 0.99, 0)) == -4 and b"128" in L.qmri_last_error(h)
    assert call(nc, CcParams(2, 0.99, 0), maps_out=vp) == -1 and b"maps_out" in L.qmri_last_error(h)
    with pytest.raises(engine_mod.QmriError) as ei:
        e.coil_compress(ys, maps, noise_cov=np.diag([1.0, 1.0, -1.0, 1.0]).astype(np.complex128), nv=2)
    assert ei.value.code == -1 and "positive definite" in str(ei.value)
    ok = e.coil_compress(ys, maps, nv=2)                                   # the context still works
    assert ok["nv"] == 2
    e.close()
    _, _, _, maps5, ys5, kw = _problem(oracle, synth, 2, nc, 52)
    for cc, word in (({"nv": 0, "energy": 0.9}, "qmri_coil_compress"), ({"nv": 2, "shared": True}, "shared"), ({"nv": 5}, "nv")):
        with pytest.raises(engine_mod.QmriError) as ei:
            batch.recon_batch([0], ys5, coil_maps=maps5, coil_compress=cc, **kw)
        assert ei.value.code == -1 and word in str(ei.value) and "qmri_recon_batch_mc_cc" in str(ei.value), cc
