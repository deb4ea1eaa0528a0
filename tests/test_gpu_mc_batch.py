"""GPU: multi-coil slice stacks, each slice with its own coil maps, on the batched image-domain LSQR with every scalar on the device (mc_kernels.hip).

An EXTENSION with no reference counterpart (the reference is single-coil, README.md:63): the checker is the oracle's restatement, Operator.lsqr_mc /
oracle.pnp_admm_mc, called once per slice with that slice's maps."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _maps(N, M, nc, phase):
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                  for a in phase + np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def _noisy(y, rng, level=0.01):
    return y + level * np.abs(y).mean() * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))


def _xupdate_case(oracle, synth, N=32, T=24, s=6, S=120, nc=4):
    rng = np.random.default_rng(7)
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    fp, k = oracle.spiral_mask(N, S, T)
    op = oracle.Operator(N, N, dic["V"], fp, k)
    maps = np.stack([_maps(N, N, nc, 0.7 * b) for b in range(3)])
    ys, zs = [], []
    for b in range(3):
        X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=b), dic)
        ys.append(_noisy(op.forward_mc(X0, maps[b]), rng))
        zs.append(X0 + 0.05 * (rng.standard_normal(X0.shape) + 1j * rng.standard_normal(X0.shape)))
    ys, zs = np.stack(ys), np.stack(zs)
    ys[1] = 0.0                                                     # slice 1: y = 0, z = x0 = 0 -> stops at iteration 0
    zs[1] = 0.0
    return dic, fp, k, op, maps, ys, zs


def test_xupdate_batch_matches_oracle_per_slice(engine_mod, oracle, synth):
    """3 slices with different maps, 4 coils through chunks of max_batch = 2 that cross slices: per slice the LSQR count and flag equal the oracle's
    and x is within 1e-10; one slice stops at iteration 0, and with maxit = 3 the active slices reach maxit (flag 1) in the same batch."""
    dic, fp, k, op, maps, ys, zs = _xupdate_case(oracle, synth)
    N = 32
    e = engine_mod.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=2)
    for tol, maxit in ((1e-4, 100), (1e-12, 3)):
        xg, ig, fg = e.xupdate_mc_batch(maps, ys, zs, 0.05, tol=tol, maxit=maxit)
        for b in range(3):
            xo, io, fo = op.lsqr_mc(ys[b], maps[b], zs[b], 0.05, tol=tol, maxit=maxit)
            assert (ig[b], fg[b]) == (io, fo), (tol, maxit, b, ig[b], io, fg[b], fo)
            if b == 1:
                assert (io, fo) == (0, 0) and not np.any(xg[b])
            else:
                assert rel_err(xg[b], xo) < 1e-10, (tol, maxit, b, rel_err(xg[b], xo))
        if maxit == 3:
            assert list(fg) == [1, 0, 1]
    # warm start
    x0 = np.stack([op.adjoint_mc(ys[b], maps[b]) for b in range(3)])
    xg, ig, fg = e.xupdate_mc_batch(maps, ys, zs, 0.05, x0=x0)
    for b in (0, 2):
        xo, io, fo = op.lsqr_mc(ys[b], maps[b], zs[b], 0.05, x0=x0[b])
        assert (ig[b], fg[b]) == (io, fo) and rel_err(xg[b], xo) < 1e-10
    e.close()


def test_xupdate_batch_is_bit_identical_alone_in_any_batch_and_chunking(engine_mod, oracle, synth):
    """A slice solved alone, at each position of a batch of 3, and with max_batch 1, 2 and 8 gives the same bits and count; repeated calls too."""
    dic, fp, k, op, maps, ys, zs = _xupdate_case(oracle, synth)
    ys, zs = ys.copy(), zs.copy()
    ys[1] = ys[0][:, ::-1]                                         # three active slices
    zs[1] = zs[2]
    N = 32
    ref = None
    for maxb in (1, 2, 8):
        e = engine_mod.Engine(0)
        e.set_operator(N, N, dic["V"], fp, k, max_batch=maxb)
        xa, ia, _ = e.xupdate_mc_batch(maps[:1], ys[:1], zs[:1], 0.05)
        if ref is None:
            ref = (xa[0].copy(), int(ia[0]))
        assert np.array_equal(xa[0], ref[0]) and ia[0] == ref[1], maxb
        for pos in range(3):
            order = [1, 2]
            order.insert(pos, 0)
            xb, ib, _ = e.xupdate_mc_batch(maps[order], ys[order], zs[order], 0.05)
            assert np.array_equal(xb[pos], ref[0]) and ib[pos] == ref[1], (maxb, pos)
        x1, i1, f1 = e.xupdate_mc_batch(maps, ys, zs, 0.05)
        x2, i2, f2 = e.xupdate_mc_batch(maps, ys, zs, 0.05)
        assert np.array_equal(x1, x2) and np.array_equal(i1, i2) and np.array_equal(f1, f2)
        e.close()


def _admm_check(engine_mod, oracle, synth, N, M, T, s, nc, nslices, spls, epi):
    rng = np.random.default_rng(11)
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    fp, k = oracle.epi_mask(N, M, 1 / 8, T) if epi else oracle.spiral_mask(N, 120, T)
    op = oracle.Operator(N, M, dic["V"], fp, k)
    maps = np.stack([_maps(N, M, nc, 0.5 * b) for b in range(nslices)])
    ys = []
    for b in range(nslices):
        q = synth.make_phantom_qmaps(max(N, M), seed=b)[:N, :M]
        ys.append(_noisy(op.forward_mc(synth.synthesize_tsmi(q, dic), maps[b]), rng))
    ys = np.stack(ys)
    netc = (8, 16, 16, 32)
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=netc, nb=2, seed=3, eps=0.05)
    e = engine_mod.Engine(0)
    e.set_operator(N, M, dic["V"], fp, k, max_batch=max(spls))
    e.set_denoiser(w, N, M, in_nc=s, out_nc=s, nc=netc, nb=2, max_batch=max(spls))
    outs = []
    for spl in spls:
        xg, lg = e.pnp_admm_mc_batch(maps, ys, slices_per_launch=spl, iters=4)
        outs.append((xg, lg))
        for b in range(nslices):
            xo, lo = oracle.pnp_admm_mc(op, oracle.Net(w, in_nc=s, out_nc=s, nc=netc, nb=2), ys[b], maps[b], iters=4)
            assert np.array_equal(lg[b], lo) and rel_err(xg[b], xo) < 1e-4, (spl, b, lg[b], lo, rel_err(xg[b], xo))
    for xg, lg in outs[1:]:                                        # the LSQR is batch-invariant; the network may round per batch: counts equal
        assert np.array_equal(lg, outs[0][1])
    e.close()


def test_pnp_admm_batch_matches_oracle_per_slice(engine_mod, oracle, synth):
    """3 slices x 4 ADMM iterations, 4 coils, slices_per_launch 1 and 3: LSQR counts equal the oracle's per slice, x within 1e-4."""
    _admm_check(engine_mod, oracle, synth, 32, 32, 24, 6, 4, 3, (1, 3), epi=False)


def test_pnp_admm_batch_rectangular_epi(engine_mod, oracle, synth):
    """The same on a rectangular EPI grid: 64 x 96, 3 coils, 2 slices."""
    _admm_check(engine_mod, oracle, synth, 64, 96, 24, 6, 3, 2, (1, 2), epi=True)


def test_config4_cut0_stack_at_size(engine_mod, oracle, synth):
    """BASELINE configs[4] as a stack (extension, parity unpinned): cut0 (T = 1000), 224^2, 8 coils, 2 slices with different maps, max_batch = 4,
    2 ADMM iterations with the full-size network.  Per slice the counts equal the oracle's and x is within 1e-4; maps of the dictionary match at
    K = 98 304 are bit-exact against oracle.dict_match of the same X."""
    T, N, nc = 1000, 224, 8
    dic = synth.make_dictionary(T=T, n_t1=384, n_t2=256)
    fp, k = oracle.spiral_mask(N, 771, T)
    op = oracle.Operator(N, N, dic["V"], fp, k)
    maps = np.stack([_maps(N, N, nc, 0.4 * b) for b in range(2)])
    ys = []
    for b in range(2):
        X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=b), dic)
        ys.append(np.stack([synth.awgn_measured(col, 30.0, seed=10 * b + j) for j, col in enumerate(op.forward_mc(X0, maps[b]).T)], axis=1))
    ys = np.stack(ys)
    w = synth.structured_weights(seed=2, eps=0.3)
    e = engine_mod.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=4)
    e.set_denoiser(w, N, N, max_batch=2)
    e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
    xg, lg = e.pnp_admm_mc_batch(maps, ys, slices_per_launch=2, iters=2)
    for b in range(2):
        xo, lo = oracle.pnp_admm_mc(op, oracle.Net(w), ys[b], maps[b], iters=2)
        err = rel_err(xg[b], xo)
        print(f"cut0 x 8 coils, slice {b}: lsqr gpu {lg[b].tolist()} oracle {lo.tolist()}, rel_err {err:.2e}")
        assert np.array_equal(lg[b], lo) and err < 1e-4
        mg = e.dict_match(xg[b])
        mx = oracle.dict_match(xg[b], dic["D"], dic["normD"], dic["lut"])
        assert np.array_equal(mg["dm"], mx["dm"]) and np.array_equal(mg["qmap"], mx["qmap"]) and np.array_equal(mg["pd"], mx["pd"])
    e.close()


def test_refusals_and_set_coils_state_kept(engine_mod, oracle, synth):
    """Refused with an error code and message, no fault: ncoil < 1, NULL maps or y, slices_per_launch > max_batch, a denoiser that does not fit,
    no operator.  After the batched calls forward_mc still uses the maps of set_coils."""
    from qmri_pnp_recon_poc_amd._lib import AdmmParams
    dic, fp, k, op, maps, ys, zs = _xupdate_case(oracle, synth)
    N, s = 32, 6
    e = engine_mod.Engine(0)
    L, h = e.L, e.h
    p = AdmmParams(0.05, 2, 1e-4, 100, 0, 0, 0.01, 0)
    x = np.zeros(3 * N * N * s, np.complex128)
    mb = np.ascontiguousarray(maps.ravel())
    yb = np.ascontiguousarray(ys.ravel())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.qmri_xupdate_mc_batch(h, 3, 4, vp(mb), vp(yb), vp(x), 0.05, 1e-4, 10, None, vp(x), None, None) == -2   # no operator: QMRI_ERR_STATE
    assert b"operator" in L.qmri_last_error(h)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=2)
    assert L.qmri_xupdate_mc_batch(h, 3, 0, vp(mb), vp(yb), vp(x), 0.05, 1e-4, 10, None, vp(x), None, None) == -1
    assert b"ncoil" in L.qmri_last_error(h)
    assert L.qmri_xupdate_mc_batch(h, 3, 4, None, vp(yb), vp(x), 0.05, 1e-4, 10, None, vp(x), None, None) == -1
    assert L.qmri_xupdate_mc_batch(h, 3, 4, vp(mb), None, vp(x), 0.05, 1e-4, 10, None, vp(x), None, None) == -1
    assert L.qmri_pnp_admm_mc_batch(h, 3, 3, 4, vp(mb), vp(yb), C.byref(p), None, vp(x), None) == -2                # no denoiser yet
    netc = (8, 16, 16, 32)
    e.set_denoiser(synth.structured_weights(in_nc=s, out_nc=s, nc=netc, nb=2, seed=3, eps=0.05), N, N, in_nc=s, out_nc=s, nc=netc, nb=2, max_batch=2)
    assert L.qmri_pnp_admm_mc_batch(h, 3, 3, 4, vp(mb), vp(yb), C.byref(p), None, vp(x), None) == -1                # 3 > max_batch 2
    assert b"max_batch" in L.qmri_last_error(h)
    e.set_denoiser(synth.structured_weights(in_nc=4, out_nc=4, nc=netc, nb=2, seed=3, eps=0.05), N, N, in_nc=4, out_nc=4, nc=netc, nb=2, max_batch=2)
    assert L.qmri_pnp_admm_mc_batch(h, 3, 1, 4, vp(mb), vp(yb), C.byref(p), None, vp(x), None) == -1                # 4 channels, s = 6
    assert b"does not fit" in L.qmri_last_error(h)
    single = _maps(N, N, 2, 2.0)
    e.set_coils(single)
    xt = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=5), dic)
    before = e.forward_mc(xt)
    e.xupdate_mc_batch(maps, ys, zs, 0.05, maxit=5)
    after = e.forward_mc(xt)
    assert np.array_equal(before, after) and rel_err(after, op.forward_mc(xt, single)) < 1e-12
    e.close()


def _stack_case(oracle, synth, nslices=5, nc=3, N=32, T=24, s=6):
    rng = np.random.default_rng(23)
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    fp, k = oracle.spiral_mask(N, 120, T)
    op = oracle.Operator(N, N, dic["V"], fp, k)
    maps = np.stack([_maps(N, N, nc, 0.3 * b) for b in range(nslices)])
    ys = np.stack([_noisy(op.forward_mc(synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=b), dic), maps[b]), rng) for b in range(nslices)])
    netc = (8, 16, 16, 32)
    w = synth.structured_weights(in_nc=s, out_nc=s, nc=netc, nb=2, seed=3, eps=0.05)
    return dic, fp, k, op, maps, ys, netc, w


def test_recon_batch_mc_two_workers_equal_one(engine_mod, oracle, synth):
    """qmri_recon_batch_mc (batch.recon_batch with coil_maps) on 5 slices, workers [0, 0] and [0]: X and the dictionary-match maps are bit-identical
    between the two runs, every slot holds its own slice (equal to the same slice reconstructed alone), and one slice matches the oracle."""
    from qmri_pnp_recon_poc_amd import batch
    dic, fp, k, op, maps, ys, netc, w = _stack_case(oracle, synth)
    s = 6
    kw = dict(N=32, M=32, V=dic["V"], frame_ptr=fp, kidx=k, weights=w, in_nc=s, out_nc=s, nc=netc, nb=2, dictionary=dic, iters=3,
              slices_per_launch=2, coil_maps=maps)
    r2 = batch.recon_batch([0, 0], ys, **kw)
    r1 = batch.recon_batch([0], ys, **kw)
    for key in ("X", "qmap", "pd"):
        assert np.array_equal(r1[key], r2[key]), key
    for b in (0, 4):
        kw1 = dict(kw, coil_maps=maps[b:b + 1], slices_per_launch=1)
        alone = batch.recon_batch([0], ys[b:b + 1], **kw1)
        assert rel_err(alone["X"][0], r1["X"][b]) < 1e-6, b                 # its own slice (the network may round per batch size)
    xo, _ = oracle.pnp_admm_mc(op, oracle.Net(w, in_nc=s, out_nc=s, nc=netc, nb=2), ys[2], maps[2], iters=3)
    assert rel_err(r1["X"][2], xo) < 1e-4
    mx = oracle.dict_match(r1["X"][2], dic["D"], dic["normD"], dic["lut"])
    assert np.array_equal(r1["qmap"][2], mx["qmap"]) and np.array_equal(r1["pd"][2], mx["pd"])
    with pytest.raises(ValueError):
        batch.recon_batch([0], ys, **dict(kw, coil_maps=maps[:4]))              # 4 sets of maps for 5 slices


def test_pnp_admm_mc_dev_equals_host_arrays_and_refuses(engine_mod, oracle, synth):
    """qmri_pnp_admm_mc_dev on device arrays gives the host-array call's bits; it refuses x_out aliasing x0 and more slices than max_batch."""
    from qmri_pnp_recon_poc_amd._lib import AdmmParams
    from qmri_pnp_recon_poc_amd.engine import _cbuf
    dic, fp, k, op, maps, ys, netc, w = _stack_case(oracle, synth, nslices=3)
    N, s, nc = 32, 6, 3
    e = engine_mod.Engine(0)
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = C.CDLL(path)                                              # device buffers from the HIP runtime libqmri itself uses
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    e.set_operator(N, N, dic["V"], fp, k, max_batch=2)
    e.set_denoiser(w, N, N, in_nc=s, out_nc=s, nc=netc, nb=2, max_batch=2)
    xh, lh = e.pnp_admm_mc_batch(maps[:2], ys[:2], slices_per_launch=2, iters=3)
    hm = np.concatenate([_cbuf(maps[b]) for b in range(3)])
    hy = np.concatenate([_cbuf(ys[b]) for b in range(3)])
    n = N * N * s
    dm, dy, dx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dm), hm.nbytes) == 0 and hip.hipMalloc(C.byref(dy), hy.nbytes) == 0 and hip.hipMalloc(C.byref(dx), 3 * n * 16) == 0
    assert hip.hipMemcpy(dm, hm.ctypes.data_as(C.c_void_p), hm.nbytes, 1) == 0 and hip.hipMemcpy(dy, hy.ctypes.data_as(C.c_void_p), hy.nbytes, 1) == 0
    li = np.zeros((2, 3), np.int32)
    p = AdmmParams(0.05, 3, 1e-4, 100, 0, 0, 0.01, 0)
    e._check(e.L.qmri_pnp_admm_mc_dev(e.h, 2, nc, dm, dy, C.byref(p), None, dx, li.ctypes.data_as(C.POINTER(C.c_int32))))
    xd = np.empty(2 * n, np.complex128)
    assert hip.hipMemcpy(xd.ctypes.data_as(C.c_void_p), dx, xd.nbytes, 2) == 0
    for b in range(2):
        assert np.array_equal(xd[b * n:(b + 1) * n].reshape((N, N, s), order="F"), xh[b]) and np.array_equal(li[b], lh[b])
    assert e.L.qmri_pnp_admm_mc_dev(e.h, 2, nc, dm, dy, C.byref(p), dx, dx, None) == -1          # x_out aliases x0
    assert b"alias" in e.L.qmri_last_error(e.h)
    assert e.L.qmri_pnp_admm_mc_dev(e.h, 3, nc, dm, dy, C.byref(p), None, dx, None) == -1        # 3 > max_batch 2
    assert b"max_batch" in e.L.qmri_last_error(e.h)
    e.close()
    hip.hipFree(dm); hip.hipFree(dy); hip.hipFree(dx)


def test_recon_batch_mc_through_the_gateway(engine_mod, oracle, synth):
    """qmri_recon_batch.m with param.coils issues qmri_mex('recon_batch_mc', Y (m x ncoil x S), maps (N x M x ncoil x S), ...): under the mock MEX
    runtime its result equals batch.recon_batch(coil_maps=...) bit for bit, and wrong sizes are MATLAB errors with identifiers."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mexmock
    from mexmock import MexError
    from qmri_pnp_recon_poc_amd import batch
    dic, fp, k, op, maps, ys, netc, w = _stack_case(oracle, synth, nslices=3)
    N, s, nc = 32, 6, 3
    q = mexmock.qmri_mex
    q("set_operator", float(N), float(N), np.asarray(dic["V"], np.float64), fp.astype(np.int32), k.astype(np.int32))
    q("set_denoiser", w.astype(np.float32), float(s), float(s), np.array([netc], np.float64), 2.0, 0.0, float(N), float(N))
    q("set_dictionary", np.asarray(dic["D"], np.float32), np.asarray(dic["normD"], np.float32), np.asarray(dic["lut"], np.float32))
    prm = {"gamma": 0.05, "iter": 2, "cg_tol": 1e-4, "multi_level": 0, "noise_std": 0.01}
    Ym = np.ascontiguousarray(ys.transpose(1, 2, 0))                       # m x ncoil x S
    Mm = np.ascontiguousarray(maps.transpose(1, 2, 3, 0))                  # N x M x ncoil x S
    dims = np.array([N, N, s], np.float64)
    X, qmap, pd = q("recon_batch_mc", Ym, Mm, prm, np.array([0.0, 0.0]), 2.0, dims, nargout=3)
    res = batch.recon_batch([0, 0], ys, N=N, M=N, V=dic["V"], frame_ptr=fp, kidx=k, weights=w, in_nc=s, out_nc=s, nc=netc, nb=2, dictionary=dic,
                            iters=2, slices_per_launch=2, coil_maps=maps)
    assert np.array_equal(np.moveaxis(X, 3, 0), res["X"])
    assert np.array_equal(np.moveaxis(qmap, 3, 0), res["qmap"]) and np.array_equal(np.moveaxis(pd, 2, 0), res["pd"])
    cases = [
        ("qmri:recon_batch_mc:size", lambda: q("recon_batch_mc", Ym[:-1], Mm, prm, np.array([0.0]), 1.0, dims, nargout=1)),
        ("qmri:recon_batch_mc:maps", lambda: q("recon_batch_mc", Ym, Mm[:, :, :2], prm, np.array([0.0]), 1.0, dims, nargout=1)),
        ("qmri:recon_batch_mc:maps", lambda: q("recon_batch_mc", Ym, np.real(Mm).copy(), prm, np.array([0.0]), 1.0, dims, nargout=1)),
    ]
    for want_id, call in cases:
        with pytest.raises(MexError) as ei:
            call()
        assert ei.value.id == want_id, (want_id, ei.value.id)
    mexmock.mex_exit()
