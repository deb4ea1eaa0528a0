"""GPU: coil sensitivity maps from calibration data (csm_kernels.hip, api_csm.cpp) -- an EXTENSION with no reference counterpart.  The checker is
the numpy restatement of the definition (tests/coil_maps_ref.py, eigenpairs by numpy.linalg.eigh) on the fixture of tests/test_coil_maps_host.py,
whose conditions (kept set, lambda_2 / lambda_1 <= 0.1) that file asserts on the CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coil_cc_ref as ccref  # noqa: E402
import coil_maps_ref as R  # noqa: E402
import test_coil_maps_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
THRESH = H.THRESH
_REF = {}


def _operator(oracle, N, M, T=8, s=2, seed=0):
    """A small operator on the N x M grid (the estimate needs its FFT passes and its grid only)."""
    V = np.linalg.qr(np.random.default_rng(seed).standard_normal((T, s)))[0]
    fp, k = oracle.spiral_mask(N, 120, T) if N == M else oracle.epi_mask(N, M, 1 / 8, T)
    return V, fp, k


def _engine(engine_mod, oracle, N, M, max_batch=None):
    V, fp, k = _operator(oracle, N, M)
    e = engine_mod.Engine(0)
    if max_batch is None:
        e.set_operator(N, M, V, fp, k)
    else:
        e.set_operator(N, M, V, fp, k, max_batch=max_batch)
    return e


def _hip():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _ref(f, **kw):
    """The restatement on a fixture, computed once per (fixture, options)."""
    key = (id(f["block"]), tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = R.coil_maps_ref(f["block"], f["N"], f["M"], full=True, **kw)
    return _REF[key]


def _compare(got, want, thresh, what):
    """maps and img to 1e-9, lambda_1 to 1e-10 on the kept pixels; the kept sets equal except where the reference's lambda_1 lies within 1e-9
    (relative) of the threshold; nothing left unconverged."""
    maps, img, lam, info = got
    Cw, iw, l1, _, kept, _, _ = want
    cut = thresh * thresh * l1.max()
    near = np.abs(l1 - cut) <= 1e-9 * cut if thresh > 0 else np.zeros_like(kept)
    gk = np.sqrt(np.sum(np.abs(maps) ** 2, axis=2)) > 0
    assert np.array_equal(gk[~near], kept[~near]), what
    sel = kept & gk
    em, ei, el = rel_err(maps[sel], Cw[sel]), rel_err(img[sel], iw[sel]), np.max(np.abs(lam - l1)) / l1.max()
    print(f"{what}: maps {em:.2e} img {ei:.2e} lambda1 {el:.2e} iterations <= {info['max_iters']}, not converged {info['not_converged']}")
    assert em <= 1e-9 and ei <= 1e-9 and el <= 1e-10, what
    assert np.all(maps[~gk] == 0) and np.all(img[~gk] == 0)
    assert info["not_converged"] == 0 and 1 <= info["max_iters"] < 256, what


@pytest.mark.parametrize("kind,phase_ref,window,patch", [
    ("kspace", "object", True, 3), ("kspace", "coil", True, 3), ("kspace", "object", False, 3), ("kspace", "coil", False, 1),
    ("kspace", "object", True, 1), ("kspace", "object", True, 0), ("kspace", "coil", True, 0),
    ("images", "object", True, 3), ("images", "coil", True, 1), ("images", "coil", True, 0),
])
def test_parity_with_the_restatement_32(engine_mod, oracle, kind, phase_ref, window, patch):
    f = H.fixture()
    kw = dict(patch=patch, phase_ref=phase_ref, thresh=THRESH)
    if kind == "kspace":
        want = _ref(f, window=window, **kw)
        calib = f["block"]
    else:
        calib = R.calib_images(f["block"], 32, 32, True)
        want = R.coil_maps_ref(calib, 32, 32, kind="images", full=True, **kw)
    e = _engine(engine_mod, oracle, 32, 32)
    got = e.coil_maps(calib, kind=kind, window=window, **kw)
    e.close()
    _compare(got, want, THRESH, (kind, phase_ref, window, patch))
    if patch == 0:                                   # closed form u = I / |I|
        I = want[5]
        u = I / np.linalg.norm(I, axis=2, keepdims=True)
        sel = want[4]
        g, u = got[0][sel], u[sel]
        assert np.max(np.abs(g * np.conj(g[:, :1]) / np.abs(g[:, :1]) - u * np.conj(u[:, :1]) / np.abs(u[:, :1]))) <= 1e-12


@pytest.mark.parametrize("N,M,cN,cM,nc,thresh", [(64, 96, 24, 16, 8, THRESH), (32, 32, 16, 16, 32, THRESH), (32, 32, 16, 16, 3, THRESH)])
def test_parity_rectangular_many_coils_ragged(engine_mod, oracle, N, M, cN, cM, nc, thresh):
    """64 x 96 with a 24 x 16 block; 32 coils (the eigen kernel stages the coil images in two LDS chunks); 3 coils (most lanes of a pixel idle);
    each in both gauges."""
    f = H.fixture(N, M, nc, cN, cM)
    for phase_ref in ("object", "coil"):
        want = R.coil_maps_ref(f["block"], N, M, phase_ref=phase_ref, thresh=thresh, full=True)
        e = _engine(engine_mod, oracle, N, M)
        got = e.coil_maps(f["block"], phase_ref=phase_ref, thresh=thresh)
        e.close()
        _compare(got, want, thresh, (N, M, nc, phase_ref))
        nrm = np.sqrt(np.sum(np.abs(got[0]) ** 2, axis=2))
        assert np.max(np.abs(nrm[nrm > 0] - 1.0)) <= 1e-12


def test_batch_invariance_and_device_entry_point_bits(engine_mod, oracle):
    """A 3-slice stack against each slice alone, max_batch 1 against 4, 8 coils (resident) and 32 coils (chunked): the same bits of maps, img and
    lambda_1.  And qmri_coil_maps_dev on device arrays against the host-array call, bit for bit."""
    hip = _hip()
    for nc in (8, 32):
        fs = [H.fixture(32, 32, nc, 16, 16, seed=sd) for sd in (0, 1, 2)]
        stack = np.stack([f["block"] for f in fs])
        base = None
        for maxb in (1, 4):
            e = _engine(engine_mod, oracle, 32, 32, max_batch=maxb)
            whole = e.coil_maps(stack, phase_ref="coil", thresh=THRESH)
            if base is None:
                base = whole
            for key in range(3):
                assert np.array_equal(whole[key], base[key]), (nc, maxb, key)
            for b in range(3):
                alone = e.coil_maps(stack[b], phase_ref="coil", thresh=THRESH)
                for key in range(3):
                    assert np.array_equal(alone[key], base[key][b]), (nc, maxb, b, key)
            if maxb == 4:
                from qmri_pnp_recon_poc_amd._lib import CsmInfo, CsmParams
                cb = np.ascontiguousarray(np.concatenate([np.asarray(stack[b]).ravel(order="F") for b in range(3)]))
                m, im, lm = np.empty(3 * nc * 1024, np.complex128), np.empty(3 * 1024, np.complex128), np.empty(3 * 1024, np.float64)
                d_c, d_m, d_i, d_l = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
                for d, nb in ((d_c, cb.nbytes), (d_m, m.nbytes), (d_i, im.nbytes), (d_l, lm.nbytes)):
                    assert hip.hipMalloc(C.byref(d), nb) == 0
                try:
                    assert hip.hipMemcpy(d_c, cb.ctypes.data, cb.nbytes, 1) == 0
                    p, info = CsmParams(0, 16, 16, 3, 1, 1, THRESH), CsmInfo()
                    e._check(e.L.qmri_coil_maps_dev(e.h, 3, nc, 32, 32, d_c, C.byref(p), d_m, d_i, d_l, C.byref(info)))
                    for host, d in ((m, d_m), (im, d_i), (lm, d_l)):
                        assert hip.hipMemcpy(host.ctypes.data, d, host.nbytes, 2) == 0
                    assert e.L.qmri_coil_maps_dev(e.h, 3, nc, 32, 32, d_c, C.byref(p), d_c, None, None, None) == -1     # maps_out aliases calib
                finally:
                    for d in (d_c, d_m, d_i, d_l):
                        hip.hipFree(d)
                for b in range(3):
                    assert np.array_equal(m[b * nc * 1024:(b + 1) * nc * 1024].reshape((32, 32, nc), order="F"), base[0][b])
                    assert np.array_equal(im[b * 1024:(b + 1) * 1024].reshape((32, 32), order="F"), base[1][b])
                    assert np.array_equal(lm[b * 1024:(b + 1) * 1024].reshape((32, 32), order="F"), base[2][b])
                assert info.max_iters == base[3]["max_iters"] and info.not_converged == 0
            e.close()


def test_rank_one_images_closed_form(engine_mod, oracle):
    """I_j = c_j g(r) with a constant c: the maps are c / |c| up to the stated phase, to 1e-12 wherever g != 0 (and the zero pixels keep e_0)."""
    N = 32
    rng = np.random.default_rng(3)
    c = rng.standard_normal(5) + 1j * rng.standard_normal(5)
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, N), indexing="ij")
    g = (1.0 + hh + 0.3 * ww ** 2) * np.exp(1j * (hh - 0.7 * ww))
    g[hh ** 2 + ww ** 2 > 0.9] = 0.0
    I = g[..., None] * c
    e = _engine(engine_mod, oracle, N, N)
    u = c / np.linalg.norm(c)
    for p in (0, 2, 4):
        maps, img, lam, info = e.coil_maps(I, kind="images", patch=p, phase_ref="coil")
        ref = int(np.argmax(np.abs(c)))
        want = u * np.exp(-1j * np.angle(u[ref]))
        nz = g != 0
        assert np.max(np.abs(maps[nz] - want)) <= 1e-12 and info["not_converged"] == 0
        maps, img, _, _ = e.coil_maps(I, kind="images", patch=p, phase_ref="object")
        assert np.max(np.abs(maps[nz] - u * (g[nz] / np.abs(g[nz]))[:, None])) <= 1e-12
        assert np.max(np.abs(img[nz] - np.abs(g[nz]) * np.linalg.norm(c))) <= 1e-12 * np.abs(img).max()
    far = np.zeros((N, N), bool)
    far[:3, :3] = True                                  # the corner's 5 x 5 patches hold zeros only
    maps, _, lam, _ = e.coil_maps(I, kind="images", patch=2)
    assert np.all(lam[far] == 0) and np.all(maps[far][:, 0] == 1) and np.all(maps[far][:, 1:] == 0)
    e.close()


def _recon_case(oracle, f, seed=5):
    V, fp, k = _operator(oracle, f["N"], f["M"])
    op = oracle.Operator(f["N"], f["M"], V, fp, k)
    X0 = f["x"][..., None] * np.array([1.0, 0.5])
    y = op.forward_mc(X0, f["C"])
    rng = np.random.default_rng(seed)
    z = 0.1 * (rng.standard_normal(X0.shape) + 1j * rng.standard_normal(X0.shape))
    return V, fp, k, op, X0, y, z


def test_through_the_reconstruction(engine_mod, oracle):
    """xupdate_mc with the maps estimated on the GPU and with the restatement's: the same x to 1e-8, equal LSQR counts and flags.  The data residual
    |A_mc(C_hat) x_hat - y| / |y| is printed beside the same figure with the true maps (oracle lsqr_mc, CPU): DESIGN.md section 17."""
    f = H.fixture()
    V, fp, k, op, X0, y, z = _recon_case(oracle, f)
    want = _ref(f, patch=3, phase_ref="object", thresh=THRESH, window=True)
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, V, fp, k)
    maps = e.coil_maps(f["block"], thresh=THRESH)[0]
    out = []
    for m in (maps, want[0]):
        e.set_coils(m)
        out.append(e.xupdate_mc(y, z, 0.05, tol=1e-6, maxit=100))
    e.close()
    assert rel_err(out[0][0], out[1][0]) <= 1e-8 and out[0][1:] == out[1][1:]
    res = []
    for m in (want[0], f["C"]):
        x, it, fl = op.lsqr_mc(y, m, z, 0.05, tol=1e-6, maxit=100)
        res.append(np.linalg.norm(op.forward_mc(x, m) - y) / np.linalg.norm(y))
    assert rel_err(out[1][0], op.lsqr_mc(y, want[0], z, 0.05, tol=1e-6, maxit=100)[0]) <= 1e-8
    print(f"data residual with the estimated maps {res[0]:.4e}, with the true maps {res[1]:.4e}; LSQR iterations {out[0][1]}")


def test_after_coil_compress(engine_mod, oracle):
    """32 coils: the calibration block and the measurements compressed with the same W (8 virtual coils), maps estimated from the compressed block, one
    x-update -- against the restatements doing the same steps, to 1e-8."""
    f = H.fixture(32, 32, 32, 16, 16)
    V, fp, k, op, X0, y, z = _recon_case(oracle, f)
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, V, fp, k)
    cc = e.coil_compress(y[None], nv=8)
    blk = f["block"] @ np.conj(cc["W"][0])
    maps = e.coil_maps(blk, thresh=THRESH)[0]
    x, it, fl = e.xupdate_mc_batch(maps[None], cc["y"], z[None], 0.05, tol=1e-6, maxit=100)
    e.close()
    rc = ccref.coil_compress(y[None], nv=8)
    rmaps = R.coil_maps_ref(f["block"] @ np.conj(rc["W"][0]), 32, 32, thresh=THRESH)[0]
    xr, itr, flr = op.lsqr_mc(rc["y"][0], rmaps, z, 0.05, tol=1e-6, maxit=100)
    print("maps after compression:", rel_err(maps, rmaps), "x:", rel_err(x[0], xr), "iterations", it[0], itr)
    assert rel_err(maps, rmaps) <= 1e-8 and rel_err(x[0], xr) <= 1e-8 and it[0] == itr and fl[0] == flr


def test_mex_coil_maps_equals_python_bits(engine_mod, oracle):
    import mexmock as mex
    f = H.fixture()
    V, fp, k = _operator(oracle, 32, 32)
    try:
        mex.qmri_mex("set_operator", 32.0, 32.0, np.asarray(V, np.float64), fp.astype(np.int32), k.astype(np.int32))
        stack = np.stack([f["block"], H.fixture(seed=1)["block"]], axis=3)           # cN x cM x ncoil x S
        m, i, l, info = mex.qmri_mex("coil_maps", np.asfortranarray(stack), {"patch": 2.0, "phase_coil": 1.0, "thresh": THRESH}, nargout=4)
    finally:
        mex.mex_exit()
    e = _engine(engine_mod, oracle, 32, 32)
    pm, pi, pl, pinfo = e.coil_maps(np.moveaxis(stack, 3, 0), patch=2, phase_ref="coil", thresh=THRESH)
    e.close()
    assert np.array_equal(np.moveaxis(m, 3, 0), pm) and np.array_equal(np.moveaxis(i, 2, 0), pi) and np.array_equal(np.moveaxis(l, 2, 0), pl)
    assert int(np.ravel(info["max_iters"])[0]) == pinfo["max_iters"] and int(np.ravel(info["not_converged"])[0]) == 0


def test_existing_calls_untouched_by_a_coil_maps_call(engine_mod, oracle):
    """set_coils / forward_mc give the same bits before and after coil_maps on the same context, and coil_maps does not touch the maps of set_coils."""
    f = H.fixture()
    V, fp, k, op, X0, y, z = _recon_case(oracle, f)
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, V, fp, k)
    e.set_coils(f["C"])
    before = e.forward_mc(X0)
    e.coil_maps(f["block"], thresh=THRESH)
    assert np.array_equal(e.forward_mc(X0), before)
    e.set_coils(f["C"])
    assert np.array_equal(e.forward_mc(X0), before) and np.array_equal(e.adjoint_mc(before), e.adjoint_mc(before))
    e.close()
