"""GPU: PnP-ADMM with complex TSMIs (include/qmri.h QMRI_DENOISER_COMPLEX) against the CPU restatement of
tests/complex_admm_ref.py (the oracle's x-update and single-precision network, Step 2 on cat(3, real(x + u), imag(x + u))).  No reference
counterpart: the reference's TSMIs are real (PnP_ADMM.m:115-118)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import complex_admm_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _phase(N, M):
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, M), indexing="ij")
    return 1.2 * hh + 0.8 * ww * ww


def _complex_tsmi(synth, dic, N, seed=0):
    """A phantom's TSMI with a smooth phase, X0 * exp(i phi)."""
    X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=seed), dic)
    return X0 * np.exp(1j * _phase(N, N))[:, :, None]


def _small(oracle, synth, multi=False, N=32, T=24, s=6, S=120, nc=(16, 16, 16, 32), seed=0, noisy=True):
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    X0 = _complex_tsmi(synth, dic, N, seed)
    fp, k = oracle.spiral_mask(N, S, T)
    op = oracle.Operator(N, N, dic["V"], fp, k)
    y = op.forward(X0)
    if noisy:
        y = synth.awgn_measured(y, 30.0, seed=seed)
    w = synth.structured_weights(in_nc=2 * s + multi, out_nc=2 * s, nc=nc, nb=2, seed=3, eps=0.05)
    return dic, X0, fp, k, op, y, nc, w


def test_network_20_and_21_channels_at_224(engine_mod, oracle, synth):
    """The full-size UNetRes with 20 -> 20 and 21 -> 20 channels at 224 x 224 against the oracle's fp32 forward; the resident-tile launch (head
    of two 16-channel input chunks, tail of 20 planar output channels) gives the bits of one launch per layer (conv_resident = 0)."""
    rng = np.random.default_rng(5)
    for cin in (20, 21):
        w = synth.structured_weights(in_nc=cin, out_nc=20, seed=4, eps=0.3)
        e = engine_mod.Engine(0)
        e.set_denoiser(w, 224, 224, in_nc=cin, out_nc=20)
        assert e.health()["resident_tile_launch_armed"]
        x = rng.random((224, 224, cin))
        got = e.denoise(x)
        ref = oracle.Net(w, in_nc=cin, out_nc=20).forward_f32(x.astype(np.float32))
        err = rel_err(got, ref)
        print(f"{cin} -> 20: rel err vs oracle {err:.2e}")
        assert got.shape == (224, 224, 20) and err < 2e-5
        e.conv_resident(0)
        per_layer = e.denoise(x)
        e.conv_resident(1)
        for _ in range(3):
            assert np.array_equal(e.denoise(x), per_layer), cin
        assert e.conv_resident(1) == 0 and e.health()["resident_tile_launch_armed"]
        e.close()


def test_same_convolution_launches_per_iteration_in_both_modes(engine_mod, synth):
    """One slice at 224 x 224, s = 10, full-size UNetRes: the convolution launches of an ADMM iteration (profile level 2 units: a resident-tile
    launch counts once, with the head / tail / down-sampling layers riding in it) are as many in complex mode (20 -> 20) as in real mode (10 -> 10)."""
    dic = synth.make_dictionary(T=200, n_t1=32, n_t2=16, s=10)
    fp, k = engine_mod.build_spiral(224, 771, 200)
    units = {}
    for dom, P in (("real", 10), ("complex", 20)):
        e = engine_mod.Engine(0)
        e.set_operator(224, 224, dic["V"], fp, k)
        e.set_denoiser(synth.structured_weights(in_nc=P, out_nc=P, seed=2, eps=0.02), 224, 224, in_nc=P, out_nc=P)
        X0 = _complex_tsmi(synth, dic, 224)
        y = synth.awgn_measured(e.forward(X0), 30.0, seed=0)
        e.pnp_admm(y, iters=1, tsmi_domain=dom)
        e.profile_enable(2)
        e.profile_get(reset=True)
        e.pnp_admm(y, iters=3, tsmi_domain=dom)
        p = e.profile_get(reset=True)
        e.profile_enable(0)
        units[dom] = ((p["n_conv3x3"] + p["n_conv2x2"]) / max(p["admm_iters"], 1), p["n_net_forward"])
        e.close()
    print(f"convolution launch units per ADMM iteration: {units}")
    assert units["real"][0] > 0 and units["real"] == units["complex"]


def test_admm_224_complex_vs_restatement(engine_mod, oracle, synth):
    """8 iterations at 224 x 224, s = 10, a 20 -> 20 network (nc[0] = 64): identical LSQR counts, x within 1e-4, diagnostics within rtol 1e-4;
    DIRECT against the restatement's DIRECT."""
    dic = synth.make_dictionary(T=200, n_t1=32, n_t2=16, s=10)
    X0 = _complex_tsmi(synth, dic, 224)
    fp, k = oracle.spiral_mask(224, 771, 200)
    op = oracle.Operator(224, 224, dic["V"], fp, k)
    y = synth.awgn_measured(op.forward(X0), 30.0, seed=0)
    w = synth.structured_weights(in_nc=20, out_nc=20, seed=2, eps=0.02)
    net = oracle.Net(w, in_nc=20, out_nc=20)
    e = engine_mod.Engine(0)
    e.set_operator(224, 224, dic["V"], fp, k)
    e.set_denoiser(w, 224, 224, in_nc=20, out_nc=20)
    xg, dg, lg = e.pnp_admm(y, iters=8, gt=X0, want_diag=True, tsmi_domain="complex")
    xo, do, lo = R.pnp_admm(op, net, y, iters=8, gt=X0, want_diag=True)
    err = rel_err(xg, xo)
    print(f"224 complex: lsqr {lg.tolist()} / {lo.tolist()}, rel err {err:.2e}")
    assert np.array_equal(lg, lo)
    assert err < 1e-4
    assert np.allclose(dg, do, rtol=1e-4, atol=0)
    xd, _, _ = e.pnp_admm(y, iters=8, solver="direct", tsmi_domain="complex")
    xod, _, _ = R.pnp_admm(op, net, y, iters=8, solver="direct")
    assert rel_err(xd, xod) < 1e-4 and rel_err(xd, xg) < 2e-3
    e.close()


@pytest.mark.parametrize("multi", [False, True])
def test_admm_small_100_iterations_complex(engine_mod, oracle, synth, multi):
    """32 x 32, s = 6, 12 (+1) -> 12 channels, 100 iterations: the tolerances of the real-mode test_admm_small_100_iterations."""
    dic, X0, fp, k, op, y, nc, w = _small(oracle, synth, multi)
    s = 6
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, dic["V"], fp, k)
    e.set_denoiser(w, 32, 32, in_nc=2 * s + multi, out_nc=2 * s, nc=nc, nb=2)
    xg, dg, lg = e.pnp_admm(y, iters=100, multi_level=multi, noise_std=0.01, gt=X0, want_diag=True, tsmi_domain="complex")
    net = oracle.Net(w, in_nc=2 * s + multi, out_nc=2 * s, nc=nc, nb=2)
    xo, do, lo = R.pnp_admm(op, net, y, iters=100, multi_level=multi, noise_std=0.01, gt=X0, want_diag=True)
    frac, err, maxdiff = float(np.mean(lg == lo)), rel_err(xg, xo), int(np.abs(lg - lo).max())
    print(f"small complex multi={multi}: same-count fraction {frac:.2f}, max diff {maxdiff}, rel err {err:.2e}")
    assert frac > 0.7 and maxdiff <= 2
    assert err < 2e-4
    assert np.allclose(dg[:, 0], do[:, 0], rtol=5e-3)
    e.close()


def test_slice_batches_complex(engine_mod, oracle, synth):
    """pnp_admm_batch with 3 and 15 slices per launch against one slice at a time (same LSQR counts, x to 1e-10), and recon_batch with two workers."""
    from qmri_pnp_recon_poc_amd import batch
    dic, X0, fp, k, op, _, nc, w = _small(oracle, synth)
    s, S = 6, 5
    ys = np.stack([synth.awgn_measured(op.forward(_complex_tsmi(synth, dic, 32, seed=b)), 30.0, seed=b) for b in range(S)])
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, dic["V"], fp, k, max_batch=15)
    e.set_denoiser(w, 32, 32, in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2, max_batch=15)
    one = [e.pnp_admm(ys[b], iters=10, tsmi_domain="complex") for b in range(S)]
    for spl in (3, 15):
        X, li = e.pnp_admm_batch(ys, slices_per_launch=spl, iters=10, tsmi_domain="complex")
        for b in range(S):
            assert np.array_equal(li[b], one[b][2]), (spl, b)
            assert rel_err(X[b], one[b][0]) < 1e-10, (spl, b, rel_err(X[b], one[b][0]))
    e.close()
    r = batch.recon_batch([0, 0], ys, N=32, M=32, V=dic["V"], frame_ptr=fp, kidx=k, weights=w, in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2,
                          iters=10, slices_per_launch=2, tsmi_domain="complex")
    for b in range(S):
        assert rel_err(r["X"][b], one[b][0]) < 1e-10, b


def _mc_maps(N, nc, phase):
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, N), indexing="ij")
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                  for a in phase + np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def test_multi_coil_complex(engine_mod, oracle, synth):
    """8 coils at 64 x 64: pnp_admm_mc and pnp_admm_mc_batch against the restatement on lsqr_mc."""
    N, s, T = 64, 6, 24
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    fp, k = oracle.spiral_mask(N, 240, T)
    op = oracle.Operator(N, N, dic["V"], fp, k)
    nc = (16, 16, 16, 32)
    w = synth.structured_weights(in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2, seed=3, eps=0.05)
    net = oracle.Net(w, in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2)
    maps = np.stack([_mc_maps(N, 8, 0.7 * b) for b in range(2)])
    ys = np.stack([op.forward_mc(_complex_tsmi(synth, dic, N, seed=b), maps[b]) for b in range(2)])
    e = engine_mod.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=2)
    e.set_denoiser(w, N, N, in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2, max_batch=2)
    ref = [R.pnp_admm(op, net, ys[b], iters=6, maps=maps[b]) for b in range(2)]
    e.set_coils(maps[0])
    x1, l1 = e.pnp_admm_mc(ys[0], iters=6, tsmi_domain="complex")
    assert np.array_equal(l1, ref[0][2]) and rel_err(x1, ref[0][0]) < 1e-4, (l1, ref[0][2], rel_err(x1, ref[0][0]))
    X, li = e.pnp_admm_mc_batch(maps, ys, slices_per_launch=2, iters=6, tsmi_domain="complex")
    for b in range(2):
        assert np.array_equal(li[b], ref[b][2]) and rel_err(X[b], ref[b][0]) < 1e-4, b
    e.close()


def test_fused_equal_separate_kernels_complex(tmp_path):
    """QMRI_DEBUG="fuse_ew=0" (separate k_minmax / k_normalise / k_unnormalise_dual) against the fused k_adj_h / k_dual_fwd_h, in two child
    processes: 8 complex-mode iterations at 224 x 224, single- and multi-level -- identical LSQR counts, x within 1e-12."""
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from qmri_pnp_recon_poc_amd import engine as E, synth\n"
        "dic = synth.make_dictionary(T=200, n_t1=32, n_t2=16)\n"
        "fp, k = E.build_spiral(224, 771, 200)\n"
        "hh, ww = np.meshgrid(np.linspace(-1, 1, 224), np.linspace(-1, 1, 224), indexing='ij')\n"
        "X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(224, seed=0), dic) * np.exp(1j * (1.2 * hh + 0.8 * ww * ww))[:, :, None]\n"
        "out = {}\n"
        "for multi in (0, 1):\n"
        "    w = synth.structured_weights(in_nc=20 + multi, out_nc=20, seed=2, eps=0.3)\n"
        "    e = E.Engine(0)\n"
        "    e.set_operator(224, 224, dic['V'], fp, k)\n"
        "    e.set_denoiser(w, 224, 224, in_nc=20 + multi, out_nc=20)\n"
        "    y = synth.awgn_measured(e.forward(X0), 30.0, seed=0)\n"
        "    x, _, li = e.pnp_admm(y, iters=8, multi_level=bool(multi), tsmi_domain='complex')\n"
        "    out[f'x{multi}'] = x; out[f'li{multi}'] = li\n"
        "    e.close()\n"
        "np.savez(sys.argv[1], **out)\n")
    res = {}
    for flag in ("1", "0"):
        path = str(tmp_path / f"fuse_{flag}.npz")
        r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, QMRI_DEBUG="fuse_ew=" + flag), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[flag] = np.load(path)
    for key in res["1"].files:
        a, b = res["1"][key], res["0"][key]
        if key.startswith("li"):
            assert np.array_equal(a, b), (key, a, b)
        else:
            assert rel_err(a, b) < 1e-12, (key, rel_err(a, b))


def _near_identity_weights(synth, P, nc, eps=0.01):
    """structured_weights with the head's blur replaced by the centre tap: the network is the identity on channels 0 .. P-1 plus eps * random
    through every layer (with eps = 0 it is the identity exactly)."""
    w = synth.structured_weights(in_nc=P, out_nc=P, nc=nc, nb=2, seed=3, eps=eps)
    head = w[: nc[0] * P * 9].reshape(nc[0], P, 3, 3)              # (a view: m_head.weight is the first tensor of the blob)
    delta = np.zeros((3, 3), np.float32)
    delta[1, 1] = 1.0
    blur = (np.outer([1.0, 2.0, 1.0], [1.0, 2.0, 1.0]) / 16.0).astype(np.float32)
    for c in range(P):
        head[c, c] += delta - blur
    return w


# Measured on the CPU restatement (32 x 32, s = 6, the phantom of _small with clean data, the near-identity network, 20 iterations):
# relative data residual 0.3235 real against 0.00417 complex (ratio 77.5), error against X0 0.458 real against 0.299 complex (ratio 1.53;
# the adjoint alone: 0.316).  The residual threshold is a third of its measured ratio; the error must be lower by at least a quarter.
RESIDUAL_RATIO_MEASURED = 77.5
ERROR_RATIO_MIN = 1.25


def test_complex_mode_keeps_the_phase(engine_mod, oracle, synth):
    """With a near-identity network and clean data, 20 iterations: complex mode fits the data far better than real mode, which throws the
    imaginary half away at every denoiser step, and lands closer to X0.  The restatement's own ratios are asserted too, so the test cannot go blind."""
    dic, X0, fp, k, op, y, nc, _ = _small(oracle, synth, noisy=False)
    s = 6
    w6, w12 = _near_identity_weights(synth, s, nc), _near_identity_weights(synth, 2 * s, nc)
    res = lambda x: np.linalg.norm(y - op.forward(x)) / np.linalg.norm(y)
    err = lambda x: rel_err(x, X0)
    xr, _, _ = R.pnp_admm(op, oracle.Net(w6, in_nc=s, out_nc=s, nc=nc, nb=2), y, iters=20, tsmi_domain="real")
    xc, _, _ = R.pnp_admm(op, oracle.Net(w12, in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2), y, iters=20, tsmi_domain="complex")
    assert res(xr) / res(xc) > RESIDUAL_RATIO_MEASURED / 3 and err(xr) / err(xc) > ERROR_RATIO_MIN
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, dic["V"], fp, k)
    e.set_denoiser(w6, 32, 32, in_nc=s, out_nc=s, nc=nc, nb=2)
    gr, _, _ = e.pnp_admm(y, iters=20)
    e.set_denoiser(w12, 32, 32, in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2)
    gc, _, _ = e.pnp_admm(y, iters=20, tsmi_domain="complex")
    print(f"data residual real {res(gr):.4f} complex {res(gc):.5f} (ratio {res(gr) / res(gc):.1f}, restatement {res(xr) / res(xc):.1f}); "
          f"error vs X0 real {err(gr):.3f} complex {err(gc):.3f}")
    assert res(gr) / res(gc) > RESIDUAL_RATIO_MEASURED / 3
    assert err(gr) / err(gc) > ERROR_RATIO_MIN
    e.close()


def test_spiral_exact_one_slice_complex(engine_mod, synth):
    """The one-slice loop on an exact spiral trajectory (NUFFT operator, through the multi-coil path) in complex mode against the restatement on
    the NUDFT operator's lsqr_mc with one unit coil."""
    import nufft_ref as NR
    N, s = 64, 6
    dic = synth.make_dictionary(T=24, n_t1=24, n_t2=16, s=s)
    fp, om = engine_mod.build_spiral_traj(N, 120, 24)
    X0 = _complex_tsmi(synth, dic, N)
    op = NR.NudftOperator(N, N, dic["V"], fp, om)
    rng = np.random.default_rng(2)
    y = op.forward(X0) + 0.005 * (rng.standard_normal(om.shape[0]) + 1j * rng.standard_normal(om.shape[0]))
    nc = (16, 16, 16, 32)
    w = synth.structured_weights(in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2, seed=3, eps=0.05)
    e = engine_mod.Engine(0)
    e.set_trajectory(N, N, dic["V"], fp, om)
    e.set_denoiser(w, N, N, in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2)
    xg, _, lg = e.pnp_admm(y, iters=5, tsmi_domain="complex")
    ones = np.ones((N, N, 1), np.complex128)
    xo, _, lo = R.pnp_admm(op, oracle_net(w, 2 * s, nc), y[:, None], iters=5, maps=ones)
    print(f"SpiralExact complex: lsqr {lg.tolist()} / {lo.tolist()}, rel err {rel_err(xg, xo):.2e}")
    assert np.array_equal(lg, lo) and rel_err(xg, xo) < 1e-4
    e.close()


def oracle_net(w, P, nc):
    from oracle import oracle as O
    return O.Net(w, in_nc=P, out_nc=P, nc=nc, nb=2)


def test_recon_tsmis_complex_end_to_end(engine_mod, synth):
    """harness.recon_tsmis(tsmi_domain="complex") on a complex TSMI from Engine.synthesize_tsmi(mode="complex") via tsmi_from_stack: it runs,
    the matched PD carries the phantom's phase, the metrics are finite."""
    from qmri_pnp_recon_poc_amd import harness as H
    N, T, s = 32, 24, 6
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    q = synth.make_phantom_qmaps(N, seed=0).astype(np.complex128)
    phi = 0.6 * _phase(N, N)
    q[:, :, 2] = np.abs(q[:, :, 2]) * np.exp(1j * phi)
    e = engine_mod.Engine(0)
    e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
    stored, _ = e.synthesize_tsmi(q, mode="complex")
    e.close()
    X0 = H.tsmi_from_stack(stored)
    nc = (16, 16, 16, 32)
    w = synth.structured_weights(in_nc=2 * s, out_nc=2 * s, nc=nc, nb=2, seed=3, eps=0.05)
    r = H.recon_tsmis(dic, X0, q, weights=w, recon_method="PnP_ADMM", spiral_sampling_curve=120, iters=8, seed=7,
                      net_arch={"nc": nc, "nb": 2}, tsmi_domain="complex")
    assert np.iscomplexobj(r["X"]) and all(np.isfinite(v) for v in r["metrics"].values())
    # the phase the same dictionary match gives the ground truth X0 (the synthesis's channel-sign convention included)
    from qmri_pnp_recon_poc_amd import reference_api as RA
    par = {"f": {"qout": 1, "pdout": 1}}
    pd0 = np.asarray(RA.mrf_dtm_cpu(dic, {"X": X0}, par)["pd"]).reshape(N, N)
    pd = r["qmap"][:, :, 2]
    fg = r["foreground_mask"] > 0
    coherence = float(np.abs(np.mean(np.exp(1j * (np.angle(pd[fg]) - np.angle(pd0[fg]))))))
    print(f"PD phase coherence with the ground truth's match: {coherence:.3f}")
    assert coherence > 0.5                                           # (measured 0.75 after 8 iterations of this synthetic network)


def test_refusals(engine_mod, oracle, synth):
    """A complex flag with an s-channel network and a 2s-channel network in real mode: QMRI_ERR_STATE naming both channel counts;
    denoiser_type = 4: QMRI_ERR_INVALID_ARG.  Through the C ABI and through Python."""
    from qmri_pnp_recon_poc_amd._lib import AdmmParams
    dic, X0, fp, k, op, y, nc, w12 = _small(oracle, synth)
    s = 6
    w6 = synth.structured_weights(in_nc=s, out_nc=s, nc=nc, nb=2, seed=3, eps=0.05)
    e = engine_mod.Engine(0)
    e.set_operator(32, 32, dic["V"], fp, k)
    L, h = e.L, e.h
    yb = np.ascontiguousarray(np.asarray(y, np.complex128).ravel(order="F"))
    x = np.zeros(32 * 32 * s, np.complex128)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for w, cin, dtype, want, text in ((w6, s, 2, -2, b"6 -> 6"), (w12, 2 * s, 0, -2, b"12 -> 12"), (w6, s, 4, -1, b"denoiser_type")):
        e.set_denoiser(w, 32, 32, in_nc=cin, out_nc=cin, nc=nc, nb=2)
        p = AdmmParams(0.05, 2, 1e-4, 100, 0, dtype, 0.01, 0)
        assert L.qmri_pnp_admm(h, vp(yb), C.byref(p), None, None, vp(x), None, None) == want, dtype
        assert text in L.qmri_last_error(h), L.qmri_last_error(h)
        if dtype != 4:
            with pytest.raises(engine_mod.QmriError) as ei:
                e.pnp_admm(y, iters=2, tsmi_domain="complex" if dtype == 2 else "real")
            assert ei.value.code == want
    with pytest.raises(ValueError):
        e.pnp_admm(y, iters=2, tsmi_domain="polar")
    e.close()
