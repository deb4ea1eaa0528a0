"""Complex TSMIs (include/qmri.h QMRI_DENOISER_COMPLEX) without a GPU: the stored 2s-channel layout, the Python
argument checks, a 21-channel ONNX export, and the properties of the CPU restatement (tests/complex_admm_ref.py) that the GPU tests rely on."""
import numpy as np
import pytest

import complex_admm_ref as R


def test_tsmi_from_stack_round_trips_the_stored_layout():
    from qmri_pnp_recon_poc_amd import harness as H
    rng = np.random.default_rng(0)
    X = (rng.standard_normal((8, 6, 10)) + 1j * rng.standard_normal((8, 6, 10)))
    stored = np.concatenate([X.real, X.imag], axis=2).astype(np.float32)     # cat(3, real(X), imag(X)), main_synthesize_tsmis.m:100-103
    Xc = H.tsmi_from_stack(stored)
    assert Xc.shape == (8, 6, 10) and np.iscomplexobj(Xc)
    assert np.array_equal(Xc, X.astype(np.complex64).astype(np.complex128))
    assert np.array_equal(R.stack(Xc).astype(np.float32), stored)
    batch = np.stack([stored, 2 * stored])                                     # a leading slice axis
    assert np.array_equal(H.tsmi_from_stack(batch)[1], 2 * Xc)
    for bad in (stored[..., :9], stored[:, :, 0], Xc):
        with pytest.raises(ValueError):
            H.tsmi_from_stack(bad)


def test_denoiser_type_bits_and_argument_checks_without_a_device():
    from qmri_pnp_recon_poc_amd import batch, engine as E, harness as H, reference_api as RA
    assert [E.denoiser_type(m, d) for d in ("real", "complex") for m in (False, True)] == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="tsmi_domain"):
        E.denoiser_type(False, "imaginary")
    with pytest.raises(ValueError, match="tsmi_domain"):
        batch.recon_batch([0], np.zeros((1, 4), complex), 8, 8, np.ones((4, 2)), [0, 4], np.arange(4), np.zeros(1, np.float32),
                          tsmi_domain="magnitude")
    with pytest.raises(ValueError, match="tsmi_domain"):
        RA.make_net(np.zeros(1, np.float32), tsmi_domain="both")
    with pytest.raises(ValueError, match="even"):
        RA.make_net(np.zeros(1, np.float32), out_nc=11, tsmi_domain="complex")
    with pytest.raises(ValueError, match="tsmi_domain"):
        H.recon_tsmis({"V": np.ones((4, 2))}, np.zeros((8, 8, 2), complex), np.zeros((8, 8, 3)), tsmi_domain="cplx")
    # the Engine methods take the keyword (their checks run before the library is called)
    import inspect
    for f in (E.Engine.pnp_admm, E.Engine.pnp_admm_batch, E.Engine.pnp_admm_mc, E.Engine.pnp_admm_mc_batch, batch.recon_batch,
              RA.make_net, H.recon_tsmis):
        assert inspect.signature(f).parameters["tsmi_domain"].default == "real", f.__name__


def test_onnx_reader_reads_a_21_channel_export(engine_mod, tmp_path):
    """A 21 -> 20 UNetRes (complex multi-level, s = 10) exported to ONNX: both readers return the channel counts and the weights."""
    import onnx_writer as ow
    from qmri_pnp_recon_poc_amd import synth, weights as Wt
    a = {"in_nc": 21, "out_nc": 20, "nc": [8, 16, 16, 32], "nb": 2}
    w = synth.structured_weights(in_nc=21, out_nc=20, nc=tuple(a["nc"]), nb=2, seed=1, eps=0.05)
    path = str(tmp_path / "complex21.onnx")
    with open(path, "wb") as f:
        f.write(ow.unetres_model(ow.split_blob(w, 21, 20, a["nc"], 2), 21, 20, a["nc"], 2))
    blob, arch = Wt.load_denoiser_weights(path)
    assert (arch["in_nc"], arch["out_nc"], list(arch["nc"]), arch["nb"]) == (21, 20, a["nc"], 2)
    assert np.array_equal(blob, w)
    nblob, narch = engine_mod.read_onnx_unetres(path)                   # libqmri's own reader, no GPU involved
    assert (narch["in_nc"], narch["out_nc"]) == (21, 20) and np.array_equal(nblob, w)


def test_restatement_imaginary_planes_of_a_real_input_are_constant():
    """imag(x + u) == 0: the imaginary planes hold (0 - lo) / range everywhere, the real planes the reference's own normalisation."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((6, 5, 3)) + 0j
    u = rng.standard_normal((6, 5, 3)) + 0j
    V, lo, rng_ = R.normalise(x, u, "complex", multi_level=True, noise_std=0.02)
    assert V.shape == (6, 5, 7)
    assert np.all(V[:, :, 3:6] == -lo / rng_)
    assert np.all(V[:, :, 6] == 0.02)
    w = np.real(x + u)
    lo_r = min(w.min(), 0.0)
    assert lo == lo_r and rng_ == max(w.max(), 0.0) - lo_r
    assert np.array_equal(V[:, :, :3], (w - lo) / rng_)


def test_restatement_unnormalise_undoes_the_normalisation():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((4, 4, 5)) + 1j * rng.standard_normal((4, 4, 5))
    u = 0.25 * (rng.standard_normal((4, 4, 5)) + 1j * rng.standard_normal((4, 4, 5)))
    V, lo, rng_ = R.normalise(x, u, "complex")
    assert V.min() == 0.0 and V.max() == 1.0
    v = R.unnormalise(V, lo, rng_, 5, "complex")
    assert np.allclose(v, x + u, rtol=0, atol=4 * np.finfo(float).eps * np.abs(x + u).max())
    Vr, lo_r, r_r = R.normalise(x, u, "real")
    assert np.allclose(R.unnormalise(Vr, lo_r, r_r, 5, "real"), np.real(x + u), rtol=0, atol=1e-15)
