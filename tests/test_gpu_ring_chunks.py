"""GPU: the resident-tile launch's ring exchange pipelined by 16-channel chunk (k_conv6r, knob res_pipe = 1: chunk 0 published early and fetched
under the epilogue, chunks 1 - 3 fetched under the next layer's loop) gives the bits of the unpipelined exchange (res_pipe = 0) and of one launch
per layer (conv_resident = 0), pass after pass.  The smallest tilings that can go wrong: 2 x 2 tiles (every tile a corner), 3 x 3 (the smallest
with a tile that has all eight neighbours), 4 x 6 (not square).  A stale or torn granule would show as a difference that varies from pass to pass;
two alternating images make sure the exchange buffers hold the OTHER image's edges when a pass starts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PASSES = 8


@pytest.mark.parametrize("cin", [10, 11])
@pytest.mark.parametrize("shape", [(32, 32), (48, 48), (64, 96)])
def test_pipelined_ring_exchange_same_bits(engine_mod, synth, shape, cin):
    H, W = shape
    w = synth.random_weights(in_nc=cin, seed=1, gain=0.7)
    rng = np.random.default_rng(100 * H + cin)
    imgs = [rng.random((H, W, cin)), rng.random((H, W, cin))]
    e = engine_mod.Engine(0)
    try:
        e.set_denoiser(w, H, W, in_nc=cin)
        assert e.health()["resident_tile_launch_armed"]
        e.conv_resident(0)
        per_layer = [e.denoise(x) for x in imgs]
        assert not np.array_equal(per_layer[0], per_layer[1])
        e.conv_resident(1)
        e._check(e.L.qmri_debug_knob(b"res_pipe", 0))
        plain = [e.denoise(imgs[p & 1]) for p in range(PASSES)]
        e._check(e.L.qmri_debug_knob(b"res_pipe", 1))
        piped = [e.denoise(imgs[p & 1]) for p in range(PASSES)]
        for p in range(PASSES):
            assert np.array_equal(plain[p], per_layer[p & 1]), f"res_pipe = 0, pass {p}: differs from one launch per layer"
            assert np.array_equal(piped[p], plain[p]), f"pass {p}: res_pipe = 1 differs from res_pipe = 0"
            assert np.array_equal(piped[p], per_layer[p & 1]), f"pass {p}: res_pipe = 1 differs from one launch per layer"
        assert e.conv_resident(1) == 0                      # no hand-off time-out
        assert e.health()["resident_tile_launch_armed"]
        assert e.denoiser_scheme() == (2, 0)                # still f16 x 3
    finally:
        e.L.qmri_debug_knob(b"res_pipe", 1)
        e.close()
