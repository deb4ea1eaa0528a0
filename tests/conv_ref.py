"""Plain fp64 restatement of the denoiser's convolutions (numpy, no GPU), and input families whose exact result does not depend
on the order of summation.  Test infrastructure only: tests/test_conv_ref_host.py proves every claim made here on the CPU,
tests/test_gpu_conv_layers.py compares the HIP kernels with it.

Tensors are [H, W, C] or [H, W, C, B] (MATLAB dims, as Engine.denoise takes them) in fp64; weights are fp32 in the blob's order
(Conv2d OIHW with kh along H, ConvTranspose2d IOHW).  Zero padding, no bias.  Products of fp32 values are exact in fp64 (24 + 24 bits);
the sums are fp64 sums (error ~1e-16 relative to sum |w||x|), and exact for the families below, whose partial sums are all
representable.
"""
import numpy as np


def _bhwc(x):
    x = np.asarray(x, np.float64)
    if x.ndim == 3:
        return x[None], True
    if x.ndim != 4:
        raise ValueError("tensor must be H x W x C (x B)")
    return np.moveaxis(x, 3, 0), False


def _out(y, squeeze):
    return y[0] if squeeze else np.ascontiguousarray(np.moveaxis(y, 0, 3))


def conv3x3(x, w, relu=False):
    """y[h, w, o] = sum_c sum_kh sum_kw W[o, c, kh, kw] x[h + kh - 1, w + kw - 1, c]; relu: on the OUTPUT."""
    xb, sq = _bhwc(x)
    w = np.asarray(w).astype(np.float64)
    B, H, W, C = xb.shape
    O = w.shape[0]
    assert w.shape == (O, C, 3, 3), (w.shape, xb.shape)
    xp = np.zeros((B, H + 2, W + 2, C))
    xp[:, 1:-1, 1:-1] = xb
    y = np.zeros((B * H * W, O))
    for kh in range(3):
        for kw in range(3):                                         # (contiguous operands: one BLAS product per tap)
            y += np.ascontiguousarray(xp[:, kh:kh + H, kw:kw + W]).reshape(-1, C) @ np.ascontiguousarray(w[:, :, kh, kw].T)
    y = y.reshape(B, H, W, O)
    if relu:
        y = np.maximum(y, 0.0)
    return _out(y, sq)


def conv2x2s2(x, w):
    """y[i, j, o] = sum_c sum_kh sum_kw W[o, c, kh, kw] x[2 i + kh, 2 j + kw, c]"""
    xb, sq = _bhwc(x)
    w = np.asarray(w).astype(np.float64)
    B, H, W, C = xb.shape
    O = w.shape[0]
    assert w.shape == (O, C, 2, 2) and H % 2 == 0 and W % 2 == 0
    y = np.zeros((B, H // 2, W // 2, O))
    for kh in range(2):
        for kw in range(2):
            y += (np.ascontiguousarray(xb[:, kh::2, kw::2]).reshape(-1, C) @ np.ascontiguousarray(w[:, :, kh, kw].T)).reshape(y.shape)
    return _out(y, sq)


def convT2x2s2(x, w):
    """y[2 i + kh, 2 j + kw, o] = sum_c x[i, j, c] W[c, o, kh, kw]"""
    xb, sq = _bhwc(x)
    w = np.asarray(w).astype(np.float64)
    B, H, W, C = xb.shape
    O = w.shape[1]
    assert w.shape == (C, O, 2, 2)
    y = np.zeros((B, 2 * H, 2 * W, O))
    for kh in range(2):
        for kw in range(2):
            y[:, kh::2, kw::2] = (np.ascontiguousarray(xb).reshape(-1, C) @ np.ascontiguousarray(w[:, :, kh, kw])).reshape(B, H, W, O)
    return _out(y, sq)


def abs_bound(x, w):
    """sum |w| |x| per output element of conv3x3(x, w): the scale every rounding error of that convolution is relative to."""
    return conv3x3(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w)))


# ---- weight blobs ----------------------------------------------------------------------------------------------------------

def seq_shapes(in_nc, out_nc, width, nb):
    if nb == 1:
        return [(out_nc, in_nc, 3, 3)]
    return [(width, in_nc, 3, 3)] + [(width, width, 3, 3)] * (nb - 2) + [(out_nc, width, 3, 3)]


def unetres_shapes(in_nc, out_nc, nc, nb):
    """(kind, shape) per layer in the blob's order; kind: '3' Conv2d 3x3, 'd' Conv2d 2x2 stride 2 (OIHW), 'u' ConvTranspose2d 2x2 stride 2 (IOHW)."""
    s = [("3", (nc[0], in_nc, 3, 3))]
    for l in range(3):
        s += [("3", (nc[l], nc[l], 3, 3))] * (2 * nb) + [("d", (nc[l + 1], nc[l], 2, 2))]
    s += [("3", (nc[3], nc[3], 3, 3))] * (2 * nb)
    for l in (3, 2, 1):
        s += [("u", (nc[l], nc[l - 1], 2, 2))] + [("3", (nc[l - 1], nc[l - 1], 3, 3))] * (2 * nb)
    return s + [("3", (out_nc, nc[0], 3, 3))]


def split_blob(w, shapes):
    w = np.asarray(w, np.float32).ravel()
    out, off = [], 0
    for shp in shapes:
        n = int(np.prod(shp))
        out.append(w[off:off + n].reshape(shp))
        off += n
    assert off == w.size, "weight blob size does not match the architecture"
    return out


def join_blob(layers):
    return np.concatenate([np.asarray(a, np.float32).ravel() for a in layers])


def seq_conv(x, w, in_nc, out_nc, width, nb, taps=None):
    """The sequential architecture: conv -> ReLU -> ... -> conv, no ReLU after the last.  taps: list that receives every layer's output."""
    ws = split_blob(w, seq_shapes(in_nc, out_nc, width, nb))
    y = np.asarray(x, np.float64)
    for i, wl in enumerate(ws):
        y = conv3x3(y, wl, relu=i != len(ws) - 1)
        if taps is not None:
            taps.append(y)
    return y


def unetres(x, w, in_nc, out_nc, nc, nb, taps=None):
    """UNetRes in the layer order of the library's layer program (csrc/net_plan.h net_plan_build; tests/test_net_plan_host.py executes that program
    against this function): head; per level nb ResBlocks cur + conv(relu(conv(cur))) then the
    strided conv; body plus skip; per level the transposed conv, ResBlocks plus skip; tail.  taps: receives every tensor a kernel writes."""
    it = iter(split_blob(w, [s for _, s in unetres_shapes(in_nc, out_nc, nc, nb)]))

    def tap(t):
        if taps is not None:
            taps.append(t)
        return t

    def resblocks(cur, skip=None):
        for b in range(nb):
            t = tap(conv3x3(cur, next(it), relu=True))
            cur = cur + conv3x3(t, next(it))
            if skip is not None and b == nb - 1:
                cur = cur + skip
            tap(cur)
        return cur

    xs = [tap(conv3x3(x, next(it)))]                                # x1 = head(x0)
    a = None
    for l in range(3):
        a = resblocks(xs[l])
        xs.append(tap(conv2x2s2(a, next(it))))
    a = resblocks(xs[3], skip=xs[3])
    for l in (3, 2, 1):
        a = tap(convT2x2s2(a, next(it)))
        a = resblocks(a, skip=xs[l - 1])
    return tap(conv3x3(a, next(it)))


# ---- the f16 x 3 operand split ---------------------------------------------------------------------

def split_f16(v):
    """hi = float16(v), lo' = float16((float32(v) - hi) * 2^11); both returned as fp64 values."""
    v32 = np.asarray(v, np.float32)
    hi = v32.astype(np.float16)
    lo = ((v32 - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def weight_scale(w):
    """The per-layer power of two that puts the largest |w| into [1, 2) (conv6_weight_scale)."""
    mx = float(np.abs(np.asarray(w, np.float32)).max())
    if not (mx > 0.0 and np.isfinite(mx)):
        return 1.0
    e = int(np.frexp(np.float32(mx))[1])
    return float(np.ldexp(1.0, min(60, max(-60, 1 - e))))


# ---- input families with an order-independent exact result -------------------------------------------------------------------

BUDGET_X3 = 682          # sum |w| per output element so that sum |w| * 3 < 2^11


def int_weights(rng, cout, cin, budget=BUDGET_X3, levels=(1, 2), fill=1.0):
    """Integer weights in +-levels, OIHW 3x3.  Per output channel: the positions (cin, tap) this channel must cover so that every
    position is non-zero for at least one channel (a cyclic share of one random permutation), plus a random `fill` fraction of the
    others, thinned until sum |w| <= budget."""
    K = 9 * cin
    w = np.zeros((cout, K), np.float32)
    perm = rng.permutation(K)
    share = -(-K // cout)
    lv = np.asarray(levels, np.float32)
    for o in range(cout):
        must = perm[(o * share + np.arange(share)) % K]
        extra = np.setdiff1d(np.arange(K), must)
        extra = rng.permutation(extra)[: int(round(fill * extra.size))]
        pos = np.concatenate([must, extra])                         # (thinning drops from the end: the share survives)
        val = rng.choice(lv, pos.size) * rng.choice(np.float32([-1, 1]), pos.size)
        keep = np.cumsum(np.abs(val)) <= budget
        assert keep[:share].all(), "the budget does not even hold the share that covers every position"
        w[o, pos[keep]] = val[keep]
    return w.reshape(cout, cin, 3, 3)


def family_I_x(rng, shape):
    """small integers 0 .. 3"""
    return rng.integers(0, 4, shape).astype(np.float64)


def family_A_x(rng, shape):
    """fine activations i + k 2^-16, i in {1, 2, 3}, |k| <= 8: hi = i, lo' = k 2^-5 exactly"""
    return rng.integers(1, 4, shape).astype(np.float64) + rng.integers(-8, 9, shape).astype(np.float64) * 2.0 ** -16


def family_B_x(rng, shape):
    """coarse activations 1 .. 3 (no low piece)"""
    return rng.integers(1, 4, shape).astype(np.float64)


def family_B_w(rng, cout, cin):
    """fine weights: the support and signs of int_weights; scaled by the layer's power of two each is +-(j / 2 + k 2^-16), j in {1, 2, 3},
    |k| <= 8 (hi = j / 2, lo' = k 2^-5 exactly), with at least one j >= 2 so that the largest lies in [1, 2).  The blob holds them times 2^-3."""
    s = int_weights(rng, cout, cin, levels=(1,))
    nz = s != 0
    j = rng.integers(1, 4, s.shape).astype(np.float64)
    k = rng.integers(-8, 9, s.shape).astype(np.float64)
    ws = np.where(nz, s * (0.5 * j + k * 2.0 ** -16), 0.0)
    o, c, a, b = np.argwhere(nz)[0]
    ws[o, c, a, b] = s[o, c, a, b] * 1.5
    w = (ws * 0.125).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), ws * 0.125)         # representable in fp32
    return w


def seq_int_blob(rng, in_nc, out_nc, width, nb):
    """Family I weights for the sequential architecture.  First layer: int_weights against inputs <= 3.  Later layers read ReLU outputs in
    the hundreds: +-1 only, each channel's covering share plus little else, so that every tensor stays an integer below 2^11 (the host test
    checks the actual tensors)."""
    shapes = seq_shapes(in_nc, out_nc, width, nb)
    ws = []
    for i, (o, c, _, _) in enumerate(shapes):
        if i == 0:
            ws.append(int_weights(rng, o, c, budget=BUDGET_X3 if nb == 1 else 24))
        else:
            ws.append(int_weights(rng, o, c, budget=-(-9 * c // o) + 1, levels=(1,), fill=0.0 if 9 * c // o >= 8 else 0.01))
    return join_blob(ws)


def routing_blob(rng, in_nc, out_nc, nc, nb, p2=0.0):
    """UNetRes weights that only route: every output channel of every layer (3x3, 2x2 stride-2, transposed) has one weight +-1 at a random
    (cin, tap), with probability p2 a second one.  With integer inputs the whole network is integer arithmetic."""
    ws = []
    for kind, shp in unetres_shapes(in_nc, out_nc, nc, nb):
        w = np.zeros(shp, np.float32)
        nout, nin = (shp[1], shp[0]) if kind == "u" else (shp[0], shp[1])
        for o in range(nout):
            for _ in range(2 if rng.random() < p2 else 1):
                c, a, b = int(rng.integers(nin)), int(rng.integers(shp[2])), int(rng.integers(shp[3]))
                if kind == "u":
                    w[c, o, a, b] = rng.choice(np.float32([-1, 1]))
                else:
                    w[o, c, a, b] = rng.choice(np.float32([-1, 1]))
        ws.append(w)
    return join_blob(ws)


def case_rng(*key):
    """one reproducible generator per (case, family, draw)"""
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def copy_weights(rng, cout, cin):
    """every output channel copies one input channel through one weight 1 at a random tap (a shift by at most one pixel, zeros from the padding):
    with a non-negative input the f16 x 3 kernels reproduce hi + lo' / 2^11 of the copied value, i.e. split_roundtrip(value), exactly"""
    w = np.zeros((cout, cin, 3, 3), np.float32)
    for o in range(cout):
        w[o, (7 * o + 3) % cin, int(rng.integers(3)), int(rng.integers(3))] = 1.0
    return w


def split_roundtrip(v):
    """what the f16 x 3 split keeps of an fp32 value: hi + lo' / 2^11 (22 significant bits and the sign of lo'; representable in fp32)"""
    hi, lo = split_f16(v)
    return hi + lo / 2048.0


def layer_case(case, family):
    """(weight blob, input [H, W, in_nc, B] fp64) of one sequential-architecture case (in_nc, out_nc, width, nb, H, W, B).
    family: 'I', 'A', 'B' (above) or 'R': dense w uniform in +-0.2, x uniform in [0, 1) as fp32 values (single layer).
    A and B are single-layer families; with nb = 3 they sit in the middle layer, between two layers of copy_weights that carry the values through
    the interior tensors (positive values: the ReLU after the first layer changes nothing)."""
    in_nc, out_nc, width, nb, H, W, B = case
    rng = case_rng(case, family)
    shape = (H, W, in_nc, B)
    if family == "I":
        return seq_int_blob(rng, in_nc, out_nc, width, nb), family_I_x(rng, shape)
    assert nb in (1, 3), "families A, B and R are single-layer families"
    mid = (width, width) if nb == 3 else (out_nc, in_nc)
    if family == "A":
        w, x = int_weights(rng, *mid), family_A_x(rng, shape)
    elif family == "B":
        w, x = family_B_w(rng, *mid), family_B_x(rng, shape)
    elif family == "R" and nb == 1:
        w = ((rng.random(out_nc * in_nc * 9) - 0.5) * 0.4).astype(np.float32)
        x = rng.random(shape, dtype=np.float32).astype(np.float64)
    else:
        raise ValueError(family)
    if nb == 3:
        return join_blob([copy_weights(rng, width, in_nc), w, copy_weights(rng, out_nc, width)]), x
    return w.ravel(), x


def unetres_nparams(in_nc, out_nc, nc, nb):
    return sum(int(np.prod(s)) for _, s in unetres_shapes(in_nc, out_nc, nc, nb))


def eta(y, y64, bound):
    """largest error of y per output element, relative to that element's sum |w||x|"""
    return float((np.abs(np.asarray(y, np.float64) - y64) / bound).max())


def channel_err(y, y64):
    """per output channel (axis 2): max |y - y64| / max |y64| over that channel"""
    ax = tuple(i for i in range(y64.ndim) if i != 2)
    return np.abs(np.asarray(y, np.float64) - y64).max(axis=ax) / np.abs(y64).max(axis=ax)
