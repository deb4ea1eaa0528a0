"""Every 3x3 launch form, one layer at a time, and whole small UNets, against the exact fp64 restatement (tests/conv_ref.py).

The end-to-end parity tests (test_gpu_net.py, test_gpu_grids.py) judge a forward pass by one relative L2 per image against an fp32 oracle: a
wrong halo pixel, a lost cross term of the f16 x 3 split in one pixel block or a wrong small-valued channel passes them.  Here

* QMRI_ARCH_SEQ_CONV with nb = 1 is exactly one bias-free 3x3 convolution, with nb = 3 it adds ReLU and blocked interior tensors: the table
  CASES reaches each branch of conv6_choose_form (csrc/conv6_form.h, the function conv6_launch executes) in isolation at the smallest shape
  that takes it.  launch_form() restates those branches, because the forms are needed here without the library's source at hand and as an
  independent statement; tests/test_conv_ref_host.py checks, without a GPU, the table against launch_form() and launch_form() against
  conv6_choose_form itself, compiled for the host, on every row, every knob setting below and a sweep of shapes;
* the inputs come from families whose exact result does not depend on the order of summation (conv_ref: I small integers, A coarse weights x
  fine activations, B fine weights x coarse activations; the host test proves the premises shape by shape), so the assertion is equality of
  bits -- np.array_equal for I, bits == float32(exact fp64 value) for A and B on forms that round once;
* split-K forms round more than once: k_conv6 stores ksplit partial sums, each rounded once (the epilogue's v * descale_hi + accl * descale_lo
  of exact accumulators), and k_conv6_reduce{,_blk} adds them in slice order with ksplit - 1 further roundings.  Every partial passes through
  at most ksplit roundings, so |y - exact| <= ((1 + 2^-24)^ksplit - 1) * sum |w||x|, asserted as ksplit * 2^-24 * (1 + 2^-20) * abs_bound.
  Family I stays bit-exact there;
* every run asserts denoiser_scheme() == (2, 0): without it a subtly wrong f16 kernel would change which kernel runs (the set-up probe moves
  the network to bf16 x 6) instead of failing.

* beyond the single-layer rows, families A and B also run through the rows with nb = 3, in the middle layer between two layers that only copy
  (conv_ref.layer_case), so that the blocked-tensor loaders and epilogues see operands with a low piece too -- family I has none, and a wrong
  cross-term scale in a blocked epilogue is invisible to it.

Per-element accuracy with dense random weights (w uniform in +-0.2, x uniform in [0, 1) as fp32 values): eta(y) = max over outputs of
|y - y64| / sum |w||x|, in units of u = 2^-24; rho = eta_gpu / eta_ref with eta_ref from oracle.Net (plain sequential fp32 FMA chain).
Measured with the library of commit e99f089 on one MI355X (eta_gpu u / eta_ref u / rho on the default f16 x 3 path; rho under conv_scheme=3):

    cfg0_16to64_64x64_B10                1.90  5.47  0.346    0.738
    cfg1_16to64_64x64_B5                 1.67  5.28  0.316    0.630
    cfg2_16to16_24x24                    0.89  2.74  0.324    0.756
    cfg2_16to16_17x9_scalar_epilogue     0.95  1.83  0.518    0.959
    cfg2_10to10_32x32_narrow             1.64  2.68  0.612    1.278
    cfg2_11to10_32x32_narrow             1.73  3.23  0.534    0.988
    splitk_256to64_16x16                 0.44  2.73  0.161    0.329
    splitk_256to64_16x16_B2              0.41  2.90  0.142    0.330
    splitk_512to128_16x16                0.46  3.94  0.118    0.285
    splitk_512to128_16x16_B2             0.43  3.22  0.133    0.340
    splitk_256to72_24x20                 0.40  2.96  0.134    0.302
    splitk_256to72_24x20_B2              0.52  3.43  0.152    0.295
    splitk_256to64_18x14_scalar_reduce   0.42  2.53  0.164    0.352
    cfg3_unsplit_256to64_40x40           1.53  4.22  0.363    0.808
    cfg2_64to64_32x32                    1.25  3.30  0.379    0.820
    cfg2_65to64_32x32                    1.56  3.37  0.464    0.974
    cfg2_72to64_32x32                    1.70  3.62  0.469    1.072
    cfg2_80to64_32x32                    1.82  4.66  0.390    0.894

The kernels are more accurate than the sequential chain (the matrix cores add 16 products at a time, split-K adds four partial sums).  Largest rho
on the default path 0.612, so M_RATIO = 2 (twice that, rounded up to a power of two).  Per output channel (max |y - y64| / max |y64| of the channel)
the largest gpu / oracle ratio was 0.945 on these rows; on the whole small UNets 0.91 on f16 x 3 and 1.69 on bf16 x 6.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import conv_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24

# ---- conv6_choose_form restated (csrc/conv6_form.h; held against it by tests/test_conv_ref_host.py), so that a row names its form without a GPU ----

KNOB_DEFAULTS = dict(conv_splitk=1, conv_persist=1, conv_midcfg=3, conv_deepcfg=3, conv_deepks=4, conv_f32=0, conv_scheme=2)
TILE = {0: (16, 16), 1: (16, 8), 2: (8, 8), 3: (16, 8)}
NCU = 256                                                           # MI355X: k_conv6p runs when a launch has more tiles than CUs


def parse_knobs(s):
    k = dict(KNOB_DEFAULTS)
    for kv in filter(None, s.split(",")):
        name, v = kv.split("=")
        k[name] = int(v)
    return k


def launch_form(cin, cout, H, W, B, blk, knobs=KNOB_DEFAULTS):
    """(cfg, ksplit, persistent) of one 3x3 layer; blk: input AND output blocked."""
    nchunk, n_ct = -(-cin // 16), -(-cout // 64)

    def ntiles(th, tw):
        return n_ct * -(-H // th) * -(-W // tw) * B

    def waste(th, tw):
        return (-(-H // th) * th) * (-(-W // tw) * tw) / (H * W)

    def persistent(cfg):                                            # k_conv6p: f16 scheme, blocked tensors, more tiles than CUs
        return bool(knobs["conv_persist"] and knobs["conv_scheme"] == 2 and cout % 64 == 0 and nchunk >= 4 and nchunk % 2 == 0 and blk and
                    ntiles(*TILE[cfg]) > NCU)

    if ntiles(16, 16) >= 160 and waste(16, 16) <= 1.35:
        return 0, 1, persistent(0)
    if ntiles(16, 8) >= 160 and waste(16, 8) <= 1.35:
        return 1, 1, persistent(1)
    deep = H * W <= 32 * 32
    cfg = knobs["conv_deepcfg"] if deep else knobs["conv_midcfg"]
    if knobs["conv_splitk"] and nchunk >= 16:
        nt = ntiles(*TILE[cfg]) * (2 if cfg == 3 else 1)
        ks = 1
        while ((deep or cfg < 2) and cfg >= 0 and ks * 2 * nt <= 256 and ks * 2 <= (knobs["conv_deepks"] if deep else 8) and
               nchunk % (ks * 2) == 0 and nchunk // (ks * 2) >= 4):
            ks *= 2
        if ks > 1 and H * W <= 64 * 64:
            return cfg, ks, False
    if nchunk >= 16 and cout % 64 == 0 and cfg == 3:
        return 3, 1, False
    return 2, 1, False


def case_forms(case, knobs=KNOB_DEFAULTS):
    """launch_form of every layer of a sequential-architecture case.  Interior tensors are blocked when nb > 1 and width % 8 == 0
    (qmri_set_denoiser: blk_ok); the network's input and output are planar."""
    in_nc, out_nc, width, nb, H, W, B = case
    shapes = R.seq_shapes(in_nc, out_nc, width, nb)
    blk = nb > 1 and width % 8 == 0
    return [launch_form(c, o, H, W, B, blk and 0 < i < len(shapes) - 1, knobs) for i, (o, c, _, _) in enumerate(shapes)]


def fmt_form(f):
    return f"cfg{f[0]}" + (f"/ks{f[1]}" if f[1] > 1 else "") + ("/persistent" if f[2] else "")


# ---- the table: (id, (in_nc, out_nc, width, nb, H, W, B), the form of the layer the row is about under the default knobs) ------------------------
# n_ct = ceil(Cout / 64) weight tiles, nchunk = ceil(Cin / 16) K chunks; ntiles(th, tw) = n_ct * ceil(H / th) * ceil(W / tw) * B.
CASES = [
    # 1 * 4 * 4 * 10 = 160 tiles of 16 x 16, no overhang: the first branch of conv6_choose_form, configuration 0; planar in and out so not persistent
    ("cfg0_16to64_64x64_B10", (16, 64, 64, 1, 64, 64, 10), "cfg0"),
    # B = 5: 80 tiles of 16 x 16 (< 160), 1 * 4 * 8 * 5 = 160 of 16 x 8: second branch, configuration 1
    ("cfg1_16to64_64x64_B5", (16, 64, 64, 1, 64, 64, 5), "cfg1"),
    # few tiles and nchunk = 1 < 16: neither split-K nor configuration 3, the last line, configuration 2; H % 4 == 0: float4 epilogue, 24 = 3 tiles of 8
    ("cfg2_16to16_24x24", (16, 16, 16, 1, 24, 24, 1), "cfg2"),
    # H = 17: vec4 = 0, the scalar epilogue; 17 x 9 leaves ragged 8 x 8 tiles in both directions
    ("cfg2_16to16_17x9_scalar_epilogue", (16, 16, 16, 1, 17, 9, 1), "cfg2"),
    # Cin <= 64: conv_plan_layer renames the layer CONV_3X3N (32-channel chunks of the f32-MFMA packing, and the tensors' channel padding);
    # 10 and 11 input channels fill one 16-channel chunk partly; Cout = 10 is a partial 64-row tile
    ("cfg2_10to10_32x32_narrow", (10, 10, 16, 1, 32, 32, 1), "cfg2"),
    ("cfg2_11to10_32x32_narrow", (11, 10, 16, 1, 32, 32, 1), "cfg2"),
    # nchunk = 16, 256 px <= 32 * 32: deep, conv_deepcfg = 3, nt = 2 * ntiles(16, 8) = 4 B; K over 2 and 4 pass (4 <= conv_deepks, 16 / 4 = 4 chunks
    # each), 8 does not: configuration 3 with ksplit = 4 into planar partials, k_conv6_reduce<true> (H % 4 == 0, planar output)
    ("splitk_256to64_16x16", (256, 64, 64, 1, 16, 16, 1), "cfg3/ks4"),
    ("splitk_256to64_16x16_B2", (256, 64, 64, 1, 16, 16, 2), "cfg3/ks4"),
    # nchunk = 32, n_ct = 2: nt = 8 B, K over 4 (conv_deepks)
    ("splitk_512to128_16x16", (512, 128, 64, 1, 16, 16, 1), "cfg3/ks4"),
    ("splitk_512to128_16x16_B2", (512, 128, 64, 1, 16, 16, 2), "cfg3/ks4"),
    # Cout = 72: n_ct = 2 with 8 rows in the second weight tile (its upper 32-row half computes nothing that is stored); 24 x 20 = 2 x 3 tiles of
    # 16 x 8, ragged in both directions; nt = 24 B, K over 4 while 4 * 24 B <= 256: B = 1 and 2
    ("splitk_256to72_24x20", (256, 72, 64, 1, 24, 20, 1), "cfg3/ks4"),
    ("splitk_256to72_24x20_B2", (256, 72, 64, 1, 24, 20, 2), "cfg3/ks4"),
    # H = 18: k_conv6_reduce<false>, the scalar reduce, and the scalar epilogue of the partial stores
    ("splitk_256to64_18x14_scalar_reduce", (256, 64, 64, 1, 18, 14, 1), "cfg3/ks4"),
    # 1600 px > 32 * 32: the mid level, conv_midcfg = 3; the split loop needs deep or cfg < 2, so ksplit stays 1 and the unsplit rule takes
    # configuration 3 (nchunk >= 16, Cout % 64 == 0)
    ("cfg3_unsplit_256to64_40x40", (256, 64, 64, 1, 40, 40, 1), "cfg3"),
    # the narrow / wide boundary (Cin <= 64 renames the layer) and K tails: nchunk = 4, 5, 5, 5 with 1, 8 and 16 channels in the last chunk
    ("cfg2_64to64_32x32", (64, 64, 64, 1, 32, 32, 1), "cfg2"),
    ("cfg2_65to64_32x32", (65, 64, 64, 1, 32, 32, 1), "cfg2"),
    ("cfg2_72to64_32x32", (72, 64, 64, 1, 32, 32, 1), "cfg2"),
    ("cfg2_80to64_32x32", (80, 64, 64, 1, 32, 32, 1), "cfg2"),
    # nb = 3: planar -> blocked, blocked -> blocked, blocked -> planar.  Middle layer: 1 * 4 * 4 * 17 = 272 tiles of 16 x 16 > 256 CUs, nchunk = 4
    # (even, >= 4), Cout % 64 == 0, blocked: k_conv6p on configuration 0, 16 workgroups walk two tiles
    ("persistent_w64_64x64_B17", (16, 64, 64, 3, 64, 64, 17), "cfg0/persistent"),
    # width 128: n_ct = 2, 2 * 16 * 9 = 288 tiles, nchunk = 8
    ("persistent_w128_64x64_B9", (16, 64, 128, 3, 64, 64, 9), "cfg0/persistent"),
    # the one-launch-per-layer kernel with blocked tensors on the same tiles: 160 tiles of 16 x 16 are not more than the CUs, so k_conv6 runs
    ("cfg0_blocked_w64_64x64_B10", (16, 64, 64, 3, 64, 64, 10), "cfg0"),
    # ... and 160 tiles of 16 x 8 (80 of 16 x 16): configuration 1, blocked in and out -- the form of the 112 x 112 level of a one-slice 224 x 224 pass
    ("cfg1_blocked_w64_64x64_B5", (16, 64, 64, 3, 64, 64, 5), "cfg1"),
    # configuration 3 unsplit with blocked tensors (the 56 x 56 level's form): middle layer 256 -> 256 at 40 x 40, n_ct = 4, two workgroups per weight tile
    ("cfg3_blocked_w256_40x40", (16, 16, 256, 3, 40, 40, 1), "cfg3"),
    # width 24: blocked interior (24 % 8 == 0), three channel blocks, Cin = 24 is 1.5 chunks; 40 x 24 = 5 x 3 tiles of 8 x 8
    ("blocked_w24_40x24", (10, 10, 24, 3, 40, 24, 1), "cfg2"),
    # width 20: not a multiple of 8, planar interior
    ("planar_w20_40x24", (10, 10, 20, 3, 40, 24, 1), "cfg2"),
    # blocked split-K: the middle layer 256 -> 256 at 16 x 16 is deep, n_ct = 4, nt = 16, K over 4, k_conv6_reduce_blk (blocked output)
    ("splitk_blocked_w256_16x16", (16, 16, 256, 3, 16, 16, 1), "cfg3/ks4"),
]
CASE_IDS = [c[0] for c in CASES]


def case_layer(case):
    """index of the layer a row is about: the only one, or the middle one"""
    return 0 if case[3] == 1 else 1


def families(case):
    return ("I", "A", "B")


_REF = {}


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def reference(case, family):
    """dict(w, x, y64: the exact fp64 result, once: the output of a form that rounds once, bound: sum |w||x| of the layer that rounds (families A, B
    and R), ab: that layer's (weights, input) for the host test).  Computed once per process, read-only afterwards.
    With nb = 3, families A and B sit in the middle layer between two copying layers (conv_ref.layer_case): the first hands the input on exactly, the
    middle layer's fp32 output passes the ReLU, and the last layer returns what the f16 x 3 split keeps of it, split_roundtrip, exactly."""
    key = (case, family)
    if key not in _REF:
        in_nc, out_nc, width, nb, H, W, B = case
        w, x = R.layer_case(case, family)
        r = dict(w=w, x=x, bound=None, ab=None)
        if family == "I":
            r["y64"] = R.seq_conv(x, w, in_nc, out_nc, width, nb)
            r["once"] = r["y64"]
        elif nb == 1:
            wl = w.reshape(out_nc, in_nc, 3, 3)
            r["y64"] = R.conv3x3(x, wl)
            r["once"], r["bound"], r["ab"] = f32(r["y64"]), R.abs_bound(x, wl), (wl, x)
        else:
            w1, w2, w3 = R.split_blob(w, R.seq_shapes(in_nc, out_nc, width, nb))
            t1 = R.conv3x3(x, w1)                                    # a copy: exact
            t2 = R.conv3x3(t1, w2)
            r["y64"] = R.conv3x3(np.maximum(t2, 0.0), w3)
            r["once"] = R.conv3x3(R.split_roundtrip(np.maximum(f32(t2), 0.0)), w3)
            r["bound"], r["ab"] = R.conv3x3(R.abs_bound(t1, w2), w3), (w2, t1)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def run_layers(e, case, family):
    """one case on the engine: (output, scheme after set_denoiser, scheme after the call)"""
    in_nc, out_nc, width, nb, H, W, B = case
    w, x = R.layer_case(case, family)
    e.set_denoiser(w, H, W, in_nc=in_nc, out_nc=out_nc, nc=(width, 0, 0, 0), nb=nb, arch=1, max_batch=B)
    s0 = e.denoiser_scheme()
    y = e.denoise(x)
    return y, s0, e.denoiser_scheme()


def check_layers(name, case, family, y, knobs=KNOB_DEFAULTS):
    """the family's assertion for the form the row takes under these knobs"""
    r = reference(case, family)
    y64, want = r["y64"], r["once"]
    assert y.shape == y64.shape and np.isfinite(y).all() and np.abs(y64).max() > 0
    forms = case_forms(case, knobs)
    ks = forms[case_layer(case)][1] if family != "I" else 1         # (families A and B round in the layer the row is about; family I nowhere)
    if family == "I":
        assert np.array_equal(y64, f32(y64))
    if knobs["conv_f32"] or knobs["conv_scheme"] == 3:
        assert family == "I"
    once = ks == 1
    d = np.abs(y - want) if once else np.abs(y - y64)
    worst = np.unravel_index(int(np.argmax(d)), d.shape)
    msg = f"{name} family {family} [{'+'.join(fmt_form(f) for f in forms)}]: max |y - exact| {d.max():.3g} at (h, w, c, b) {worst}, {int((d > 0).sum())} elements differ"
    if once:
        assert np.array_equal(y, want), msg
    else:                                                           # split-K: ksplit roundings per partial (module docstring); nb = 3: and the last layer's split of the value, 2^-22
        tol = ks * U * (1 + 2.0 ** -20) * r["bound"] + (2.0 ** -22 * np.abs(y64) if case[3] > 1 else 0.0)
        assert (d <= tol).all(), msg + f", largest error / bound {(d / tol).max():.3g}"


# ---- part 3: the table in this process (default knobs) --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,case,form", CASES, ids=CASE_IDS)
def test_layer_forms_exact_families(engine_mod, name, case, form):
    assert fmt_form(case_forms(case)[case_layer(case)]) == form     # the row reaches the form it names (by the restated launch rules)
    e = engine_mod.Engine(0)
    for fam in families(case):
        y, s0, s1 = run_layers(e, case, fam)
        assert s0 == (2, 0) and s1 == (2, 0), (name, fam, s0, s1)   # f16 x 3 kernels, neither the probe nor a guard moved the network
        check_layers(name, case, fam, y)
    e.close()


_CHILD = (
    "import sys, numpy as np\n"
    "sys.path[:0] = [%r, %r]\n"
    "import test_gpu_conv_layers as T\n"
    "from qmri_pnp_recon_poc_amd import engine as E\n"
    "T.child_main(E, sys.argv[1], sys.argv[2])\n" % (ROOT, os.path.join(ROOT, "tests")))


def child_main(E, mode, out):
    res = {}
    e = E.Engine(0)
    if mode == "layers":
        for name, case, _ in CASES:
            for fam in families(case) + (("R",) if case[3] == 1 else ()):
                y, s0, s1 = run_layers(e, case, fam)
                res[f"{name}:{fam}"] = y.astype(np.float32)         # (fp32 values in a double array: nothing is lost)
                res[f"{name}:{fam}:scheme"] = np.array(s0 + s1)
    else:
        for name, net, hw, in_nc in UNET_CASES:
            for draw in range(N_DRAWS):
                y, s, h = run_unet(e, net, hw, in_nc, draw, 1)
                res[f"{name}:{draw}"] = y.astype(np.float32)
                res[f"{name}:{draw}:state"] = np.array(s + (int(h["resident_tile_launch_armed"]), h["resident_tile_timeouts"]))
    e.close()
    np.savez(out, **res)


def run_child(mode, knobs):
    """one fresh process per setting, under its own time limit; a failing one raises"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "y.npz")
        env = dict(os.environ)
        if knobs:
            env["QMRI_DEBUG"] = knobs
        r = subprocess.run([sys.executable, "-c", _CHILD, mode, out], env=env, timeout=240, capture_output=True, text=True)
        assert r.returncode == 0, (knobs, r.returncode, r.stderr[-3000:])
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


LAYER_KNOBS = ["conv_scheme=3", "conv_f32=1", "conv_splitk=0", "conv_persist=0", "conv_wt=0", "conv_xcd=0",
               "conv_midcfg=0,conv_deepcfg=0,conv_deepks=8", "conv_midcfg=1,conv_deepcfg=1", "conv_midcfg=2,conv_deepcfg=2,conv_deepks=2"]


@pytest.mark.parametrize("setting", LAYER_KNOBS)
def test_layer_forms_under_knobs(oracle, setting):
    """The same table in a fresh process per knob setting (the knobs are read when the plan is made).  bf16 x 6 and the f32-MFMA kernels: family I
    bit-exact; every other setting keeps the f16 x 3 scheme and must pass all families on whatever form the knob selects."""
    knobs = parse_knobs(setting)
    res = run_child("layers", setting)
    other_arith = knobs["conv_scheme"] == 3 or knobs["conv_f32"]
    want = (3, 0, 3, 0) if knobs["conv_scheme"] == 3 else (2, 0, 2, 0)   # (conv_scheme=3 itself selects the bf16 scheme)
    for name, case, _ in CASES:
        for fam in families(case):
            assert tuple(res[f"{name}:{fam}:scheme"]) == want, (setting, name, fam, res[f"{name}:{fam}:scheme"])
            if fam == "I" or not other_arith:
                check_layers(f"{setting} {name}", case, fam, res[f"{name}:{fam}"].astype(np.float64), knobs)
        if case[3] == 1:                                            # the a-priori per-element bound holds on every arithmetic; rho is reported
            eg, er = accuracy(oracle, case, res[f"{name}:R"].astype(np.float64))[:2]
            print(f"{setting} {name}: eta_gpu {eg / U:.2f} u, eta_ref {er / U:.2f} u, rho {eg / er:.3f}")
            assert eg <= (9 * case[0] + 8) * U, (setting, name, eg / U)


# ---- part 4: per-element accuracy with dense random weights --------------------------------------------------------------------------------

M_RATIO = 2         # eta_gpu <= M_RATIO * eta_ref: twice the largest rho measured on the default path, rounded up to a power of two (module docstring)

_ACC = {}


def accuracy(oracle, case, y):
    """(eta_gpu, eta_ref, per-channel error gpu, per-channel error ref); the oracle's forward is computed once per case"""
    in_nc, out_nc, width, nb, H, W, B = case
    r = reference(case, "R")
    w, x, y64, bound = r["w"], r["x"], r["y64"], r["bound"]
    if case not in _ACC:
        yo = oracle.Net(w, in_nc=in_nc, out_nc=out_nc, nc=(width, 0, 0, 0), nb=1, arch=1).denoise(x)
        _ACC[case] = (R.eta(yo, y64, bound), R.channel_err(yo, y64))
    return R.eta(y, y64, bound), _ACC[case][0], R.channel_err(y, y64), _ACC[case][1]


@pytest.mark.parametrize("name,case,form", [c for c in CASES if c[1][3] == 1], ids=[c[0] for c in CASES if c[1][3] == 1])
def test_layer_per_element_accuracy(engine_mod, oracle, name, case, form):
    """Dense random weights: no element may be further from the fp64 result than an fp32 accumulation of K = 9 Cin terms allows (a-priori:
    (K - 1) roundings of the sum, the split's 2^-22 per product and the final rounding, (9 Cin + 8) 2^-24 in all, relative to sum |w||x|),
    nor M_RATIO times further than the plain sequential fp32 oracle is; the same per output channel relative to that channel's own maximum, so
    that a small-valued channel counts for itself."""
    e = engine_mod.Engine(0)
    y, s0, s1 = run_layers(e, case, "R")
    e.close()
    assert s0 == (2, 0) and s1 == (2, 0)
    eg, er, cg, cr = accuracy(oracle, case, y)
    print(f"{name} [{form}]: eta_gpu {eg / U:.2f} u, eta_ref {er / U:.2f} u, rho {eg / er:.3f}; per channel: gpu {cg.max():.3g}, ref {cr.max():.3g}, "
          f"largest ratio {(cg / cr).max():.3f}")
    assert er > 0 and eg <= (9 * case[0] + 8) * U
    assert eg <= M_RATIO * er
    assert (cg <= M_RATIO * cr).all(), (cg / cr).max()


# ---- part 5: whole small UNets, the resident-tile launch included ----------------------------------------------------------------------------
# nc[0] = 64 is what k_conv6r needs (conv6r_try: 64 -> 64 ResBlock layers, H and W multiples of 16); the other widths are the smallest
# qmri_set_denoiser takes with blocked tensors.  B = 1: head + ResBlocks in one resident launch, ResBlocks + tail in another (2 x 2, 3 x 2 and
# 2 x 3 tiles: every tile a corner or an edge, the non-square ones catch a transposed seam).  The level's down-sampling convolution joins the first
# launch only when it is 64 -> 128 (conv6r_try), hence the second network; in the first it runs as k_conv6s.  B = 3: one launch per layer.
NET_SMALL = ((64, 16, 16, 16), 1)
NET_DOWN = ((64, 128, 16, 16), 1)
NET_NB2 = ((64, 16, 16, 16), 2)
N_DRAWS = 8                                                         # one draw touches Cout of a layer's 9 Cin positions
UNET_CASES = [(f"{'x'.join(map(str, nc))}_nb{nb}_{hw[0]}x{hw[1]}_{in_nc}ch", (nc, nb), hw, in_nc)
              for (nc, nb), hws, in_ncs in ((NET_SMALL, ((32, 32), (48, 32), (32, 48)), (10, 11, 20)), (NET_DOWN, ((48, 32), (32, 48)), (10,)),
                                            (NET_NB2, ((32, 48),), (11,)))
              for hw in hws for in_nc in in_ncs]
UNET_IDS = [c[0] for c in UNET_CASES]
P2 = {1: 0.25, 2: 0.0}                                              # second weights per channel, by nb (the host test proves |tensor| < 2^11)


def unet_case(net, hw, in_nc, draw):
    """routing weights and an input in {1, 2, 3}, batch of three (slice 0 is the B = 1 input)"""
    (nc, nb) = net
    rng = R.case_rng(net, hw, in_nc, draw)
    return R.routing_blob(rng, in_nc, 10, nc, nb, p2=P2[nb]), rng.integers(1, 4, (hw[0], hw[1], in_nc, 3)).astype(np.float64)


def run_unet(e, net, hw, in_nc, draw, B, wx=None):
    (nc, nb) = net
    w, x = wx if wx is not None else unet_case(net, hw, in_nc, draw)
    e.set_denoiser(w, hw[0], hw[1], in_nc=in_nc, out_nc=10, nc=nc, nb=nb, max_batch=3)
    s0 = e.denoiser_scheme()
    y = e.denoise(x[..., 0] if B == 1 else x[..., :B])
    return y, s0 + e.denoiser_scheme(), e.health()


_UREF = {}


def unet_reference(net, hw, in_nc, draw):
    key = (net, hw, in_nc, draw)
    if key not in _UREF:
        w, x = unet_case(net, hw, in_nc, draw)
        y = R.unetres(x, w, in_nc, 10, net[0], net[1])
        y.setflags(write=False)
        _UREF[key] = y
    return _UREF[key]


@pytest.mark.parametrize("name,net,hw,in_nc", UNET_CASES, ids=UNET_IDS)
def test_unet_routing_weights_exact(engine_mod, name, net, hw, in_nc):
    """Every tensor of the network is an integer below 2^11: any wrong halo, ring-exchange chunk, skip operand or stride-2 index changes an output
    element by at least 1.  B = 1 on the resident-tile launches, B = 3 with one launch per layer."""
    e = engine_mod.Engine(0)
    for draw in range(N_DRAWS):
        y64 = unet_reference(net, hw, in_nc, draw)
        assert np.abs(y64).max() > 0
        for B in (1, 3):
            y, s, h = run_unet(e, net, hw, in_nc, draw, B)
            assert s == (2, 0, 2, 0), (name, draw, B, s)
            assert h["resident_tile_launch_armed"] and h["resident_tile_timeouts"] == 0, (name, draw, B, h)
            want = y64[..., 0] if B == 1 else y64
            d = np.abs(y - want)
            assert np.array_equal(y, want), f"{name} draw {draw} B {B}: {int((d > 0).sum())} elements differ, max {d.max():.3g} at {np.unravel_index(int(np.argmax(d)), d.shape)}"
    e.close()


@pytest.mark.parametrize("setting", ["res_head=0", "res_tail=0", "res_down=0", "res_pipe=0", "conv_resident=0"])
def test_unet_routing_weights_exact_under_knobs(setting):
    """The one-slice runs again in a fresh process per knob of the resident-tile launch: head / tail / down-sampling convolution kept out of it,
    the ring exchange not pipelined, the launch off."""
    res = run_child("unet", setting)
    armed = 0 if setting == "conv_resident=0" else 1
    for name, net, hw, in_nc in UNET_CASES:
        for draw in range(N_DRAWS):
            assert tuple(res[f"{name}:{draw}:state"]) == (2, 0, 2, 0, armed, 0), (setting, name, draw, res[f"{name}:{draw}:state"])
            y, want = res[f"{name}:{draw}"].astype(np.float64), unet_reference(net, hw, in_nc, draw)[..., 0]
            assert np.array_equal(y, want), f"{setting} {name} draw {draw}: {int((y != want).sum())} elements differ"


DENSE_AMPLITUDES = (0.25, 0.125)


@pytest.mark.parametrize("name,net,hw,in_nc", UNET_CASES, ids=UNET_IDS)
def test_unet_dense_weights_per_channel(engine_mod, oracle, name, net, hw, in_nc):
    """Dense random weights, uniform in +-0.25: per output channel, the largest error against the fp64 network must not exceed M_RATIO times the fp32
    oracle's own.  A 64-channel layer of such weights has a gain of about 3, so some of these networks leave the range the f16 split carries
    (6e4; inputs are rescaled to unit scale, so a smaller input does not help) and run on bf16 x 6, by the set-up probe or by the range guard --
    rightly, but then the f16 kernels and the resident launch are not what is measured.  Where the fp64 network says so (a tensor above 3e4: half
    the range, because the set-up probe judges on an input of its own) the case is repeated with +-0.125, and the first amplitude that fits must
    stay on f16 x 3 with the resident launch armed."""
    (nc, nb) = net
    e = engine_mod.Engine(0)
    fits = False
    for amp in DENSE_AMPLITUDES:
        rng = R.case_rng("dense", net, hw, in_nc, amp)
        w = ((rng.random(R.unetres_nparams(in_nc, 10, nc, nb)) - 0.5) * 2 * amp).astype(np.float32)
        x = rng.random((hw[0], hw[1], in_nc, 3), dtype=np.float32).astype(np.float64)
        taps = []
        y64 = R.unetres(x, w, in_nc, 10, nc, nb, taps=taps)
        peak = max(float(np.abs(t).max()) for t in taps)
        fits = peak < 3e4
        yo = oracle.Net(w, in_nc=in_nc, out_nc=10, nc=nc, nb=nb).denoise(x)
        for B in (1, 3):
            y, s, h = run_unet(e, net, hw, in_nc, 0, B, wx=(w, x))
            sl = (Ellipsis, slice(0, 1)) if B == 1 else (Ellipsis,)
            eg = np.abs(y.reshape(y64[sl].shape) - y64[sl]).max(axis=(0, 1, 3))
            er = np.abs(yo[sl] - y64[sl]).max(axis=(0, 1, 3))
            print(f"{name} +-{amp} B {B}: largest |tensor| {peak:.3g}, scheme {s}, per-channel max |err| gpu {eg.max():.3g} ref {er.max():.3g}, "
                  f"largest ratio {(eg / er).max():.3f}")
            assert (er > 0).all() and (eg <= M_RATIO * er).all(), (name, amp, B, (eg / er).max())
            if fits:
                assert s == (2, 0, 2, 0) and h["resident_tile_launch_armed"] and h["resident_tile_timeouts"] == 0, (name, amp, B, s, h)
        if fits:
            break
    e.close()
    assert fits, "no amplitude keeps this network inside the f16 range"
