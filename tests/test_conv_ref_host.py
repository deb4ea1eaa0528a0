"""CPU proofs behind tests/test_gpu_conv_layers.py: the fp64 restatement (tests/conv_ref.py) agrees with the oracle, the table's rows take
the launch forms they name (by the restated launch rules, launch_form()), those restated rules give what the library's own decision
function gives (conv6_choose_form of csrc/conv6_form.h, compiled for the host into tests/cpp/conv6_form_test.cpp), and every exact input
family satisfies, shape by shape, the conditions under which its result does not depend on the order of summation."""
import os
import subprocess

import numpy as np
import pytest

import conv_ref as R
import test_gpu_conv_layers as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _is_int(a, q=1.0):
    return np.array_equal(np.round(a / q), a / q)


# ---- the restatement against the oracle, to fp32 rounding ------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_nc,out_nc,width,nb,H,W", [(10, 10, 32, 1, 17, 9), (11, 7, 20, 3, 12, 16), (16, 16, 24, 4, 24, 8)])
def test_seq_conv_restatement_vs_oracle(oracle, in_nc, out_nc, width, nb, H, W):
    rng = np.random.default_rng(nb)
    n = sum(int(np.prod(s)) for s in R.seq_shapes(in_nc, out_nc, width, nb))
    w = ((rng.random(n) - 0.5) * 0.4).astype(np.float32)
    x = rng.random((H, W, in_nc, 2), dtype=np.float32).astype(np.float64)
    taps = []
    y = R.seq_conv(x, w, in_nc, out_nc, width, nb, taps=taps)
    yo = oracle.Net(w, in_nc=in_nc, out_nc=out_nc, nc=(width, 0, 0, 0), nb=nb, arch=1).denoise(x)
    # fp32 accumulation of K terms per layer: K 2^-24 relative to sum |w||x| <= K * 0.2 * max |input|, layer by layer; 4 x for the layers in front
    K = 9 * max(in_nc, width)
    tol = 4 * nb * K * U * K * 0.2 * max(1.0, max(np.abs(t).max() for t in taps))
    assert y.shape == yo.shape and np.abs(y - yo).max() <= tol
    assert np.abs(y - yo).max() <= 1e-5 * np.abs(y).max()


@pytest.mark.parametrize("in_nc,nc,nb,H,W", [(10, (8, 16, 24, 32), 1, 16, 24), (11, (16, 8, 8, 16), 2, 24, 16), (5, (8, 8, 8, 8), 1, 8, 8)])
def test_unetres_restatement_vs_oracle(oracle, in_nc, nc, nb, H, W):
    rng = np.random.default_rng(H)
    w = ((rng.random(R.unetres_nparams(in_nc, 10, nc, nb)) - 0.5) * 0.5).astype(np.float32)
    x = rng.random((H, W, in_nc, 2), dtype=np.float32).astype(np.float64)
    y = R.unetres(x, w, in_nc, 10, nc, nb)
    yo = oracle.Net(w, in_nc=in_nc, out_nc=10, nc=nc, nb=nb).denoise(x)
    assert y.shape == yo.shape and np.abs(y - yo).max() <= 2e-5 * np.abs(y).max()
    assert np.abs(R.unetres(x[..., 1], w, in_nc, 10, nc, nb) - y[..., 1]).max() <= 1e-13 * np.abs(y).max()      # a batch is its slices


def test_strided_convolutions_index_by_index():
    rng = np.random.default_rng(0)
    x = rng.integers(-3, 4, (4, 6, 3)).astype(np.float64)
    wd = rng.integers(-2, 3, (5, 3, 2, 2)).astype(np.float32)
    wu = rng.integers(-2, 3, (3, 5, 2, 2)).astype(np.float32)
    w3 = rng.integers(-2, 3, (5, 3, 3, 3)).astype(np.float32)
    yd, yu, y3 = R.conv2x2s2(x, wd), R.convT2x2s2(x, wu), R.conv3x3(x, w3)
    xp = np.zeros((6, 8, 3))
    xp[1:-1, 1:-1] = x
    for o in range(5):
        for i in range(2):
            for j in range(3):
                assert yd[i, j, o] == sum(wd[o, c, a, b] * x[2 * i + a, 2 * j + b, c] for c in range(3) for a in range(2) for b in range(2))
        for i in range(4):
            for j in range(6):
                assert y3[i, j, o] == sum(w3[o, c, a, b] * xp[i + a, j + b, c] for c in range(3) for a in range(3) for b in range(3))
                for a in range(2):
                    for b in range(2):
                        assert yu[2 * i + a, 2 * j + b, o] == sum(x[i, j, c] * wu[c, o, a, b] for c in range(3))


def test_split_f16_is_the_design_documents_split():
    v = np.float32([1.0, 3.0 + 8 * 2.0 ** -16, 0.75 - 2.0 ** -16, 1.2345678, -0.1, 2047.0, 6.0e4])
    hi, lo = R.split_f16(v)
    assert np.array_equal(hi, v.astype(np.float16).astype(np.float64))
    assert np.abs(hi + lo / 2048.0 - v.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(v).max()      # 22 significant bits
    assert R.weight_scale(np.float32([0.1, -0.19])) == 8.0 and R.weight_scale(np.float32([2.0, 1.0])) == 0.5 and R.weight_scale(np.float32([1.5])) == 1.0


# ---- the table ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,case,form", G.CASES, ids=G.CASE_IDS)
def test_rows_reach_the_forms_they_name(name, case, form):
    assert G.fmt_form(G.case_forms(case)[G.case_layer(case)]) == form
    in_nc, out_nc, width, nb, H, W, B = case
    assert max(o * c for o, c, _, _ in R.seq_shapes(in_nc, out_nc, width, nb)) <= 512 * 128                # the largest weight tensor
    assert H * W * max(in_nc, out_nc) * B <= 64 * 64 * 64 * 17                                               # the largest input / output


# (row, knob setting, the forms of the row's layers under it)
KNOB_FORMS = [
    ("splitk_512to128_16x16", "conv_midcfg=0,conv_deepcfg=0,conv_deepks=8", ["cfg0/ks8"]),
    ("splitk_256to64_16x16", "conv_midcfg=0,conv_deepcfg=0,conv_deepks=8", ["cfg0/ks4"]),
    ("cfg3_unsplit_256to64_40x40", "conv_midcfg=0,conv_deepcfg=0,conv_deepks=8", ["cfg0/ks4"]),
    ("cfg3_unsplit_256to64_40x40", "conv_midcfg=1,conv_deepcfg=1", ["cfg1/ks4"]),
    ("splitk_256to72_24x20", "conv_midcfg=1,conv_deepcfg=1", ["cfg1/ks4"]),
    ("splitk_256to64_16x16", "conv_midcfg=2,conv_deepcfg=2,conv_deepks=2", ["cfg2/ks2"]),
    ("cfg3_unsplit_256to64_40x40", "conv_midcfg=2,conv_deepcfg=2,conv_deepks=2", ["cfg2"]),
    ("splitk_256to64_16x16", "conv_splitk=0", ["cfg3"]),
    ("splitk_256to72_24x20", "conv_splitk=0", ["cfg2"]),                                  # (configuration 3 unsplit needs Cout % 64 == 0)
    ("persistent_w64_64x64_B17", "conv_persist=0", ["cfg0", "cfg0", "cfg0"]),
    ("splitk_blocked_w256_16x16", "", ["cfg2", "cfg3/ks4", "cfg3/ks4"]),
]


def test_knob_settings_select_other_forms():
    """What the tile knobs do to the deep and mid rows (conv6_choose_form), so that the subprocess runs are known to run something else."""
    cases = dict((c[0], c[1]) for c in G.CASES)
    for name, setting, forms in KNOB_FORMS:
        assert [G.fmt_form(f) for f in G.case_forms(cases[name], G.parse_knobs(setting))] == forms, (name, setting)


# ---- the restatement against the function the library calls ------------------------------------------------------------------------------------

# the reduce kernel each split-K row's comment names (test_gpu_conv_layers.CASES); every other row has none
ROW_REDUCE = {"splitk_256to64_16x16": "float4", "splitk_256to64_16x16_B2": "float4", "splitk_512to128_16x16": "float4", "splitk_512to128_16x16_B2": "float4",
              "splitk_256to72_24x20": "float4", "splitk_256to72_24x20_B2": "float4", "splitk_256to64_18x14_scalar_reduce": "scalar",
              "splitk_blocked_w256_16x16": "blocked"}
REDUCE_KINDS = ["none", "scalar", "float4", "blocked"]


def test_launch_form_restatement_follows_the_library(tmp_path):
    """launch_form() (test_gpu_conv_layers.py) against conv6_choose_form (csrc/conv6_form.h), the function conv6_launch executes, through the
    stand-alone program tests/cpp/conv6_form_test.cpp: every layer of every table row, under the default knobs and under every setting the
    tests use, and a sweep of shapes around every threshold of the decision.  The program first checks by itself what launch_form() does
    not model (residual operands, the format-mismatch code)."""
    exe = tmp_path / "conv6_form_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "conv6_form_test.cpp"), "-o", str(exe)], check=True)
    settings = [""] + sorted(set(G.LAYER_KNOBS) | set(s for _, s, _ in KNOB_FORMS if s))
    rows = []                                                       # (cin, cout, H, W, B, blk, setting, table row or None)
    for setting in settings:
        for name, case, _ in G.CASES:
            in_nc, out_nc, width, nb, H, W, B = case
            shapes = R.seq_shapes(in_nc, out_nc, width, nb)
            for i, (o, c, _, _) in enumerate(shapes):
                blk = nb > 1 and width % 8 == 0 and 0 < i < len(shapes) - 1
                rows.append((c, o, H, W, B, int(blk), setting, name if setting == "" and i == G.case_layer(case) else None))
        sizes = [(n, n) for n in (9, 16, 17, 24, 28, 32, 40, 56, 64, 112, 224)] + [(17, 9), (24, 20), (18, 14), (40, 24)]
        for cin in (10, 16, 64, 65, 80, 256, 512):
            for cout in (10, 64, 72, 128, 256, 512):
                for H, W in sizes:
                    for B in (1, 2, 5, 15, 17, 30):
                        for blk in (0, 1):
                            if not (blk and cout % 8):              # (a blocked tensor holds whole channel blocks)
                                rows.append((cin, cout, H, W, B, blk, setting, None))
    knobs = {s: G.parse_knobs(s) for s in settings}
    text = "".join("%d %d %d %d %d %d " % r[:6] + "%d %d %d %d %d %d\n" % tuple(
        knobs[r[6]][k] for k in ("conv_splitk", "conv_persist", "conv_midcfg", "conv_deepcfg", "conv_deepks", "conv_scheme")) for r in rows)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [tuple(map(int, ln.split())) for ln in r.stdout.splitlines()]
    assert len(got) == len(rows) >= 40000
    seen = set()
    for row, (cfg, ks, persistent, reduce, vec4, grid) in zip(rows, got):
        want = G.launch_form(*row[:5], bool(row[5]), knobs[row[6]])
        assert (cfg, ks, bool(persistent)) == want, (row, (cfg, ks, persistent), want)
        seen.add(want)
        if row[7] is not None:
            assert REDUCE_KINDS[reduce] == ROW_REDUCE.get(row[7], "none"), (row, REDUCE_KINDS[reduce])
    # the sets reach every form there is: each configuration unsplit, both persistent ones, and K over 2, 4 and 8
    assert {(c, 1, False) for c in range(4)} | {(0, 1, True), (1, 1, True)} <= seen and {f[1] for f in seen} == {1, 2, 4, 8}


# ---- the exact families, shape by shape -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,case,form", G.CASES, ids=G.CASE_IDS)
def test_family_I_conditions(name, case, form):
    in_nc, out_nc, width, nb, H, W, B = case
    r = G.reference(case, "I")
    w, x, y64 = r["w"], r["x"], r["y64"]
    assert x.shape == (H, W, in_nc, B) and _is_int(x) and x.min() == 0 and x.max() == 3
    ws = R.split_blob(w, R.seq_shapes(in_nc, out_nc, width, nb))
    taps = []
    assert np.array_equal(R.seq_conv(x, w, in_nc, out_nc, width, nb, taps=taps), y64)
    t_in = x
    for l, (wl, t) in enumerate(zip(ws, taps)):
        assert _is_int(wl) and np.abs(wl).max() <= 2
        assert (np.abs(wl).max(axis=0) > 0).all(), "a (cin, tap) position is zero for every output channel"
        hi, lo = R.split_f16(wl * R.weight_scale(wl))
        assert not lo.any() and np.array_equal(hi, wl * R.weight_scale(wl))                   # weights: one f16 piece
        assert _is_int(t_in) and np.abs(t_in).max() < 2 ** 11                                 # activations: integers an f16 holds, no low piece
        hi, lo = R.split_f16(t_in)
        assert not lo.any() and np.array_equal(hi, t_in)
        # (bf16 x 6: three 8-bit pieces hold 24 bits, so any fp32 value and these 11-bit integers in particular)
        ab = R.abs_bound(t_in, wl)
        assert ab.max() < 2 ** 24 / 2                                                          # every partial sum, in any order, in units of 1/2 (scaled weights)
        if l == 0:
            assert np.abs(wl).sum(axis=(1, 2, 3)).max() * 3 < 2 ** 11
        assert _is_int(t) and np.abs(t).max() < 2 ** 11 and t.max() > 0
        assert np.abs(t).max() < 6e4
        t_in = t
    assert np.array_equal(y64, y64.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name,case,form", G.CASES, ids=G.CASE_IDS)
@pytest.mark.parametrize("fam", ["A", "B"])
def test_family_A_and_B_conditions(name, case, form, fam):
    """(w, x): the operands of the layer that rounds -- the only layer, or the middle one between two copying layers."""
    in_nc, out_nc, width, nb, H, W, B = case
    r = G.reference(case, fam)
    w, x = r["ab"]
    y64 = R.conv3x3(x, w)
    assert (np.abs(w).max(axis=0) > 0).all()
    s = R.weight_scale(w)
    assert 1.0 <= np.abs(w).max() * s < 2.0
    whi, wlo = R.split_f16(w * np.float32(s))
    xhi, xlo = R.split_f16(x)
    assert np.array_equal(whi + wlo / 2048.0, w.astype(np.float64) * s) and np.array_equal(xhi + xlo / 2048.0, x)    # the split loses nothing
    # quanta of the pieces
    qwh, qxh, ql = 0.5, 1.0, 2.0 ** -5
    assert _is_int(whi, qwh) and _is_int(xhi, qxh) and _is_int(wlo, ql) and _is_int(xlo, ql)
    if fam == "A":
        assert not wlo.any() and xlo.any() and np.array_equal(xhi, np.round(x)) and np.abs(xlo).max() == 8 * ql
    else:
        assert not xlo.any() and wlo.any() and np.abs(wlo).max() == 8 * ql
    assert not (R.abs_bound(xlo, wlo)).any()                         # lo'_w * lo'_x = 0 wherever a weight meets an activation
    # both accumulators hold every partial sum exactly: below 2^24 of their quantum
    assert R.abs_bound(xhi, whi).max() / (qwh * qxh) < 2 ** 24
    assert (R.abs_bound(xhi, wlo) + R.abs_bound(xlo, whi)).max() / (ql * min(qwh, qxh)) < 2 ** 24
    # ... so the kernel's epilogue value hi * descale + cross * descale / 2^11 is the exact result, rounded once
    exact = (R.conv3x3(xhi, whi) + (R.conv3x3(xhi, wlo) + R.conv3x3(xlo, whi)) / 2048.0) / s
    assert np.array_equal(exact, y64)
    assert 0.0625 <= np.abs(r["x"]).max() < 256 and r["x"].min() > 0.99                        # qmri_denoise applies no rescale
    assert np.abs(y64).max() < 6e4 and np.abs(y64).max() > 0                                   # no range guard trips
    if nb == 1:
        assert np.array_equal(r["y64"], y64) and np.array_equal(r["once"], G.f32(y64)) and (r["bound"] >= np.abs(y64)).all()
        return
    # nb = 3: the first layer copies (x is the network input's values and the padding's zeros, so the ReLU after it changes nothing) ...
    w1, w2, w3 = R.split_blob(r["w"], R.seq_shapes(in_nc, out_nc, width, nb))
    for wc in (w1, w3):
        assert set(np.unique(wc)) == {0.0, 1.0} and (wc.sum(axis=(1, 2, 3)) == 1).all()
    assert np.array_equal(w2, w) and x.min() >= 0 and set(np.unique(x)) <= set(np.unique(r["x"])) | {0.0}
    # ... and the last layer returns hi + lo' / 2^11 of the middle layer's fp32 output after the ReLU: an fp32 value within 2^-22 of it
    t2 = np.maximum(G.f32(y64), 0.0)
    rt = R.split_roundtrip(t2)
    assert np.array_equal(rt, G.f32(rt)) and (np.abs(rt - t2) <= 2.0 ** -22 * np.abs(t2)).all() and rt.max() > 0
    assert np.array_equal(r["once"], R.conv3x3(rt, w3)) and set(np.unique(r["once"])) <= set(np.unique(rt)) | {0.0}
    assert (r["bound"] >= np.abs(r["y64"])).all()


@pytest.mark.parametrize("name,net,hw,in_nc", G.UNET_CASES, ids=G.UNET_IDS)
def test_routing_weights_keep_every_tensor_an_integer_below_2048(name, net, hw, in_nc):
    (nc, nb) = net
    for draw in range(G.N_DRAWS):
        w, x = G.unet_case(net, hw, in_nc, draw)
        assert set(np.unique(w)) <= {-1.0, 0.0, 1.0} and set(np.unique(x)) == {1.0, 2.0, 3.0}
        for (kind, shp), wl in zip(R.unetres_shapes(in_nc, 10, nc, nb), R.split_blob(w, [s for _, s in R.unetres_shapes(in_nc, 10, nc, nb)])):
            per_out = np.abs(wl).sum(axis=(0, 2, 3) if kind == "u" else (1, 2, 3))
            assert per_out.min() >= 1 and per_out.max() <= 2                                   # one weight per output channel, or two
        taps = []
        y = R.unetres(x, w, in_nc, 10, nc, nb, taps=taps)
        assert np.array_equal(y, G.unet_reference(net, hw, in_nc, draw))
        for t in taps:
            assert _is_int(t) and np.abs(t).max() < 2 ** 11 and np.abs(t).max() > 0
        assert len(set(np.unique(y))) > 8                                                      # the output is not trivial
