"""CPU: the EPG simulation of prepared, repeated FISP trains (include/qmri.h qmri_dict_simulate_seq) without a device -- the
numpy restatement tests/epgseq_ref.py against tests/epg_ref.py (one block), against closed forms that are not its own recursion, and against
itself (cycles equal tiling); the fixture facts the GPU tolerances of tests/test_gpu_epgseq.py rest on; the host plan of csrc/epg_seq_plan.h; the
block builders of synth.py; every refusal of both entry points; the Python and MEX argument rules; the symbol list, the header text and the
documents."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import epg_ref as R
import epgseq_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
NEW = ["qmri_dict_simulate_seq", "qmri_dict_simulate_seq_dev"]


@pytest.mark.parametrize("name", [n for n in sorted(R.CASES) if n not in ("t1024", "k5000", "chain")])
def test_one_block_is_epg_fisp(name):
    """One block {T, inversion, wait 0, ti, inv_eff} (or {T, none, 0, 0, 1}) in one cycle is the plain simulation, number for number."""
    inp = R.case_inputs(name)
    F = Q.epg_fisp_seq(inp["alpha"], inp["tr"], inp["te"], inp["t1"], inp["t2"], Q.degenerate_blocks(inp), 1, b1=inp["b1"], nstates=inp["nstates"])
    assert np.array_equal(F, R.case_ref(name))


def test_zero_flip_angles_give_zero_signal_exactly():
    t1, t2 = R.grid(5, 3)
    F = Q.epg_fisp_seq(np.zeros(48), R.TR0, R.TE0, t1, t2, Q.MIX, 3, nstates=8)
    assert np.all(F == 0.0)


def test_first_frame_after_a_preparation_against_its_closed_form():
    """From equilibrium the first frame behind a preparation reads sin(alpha_0 b1) Mz exp(-TE_0 / T2) with Mz = eff exp(-prep_time / T2) behind a
    T2 preparation and 1 - (1 + eff) exp(-TI / T1) behind an inversion: to 1e-14, for every atom of the 9 x 5 grid on a b1 ramp."""
    from qmri_pnp_recon_poc_amd import synth
    t1, t2 = R.grid(9, 5)
    b1 = np.linspace(0.8, 1.2, t1.size)
    alpha = synth.flip_angle_train(12)
    tr, te = R._timing_varying(12)
    for eff, pt in ((1.0, 0.040), (0.9, 0.080)):
        F = Q.epg_fisp_seq(alpha, tr, te, t1, t2, [Q.blk(12, "t2", 0.0, pt, eff)], 1, b1=b1)
        want = np.sin(alpha[0] * b1) * eff * np.exp(-pt / t2) * np.exp(-te[0] / t2)
        print("T2 preparation", eff, pt, np.max(np.abs(F[:, 0] - want)))
        assert np.max(np.abs(F[:, 0] - want)) <= 1e-14
    for eff, ti in ((1.0, 0.021), (0.95, 0.2)):
        F = Q.epg_fisp_seq(alpha, tr, te, t1, t2, [Q.blk(12, "inversion", 0.0, ti, eff)], 1, b1=b1)
        want = np.sin(alpha[0] * b1) * (1 - (1 + eff) * np.exp(-ti / t1)) * np.exp(-te[0] / t2)
        print("inversion", eff, ti, np.max(np.abs(F[:, 0] - want)))
        assert np.max(np.abs(F[:, 0] - want)) <= 1e-14
    # a wait in front of the first block changes nothing at equilibrium: Z_0 <- E1 + (1 - E1)
    F0 = Q.epg_fisp_seq(alpha, tr, te, t1, t2, [Q.blk(12, "t2", 0.0, 0.040)], 1, b1=b1)
    Fw = Q.epg_fisp_seq(alpha, tr, te, t1, t2, [Q.blk(12, "t2", 0.7, 0.040)], 1, b1=b1)
    assert np.max(np.abs(F0 - Fw)) <= 1e-14


def test_a_long_wait_forgets_the_cycle_before():
    """wait = 60 s on the first block: what the cycles before left has decayed by exp(-60 / T1) <= 1e-13 for T1 <= 2 s (and far more in the
    transverse states), so every C gives the C = 1 result to 1e-12.  The atoms are the 9 x 5 grid's with T1 <= 2 s for that reason."""
    from qmri_pnp_recon_poc_amd import synth
    t1, t2 = R.grid(9, 5)
    keep = t1 <= 2.0
    t1, t2 = t1[keep], t2[keep]
    assert t1.size >= 30 and t1.max() > 1.5
    alpha = synth.flip_angle_train(48)
    blocks = [dict(b) for b in Q.MIX]
    blocks[0]["wait"] = 60.0
    one = Q.epg_fisp_seq(alpha, R.TR0, R.TE0, t1, t2, blocks, 1)
    for Cn in (2, 3, 5):
        d = np.max(np.abs(Q.epg_fisp_seq(alpha, R.TR0, R.TE0, t1, t2, blocks, Cn) - one))
        print("C =", Cn, "difference from C = 1:", d)
        assert d <= 1e-12


def test_a_short_pause_drives_a_steady_state():
    """One train of 48 frames repeated with a 1 s pause (synth.repeated_train_blocks): the change from C to C + 1 cycles shrinks monotonically for
    C = 1 .. 6, and C = 1 differs from C = 6 by more than 1e-3 -- the cycles are not a no-op, and they converge."""
    from qmri_pnp_recon_poc_amd import synth
    t1, t2 = R.grid(9, 5)
    alpha = synth.flip_angle_train(48)
    blocks = synth.repeated_train_blocks(48, 1.0)
    F = [Q.epg_fisp_seq(alpha, R.TR0, R.TE0, t1, t2, blocks, Cn) for Cn in range(1, 8)]
    d = [np.max(np.abs(F[i + 1] - F[i])) for i in range(6)]
    print("change from C to C + 1:", d, "C = 1 against C = 6:", np.max(np.abs(F[0] - F[5])))
    assert all(d[i + 1] < d[i] for i in range(5)) and d[5] > 0.0
    assert np.max(np.abs(F[0] - F[5])) > 1e-3


def test_cycles_equal_tiling():
    """C = 3 cycles of the four-block fixture are the last 48 frames of one cycle on the 3-fold tiled train and block list, number for number."""
    inp = Q.case_inputs("timing")
    al, tr, te, bl = Q.tiled(inp["alpha"], inp["tr"], inp["te"], inp["blocks"], 3)
    big = Q.epg_fisp_seq(al, tr, te, inp["t1"], inp["t2"], bl, 1)
    assert big.shape == (45, 144)
    assert np.array_equal(Q.epg_fisp_seq(**dict(inp, ncycles=3)), big[:, 96:])
    assert not np.array_equal(big[:, :48], big[:, 96:])


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_fixture_facts_the_gpu_tolerance_rests_on(name):
    """Per GPU fixture, by section 19's method, on the restatement alone: how far the fp64 run is from its np.longdouble run, and from its two runs
    with every exponential moved one fp64 ulp.  Q.SENS holds these figures with a factor 2 of room (asserted from above, and from below at a
    quarter: the table is the measurement, not a loose guess); the GPU tolerance Q.atol is 16 x the larger of the two."""
    inp, F = Q.case_inputs(name), Q.case_ref(name)
    ld = float(np.max(np.abs(F - Q.epg_fisp_seq(**inp, dtype=np.longdouble))))
    ex = max(float(np.max(np.abs(F - Q.epg_fisp_seq(**inp, exp=R.exp_neighbour(d))))) for d in (+1, -1))
    print(name, "fp64 - longdouble:", ld, "exponentials one ulp away:", ex, "table:", Q.SENS[name], "GPU atol:", Q.atol(name), "peak |F|:", np.abs(F).max())
    c = Q.CASES[name]
    assert F.shape == (c["grid"][0] * c["grid"][1], c["T"]) and np.all(np.isfinite(F)) and np.abs(F).max() <= 1.0
    assert sum(b["nframes"] for b in inp["blocks"]) == c["T"]
    assert Q.SENS[name][0] / 4 <= ld <= Q.SENS[name][0]
    assert Q.SENS[name][1] / 4 <= ex <= Q.SENS[name][1]
    assert Q.atol(name) == 16 * max(Q.SENS[name]) <= 1e-11


def test_the_fixtures_are_what_they_claim():
    """The four-block list has its boundaries inside the kernel's 16-frame blocks and one block exactly 16 long; the prepared result is far from
    the plain one; t1024 fills every limit at once."""
    assert [b["nframes"] for b in Q.MIX] == [5, 16, 17, 10] and [b["prep"] for b in Q.MIX] == ["none", "inversion", "t2", "t2"]
    t = Q.case_inputs("t1024")
    assert len(t["blocks"]) == 64 and t["ncycles"] == 16 and t["alpha"].size == 1024
    o = Q.case_inputs("ones")
    assert len(o["blocks"]) == 48 and {b["prep"] for b in o["blocks"]} == {"none", "inversion", "t2"}
    assert np.max(np.abs(Q.case_ref("s32") - R.case_ref("s32"))) > 1e-3
    assert np.max(np.abs(Q.case_ref("s32") - Q.epg_fisp_seq(**dict(Q.case_inputs("s32"), ncycles=1)))) > 1e-3


def test_the_chain_fixture_has_separated_eigenvalues_and_every_atom_matches_itself():
    """The cardiac block list on 24 x 11 atoms, T = 48, S = 32, s = 6: the kept eigenvalues have a smallest relative gap above 1e-6 (the
    precondition of the chain test's bound on V), and under the reference compression every pixel of epg_ref.chain_match_input returns its own
    atom with the runner-up's normalised inner product at least 1e-5 below 1 (fp32 atoms resolve 6e-8)."""
    import dict_svd_ref as DR
    from oracle import oracle as O
    F = Q.case_ref("chain")
    r = DR.dict_compress_ref(F, s=6)
    print("gaps", r["gaps"], "energy kept", r["energy_kept"])
    assert r["gaps"].min() > 1e-6
    t1, t2 = R.grid(24, 11)
    lut = np.stack([t1, t2], axis=1).astype(np.float32)
    m = O.dict_match(R.chain_match_input(r), r["D"], r["normD"], lut)
    idx = np.arange(1024) * F.shape[0] // 1024
    assert np.array_equal(np.asarray(m["dm"]), (idx + 1).reshape(32, 32))
    D = r["D64"] / np.linalg.norm(r["D64"], axis=1, keepdims=True)
    G = np.abs(D @ D.T)
    np.fill_diagonal(G, 0.0)
    print("largest inner product between two atoms:", G.max())
    assert G.max() <= 1.0 - 1e-5


def test_plan_header_stands_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "epg_seq_plan.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_plan_sweep_under_address_and_ub_sanitizer(tmp_path):
    """tests/cpp/epg_seq_plan_test.cpp: every block list of every T <= 8 (255 compositions) with segment lengths 1, 2, 3, 5, 16, and 2004 longer
    lists with the kernel's 16 -- segments never straddle a block, cover 0 .. T-1 once and in order, hold at most fb frames, and exactly one per
    block carries the block's event."""
    exe = tmp_path / "epg_seq_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "epg_seq_plan_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "EPG_SEQ_PLAN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert int(re.search(r"swept (\d+)", r.stdout).group(1)) == 255 * 5 + 2004


def test_block_builders():
    """synth.repeated_train_blocks and synth.cmrf_blocks against a hand-computed five-beat example: 10 frames of 10 ms behind the default
    preparations (inversion 21 ms, none, T2 40 ms, T2 80 ms, inversion again)."""
    from qmri_pnp_recon_poc_amd import synth
    assert synth.repeated_train_blocks(200, 1.5) == [dict(nframes=200, prep="none", wait=1.5, prep_time=0.0, prep_eff=1.0)]
    for bad in ((0, 1.0), (10, -0.1), (10, np.inf), (2.5, 1.0)):
        with pytest.raises(ValueError):
            synth.repeated_train_blocks(*bad)
    b = synth.cmrf_blocks([1.0, 0.9, 1.1, 0.8, 1.2], 10, 0.010)
    assert [x["nframes"] for x in b] == [10] * 5 and [x["prep"] for x in b] == ["inversion", "none", "t2", "t2", "inversion"]
    assert [x["prep_time"] for x in b] == [0.021, 0.0, 0.040, 0.080, 0.021] and all(x["prep_eff"] == 1.0 for x in b)
    # beat b >= 1 starts rr[b - 1] after beat b - 1: wait = rr[b - 1] - 0.1 - prep_time_b -> 0.9, 0.76, 0.92, 0.679
    assert b[0]["wait"] == 0.0 and np.allclose([x["wait"] for x in b[1:]], [0.9, 0.76, 0.92, 0.679], rtol=0, atol=1e-15)
    b = synth.cmrf_blocks([1.0, 1.0, 1.0], 4, 0.012, preps=(("t2", 0.03), ("none", 0.0)))
    assert [x["prep"] for x in b] == ["t2", "none", "t2"] and np.allclose([x["wait"] for x in b], [0.0, 0.952, 0.922], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="beat 3"):
        synth.cmrf_blocks([1.0, 0.9, 0.17, 0.8, 1.2], 10, 0.010)             # 0.17 - 0.1 - 0.08 < 0
    assert synth.cmrf_blocks([1.0, 0.9, 0.19, 0.8], 10, 0.010)[3]["wait"] == pytest.approx(0.01, abs=1e-15)
    for bad in (dict(rr_s=[]), dict(rr_s=[1.0, np.nan]), dict(frames_per_beat=0), dict(tr_s=0.0), dict(preps=()), dict(preps=(("spin", 0.0),)),
                dict(preps=(("none", 0.01),)), dict(preps=(("t2", -0.01),))):
        kw = dict(rr_s=[1.0, 1.0], frames_per_beat=4, tr_s=0.012)
        kw.update(bad)
        with pytest.raises(ValueError):
            synth.cmrf_blocks(**kw)


def test_symbols_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert re.search(r"\}\s*qmri_epg_block\s*;", header) and re.search(r"\}\s*qmri_epg_seq\s*;", header)
    section = header[header.index("EPG simulation of prepared, repeated FISP trains"):]
    head = section[:section.index("*/")]
    assert "extension" in head and "no reference counterpart" in head and "parity unpinned" in head and "section 33" in head
    body = section[:section.index("qmri_dict_simulate_seq_dev(")]
    for phrase in ("Z_0 += 1 - E1", "(-eff Z_0) e + (1 - e)", "(eff Z_n) e2", "IDEALISED", "T1 relaxation during the module is neglected", "NOT scaled by b1",
                   "only the last is recorded", "no atomics", "sign of a zero is not pinned", "tiled", "Out of scope", "slice profile", "Cramer-Rao",
                   "complex", "diffusion", "p->inversion must be 0", "nothing is written"):
        assert phrase in body, phrase
    assert "NaN in every frame" in section[:section.index("field map from multi-echo")]
    assert re.search(r"#define\s+QMRI_ABI_VERSION\s+1\b", header) and _lib.lib().qmri_abi_version() == 1
    B, S = _lib.EpgBlock, _lib.EpgSeq
    assert C.sizeof(B) == 32 and (B.nframes.offset, B.prep.offset, B.wait.offset, B.prep_time.offset, B.prep_eff.offset) == (0, 4, 8, 16, 24)
    assert C.sizeof(S) == 32 and (S.nblocks.offset, S.ncycles.offset, S.blocks.offset, S.reserved.offset) == (0, 4, 8, 16)


def test_every_refusal_of_both_entry_points_without_a_device():
    """With ctx == NULL each call returns QMRI_ERR_INVALID_ARG for its first failing check and leaves the message in qmri_last_error(NULL): the
    refusals of qmri_dict_simulate first, then the schedule's own; a call whose arguments are all fine is refused for the missing context.  No
    refused call writes to its output."""
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import EpgBlock, EpgParams, EpgSeq
    L = _lib.lib()
    K, T = 3, 4
    base = dict(al=[0.1, 0.2, 0.0, 0.4], tr=[0.012, 0.012, 0.013, 0.012], te=[0.002, 0.0, 0.013, 0.002], t1=[1.0, 0.5, 2.0], t2=[0.1, 0.05, 0.2], b1=[1.0, 0.0, 1.2])
    Fb = np.full(K * T, -7.0)
    good = [(1, 1, 0.0, 0.021, 0.95), (2, 0, 0.5, 0.0, 1.0), (1, 2, 0.3, 0.040, 1.0)]
    keep = []

    def P(nstates=32, inversion=0, ti=0.0, inv_eff=1.0, f64=1):
        return EpgParams(nstates, inversion, ti, inv_eff, f64)

    def S(blocks=good, nblocks=None, ncycles=2, reserved=(0, 0, 0, 0), null=False):
        arr = (EpgBlock * len(blocks))(*[EpgBlock(*b) for b in blocks])
        keep.append(arr)
        return EpgSeq(len(blocks) if nblocks is None else nblocks, ncycles, None if null else arr, (C.c_int32 * 4)(*reserved))

    def call(fn, K=K, T=T, p=P(), sq=S(), F=Fb, **kw):
        arrs = {k: (None if k in kw and kw[k] is None else np.array(kw.get(k, v), dtype=np.float64)) for k, v in base.items()}
        ptr = {k: (a.ctypes.data_as(C.c_void_p) if a is not None else None) for k, a in arrs.items()}
        st = fn(None, K, T, ptr["al"], ptr["tr"], ptr["te"], ptr["t1"], ptr["t2"], ptr["b1"], C.byref(p) if p is not None else None,
                C.byref(sq) if sq is not None else None, F.ctypes.data_as(C.c_void_p) if F is not None else None)
        return st, L.qmri_last_error(None)

    def with_(key, i, v):
        x = list(base[key])
        x[i] = v
        return {key: x}

    def blk(i, field, v):
        b = [list(x) for x in good]
        b[i][("nframes", "prep", "wait", "prep_time", "prep_eff").index(field)] = v
        return dict(sq=S(blocks=[tuple(x) for x in b]))

    nan, inf = float("nan"), float("inf")
    common = [(dict(p=None), b"params"), (dict(al=None), b"alpha /"), (dict(tr=None), b"alpha /"), (dict(te=None), b"alpha /"), (dict(t1=None), b"alpha /"),
              (dict(t2=None), b"alpha /"), (dict(F=None), b"F_out"), (dict(K=0), b"K must"), (dict(K=-1), b"K must"), (dict(T=0), b"T must"), (dict(T=1025), b"T must"),
              (dict(p=P(nstates=0)), b"nstates"), (dict(p=P(nstates=257)), b"nstates"), (dict(p=P(inversion=2)), b"inversion must be 0 or 1"),
              (dict(p=P(f64=2)), b"out_is_f64"), (dict(p=P(inversion=1, ti=-1.0)), b"ti must"), (dict(p=P(inversion=1, inv_eff=0.0)), b"inv_eff"),
              (dict(p=None, sq=None), b"params"), (dict(T=0, sq=None), b"T must")]
    for bad in (-0.1, nan, inf):
        common += [(with_("al", 2, bad), b"alpha must"), (with_("tr", 3, bad), b"tr must"), (with_("te", 1, bad), b"te must")]
        common += [(blk(2, "wait", bad), b"wait must"), (blk(0, "prep_time", bad), b"prep_time must")]
    common += [(with_("tr", 1, 0.0), b"tr must"), (with_("te", 0, 0.0125), b"te must not exceed tr"),
               (dict(p=P(inversion=1)), b"stated in the blocks"), (dict(p=P(inversion=1), sq=None), b"stated in the blocks"),
               (dict(sq=None), b"seq / blocks"), (dict(sq=S(null=True)), b"seq / blocks"),
               (dict(sq=S(nblocks=0)), b"nblocks must"), (dict(sq=S(nblocks=-1)), b"nblocks must"), (dict(sq=S(nblocks=65)), b"nblocks must"),
               (dict(sq=S(ncycles=0)), b"ncycles must"), (dict(sq=S(ncycles=-2)), b"ncycles must"), (dict(sq=S(ncycles=17)), b"ncycles must"),
               (dict(sq=S(reserved=(0, 0, 0, 1))), b"reserved"), (dict(sq=S(reserved=(5, 0, 0, 0))), b"reserved"),
               (blk(2, "nframes", 0), b"nframes must"), (blk(0, "nframes", -4), b"nframes must"), (blk(1, "prep", -1), b"prep must"), (blk(1, "prep", 3), b"prep must"),
               (blk(0, "prep_eff", 0.0), b"prep_eff must"), (blk(0, "prep_eff", -0.5), b"prep_eff must"), (blk(2, "prep_eff", 1.0001), b"prep_eff must"),
               (blk(2, "prep_eff", nan), b"prep_eff must"), (blk(1, "prep_time", 0.01), b"without a preparation"), (blk(1, "prep_eff", 0.9), b"without a preparation"),
               (blk(1, "nframes", 3), b"sum to T"), (blk(1, "nframes", 1), b"sum to T"), (dict(sq=S(blocks=good[:2])), b"sum to T"), (dict(T=5), b"sum to T"),
               (dict(), b"ctx"), (dict(b1=None), b"ctx"), (dict(sq=S(ncycles=16)), b"ctx"), (dict(sq=S(blocks=[(4, 0, 0.0, 0.0, 1.0)], ncycles=1)), b"ctx"),
               (dict(p=P(inversion=0, ti=-1.0, inv_eff=9.0)), b"ctx"), (with_("b1", 0, 0.0), b"ctx"), (blk(0, "prep_time", 0.0), b"ctx"), (blk(2, "wait", 0.0), b"ctx")]
    atoms = []
    for bad in (0.0, -1.0, nan, inf):
        atoms += [(with_("t1", 2, bad), b"t1 must"), (with_("t2", 0, bad), b"t2 must")]
        if bad != 0.0:
            atoms.append((with_("b1", 1, bad), b"b1 must"))
    for fn, host in ((L.qmri_dict_simulate_seq, True), (L.qmri_dict_simulate_seq_dev, False)):
        for kw, word in common + [(kw, word if host else b"ctx") for kw, word in atoms]:
            if kw.get("T") == 5:                             # a fifth frame for the arrays that are read up to T
                kw = dict(kw, al=base["al"] + [0.1], tr=base["tr"] + [0.012], te=base["te"] + [0.002])
            st, msg = call(fn, **kw)
            assert st == -1 and word in msg, (host, kw, st, msg)
    assert np.all(Fb == -7.0)


def test_python_argument_rules():
    """blocks are dicts with nframes and the optional prep / wait / prep_time / prep_eff; they become the library's structs unchanged.  The
    harness hands blocks and ncycles through, leaves the old keywords alone without them, and refuses them with a slice profile or crb=True."""
    from qmri_pnp_recon_poc_amd import engine, harness
    arr, seq = engine.sequence_arguments([dict(nframes=3), dict(nframes=4, prep="t2", wait=0.5, prep_time=0.04, prep_eff=0.9), dict(nframes=1, prep="inversion", prep_time=0.02)], 3, 8)
    assert (seq.nblocks, seq.ncycles, list(seq.reserved)) == (3, 3, [0, 0, 0, 0]) and C.addressof(seq.blocks.contents) == C.addressof(arr)
    assert [(b.nframes, b.prep, b.wait, b.prep_time, b.prep_eff) for b in arr] == [(3, 0, 0.0, 0.0, 1.0), (4, 2, 0.5, 0.04, 0.9), (1, 1, 0.0, 0.02, 1.0)]
    ok = [dict(nframes=8)]
    for blocks, nc in (([], 1), ([dict(nframes=1)] * 65, 1), (ok, 0), (ok, 17), (ok, 1.5), ([dict(nframes=7)], 1), ([dict(nframes=9)], 1), ([dict(prep="t2")], 1),
                       ([dict(nframes=8, prep="spin")], 1), ([dict(nframes=8, prep=1)], 1), ([dict(nframes=8, ti=0.02)], 1), ([dict(nframes=8.5)], 1),
                       ([dict(nframes=0), dict(nframes=8)], 1)):
        with pytest.raises(ValueError):
            engine.sequence_arguments(blocks, nc, 8)
    al = np.linspace(0.1, 0.5, 8)
    e = engine.Engine.__new__(engine.Engine)
    with pytest.raises(ValueError):
        e.simulate_dictionary_seq(al, 0.012, 0.002, [1.0], [0.1], [dict(nframes=7)])
    with pytest.raises(ValueError):
        e.simulate_compress_dictionary(al, 0.012, 0.002, [1.0, 2.0], [0.1], s=1, blocks=ok, slice_profile=np.ones(3))
    seen = {}

    class Stub:
        def __init__(self, device):
            pass

        def simulate_compress_dictionary(self, alpha, tr, te, t1, t2, **kw):
            seen.update(kw=kw, K=len(t1))
            return {"V": np.zeros((len(alpha), 2)), "D": np.zeros((len(t1), 2), np.float32), "normD": np.zeros(len(t1), np.float32), "eig": np.zeros(2), "info": {"s": 2}}

        def close(self):
            pass

    real = engine.Engine
    engine.Engine = Stub
    try:
        out = harness.simulate_dictionary(al, 0.012, 0.002, [1.0, 2.0], [0.1, 0.2, 0.3], s=2, b1_grid=[0.9, 1.1], blocks=ok, ncycles=4)
        assert seen["kw"]["blocks"] is ok and seen["kw"]["ncycles"] == 4 and seen["K"] == 12
        assert out["lut"].shape == (12, 3) and out["group_ptr"].tolist() == [0, 6, 12] and seen["kw"]["b1"].tolist() == [0.9] * 6 + [1.1] * 6
        harness.simulate_dictionary(al, 0.012, 0.002, [1.0, 2.0], [0.1, 0.2, 0.3], s=2)
        assert "blocks" not in seen["kw"] and "ncycles" not in seen["kw"]
        with pytest.raises(ValueError, match="slice profile"):
            harness.simulate_dictionary(al, 0.012, 0.002, [1.0], [0.1], s=1, blocks=ok, slice_profile=np.ones(3))
        with pytest.raises(ValueError, match="crb"):
            harness.simulate_dictionary(al, 0.012, 0.002, [1.0], [0.1], s=1, blocks=ok, crb=True)
    finally:
        engine.Engine = real


def test_mex_dict_simulate_seq_checks_its_arguments_under_the_mock_gateway():
    from mexmock import MexError, qmri_mex
    al, t1, t2, e = np.full(4, 0.2), np.array([1.0, 2.0]), np.array([0.1, 0.2]), np.zeros((0, 0))
    B = np.array([[1.0, 1.0, 0.0, 0.02, 1.0], [3.0, 2.0, 0.5, 0.04, 0.9]]).T                  # 5 x 2
    ok = (al, np.array([0.012]), np.array([0.002]), t1, t2, e, {}, B, 2.0)

    def swap(i, v):
        return ok[:i] + (v,) + ok[i + 1:]

    def col(r, v):
        x = B.copy()
        x[r, 1] = v
        return x
    sq = "qmri:dict_simulate_seq:"
    for args, ident in ((ok[:8], "qmri:usage"), (swap(6, 1.0), sq + "params"), (swap(0, al + 0j), sq + "alpha"), (swap(0, np.zeros(1025)), sq + "alpha"),
                        (swap(0, al.astype(np.float32)), sq + "alpha"), (swap(1, np.full(3, 0.012)), sq + "tr"), (swap(2, np.full(5, 0.002)), sq + "te"),
                        (swap(3, t1 + 0j), sq + "atoms"), (swap(4, np.array([0.1])), sq + "atoms"), (swap(5, np.ones(3)), sq + "atoms"),
                        (swap(6, {"nstates": 0.0}), sq + "params"), (swap(6, {"nstates": 2.5}), sq + "params"), (swap(6, {"single": 3.0}), sq + "params"),
                        (swap(7, B + 0j), sq + "blocks"), (swap(7, B.astype(np.float32)), sq + "blocks"), (swap(7, B.T.copy()), sq + "blocks"),
                        (swap(7, np.zeros((5, 0))), sq + "blocks"), (swap(7, np.ones((5, 65))), sq + "blocks"), (swap(7, col(0, 0.0)), sq + "blocks"),
                        (swap(7, col(0, 2.5)), sq + "blocks"), (swap(7, col(0, np.nan)), sq + "blocks"), (swap(7, col(1, 3.0)), sq + "blocks"),
                        (swap(7, col(1, -1.0)), sq + "blocks"), (swap(7, col(1, np.inf)), sq + "blocks"),
                        (swap(8, 0.0), sq + "ncycles"), (swap(8, 17.0), sq + "ncycles"), (swap(8, 1.5), sq + "ncycles"), (swap(8, np.ones(2)), sq + "ncycles")):
        with pytest.raises(MexError) as err:
            qmri_mex("dict_simulate_seq", *args, nargout=1)
        assert err.value.id == ident, (ident, err.value.id, err.value.msg)
    m = open(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "matlab", "qmri_dict_simulate_seq.m")).read()
    assert "qmri_mex('dict_simulate_seq'" in m and "qmri:dict_simulate_seq:blocks" in m and "'inversion'" in m


def test_design_section_and_documents_exist():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 33\. .*prepared", design, re.M | re.I)
    assert m, "DESIGN.md section 33"
    sec = design[m.start():]
    for word in ("k_epg_seq", "epg_seq_plan.h", "ScratchSize", "idealis", "epgseq_times", "tiled", "no reference counterpart"):
        assert word in sec, word
    for name, tab in Q.SENS.items():                         # the measured tolerance table is the one in the document
        assert ("%.2g" % tab[1]) in sec, (name, tab)
    assert "qmri_dict_simulate_seq" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "epgseq_times.py")) and os.path.exists(os.path.join(ROOT, "profiles", "epgseq_times.json"))
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "epg_seq_plan.h" in make and "host_asan_epgseq" in make


def test_refusals_and_plan_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_epgseq.cpp against the host-only sanitised library: every refusal of qmri_dict_simulate_seq and
    qmri_dict_simulate_seq_dev without a context and with one (a block array of exactly nblocks entries is read to its last entry and no further;
    no refused call writes its output), and the plan of the GPU tests' block list, as a stand-alone program."""
    subprocess.run(["make", "-C", CSRC, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    assert rt_dirs, "clang sanitizer runtime not found"
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_build_asan", "host_asan_epgseq")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_EPGSEQ_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
