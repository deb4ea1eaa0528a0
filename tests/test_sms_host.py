"""CPU: simultaneous multi-slice groups (include/qmri.h qmri_set_sms / qmri_*_sms) without a device -- the numpy restatement
tests/sms_ref.py against itself (adjointness), against mc_ref in the degenerate case Z = 1, E = 1, and the conditions tests/test_gpu_sms.py relies on,
measured with the CPU oracle alone: the oracle's (iterations, flag) does not sit on a stop-rule boundary and its x does not move under one-ulp
perturbations, the tables of sms_ref bound what they say from above, the slices of the separation fixture really come apart and the E = 1 control does
not.  Then every refusal of the new entry points, the symbol list, the Python and gateway argument checks, the documents, the host plan's sweep and the
two stand-alone sanitizer programs.

Measured: adjointness 2.3e-16 .. 3.8e-15; under the perturbations x moves by 3.1e-16 .. 6.0e-16 (4.6e-15 on stagger's long group, 2.8e-14 on the
masked maps) and no count moves; tol 1e-13 against minimiser_sms 3.1e-14 .. 1.3e-13 (1.4e-12 on stagger's long group); separation 3.4e-5 / 3.2e-5 in
152 iterations against 6.5e-4 / 7.2e-4 for the control, which has not converged after 400."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mc_ref as MC
import sms_ref as SR
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
NEW = ["qmri_set_sms", "qmri_forward_sms", "qmri_adjoint_sms", "qmri_xupdate_sms", "qmri_pnp_admm_sms", "qmri_pnp_admm_sms_dev"]


def test_case_table_is_the_one_the_design_names():
    C_ = SR.CASES
    want = {"z2c4": (32, 32, 6, 24, 4, 2, 1, (1, 3, 8)), "z3c3g2": (32, 32, 6, 24, 3, 3, 2, (2, 4, 5, 18)), "z8c2": (32, 32, 6, 24, 2, 8, 1, (3,)),
            "z1c4g3": (32, 32, 6, 24, 4, 1, 3, (4,)), "z4c3masked": (32, 32, 6, 24, 3, 4, 1, (4,)), "genE": (32, 32, 6, 24, 4, 2, 1, (3,)),
            "stride": (128, 64, 10, 12, 3, 2, 1, (4,)), "epi64x32": (64, 32, 6, 12, 3, 2, 1, (4,)), "stagger": (32, 32, 6, 24, 4, 2, 3, (3, 24))}
    assert {n: (c["N"], c["M"], c["s"], c["T"], c["nc"], c["Z"], c["G"], c["max_batch"]) for n, c in C_.items()} == want
    for n in SR.ALL:
        c = SR.inputs(n)
        assert c["maps"].shape == (c["G"], c["Z"], c["N"], c["M"], c["nc"]) and c["y"].shape == (c["G"], c["m"], c["nc"]) and c["E"].shape == (c["T"], c["Z"])
        if n not in ("stride", "epi64x32"):
            assert np.all(np.diff(c["fp"]) == 100)
    c = SR.inputs("stride")
    assert c["m"] == 24576 > 64 * 256 and c["Z"] * c["N"] * c["M"] * c["s"] == 163840 and c["N"] * c["M"] * c["s"] > 256 * 256
    assert np.all(SR.inputs("z1c4g3")["E"] == 1.0) and np.allclose(np.abs(SR.inputs("z2c4")["E"]), 1.0) and np.abs(np.abs(SR.inputs("genE")["E"]) - 1.0).max() > 0.5
    out = ~MC.ellipse(32, 32)
    assert not np.any(SR.inputs("z4c3masked")["maps"][:, :, out, :])
    # z3c3g2: some chunk begins inside a (g, j) sum (forward order, unit Z) and some inside a slice's coil sum (adjoint order, unit nc); 18 is the whole call
    assert any(q0 % 3 for mb in (2, 4, 5) for q0 in range(0, 18, mb)) and 18 == C_["z3c3g2"]["G"] * C_["z3c3g2"]["Z"] * C_["z3c3g2"]["nc"]
    s = SR.inputs("stagger")
    assert not np.any(s["y"][1]) and not np.any(s["z"][1]) and not np.any(s["x0"][1])
    ss = np.sum(np.abs(s["maps"][2]) ** 2, axis=3)
    assert ss.min() < 0.03 and ss.max() > 11.0 and np.allclose(np.sum(np.abs(s["maps"][0]) ** 2, axis=3), 1.0)
    assert np.array_equal(SR.caipi(5, 3)[4], np.exp(2j * np.pi * np.arange(3) * 1 / 3))
    assert set(SR.LSQR_SENS) <= set(SR.ALL) and 4 * len(SR.LSQR_SENS) <= len(SR.ALL)


@pytest.mark.parametrize("name", SR.ALL)
def test_restatement_is_adjoint(name):
    c = SR.inputs(name)
    for g in range(c["G"]):
        yr, xr = c["op"].forward_mc(c["xop"], c["maps"][g]), c["op"].adjoint_mc(c["yn"], c["maps"][g])
        lhs, rhs = np.vdot(c["yn"], yr), np.vdot(xr, c["xop"])
        print(f"{name} group {g}: adjointness {abs(lhs - rhs) / abs(lhs):.2e}")
        assert yr.shape == (c["m"], c["nc"]) and xr.shape == c["xop"].shape
        assert abs(lhs - rhs) / abs(lhs) <= 1e-12


class _McOperator:
    """mc_ref's pair under the names oracle.Operator.lsqr_mc calls: the multi-coil restatement of one slice, duck-typed as sms_ref.SmsOperator is."""

    def __init__(self, c):
        self.N, self.M, self.s, self.c = c["N"], c["M"], c["s"], c

    def forward_mc(self, x, maps):
        return MC.forward_mc(x, maps, self.c["V"], self.c["fp"], self.c["k"])

    def adjoint_mc(self, y, maps):
        return MC.adjoint_mc(y, maps, self.c["V"], self.c["fp"], self.c["k"], self.N, self.M)


def test_one_slice_with_unit_phases_is_the_multi_coil_restatement(oracle):
    """Z = 1, E = 1: the operator equals mc_ref exactly, and the oracle's lsqr_mc gives the same (x, iterations, flag) on either restatement."""
    c = SR.inputs("z1c4g3")
    V, fp, k, N, M = c["V"], c["fp"], c["k"], c["N"], c["M"]
    mc = _McOperator(c)
    for g in range(c["G"]):
        maps = c["maps"][g]
        assert np.array_equal(c["op"].forward_mc(c["xop"], maps), MC.forward_mc(c["xop"][0], maps[0], V, fp, k))
        assert np.array_equal(c["op"].adjoint_mc(c["yn"], maps)[0], MC.adjoint_mc(c["yn"], maps[0], V, fp, k, N, M))
        xs, its, fls = SR.oracle_lsqr("z1c4g3", g)
        xm, itm, flm = oracle.Operator.lsqr_mc(mc, c["y"][g], maps[0], c["z"][g][0], SR.R, tol=1e-4, maxit=100, x0=c["x0"][g][0])
        print(f"z1c4g3 group {g}: ({its}, {fls}) / ({itm}, {flm}), x {rel_err(xs[0], xm):.2e}")
        assert (its, fls) == (int(itm), int(flm)) and np.array_equal(xs[0], xm)


@pytest.mark.parametrize("name", SR.ALL)
def test_oracle_lsqr_is_off_the_stop_rule_boundary_and_insensitive(oracle, name):
    """tol 1e-4, maxit 100 per group: five one-ulp perturbations of (y, z) leave (iterations, flag) unchanged and move x by <= 1e-12 (the case takes
    the project's 1e-10 on the device) or by <= the case's entry in sms_ref.LSQR_SENS."""
    c = SR.inputs(name)
    for g in range(c["G"]):
        _, it, fl = SR.oracle_lsqr(name, g)
        worst, counts = SR.lsqr_sensitivity(name, g)
        print(f"{name} group {g}: ({it}, {fl}), x moves by {worst:.2e} (recorded {SR.LSQR_SENS.get(name, 1e-12):.1e}, device bound {SR.lsqr_bound(name):.1e})")
        assert fl == 0 and set(counts) == {(it, fl)}, (name, g, it, fl, counts)
        assert worst <= SR.LSQR_SENS.get(name, 1e-12)
        if c["kind"] == "generic":
            assert it >= 5


@pytest.mark.parametrize("name", SR.ALL)
def test_oracle_tight_lsqr_reaches_the_minimiser(oracle, name):
    """tol 1e-13, maxit 300 against minimiser_sms (conjugate gradients on the normal equations, 1e-13 on the true residual), per group: within the
    case's entry in sms_ref.TIGHT_SENS, from which the device's bound follows (entered at 3 x the figure)."""
    c = SR.inputs(name)
    xm = SR.minimisers(name)
    worst = 0.0
    for g in range(c["G"]):
        xt, it, fl = SR.oracle_lsqr(name, g, 1e-13, 300)
        e = rel_err(xt, xm[g]) if np.any(xm[g]) else float(np.linalg.norm(xt))
        worst = max(worst, e)
        print(f"{name} group {g}: tol 1e-13 ({it}, {fl}) against the minimiser {e:.2e}")
        assert it < 300
    print(f"{name}: {worst:.2e} (recorded {SR.TIGHT_SENS[name]:.1e}, device bound {SR.tight_bound(name):.1e})")
    assert worst <= SR.TIGHT_SENS[name]


def test_minimiser_raises_instead_of_returning_a_loose_solve():
    c = SR.inputs("z2c4")
    with pytest.raises(RuntimeError):
        SR.minimiser_sms(c["op"], c["y"][0], c["maps"][0], c["z"][0], SR.R, maxit=5)


def test_staggered_case_staggers(oracle):
    counts = [SR.oracle_lsqr("stagger", g)[1] for g in range(3)]
    print(f"stagger: counts {counts}")
    assert counts[1] == 0 and not np.any(SR.oracle_lsqr("stagger", 1)[0]) and counts[0] >= 5 and counts[2] >= counts[0] + 5


def test_the_slices_separate_with_the_oracle_alone(oracle):
    """Two different phantoms, 8 coils, noise-free, r = 1e-6, z = x0 = 0, tol 1e-10, maxit 400, E the CAIPI cycle: every slice comes back within 1e-4
    of its own phantom and stays more than 0.3 from the other's; the same data under E = 1 (coils alone) is at least 5 x worse."""
    f = SR.separate()
    x, it, fl = SR.separate_oracle()
    x1, it1, fl1 = SR.separate_oracle(control=True)
    err, err1 = SR.slice_errors(x, f), SR.slice_errors(x1, f)
    print(f"separation: ({it}, {fl}) {err}; control ({it1}, {fl1}) {[err1[b][b] for b in range(f['Z'])]}")
    own = [err[b][b] for b in range(f["Z"])]
    assert fl == 0 and it < f["maxit"] and max(own) < 1e-4
    assert all(err[b][c] > 0.3 for b in range(f["Z"]) for c in range(f["Z"]) if b != c)
    assert rel_err(f["x"][0], f["x"][1]) > 0.3                                # the phantoms differ
    assert min(err1[b][b] for b in range(f["Z"])) >= 5.0 * max(own)


# ---- the library without a device ---------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    section = header[header.index("simultaneous multi-slice (SMS) groups"):]
    head = section[:section.index("*/")]
    for word in ("EXTENSION", "no reference counterpart", "parity unpinned", "E[t + T*b]", "QMRI_ERR_UNSUPPORTED", "field map", "TOEPLITZ", "bit for bit"):
        assert word in head, word
    assert re.search(r"#define\s+QMRI_ABI_VERSION\s+1\b", header) and _lib.lib().qmri_abi_version() == 1


def test_every_refusal_that_needs_no_context():
    from qmri_pnp_recon_poc_amd import _lib
    from qmri_pnp_recon_poc_amd._lib import AdmmParams
    L = _lib.lib()
    a = np.zeros(64)
    vp = a.ctypes.data_as(C.c_void_p)
    p = AdmmParams(0.05, 2, 1e-4, 10, 0, 0, 0.01, 0)
    err = lambda: L.qmri_last_error(None)
    assert L.qmri_set_sms(None, -1, vp) == -1 and b"0 <= Z <= 8" in err()
    assert L.qmri_set_sms(None, 9, vp) == -1 and b"0 <= Z <= 8" in err()
    assert L.qmri_set_sms(None, 2, vp) == -1 and b"ctx" in err()
    assert L.qmri_forward_sms(None, 0, 2, vp, vp, 1, vp) == -1 and b"G >= 1" in err()
    assert L.qmri_forward_sms(None, 1, 0, vp, vp, 1, vp) == -1 and b"ncoil" in err()
    assert L.qmri_forward_sms(None, 1, 2, None, vp, 1, vp) == -1 and b"maps / y" in err()
    assert L.qmri_adjoint_sms(None, 1, 1025, vp, vp, vp) == -1 and b"ncoil" in err()
    assert L.qmri_adjoint_sms(None, 1, 2, vp, None, vp) == -1 and b"maps / y" in err()
    assert L.qmri_xupdate_sms(None, 1, 2, vp, vp, vp, 0.05, 1e-4, 10, None, vp, None, None) == -1 and b"ctx" in err()
    assert L.qmri_pnp_admm_sms(None, 1, 1, 2, vp, vp, C.byref(p), None, vp, None) == -1 and b"ctx" in err()
    assert L.qmri_pnp_admm_sms_dev(None, -1, 2, vp, vp, C.byref(p), None, vp, None) == -1 and b"G >= 1" in err()


def test_python_argument_checks():
    from qmri_pnp_recon_poc_amd import engine as E
    assert np.allclose(E.caipi_phases(24, 3), SR.caipi(24, 3)) and E.caipi_phases(7, 1).shape == (7, 1) and np.all(E.caipi_phases(7, 1) == 1.0)
    for T, Z in ((0, 2), (4, 0), (4, 9)):
        with pytest.raises(ValueError):
            E.caipi_phases(T, Z)
    e = E.Engine.__new__(E.Engine)                          # the checks run before any library call: no context is made
    e.N, e.M, e.s, e.T, e.m, e.sms_Z = 32, 32, 6, 24, 2400, 0
    for bad in (np.ones((23, 2), complex), np.ones((24, 9), complex), np.ones(24, complex), np.full((24, 2), np.nan + 0j)):
        with pytest.raises(ValueError):
            e.set_sms(bad)
    maps, y, x = np.ones((1, 2, 32, 32, 4), complex), np.ones((1, 2400, 4), complex), np.ones((1, 2, 32, 32, 6), complex)
    with pytest.raises(ValueError, match="set_sms was given 0"):
        e.forward_sms(maps, x)
    e.sms_Z = 2
    for call in (lambda: e.forward_sms(maps[0], x), lambda: e.forward_sms(maps[:, :, :16], x), lambda: e.forward_sms(maps, x[:, :1]),
                 lambda: e.adjoint_sms(maps, y[:, :100]), lambda: e.xupdate_sms(maps, y, x[0], 0.05), lambda: e.xupdate_sms(maps, y, None, 0.05),
                 lambda: e.pnp_admm_sms(maps, y[..., :3]), lambda: e.pnp_admm_sms(maps, y, x0=x[:, :, :8]), lambda: e.pnp_admm_sms(maps, y, tsmi_domain="both")):
        with pytest.raises(ValueError):
            call()


def test_mex_commands_check_their_arguments_under_the_mock_gateway():
    """The checks that come before the gateway looks at its plans (what it holds depends on the tests that ran before; the state refusals are
    tests/test_gpu_sms_mex.py's, on a fresh gateway)."""
    from mexmock import MexError, qmri_mex
    E = np.ones((24, 2), complex)
    mp, y, x = np.ones((32, 32, 4, 2), complex), np.ones((100, 4), complex), np.ones((32, 32, 6, 2), complex)
    none = np.zeros((0, 0))
    cases = [("set_sms", (), "qmri:usage"), ("set_sms", (E.real,), "qmri:set_sms:type"), ("set_sms", (np.ones((24, 2, 2), complex),), "qmri:set_sms:type"),
             ("set_sms", (np.ones((24, 9), complex),), "qmri:set_sms:size"), ("set_sms", (E * np.nan,), "qmri:set_sms:value"),
             ("set_sms", (np.full((24, 2), np.inf + 0j),), "qmri:set_sms:value"),
             ("forward_sms", (mp,), "qmri:usage"), ("forward_sms", (mp.real, x), "qmri:forward_sms:size"),
             ("adjoint_sms", (mp,), "qmri:usage"), ("adjoint_sms", (np.ones((2, 2, 2, 2, 2, 2), complex), y), "qmri:adjoint_sms:size"),
             ("xupdate_sms", (mp, y, x), "qmri:usage"), ("xupdate_sms", (mp, y, x, -1.0), "qmri:xupdate_sms:r"), ("xupdate_sms", (mp, y, x, 0.0), "qmri:xupdate_sms:r"),
             ("xupdate_sms", (mp, y, x, np.nan), "qmri:xupdate_sms:r"), ("xupdate_sms", (mp, y, x, 0.05, -1.0), "qmri:xupdate_sms:tol"),
             ("xupdate_sms", (mp, y, x, 0.05, 1e-4, 2.5), "qmri:xupdate_sms:maxit"), ("xupdate_sms", (mp, y, x, 0.05, 1e-4, -1.0), "qmri:xupdate_sms:maxit"),
             ("pnp_admm_sms", (mp, y), "qmri:usage"), ("pnp_admm_sms", (mp, y, 1.0), "qmri:pnp_admm_sms:type"),
             ("pnp_admm_sms", (mp, y, {"iter": 2}, none, 0.0), "qmri:pnp_admm_sms:groups"), ("pnp_admm_sms", (mp, y, {"iter": 2}, none, 1.5), "qmri:pnp_admm_sms:groups"),
             ("pnp_admm_sms", (mp.real, y, {"iter": 2}), "qmri:pnp_admm_sms:size")]
    for cmd, args, ident in cases:
        with pytest.raises(MexError) as err:
            qmri_mex(cmd, *args, nargout=1)
        assert err.value.id == ident, (cmd, ident, err.value.id, err.value.msg)
    mdir = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "matlab")
    src = open(os.path.join(mdir, "PnP_ADMM_sms_hip.m")).read()
    assert "qmri_mex('pnp_admm_sms'" in src and "groups_per_launch" in src
    assert "qmri_mex('set_sms'" in open(os.path.join(mdir, "qmri_set_sms.m")).read()


def test_design_section_and_documents_exist():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 31\. .*multi-slice", design, re.M | re.I)
    assert m, "DESIGN.md section 31"
    sec = design[m.start():]
    for word in ("sms_plan.h", "k_sms_combine", "k_sms_expand", "k_sms_scalar", "bit for bit", "Not built", "Z^2", "qmri_problem", "sms_times", "Launches per iteration"):
        assert word in sec, word
    assert "qmri_pnp_admm_sms" in open(os.path.join(ROOT, "README.md")).read() and "qmri_set_sms" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "sms_times.py")) and os.path.exists(os.path.join(ROOT, "profiles", "sms_times.json"))
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "sms_kernels.hip" in make and "api_sms.cpp" in make and "FLAGS_sms_kernels = -Rpass-analysis=kernel-resource-usage" in make and "host_asan_sms" in make


def test_sms_plan_header_stands_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "sms_plan.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_sms_plan_sweep_under_address_and_ub_sanitizer(tmp_path):
    """tests/cpp/sms_plan_test.cpp: both image orders over ncoil 1 .. 13, Z 1 .. 8, G 1 .. 3, max_batch 1 .. 20 -- every image exactly once and
    ascending, begin / continue / finish consistent, no partial-sum slot overlapping."""
    exe = tmp_path / "sms_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "sms_plan_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SMS_PLAN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert int(re.search(r"swept (\d+)", r.stdout).group(1)) == 13 * 8 * 3 * 20 * 2


def test_refusals_and_state_lifetime_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_sms.cpp against the host-only sanitised library: every refusal of the six entry points without a
    context and with one, and the state of qmri_set_sms across the operator's replacement, as a stand-alone program."""
    subprocess.run(["make", "-C", CSRC, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    assert rt_dirs, "clang sanitizer runtime not found"
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_build_asan", "host_asan_sms")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_SMS_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
