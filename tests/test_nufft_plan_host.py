"""CPU: the host planning of the trajectory (NUFFT) family -- csrc/nufft_plan.h (bins, spreading lists, segments and partial-sum slots,
deapodisation, ramps, phases, the exact spiral, the density compensation's kernel sums) and csrc/offres_plan.h (field-map histogram, segment times,
coefficient system and Cholesky factor, difference histogram, QR tables) -- through the stand-alone programs tests/cpp/nufft_plan_test.cpp and
tests/cpp/offres_plan_test.cpp, built with the address and undefined-behaviour sanitizers.  The programs check, case by case, what holds whatever the
thresholds are; this file holds what the thresholds give, and compares the float tables with the numpy restatements the GPU tests already use."""
import os
import subprocess

import numpy as np
import pytest

import dcf_ref as D
import nufft_ref as R
import offres_normal_ref as FN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")
EPS = np.finfo(np.float64).eps

# case -> (m, segments, split tiles, partial slots, list entries, digest of perm / t / list / segs / reds).  Recorded from the planning block as it
# stood inside qmri_set_operator_nufft before it moved into nufft_plan.h (the block copied verbatim into a scratch program and run on these
# trajectories), NOT from nu_plan: a changed tile side, window rule, wrap, segment cut, slot numbering or sort order changes a line here.  That scratch
# program also compared the float tables (u, ph, dp, ramps) of old and new code on every case: identical bits.
EXPECTED = {
    "A_16x24/w2/seg512":      (64, 6, 0, 0, 80, "b2389cbcfe6a70e8"),
    "A_16x24/w2/seg32":       (64, 6, 0, 0, 80, "b2389cbcfe6a70e8"),
    "A_16x24/w7/seg512":      (64, 6, 0, 0, 129, "a10f0c95e9d2858c"),
    "A_16x24/w7/seg32":       (64, 6, 0, 0, 129, "a10f0c95e9d2858c"),
    "A_16x24/w12/seg512":     (64, 6, 0, 0, 188, "51c938b979446a66"),
    "A_16x24/w12/seg32":      (64, 8, 2, 4, 188, "dcf1bd16c965776c"),        # two tiles' lists exceed 32 entries
    "A_16x24/w16/seg512":     (64, 6, 0, 0, 238, "e13ddc6bffdffdd7"),
    "A_16x24/w16/seg32":      (64, 11, 5, 10, 238, "1bd58d40c5206428"),      # five of the six tiles are split in two
    "B_spiral32/w12/seg512":  (2880, 28, 4, 16, 9303, "d0e8e899732c9bdf"),   # the spiral's centre: the four middle tiles of 16 are split
    "B_spiral32/w12/seg32":   (2880, 300, 16, 300, 9303, "1a8e08271bca0219"),  # every tile is split
    "C_32x64/w12/seg512":     (700, 32, 0, 0, 1992, "be8ee3574b2013d0"),     # rectangular: 4 x 8 tiles
    "D_corner16/w2/seg512":   (1, 4, 0, 0, 4, "a3685ce4325d098f"),           # (pi, -pi): the window straddles the wrap on both axes, all 2 x 2 tiles
    "D_corner16/w16/seg512":  (1, 4, 0, 0, 4, "a3685ce4325d098f"),
    "E_pile16/w12/seg512":    (1100, 12, 4, 12, 4400, "06638ad14c5980fc"),   # 1100 > 2 x 512: 3 segments per tile, ties keep tile order
}

# map -> (pixels, bins, digest of the counts), recorded the same way from the histogram block of qmri_set_field_map before it moved into
# offres_plan.h.  The same scratch program compared every table of both L searches (segment times, G, Cholesky factor, difference histogram, G, Qw, U)
# of old and new code for L = 1 .. 16 and L' = 2 .. 32 on these maps, the kernel sums and kappa at every width, and the spiral: identical bits, but
# for the last segment time where the formula rounds an ulp off t_max (here L' = 28, 30, 32), which is now t_max itself, and the tables that follow from it.
EXPECTED_HIST = {
    "map16/nbins16":  (256, 16, "850be71145a2d153"),
    "map16/nbins256": (256, 256, "196aa7951d741d53"),
    "map32/nbins16":  (1024, 16, "e1c2948430831763"),
    "map32/nbins256": (1024, 256, "55d9e9ca6eb64f63"),
    "constant16":     (256, 1, "0000000000000100"),
}


def _build_and_run(tmp, name):
    exe = tmp / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def nufft_run(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("nufft_plan"), "nufft_plan_test")


@pytest.fixture(scope="module")
def offres_run(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("offres_plan"), "offres_plan_test")


def _dumps(stdout):
    return {ln.split()[1]: np.array([float(v) for v in ln.split()[2:]]) for ln in stdout.splitlines() if ln.startswith("dump ")}


def test_nufft_plan_on_the_host_under_sanitizers(nufft_run):
    r = nufft_run
    assert r.returncode == 0, r.stderr[-4000:]
    got = {}
    for ln in r.stdout.splitlines():
        name, *fields = ln.split()
        if "/" in name:
            kv = dict(f.split("=") for f in fields)
            got[name] = (int(kv["m"]), int(kv["nseg"]), int(kv["nred"]), int(kv["nslot"]), int(kv["list"]), kv["digest"])
    assert sorted(got) == sorted(EXPECTED)
    wrong = {k: (got[k], EXPECTED[k]) for k in EXPECTED if got[k] != EXPECTED[k]}
    assert not wrong, wrong


def test_nufft_plan_float_tables_against_the_restatements(nufft_run):
    """Case A (16 x 24, 64 samples) at width 12: u is omega N / pi exactly; the sample phases and the half-bin ramps are numpy's cos and sin within
    4 ulp of 1 (libm and numpy each round within an ulp); 1 / Phi is nufft_ref.deapodisation within 1e-12 relative (the same 200-point rule, 200 terms
    of a few ulp each, a decade of margin); the kernel sum and kappa are dcf_ref's within 1e-14 relative (16 terms at most)."""
    d = _dumps(nufft_run.stdout)
    N, M, w = 16, 24, 12
    om, perm = d["omega"].reshape(-1, 2), d["perm"].astype(int)
    u, ph, ramp = d["u"].reshape(-1, 2), d["ph"].reshape(-1, 2), d["ramp"].reshape(-1, 2)
    assert sorted(perm) == list(range(64)) and u.shape == (64, 2) and ramp.shape == (N + M, 2) and d["dp"].shape == (N + M,)
    assert np.array_equal(u[:, 0], om[perm, 0] * N / np.pi) and np.array_equal(u[:, 1], om[perm, 1] * M / np.pi)
    a = -(om[perm, 0] * (N // 2) + om[perm, 1] * (M // 2))
    err_ph = max(np.abs(ph[:, 0] - np.cos(a)).max(), np.abs(ph[:, 1] - np.sin(a)).max())
    ar = np.concatenate([-np.pi * (np.arange(N) - N // 2) / N, -np.pi * (np.arange(M) - M // 2) / M])
    err_ramp = max(np.abs(ramp[:, 0] - np.cos(ar)).max(), np.abs(ramp[:, 1] - np.sin(ar)).max())
    beta = D.plan_beta(w)
    ref = np.concatenate([R.deapodisation(N, w, beta), R.deapodisation(M, w, beta)])
    err_dp = np.abs(d["dp"] / ref - 1).max()
    print(f"ph {err_ph:.3g}  ramp {err_ramp:.3g} (limit {4 * EPS:.3g})  dp {err_dp:.3g} (limit 1e-12)")
    assert err_ph <= 4 * EPS and err_ramp <= 4 * EPS
    assert err_dp <= 1e-12
    worst = 0.0
    for ln in nufft_run.stdout.splitlines():
        f = ln.split()
        if f[0] == "ksum":
            worst = max(worst, abs(float(f[2]) / D.kernel_sum(int(f[1]), D.plan_beta(int(f[1]))) - 1))
        if f[0] == "kappa":
            worst = max(worst, abs(float(f[3]) / D.kappa(int(f[1]), int(f[2]), D.plan_beta(int(f[2]))) - 1))
    print(f"kernel sum / kappa {worst:.3g} (limit 1e-14)")
    assert sum(ln.startswith("ksum") for ln in nufft_run.stdout.splitlines()) == 15 and worst <= 1e-14


def test_offres_tables_on_the_host_under_sanitizers(offres_run):
    """The program's own checks (histogram, Cholesky and QR bounds, refusals, difference histogram, segment times), the pinned counts,
    and the difference histogram against offres_normal_ref.diff_histogram within 4 nbins eps."""
    r = offres_run
    assert r.returncode == 0, r.stderr[-4000:]
    got = {}
    for ln in r.stdout.splitlines():
        name, *fields = ln.split()
        if "digest=" in ln:
            kv = dict(f.split("=") for f in fields)
            got[name] = (int(kv["pixels"]), int(kv["nbins"]), kv["digest"])
    assert got == EXPECTED_HIST
    print([ln for ln in r.stdout.splitlines() if ln.startswith("worst")])
    d = _dumps(r.stdout)
    for nbins in (16, 256):
        p, dh = d[f"p{nbins}"], d[f"dh{nbins}"]
        assert p.shape == (nbins,) and dh.shape == (2 * nbins - 1,)
        assert np.abs(dh - FN.diff_histogram(p)).max() <= 4 * nbins * EPS


@pytest.mark.parametrize("header", ["nufft_plan.h", "offres_plan.h"])
def test_plan_headers_stand_alone(header):
    """plain C++17: each compiles on its own, without HIP and without the library's other headers (nufft_plan.h includes op_plan.h for the spiral)."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, header)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
